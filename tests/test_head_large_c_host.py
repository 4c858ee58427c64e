"""CPU tests of the head above 1024 classes: the contract written in the header, the unchanged C ABI, the refusals that need no device and
the presence of the class-tiled kernels in the product library (which the spill and barrier checks of tests/test_host_logic.py walk)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 16      # a non-null, 16-byte-aligned address that is never dereferenced: the argument checks fail first


def header():
    return open(os.path.join(ROOT, "include", "gslora_hip.h")).read()


def test_header_states_the_workspace_contract_and_the_class_range():
    hdr = header()
    comment = hdr[hdr.index("gsl_cosface_prep"):hdr.index("GSL_API int gsl_head_bwd(")]
    for words in ("C <= 1024", "C > 1024", "amax_ws is", "REQUIRED in every mode", "gscale == NULL", "B*(D+1) floats", "[B, B + B*D)", "Any C >= 1",
                  "B*C and C*D below 2^31", "before any launch"):
        assert words in comment, words


def test_no_entry_point_was_added_or_changed():
    from gslora_hip import _lib
    declared = set(re.findall(r"\b(gsl_[a-z0-9_]+)\s*\(", header())) - {"gsl_dropout_keep"}
    assert declared == set(_lib.SIGNATURES) and len(_lib.SIGNATURES) == 59      # (56 + gsl_attention_kernel_choice + the two LoRA-gradient plan queries)
    assert len(_lib.SIGNATURES["gsl_head_fwd"]) == 21 and len(_lib.SIGNATURES["gsl_head_fwd_margin"]) == 25
    assert len(_lib.SIGNATURES["gsl_head_bwd"]) == 28 and len(_lib.SIGNATURES["gsl_head_bwd_margin"]) == 33


def bwd(L, margin, **kw):
    a = dict(dl=P, de=None, x=P, xdt=0, T=2, g=P, mean=P, rstd=P, emb=P, Wn=P, dx=P, dxb=P, B=4, D=64, C=1100, s=64.0, dt=0, sdt=0, p=0.0, seed=0,
             site=0, linear=0, pool=0, compact=0, gscale=None, ws=P, texp=0)
    a.update(kw)
    from gslora_hip import _lib
    a["xdt"] = a["dt"] = a["sdt"] = _lib.F32
    args = [a[k] for k in ("dl", "de", "x", "xdt", "T", "g", "mean", "rstd", "emb", "Wn", "dx", "dxb", "B", "D", "C", "s", "dt", "sdt", "p", "seed", "site",
                           "linear", "pool", "compact", "gscale", "ws", "texp")]
    if margin:
        return L.gsl_head_bwd_margin(*args, 1, 0.5, 0, P, P, None)
    return L.gsl_head_bwd(*args, None)


def fwd(L, margin, **kw):
    from gslora_hip import _lib
    a = dict(x=P, T=2, g=P, b=P, Wn=P, y=P, emb=P, mean=P, rstd=P, logits=P, B=4, D=64, C=1100)
    a.update(kw)
    args = [a["x"], _lib.F32, a["T"], a["g"], a["b"], 1e-5, a["Wn"], a["y"], a["emb"], a["mean"], a["rstd"], a["logits"], a["B"], a["D"], a["C"], 64.0,
            0.35, None, 0, 0]
    if margin:
        return L.gsl_head_fwd_margin(*args, 1, 0.5, 0, P, None)
    return L.gsl_head_fwd(*args, None)


@pytest.mark.parametrize("margin", [False, True])
def test_entry_points_refuse_before_any_launch(margin):
    from gslora_hip import _lib
    L = _lib.load()
    name = b"gsl_head_bwd_margin" if margin else b"gsl_head_bwd"
    # above 1024 classes the workspace is required, also without gscale
    assert bwd(L, margin, ws=None) == -1
    err = L.gsl_last_error()
    assert name in err and b"amax_ws" in err and b"C > 1024" in err
    assert bwd(L, margin, ws=None, dl=None) == -1 and b"amax_ws" in L.gsl_last_error()
    # the class range: B*C and C*D below 2^31 elements
    for bad in (dict(C=(1 << 31) - 1), dict(C=(1 << 25), D=64), dict(C=(1 << 20), B=2048)):
        assert bwd(L, margin, **bad) == -1, bad
        err = L.gsl_last_error()
        assert name in err and b"C out of range" in err and b"2^31" in err, (bad, err)
    assert bwd(L, margin, Wn=P + 4) == -1 and b"16-byte aligned" in L.gsl_last_error()
    # the old bounds are what they were
    assert bwd(L, margin, D=1028) == -1 and bwd(L, margin, D=66) == -1 and bwd(L, margin, C=100, gscale=P, ws=None) == -1
    fname = b"gsl_head_fwd_margin" if margin else b"gsl_head_fwd"
    for bad in (dict(C=(1 << 31) - 1), dict(C=(1 << 25), D=64), dict(C=(1 << 20), B=2048)):
        assert fwd(L, margin, **bad) == -1, bad
        err = L.gsl_last_error()
        assert fname in err and b"C out of range" in err, (bad, err)
    assert fwd(L, margin, Wn=P + 8) == -1 and b"16-byte aligned" in L.gsl_last_error()


def test_ops_sizes_the_workspace_by_the_class_count():
    from gslora_hip import ops
    assert ops.HEAD_TILED_C == 1024
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.head_bwd(torch.zeros(2, 1100), None, torch.zeros(4, 64), 2, 2, 64, torch.ones(64), torch.zeros(2), torch.ones(2), torch.zeros(2, 64),
                     torch.zeros(1100, 64), 64.0, torch.float32)
    src = open(os.path.join(ROOT, "gs-lora_amd", "gslora_hip", "ops.py")).read()
    assert "B * (D + 1) if C > HEAD_TILED_C else (B if gscale is not None else 0)" in src


def test_tiled_kernels_are_in_the_product_library():
    """... so the register-spill and LDS-barrier disassembly checks cover them; and no LDS array of head.hip is sized by C."""
    from gslora_hip import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    for name in (b"head_logits_tiled_kernel", b"head_de_tiled_kernel"):
        assert name in blob, name
    src = open(os.path.join(ROOT, "gs-lora_amd", "csrc", "head.hip")).read()
    tiled = src[src.index("K10t class-tiled head"):src.index("struct HeadCall {")]
    tiled += src[src.index("// Stage 1 of the class-tiled backward"):src.index("// compact != 0 (pool = 'cls' only)")]
    shared = re.findall(r"__shared__[^;]*;", tiled)
    assert len(shared) == 8
    for decl in shared:
        dims = re.findall(r"\[([^\]]*)\]", decl)
        assert dims and all(re.fullmatch(r"[A-Z_0-9 *+]+", d) for d in dims), decl      # compile-time tile constants only
