"""The head kernels (csrc/head.hip: gsl_cosface_prep, gsl_head_fwd[_margin], gsl_head_bwd[_margin], gsl_head_wgrad) at their edges, on the
probes of oracle/head_probes.py: every end of the forward's 5-class rounds on both launch widths (C = 79 / 80 / 81 on 1024 threads,
19 / 20 / 21 on 256), D at the lane-stride and workgroup ends, cls and mean pool at T = 1 / 2 / 5, the three stream formats, labels at
0 / 63 / 64 / C - 1 / -1 / C / 2^32 + 3 and NULL, x shifted by 1e3, a zero embedding, a zero and a sub-clamp row of W, label rows parallel
and antiparallel to the embedding; the backward at C = 255 / 256 / 257 / 1023 / 1024 with labels on both sides of thread 255, dense
(Tn = 1 / 2 / 5), compact and mean-pool layouts, dropout at the dense counter, the eleven dtype rows, cos_y planted at +-1, 1 - 2^-24,
th and the float above it, +-0, 1e-30 and the float above 1, the loss-scaled form (an ordinary batch, a maximum that is exactly a power
of two, a zero gradient, a NaN row, an Inf row); the per-class weight gradient at the ends of its wave rounds, lane columns and class
tiles and on its fallback above 1024 classes; the class-tiled kernels at their tile ends; the refusals above 1024 classes.

Every entry point is called through gslora_hip._lib on raw addresses, so that every tensor sits between NaN bands
(tests/guard_bands.py): inputs unchanged, no output element unwritten, nothing written outside. Results are held per element to the
float64 references under the bounds of oracle/head_probes.py (no tolerance of this file's own; tests/test_head_probes_host.py shows on
the CPU that an f32 restatement of the kernels stays under them and that each fault model exceeds them). Each comparison prints its
largest error / bound ratio (pytest -s; profiles/head_kernel_tests.md).

Finding this file was written against: head_bwd_kernel took an embedding below F.normalize's clamp (0 < ||e|| < 1e-12) through the
projection formula, where the clamp's derivative is 0 and d e = d e-hat / 1e-12 — the rule head_wgrad_kernel already had for a row of W
(test_backward[bwd_tiny_emb])."""
import math

import numpy as np
import pytest
import torch

from guard_bands import NAN_SENTINEL, Banded, ptr
from oracle import head_probes as P

pytestmark = pytest.mark.gpu

TD = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CODE = {"f32": 0, "bf16": 1, "f16": 2}
GSL_ERR_ARG = -1
SEED, SITE = P.DROP_SEED_SITE


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    from gslora_hip import _lib
    _lib.load()
    return _lib


def stream():
    return torch.cuda.current_stream().cuda_stream


def In(a, fmt="f32"):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype.is_floating_point:
        t = t.to(TD[fmt])      # (exact: the probes hand out values of the format)
    return Banded(t.shape, t.dtype, t)


def Out(*shape, fmt="f32"):
    return Banded(shape, TD[fmt], sentinel=NAN_SENTINEL[TD[fmt]])


def ReadWrite(a):
    b = In(a)
    b.accumulates = True
    return b


def call(lib, entry, *args):
    lib.check(getattr(lib.load(), entry)(*args, stream()), entry)


def settled(t, partial=()):
    """Inputs unchanged, bands of the outputs intact, no output element unwritten (partial: outputs the call may leave elements of)."""
    torch.cuda.synchronize()
    for n, b in t.items():
        if b is None:
            continue
        if getattr(b, "accumulates", False):
            assert b.outside_intact(), ("something outside changed:", n)
        else:
            assert b.bands_intact(), ("input changed or bands of" if b.is_input else "bands of", n)
            if not b.is_input and n not in partial:
                assert b.unwritten() == 0, ("unwritten elements in", n)


def host(b):
    return None if b is None else b.view.float().cpu().numpy()


def report(case, r):
    print("RATIO", case.name, " ".join(f"{k}={v:.3f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, (case.name, r)


def ids(c):
    return c.name


def kind_args(case):
    m, easy = P.ARC_M.get(case.form, (0.0, 0))
    return (1 if P.is_arc(case.form) else 0), float(m), int(easy)


# ---------------------------------------------------------------------------------------------------------------- the entry points, banded
def cosface_prep(lib, W):
    C, D = W.shape
    t = dict(W=In(W), Wn=Out(C, D))
    call(lib, "gsl_cosface_prep", ptr(t["W"]), ptr(t["Wn"]), C, D)
    settled(t)
    return host(t["Wn"])


def head_fwd(lib, d, case, want_logits=True, label=True):
    B, T, D, C = case.B, case.T, case.D, case.C
    xf = P.triple(case)[2]
    arc, lin = P.is_arc(case.form), P.is_linear(case.form)
    t = dict(x=In(d["x"], xf), gamma=In(d["gamma"]), beta=In(d["beta"]), Wn=In(d["Wn"]), label=In(d["label"]) if label else None,
             bias=In(d["bias"]), emb=Out(B, D), mean=Out(B), rstd=Out(B), logits=Out(B, C) if want_logits else None, cos_y=Out(B) if arc else None)
    head = (ptr(t["x"]), CODE[xf], T, ptr(t["gamma"]), ptr(t["beta"]), float(d["eps"]), ptr(t["Wn"]), ptr(t["label"]), ptr(t["emb"]),
            ptr(t["mean"]), ptr(t["rstd"]), ptr(t["logits"]), B, D, C, P.COS_S, P.COS_M, ptr(t["bias"]), int(lin), int(case.pool == "mean"))
    if arc:
        call(lib, "gsl_head_fwd_margin", *head, *kind_args(case), ptr(t["cos_y"]))
    else:
        call(lib, "gsl_head_fwd", *head)
    settled(t, partial=("cos_y",))
    if arc:      # cos_y is written at the images whose label names a class, and nowhere else
        want = int((~P.valid_labels(d["label"], C)).sum()) if want_logits else B
        assert t["cos_y"].unwritten() == want, "cos_y: written without a label in range, or not written with one"
    return {k: host(t[k]) for k in ("emb", "mean", "rstd", "logits", "cos_y")}


def dropout_keep(lib, n, p):
    keep = torch.empty(n, device="cuda", dtype=torch.uint8)
    call(lib, "gsl_dropout_mask", keep.data_ptr(), n, float(p), SEED, SITE)
    return keep.cpu().numpy()


def head_bwd(lib, d, case, gscale0=None):
    B, T, D, C = case.B, case.T, case.D, case.C
    tT, tS, tX = P.triple(case)
    arc, lin = P.is_arc(case.form), P.is_linear(case.form)
    p = 0.1 if P.opt(case, "p0.1") else 0.0
    compact, scaled = P.opt(case, "compact"), P.opt(case, "scaled")
    shape = (B, D) if compact else (B, T, D)
    t = dict(dl=None if P.opt(case, "de") else In(d["dl"]), demb=None if P.opt(case, "dl") else In(d["demb"]), x=In(d["x"], tX),
             gamma=In(d["gamma"]), mean=In(d["mean"]), rstd=In(d["rstd"]), emb=In(d["emb"]), Wn=In(d["Wn"]), cos_y=In(d["cos_y"]) if arc else None,
             label=In(d["label"]) if arc else None, dx=Out(*shape, fmt=tS), dxb=Out(*shape, fmt=tT),
             gscale=ReadWrite(np.zeros(4, np.float32) if gscale0 is None else gscale0) if scaled else None,
             ws=Out(B * (D + 1) if C > P.HEAD_TILED_C else B) if (scaled or C > P.HEAD_TILED_C) else None)
    head = (ptr(t["dl"]), ptr(t["demb"]), ptr(t["x"]), CODE[tX], T, ptr(t["gamma"]), ptr(t["mean"]), ptr(t["rstd"]), ptr(t["emb"]), ptr(t["Wn"]),
            ptr(t["dx"]), ptr(t["dxb"]), B, D, C, 1.0 if lin else P.COS_S, CODE[tT], CODE[tS], p, SEED, SITE, int(lin), int(case.pool == "mean"),
            int(compact), ptr(t["gscale"]), ptr(t["ws"]), 0)
    if arc:
        call(lib, "gsl_head_bwd_margin", *head, *kind_args(case), ptr(t["cos_y"]), ptr(t["label"]))
    else:
        call(lib, "gsl_head_bwd", *head)
    settled(t, partial=("ws",))
    keep = dropout_keep(lib, B * T * D, p)
    assert (keep == P.drop_keep(np.arange(B * T * D, dtype=np.uint64), p, SEED, SITE)).all(), "the probes' restatement of the dropout hash"
    got = dict(dx=host(t["dx"]), dxb=host(t["dxb"]), gscale=host(t["gscale"]))
    return got, keep, p


def head_wgrad(lib, d, case):
    B, D, C = case.B, case.D, case.C
    arc, lin = P.is_arc(case.form), P.is_linear(case.form)
    if P.opt(case, "off4"):      # emb one float into a 16-byte aligned buffer: the class-tiled kernel's float4 loads are not legal
        emb = In(np.concatenate([[np.nan], d["emb"].ravel()]).astype(np.float32))
        emb_ptr = ptr(emb) + 4
    else:
        emb = In(d["emb"])
        emb_ptr = ptr(emb)
    t = dict(dl=In(d["dl"]), emb=emb, W=None if lin else In(d["W"]), label=In(d["label"]) if arc else None, cos_y=In(d["cos_y"]) if arc else None,
             dW=Out(C, D), dbias=Out(C) if case.form == "linear_bias" else None)
    kind, m, easy = kind_args(case)
    call(lib, "gsl_head_wgrad", ptr(t["dl"]), emb_ptr, ptr(t["W"]), ptr(t["label"]), ptr(t["cos_y"]), ptr(t["dW"]), ptr(t["dbias"]), B, C, D,
         2 if lin else kind, P.COS_S, m, easy)
    settled(t)
    return dict(dW=host(t["dW"]), dbias=host(t["dbias"]))


# ---------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("case", P.cases("fwd") + P.cases("logits_t"), ids=ids)
def test_forward(lib, case):
    d = P.make(case)
    if case.regime in ("zero_w", "tiny_w"):      # the zero row goes through gsl_cosface_prep: 0 / 1e-12 = 0
        d["Wn"] = cosface_prep(lib, d["W"])
        assert (d["Wn"][1] == 0).all()
    got = head_fwd(lib, d, case)
    r, _ = P.judge_fwd(d, case, got)
    report(case, r)


@pytest.mark.parametrize("name", ["fwd_d68", "fwd_zero_w_cosface", "fwd_d1024", "fwd_c1024"])
def test_cosface_prep_rows(lib, name):
    """Wn = W / max(||W||, 1e-12): a wave per row, four rows a workgroup (C = 17 and 21: a last workgroup with dead waves)."""
    case = P.BY_NAME[name]
    W = P.make(case)["W"]
    got = cosface_prep(lib, W)
    W64 = W.astype(np.float64)
    ref = W64 / np.maximum(np.sqrt((W64 * W64).sum(1, keepdims=True)), P.CLAMP)
    r = P.ratio(got, ref, ((-(-case.D // 64) + 7) / 2 + 3) * P.E * np.abs(ref))      # the row sum, sqrtf, the division, the product
    print(f"RATIO prep_{name} {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("name", ["fwd_t5_mean", "fwd_c81_arcface"])
def test_forward_without_logits(lib, name):
    """logits = NULL: emb / mean / rstd alone, cos_y untouched, Wn and label not read (NULL)."""
    case = P.BY_NAME[name]
    d = P.make(case)
    got = head_fwd(lib, d, case, want_logits=False)
    r, _ = P.judge_fwd(d, case, got)
    report(case, r)
    full = head_fwd(lib, d, case)
    assert all(np.array_equal(got[k], full[k]) for k in ("emb", "mean", "rstd"))


@pytest.mark.parametrize("name", ["fwd_c80_cosface", "fwd_b129_c21"])
def test_cosface_without_labels(lib, name):
    """label = NULL: no column takes the margin."""
    case = P.BY_NAME[name]._replace(form="cosface")
    d = P.make(case)
    got = head_fwd(lib, d, case, label=False)
    d["label"][:] = -1
    r, _ = P.judge_fwd(d, case, got)
    report(case, r)


# ---------------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("case", P.cases("bwd") + P.cases("de_t"), ids=ids)
def test_backward(lib, case):
    d = P.make(case)
    got, keep, p = head_bwd(lib, d, case)
    report(case, P.judge_bwd(d, case, got, keep, p))
    if P.opt(case, "scaled"):
        assert got["gscale"][2] == 0.0 and got["gscale"][3] == 11.0      # a zeroed buffer: the default exponent, the guard cleared


def test_loss_scaled_zero_gradient(lib):
    """Every gradient zero: S = 1, every store +0."""
    case = P.BY_NAME["bwd_scaled"]
    d = P.make(case)
    d["dl"][:], d["demb"][:] = 0, 0
    got, _, _ = head_bwd(lib, d, case)
    assert got["gscale"][:2].tolist() == [1.0, 1.0]
    assert (got["dx"] == 0).all() and (got["dxb"] == 0).all()


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan_row", "inf_row"])
def test_loss_scaled_nonfinite_row(lib, bad):
    """One image's dlogits row NaN or +Inf: that image's dx is non-finite, gscale[0..1] stay finite powers of two — the scale the rule
    gives for the largest FINITE image maximum (a NaN maximum is passed over), or 1 if an image's maximum came out Inf — and every other
    image is that scale times its reference."""
    case = P.BY_NAME["bwd_scaled"]
    d = P.make(case)
    d["dl"][1, :] = bad
    got, keep, p = head_bwd(lib, d, case)
    S, inv = float(got["gscale"][0]), float(got["gscale"][1])
    assert math.isfinite(S) and math.frexp(S)[0] == 0.5 and inv == 1.0 / S
    assert not np.isfinite(got["dx"][1, 0]).any() and not np.isfinite(got["dxb"][1, 0][keep.reshape(case.B, case.T, case.D)[1, 0] == 1]).any()
    d["dl"][1, :] = 0
    ref = P.bwd64(d, case)
    rest = np.arange(case.B) != 1
    print(f"S = {S} with a {bad} row; the finite images ask for {sorted(P.allowed_scales(ref['amax'][rest], ref['b_amax'][rest]))}")
    assert S in P.allowed_scales(ref["amax"][rest], ref["b_amax"][rest]) | {1.0}
    dx, b_dx, dxb, b_dxb = P.bwd_layout(case, ref["g"], ref["bound"], S, keep, p)
    r = dict(dx=P.ratio(got["dx"][rest], dx[rest], b_dx[rest]), dxb=P.ratio(got["dxb"][rest], dxb[rest], b_dxb[rest]))
    report(case, r)


def test_loss_scaled_guard_state(lib):
    """gscale[2..3] carried over from a step that saturated: the exponent drops by 2 and the scale with it."""
    case = P.BY_NAME["bwd_scaled"]
    d = P.make(case)
    got, keep, p = head_bwd(lib, d, case, gscale0=np.array([0, 0, 65504.0, 11.0], np.float32))
    assert got["gscale"][2] == 0.0 and got["gscale"][3] == 9.0
    ref = P.bwd64(d, case)
    S = float(got["gscale"][0])
    assert S in {P.loss_scale(a, 9) for a in (ref["amax"].max() - ref["b_amax"].max(), ref["amax"].max(), ref["amax"].max() + ref["b_amax"].max())}
    dx, b_dx, _, _ = P.bwd_layout(case, ref["g"], ref["bound"], S, keep, p)
    assert P.ratio(got["dx"], dx, b_dx) <= 1.0 and got["gscale"][1] == 1.0 / S


# ---------------------------------------------------------------------------------------------------------------- weight gradient
@pytest.mark.parametrize("case", P.cases("wgrad") + P.cases("wgrad_t"), ids=ids)
def test_weight_gradient(lib, case):
    d = P.make(case)
    got = head_wgrad(lib, d, case)
    report(case, P.judge_wgrad(d, case, got))
    if case.regime in ("zero_w", "tiny_w"):
        assert np.abs(got["dW"][1]).max() > 1e9      # d What / 1e-12


def test_linear_weight_gradient_without_dbias(lib):
    case = P.BY_NAME["wg_linear"]
    with_bias = head_wgrad(lib, P.make(case), case._replace(form="linear_bias"))
    without = head_wgrad(lib, P.make(case), case)
    assert without["dbias"] is None and np.array_equal(with_bias["dW"], without["dW"])


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("which", ["Wn", "emb"])
def test_misaligned_operands_are_refused_above_1024_classes(lib, which):
    """Above 1024 classes the class-tiled kernels load float4: a Wn or an emb that is not 16-byte aligned is an argument error on the forward
    and on the backward, nothing is launched, every output keeps its sentinel."""
    case = P.BY_NAME["lt_b1"]
    B, T, D, C = case.B, case.T, case.D, case.C
    d = P.make(case)
    off = lambda b, yes: ptr(b) + (4 if yes else 0)
    t = dict(x=In(d["x"]), gamma=In(d["gamma"]), beta=In(d["beta"]), Wn=In(np.zeros(C * D + 1, np.float32)), emb=Out(B * D + 1), mean=Out(B),
             rstd=Out(B), logits=Out(B, C), dl=In(d["dl"]), dx=Out(B, T, D), ws=Out(B * (D + 1)))
    fn = lib.load()
    rc = fn.gsl_head_fwd(ptr(t["x"]), 0, T, ptr(t["gamma"]), ptr(t["beta"]), P.EPS, off(t["Wn"], which == "Wn"), None, off(t["emb"], which == "emb"),
                         ptr(t["mean"]), ptr(t["rstd"]), ptr(t["logits"]), B, D, C, P.COS_S, P.COS_M, None, 0, 0, stream())
    assert rc == GSL_ERR_ARG and b"16-byte aligned" in fn.gsl_last_error()
    rc = fn.gsl_head_bwd(ptr(t["dl"]), None, ptr(t["x"]), 0, T, ptr(t["gamma"]), ptr(t["mean"]), ptr(t["rstd"]), off(t["emb"], which == "emb"),
                         off(t["Wn"], which == "Wn"), ptr(t["dx"]), None, B, D, C, P.COS_S, 0, 0, 0.0, 0, 0, 0, 0, 0, None, ptr(t["ws"]), 0, stream())
    assert rc == GSL_ERR_ARG and b"16-byte aligned" in fn.gsl_last_error()
    torch.cuda.synchronize()
    for n in ("emb", "mean", "rstd", "logits", "dx", "ws"):
        assert t[n].bands_intact() and t[n].unwritten() == t[n].view.numel(), n
