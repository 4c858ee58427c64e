"""The fp32x3 mode on the host: the split rule of GSL_F32X3 (gslora_hip.ops.f32x3_split_reference restates what include/gslora_hip.h says), what its
six-product set costs against the exact product — and that five products cost visibly more —, and the names the mode goes by."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = np.float32(2.0 ** 127) * np.float32(2.0 - 2.0 ** -8)      # 2^128 - 2^119 (bits 0x7f7f8000): from here on round-to-nearest alone would give Inf


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def is_bf16(x):
    return (bits(x) & 0xFFFF) == 0


def check_exact(x):
    from gslora_hip import ops
    hi, mid, lo = ops.f32x3_split_reference(x)
    assert is_bf16(hi).all() and is_bf16(mid).all() and is_bf16(lo).all()
    s = hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64)      # (exact in f64: three 8-bit significands within 2^-27)
    assert np.array_equal(s, x.astype(np.float64))
    f = (x != 0) & (np.abs(x) < TOP)                                                # (at the very top hi + mid alone is 2^128: no f32)
    with np.errstate(over="ignore"):
        assert np.array_equal(bits((hi + mid) + lo)[f], bits(x)[f])                 # ... and in f32, largest pieces first
    # the pieces shrink: |mid| within an ulp of hi's 8-bit significand (half of one below the saturating top), |lo| 2^-9 below that
    assert (np.abs(mid)[f] <= np.abs(x)[f] * 2.0 ** -8).all() and (np.abs(mid) <= np.abs(x) * 2.0 ** -7).all() and (np.abs(lo) <= np.abs(x) * 2.0 ** -16).all()
    return hi, mid, lo


def test_split_is_exact_on_random_values_over_200_binades():
    rng = np.random.default_rng(7)
    x = (rng.uniform(1.0, 2.0, 1_000_000) * np.exp2(rng.integers(-100, 101, 1_000_000)) * rng.choice([-1.0, 1.0], 1_000_000)).astype(np.float32)
    check_exact(x)


def test_split_at_powers_of_two_their_neighbours_zeros_and_the_top_of_the_range():
    from gslora_hip import ops
    p2 = np.exp2(np.arange(-109, 128)).astype(np.float32)      # (the exact range starts at 2^-110: the value below 2^-109 is still inside)
    around = np.concatenate([p2, np.nextafter(p2, np.float32(np.inf)), np.nextafter(p2, np.float32(0))])
    check_exact(np.concatenate([around[around < TOP], -around[around < TOP]]))
    hi, mid, lo = check_exact(np.array([0.0, -0.0], np.float32))
    assert np.array_equal(bits(hi), bits(np.array([0.0, -0.0], np.float32)))      # the sign of zero stays in hi
    # below 2^-110 the last piece can fall under bf16's denormal grid (2^-133): the header's absolute bound 2^-134, nothing worse
    tiny = np.concatenate([np.exp2(np.arange(-149.0, -109.0)), np.nextafter(np.exp2(np.arange(-126, -109)).astype(np.float32), np.float32(0)), [1e-45, 3e-39, -1.1754942e-38]]).astype(np.float32)
    h, m, l = ops.f32x3_split_reference(tiny)
    assert (np.abs(h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64) - tiny.astype(np.float64)) <= 2.0 ** -134).all()
    # the top of the range: from 2^128 - 2^119 on, round-to-nearest would take hi to Inf; the rule saturates it at the largest finite bf16 instead, as the
    # header says, and the split stays exact up to FLT_MAX
    fmax = np.finfo(np.float32).max
    last = np.nextafter(TOP, np.float32(0))
    x = np.array([last, -last, TOP, -TOP, np.nextafter(TOP, np.float32(np.inf)), fmax, -fmax], np.float32)
    assert bits(x)[2] == 0x7F7F8000
    hi, _, _ = check_exact(x)
    assert np.isfinite(hi).all() and (bits(hi) & 0x7FFFFFFF == 0x7F7F0000).all()
    # Inf and NaN stay themselves in hi, and x - hi is NaN: the flag of the kernel's non-finite rule
    x = np.array([np.inf, -np.inf, np.nan], np.float32)
    hi, mid, lo = ops.f32x3_split_reference(x)
    assert np.array_equal(hi[:2], x[:2]) and np.isnan(hi[2]) and np.isnan(mid).all()


def operands(family, M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    if family == "uniform":
        mk = lambda r: torch.rand(r, K, generator=g) * 2 - 1
    else:
        mk = lambda r: torch.randn(r, K, generator=g) * torch.exp(4 * torch.randn(r, K, generator=g))
    return mk(M).numpy(), mk(N).numpy()


@pytest.mark.parametrize("family", ["uniform", "wide"])
@pytest.mark.parametrize("K", [64, 512])
def test_six_products_carry_the_f32_product_and_five_do_not(family, K):
    """max |sum of products - exact| / sum_k |a w|, float64 accumulation. Bound of the six: 2^-24 (the three dropped products are <= 2^-26 |a w| each
    at worst; measured 1e-9 - 4e-8). The five-product set (no mid * mid, up to 2^-18 |a w| per term) exceeds it: the cap is not idle."""
    from gslora_hip import ops
    A, W = operands(family, 48, 40, K, seed=K + len(family))
    exact = A.astype(np.float64) @ W.astype(np.float64).T
    scale = np.abs(A).astype(np.float64) @ np.abs(W).astype(np.float64).T
    e6 = (np.abs(ops.f32x3_product_reference(A, W) - exact) / scale).max()
    e5 = (np.abs(ops.f32x3_product_reference(A, W, ops.F32X3_FIVE) - exact) / scale).max()
    print(f"{family} K={K}: six {e6:.2e}, five {e5:.2e}, bound {2.0 ** -24:.2e}")
    assert e6 <= 2.0 ** -24
    assert e5 > 2.0 ** -24
    assert len(ops.F32X3_PRODUCTS) == 6 and len(ops.F32X3_FIVE) == 5 and ("mid", "mid") not in ops.F32X3_FIVE


def test_mode_names():
    from gslora_hip import _lib as L, ops
    from vit_pytorch_face import vit_face as V
    assert V.compute_dtype_of("fp32x3") is torch.float32 and V.compute_dtype_of("FP32X3") is torch.float32
    assert V.gemm_mode_of("fp32x3") == "x3" and V.gemm_mode_of("fp32") is None and V.gemm_mode_of(torch.float32) is None
    assert [V.compute_mode_name(V.compute_dtype_of(n), V.gemm_mode_of(n)) for n in ("fp16", "bf16", "fp32", "fp32x3")] == ["fp16", "bf16", "fp32", "fp32x3"]
    with pytest.raises(ValueError, match="fp32x3"):      # the error lists the allowed names, the new one among them
        V.compute_dtype_of("fp32x4")
    assert L.F32X3 == 3 and (L.F32, L.BF16, L.F16) == (0, 1, 2)
    assert ops.gemm_code(torch.float32) == L.F32 and ops.gemm_code(torch.float32, "x3") == L.F32X3
    assert ops.gemm_code(torch.bfloat16) == L.BF16 and ops.gemm_code(torch.float16) == L.F16
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(RuntimeError, match="float32"):
            ops.gemm_code(dt, "x3")
    with pytest.raises(ValueError):
        ops.gemm_code(torch.float32, "x2")


def test_set_compute_dtype_sets_and_resets_the_mode():
    from vit_pytorch_face import ViT_face
    m = ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=8, image_size=40, patch_size=8, dim=64, depth=1, heads=1, mlp_dim=64, lora_rank=2)
    assert m.gemm_mode is None and m.compute_mode in ("fp16", "bf16", "fp32")
    assert m.set_compute_dtype("fp32x3") is m
    assert m.compute_dtype is torch.float32 and m.gemm_mode == "x3" and m.compute_mode == "fp32x3"
    for name, dt in (("fp32", torch.float32), ("fp16", torch.float16), ("bf16", torch.bfloat16)):
        m.set_compute_dtype("fp32x3").set_compute_dtype(name)
        assert m.compute_dtype is dt and m.gemm_mode is None and m.compute_mode == name
    m.set_compute_dtype("fp32x3").set_compute_dtype(torch.float32)      # a torch dtype names the plain mode
    assert m.compute_mode == "fp32"
    m.set_compute_dtype(m.set_compute_dtype("fp32x3").compute_mode)     # the name round-trips: what the evaluations save and restore
    assert m.compute_mode == "fp32x3"
    with pytest.raises(AttributeError):
        m.compute_mode = "fp32"


def test_mode_from_the_environment(monkeypatch):
    from vit_pytorch_face import ViT_face
    monkeypatch.setenv("GSLORA_DTYPE", "fp32x3")
    m = ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=8, image_size=40, patch_size=8, dim=64, depth=1, heads=1, mlp_dim=64, lora_rank=2)
    assert m.compute_mode == "fp32x3" and m.compute_dtype is torch.float32


def test_header_enum_exports_and_signatures():
    from gslora_hip import _lib as L
    hdr = open(os.path.join(ROOT, "include", "gslora_hip.h")).read()
    enum = re.search(r"enum gsl_dtype \{([^}]*)\}", hdr).group(1)
    assert dict((k, int(v)) for k, v in re.findall(r"(GSL_\w+) = (\d+)", enum)) == {"GSL_F32": 0, "GSL_BF16": 1, "GSL_F16": 2, "GSL_F32X3": 3}
    # no entry point was added for the mode: header = exports = _lib.SIGNATURES, as before
    declared = set(re.findall(r"\b(gsl_[a-z0-9_]+)\s*\(", hdr)) - {"gsl_dropout_keep"}      # as tests/test_host_logic.py
    assert declared == set(L.SIGNATURES)
    assert not any("x3" in n for n in declared)
    lib = L.load()
    assert all(hasattr(lib, n) for n in declared)
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:
        exported = {ln.split()[-1] for ln in nm.stdout.splitlines() if ln.split()[-1].startswith("gsl_") and ln.split()[-2] in "TW"}
        assert exported == declared, exported ^ declared
    # the header states the rule the host restates
    text = " ".join(hdr.split())
    for phrase in ("ROUND TO NEAREST EVEN", "2^-110", "2^-134", "hi*hi, hi*mid, mid*hi, mid*mid, hi*lo, lo*hi", "SATURATING", "0x7f7f8000", "NOT the k-ordered fmaf chain", "non-finite rule"):
        assert phrase in text, phrase
