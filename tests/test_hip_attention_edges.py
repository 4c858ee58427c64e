"""Attention at the edges of its kernels: the probes of oracle/attn_probes.py (a leaked padded key, a dropped last key, swapped V rows
and a missing max subtraction each cost an error of order 1: tests/test_attention_probes_host.py) through every dispatch path of
csrc/attention.hip at the token counts around its tile and kernel seams, and NaN guard bands around every input and output.

Tolerances are test_attention's (o 2e-5 / 2e-2, lse 2e-5 / 2e-3, gradients 5e-5 / 3e-2 for f32 / 16-bit), with two differences: the
gradient bound holds per part — dQ, dK and dV each against max(1, max|its reference|) —, and the `o` bound is tol * max(1, max|o_ref|)
(the probes' v = 1 + n puts |o| up to 4 at T = 2, where one bf16 half-ulp is 8e-3; the host test holds a rounding model of a correct
kernel within half of every bound). One bound is not the project's: lse in f32 on `pos`, where |lse| is about 95 and an f32 ulp is
7.6e-6. There torch.logsumexp over the f32 scores on the CPU misses float64 by 5.2e-6 to 1.2e-5 over the cases here (measured per case,
build_case(); up to 1.9e-5 at one image and one head in the host test); the bound is 4x that measured error (the summation order
differs), never below 2e-5: 2.1e-5 to 4.7e-5 here. The kernels' worst lse error on `pos` in f32 was 1.3e-5 against a bound of 4.1e-5.

The reference is float64 torch on the dtype-rounded inputs: on the CPU for a few items, on the device (plain torch, every item
compared) for the many-item rows. `uniform` (q = 0) is checked against its closed forms instead."""
import functools

import pytest
import torch

from guard_bands import Banded, ptr
from oracle import attn_probes as P

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
H16 = [BF16, F16]
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
TOL_O = {F32: 2e-5, BF16: 2e-2, F16: 2e-2}
TOL_LSE = {F32: 2e-5, BF16: 2e-3, F16: 2e-3}
TOL_G = {F32: 5e-5, BF16: 3e-2, F16: 3e-2}
TOL_CLS = {F32: 2e-5, BF16: 2e-2, F16: 2e-2}      # cls kernels against the dense ones (test_long_cls_kernels)
SCALE = P.SCALE


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    from gslora_hip import ops as _ops
    from gslora_hip import _lib
    _lib.load()
    return _ops


def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def amax(x):
    return x.abs().max().item()


def build_case(tag, B, T, H, dt):
    """The probe rounded to dt on the device, its float64 reference (closed forms for `uniform`) and the lse bound."""
    qkv, d_o = (t.to(dt) for t in P.make(tag, B, T, H))
    qd, gd = qkv.cuda(), d_o.cuda()
    rq, rg = (qd, gd) if B * H >= 64 else (qkv, d_o)
    if tag == "uniform":
        o_r, l_r, g_r = P.uniform_closed_form(rq.float(), rg.float(), B, T, H, SCALE)
    else:
        o_r, l_r, g_r = P.reference(rq.float(), rg.float(), B, T, H, SCALE)
    tol_l = TOL_LSE[dt]
    if tag == "pos" and dt == F32:
        q, k, _ = P.split(qkv, B, T, H)
        s32 = (q.float() @ k.float().transpose(-1, -2)) * SCALE
        err = amax(torch.logsumexp(s32, -1).double() - l_r)
        tol_l = max(2e-5, 4 * err)
        print(f"pos f32 B={B} H={H} T={T}: CPU f32 logsumexp error {err:.2e} -> lse bound {tol_l:.2e}")
    return dict(qkv=qd, d_o=gd, o=o_r, lse=l_r, g=g_r, tol_l=tol_l)


cached_case = functools.lru_cache(maxsize=None)(build_case)


def get_case(tag, B, T, H, dt):
    """The cases several tests use (neg / spike_last on a few items) are built once, shared and never written to."""
    return (cached_case if tag in ("neg", "spike_last") and B * H <= 4 else build_case)(tag, B, T, H, dt)


def ident(v):
    return NAME.get(v, str(v))


def err(a, r):
    return amax(a.double().to(r.device) - r)


def check_fwd(c, o, lse, dt, what):
    e_o, e_l = err(o, c["o"]), err(lse, c["lse"])
    b_o = TOL_O[dt] * max(1.0, amax(c["o"]))
    print(f"{what}: o {e_o:.2e} (bound {b_o:.1e}) lse {e_l:.2e} (bound {c['tol_l']:.1e})")
    assert torch.isfinite(o).all() and torch.isfinite(lse).all(), what
    assert e_o < b_o, (what, "o", e_o)
    assert e_l < c["tol_l"], (what, "lse", e_l)


def check_parts(got, ref, tol, what, names=("dq", "dk", "dv")):
    """got / ref [rows, len(names) * inner]: every part within tol * max(1, max|its reference|)."""
    assert torch.isfinite(got).all(), what
    g, r = got.view(got.shape[0], len(names), -1), ref.view(ref.shape[0], len(names), -1)
    for i, n in enumerate(names):
        e, b = err(g[:, i], r[:, i]), tol * max(1.0, amax(r[:, i]))
        print(f"{what}: {n} {e:.2e} (bound {b:.1e})")
        assert e < b, (what, n, e)


def run_dense(ops, c, B, T, H, dt, what, layout=0):
    qin = P.to_head_major(c["qkv"], B, T, H) if layout else c["qkv"]
    o, lse = ops.attention_fwd(qin, B, T, H, SCALE, layout=layout)
    check_fwd(c, o, lse, dt, what)
    dqkv = ops.attention_bwd(qin, o, c["d_o"], lse, B, T, H, SCALE, layout=layout)
    check_parts(dqkv, c["g"], TOL_G[dt], what)
    return o, lse, dqkv


def run_both_layouts(ops, c, B, T, H, dt, what):
    a = run_dense(ops, c, B, T, H, dt, what)
    if dt != F32:      # head-major input (a 16-bit layout): against the reference, and bit-identical to the token-major run
        b = run_dense(ops, c, B, T, H, dt, what + " head-major", layout=1)
        for x, y, n in zip(a, b, ("o", "lse", "dqkv")):
            assert torch.equal(x, y), (what, "head-major input differs in", n)
    return a


# ---------------------------------------------------------------------------------------------------------------- few items: every probe
T_NKT4 = [2, 3, 15, 16, 17, 31, 32, 33, 48, 49, 63, 64]                                  # attn_fwd_bf16_kernel<4>, dq<4> + dkv<4, 2>
T_NKT14 = [65, 80, 81, 128, 129, 177, 192, 193, 207, 208, 209, 223, 224]                 # <14, 1024> forward, fused backward 1024 (FAST: 193 ... 208)
T_F32 = [2, 3, 16, 17, 63, 64, 65, 193, 224]                                             # f32 <64> / <224>
T_LONG = [225, 256, 257, 289]                                                            # panel kernels; 257: one key in the last 64-key panel
FEW = ([(B, H, T, dt) for B, H in ((2, 2), (3, 1)) for T in T_NKT4 + T_NKT14 for dt in H16]
       + [(2, 2, T, F32) for T in T_F32]
       + [(B, H, T, dt) for B, H in ((2, 1), (1, 2)) for T in T_LONG for dt in (F32, BF16, F16)])


@pytest.mark.parametrize("B,H,T,dt,tag", [(*f, tag) for f in FEW for tag in P.PROBES if not (tag.startswith("spike_tile") and f[2] <= 16)],
                         ids=ident)      # (spike_tile*: the first key of the last 16-key tile and its neighbour need a second tile)
def test_probes_with_fewer_items_than_cus(ops, B, H, T, dt, tag):
    """B * H < CUs: the T <= 64 kernels, the sixteen-wave forward and fused backward (with and without the compile-time tail mask), the
    f32 kernels and the panel kernels above 224 tokens, each on every probe, forward and backward, both input layouts."""
    assert B * H < ncu()
    run_both_layouts(ops, get_case(tag, B, T, H, dt), B, T, H, dt, f"{tag} {NAME[dt]} B={B} H={H} T={T}")


# ---------------------------------------------------------------------------------------------------------------- many items
BATCH = {"cus/8": lambda n: n // 8, "cus/8+1": lambda n: n // 8 + 1, "cus/4+1": lambda n: n // 4 + 1, "cus+8": lambda n: n + 8}
MANY = ([(b, T) for b in ("cus/8", "cus/8+1") for T in (65, 193, 208, 209, 224)]       # 512-thread forward and fused backward; item_remap on / off
        + [("cus/4+1", T) for T in (65, 192, 193, 208)]                                 # persistent forward <14, false / true>, ragged last round
        + [("cus+8", T) for T in (193, 208)])                                           # merged backward


@pytest.mark.parametrize("tag", ["neg", "spike_last", "uniform"])
@pytest.mark.parametrize("dt", H16, ids=NAME.get)
@pytest.mark.parametrize("batch,T", MANY)
def test_probes_with_more_items_than_cus(ops, batch, T, dt, tag):
    """H = 8 and B a function of the CU count, so that B * H lands in [CUs, 2 CUs) (one 512-thread workgroup per item; B a multiple of 8
    or not: the XCD item remap of the backward), in [2 CUs, 8 CUs) (persistent forward with a ragged last round) and above 8 CUs (merged
    backward). The float64 reference runs on the device; every item is compared."""
    H, B = 8, BATCH[batch](ncu())
    items = B * H
    assert {"cus/8": ncu() <= items < 2 * ncu(), "cus/8+1": ncu() <= items < 2 * ncu(), "cus/4+1": 2 * ncu() <= items < 8 * ncu(),
            "cus+8": items >= 8 * ncu()}[batch]
    run_both_layouts(ops, get_case(tag, B, T, H, dt), B, T, H, dt, f"{tag} {NAME[dt]} B={B} H={H} T={T}")


# ---------------------------------------------------------------------------------------------------------------- cls kernels
T_CLS = [2, 3, 64, 65, 255, 256, 257]      # the cls forward switches kernels at 256 / 257


def cls_inputs(qkv, B, T, H, layout):
    inner = H * 64
    if layout == 2:
        return qkv[:, inner:].contiguous(), qkv.view(B, T, 3 * inner)[:, 0, :inner].contiguous()
    return (P.to_head_major(qkv, B, T, H) if layout else qkv), None


def cls_full(got, B, T, H, layout, dt):
    """The cls backward's result as a dqkv [B*T, 3*H*64] (layout 2 returns dkv and dq_cls)."""
    if layout != 2:
        return got
    dkv, dq = got
    full = torch.cat([torch.zeros(B * T, H * 64, device="cuda", dtype=dt), dkv], 1)
    full.view(B, T, -1)[:, 0, :H * 64] = dq
    return full


@functools.lru_cache(maxsize=None)
def cls_case(tag, B, T, H, dt):
    """float64 row 0 of the forward and the backward under an output gradient that is zero off the cls row."""
    qkv, d_o = (t.to(dt) for t in P.make(tag, B, T, H))
    d_full = torch.zeros_like(d_o)
    d_full.view(B, T, -1)[:, 0] = d_o.view(B, T, -1)[:, 0]
    o_r, l_r, g_r = P.reference(qkv.float(), d_full.float(), B, T, H, SCALE)
    return dict(qkv=qkv.cuda(), d_cls=d_o.view(B, T, -1)[:, 0].contiguous().cuda(), d_full=d_full.cuda(),
                o=o_r.view(B, T, -1)[:, 0], lse=l_r[:, :, 0], g=g_r)


CLS_FORMS = [(F32, 0), (F32, 2), (BF16, 0), (BF16, 1), (BF16, 2), (F16, 0), (F16, 1), (F16, 2)]      # head-major qkv (1) is a 16-bit layout


@pytest.mark.parametrize("tag", ["neg", "spike_last"])
@pytest.mark.parametrize("dt,layout", CLS_FORMS, ids=ident)
@pytest.mark.parametrize("T", T_CLS)
def test_cls_kernels_on_the_probes(ops, T, dt, layout, tag):
    """The cls forward (one kernel up to 256 keys, chunks with an online max above) against float64 and row 0 of the dense forward; the cls
    backward, fed the compact and the full forward tensors, against the dense backward fed zeros off the cls row and against float64. On
    `neg` the cls query's own score row is the whole computation; on spike_last the cls query is one of the chosen ones."""
    B, H = 3, 2
    c = cls_case(tag, B, T, H, dt)
    what = f"cls {tag} {NAME[dt]} T={T} layout {layout}"
    qkv = c["qkv"]
    o_d, lse_d = ops.attention_fwd(qkv, B, T, H, SCALE)
    qin, q_cls = cls_inputs(qkv, B, T, H, layout)
    o_c, lse_c = ops.attention_fwd_cls(qin, B, T, H, SCALE, layout=layout, q_cls=q_cls)
    check_fwd(dict(c, tol_l=TOL_LSE[dt]), o_c, lse_c, dt, what)
    big = max(1.0, amax(c["o"]))
    assert amax(o_c.float() - o_d.view(B, T, -1)[:, 0].float()) < (2e-5 if dt == F32 else 3e-2) * big, what
    assert amax(lse_c - lse_d[:, :, 0]) < TOL_LSE[dt], what
    dense = ops.attention_bwd(qkv, o_d, c["d_full"], lse_d, B, T, H, SCALE)
    for o_, l_, form in ((o_c, lse_c, "compact"), (o_d, lse_d, "full")):
        got = cls_full(ops.attention_bwd_cls(qin, o_, c["d_cls"], l_, B, T, H, SCALE, layout=layout, q_cls=q_cls), B, T, H, layout, dt)
        check_parts(got, dense.double(), TOL_CLS[dt], f"{what} {form} vs dense")
        check_parts(got, c["g"], TOL_G[dt], f"{what} {form} vs float64")
        assert (got.view(B, T, 3, -1)[:, 1:, 0] == 0).all(), what


# ---------------------------------------------------------------------------------------------------------------- development-build variants
VARIANTS = {"per_item_fwd": {"GSL_ATTN_PERSISTENT": "0"}, "split_nt1": {"GSL_ATTN_BWD_SPLIT": "1", "GSL_ATTN_NT": "1"},
            "split_nt2": {"GSL_ATTN_BWD_SPLIT": "1", "GSL_ATTN_NT": "2"}, "fused_not_merged": {"GSL_ATTN_BWD_MERGED": "0"}}


@pytest.mark.parametrize("tag", ["neg", "spike_last"])
@pytest.mark.parametrize("dt", H16, ids=NAME.get)
@pytest.mark.parametrize("T", [65, 193, 208, 209])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_development_build_variants_on_the_probes(ops, monkeypatch, variant, T, dt, tag):
    """The kernels only the development build reaches (the two-kernel backward with one and two key tiles per wave) and its copies of the
    product kernels, against float64; bit-identical to the product library where the existing tests assert that: the forward (bf16), the
    two-kernel backward at its default tiling (bf16) and the fused backward."""
    from gslora_hip import _lib as L
    B, H = 2, 2
    # four items, fewer than CUs: the product library runs the sixteen-wave forms of the per-item forward and of the fused backward at all four T
    assert ops.attention_kernel(B, T, H, dt) == L.ATTN_FWD_1024 and ops.attention_kernel(B, T, H, dt, direction="bwd") == L.ATTN_BWD_FUSED_1024
    c = get_case(tag, B, T, H, dt)
    o, lse = ops.attention_fwd(c["qkv"], B, T, H, SCALE)
    dqkv = ops.attention_bwd(c["qkv"], o, c["d_o"], lse, B, T, H, SCALE)
    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, v)      # knobs of the development build only
    what = f"{variant} {tag} {NAME[dt]} T={T}"
    with L.use_dev():
        o_v, lse_v = ops.attention_fwd(c["qkv"], B, T, H, SCALE)
        check_fwd(c, o_v, lse_v, dt, what)
        dqkv_v = ops.attention_bwd(c["qkv"], o, c["d_o"], lse, B, T, H, SCALE)
        check_parts(dqkv_v, c["g"], TOL_G[dt], what)
    if dt == BF16:
        assert torch.equal(o_v, o) and torch.equal(lse_v, lse), what
    if variant == "fused_not_merged" or (dt == BF16 and variant != "split_nt2"):
        assert torch.equal(dqkv_v, dqkv), what


# ---------------------------------------------------------------------------------------------------------------- guard bands
GUARD = ([("dense", 2, 2, T, dt, lay) for T in T_NKT14 for dt in H16 for lay in (0, 1)]
         + [("dense", 2, 2, T, F32, 0) for T in T_F32]
         + [("dense", 2, 1, T, dt, lay) for T in T_LONG for dt, lay in ((F32, 0), (BF16, 0), (BF16, 1), (F16, 0), (F16, 1))]
         + [("cls", 3, 2, T, dt, lay) for T in T_CLS for dt, lay in CLS_FORMS])


@pytest.mark.parametrize("kind,B,H,T,dt,layout", GUARD, ids=ident)
def test_guard_bands(ops, kind, B, H, T, dt, layout):
    """Every tensor the kernels read sits between two bands of NaN, every tensor they write between two bands of a sentinel: the results
    must be finite and within tolerance (a read past an item that feeds a 0 * x product shows once x is NaN), the sentinel bands
    untouched (a store past row T-1 of the last item, or in front of item 0) and the inputs unchanged. Everything stays inside live
    allocations."""
    from gslora_hip import _lib as L
    lib, code, st = L.load(), ops.code(dt), ops._stream()
    inner = H * 64
    what = f"guard {kind} {NAME[dt]} B={B} H={H} T={T} layout {layout}"
    if kind == "dense":
        c = get_case("neg", B, T, H, dt)
        qkv = Banded((B * T, 3 * inner), dt, P.to_head_major(c["qkv"], B, T, H) if layout else c["qkv"])
        o, lse = Banded((B * T, inner), dt), Banded((B, H, T), F32)
        L.check(lib.gsl_attention_fwd(ptr(qkv), ptr(o), ptr(lse), B, T, H, SCALE, code, layout, st), "gsl_attention_fwd")
        torch.cuda.synchronize()
        check_fwd(c, o.view, lse.view, dt, what)
        o_in, lse_in, g = Banded((B * T, inner), dt, o.view), Banded((B, H, T), F32, lse.view), Banded((B * T, inner), dt, c["d_o"])
        dqkv, delta = Banded((B * T, 3 * inner), dt), Banded((B, H, T), F32)
        L.check(lib.gsl_attention_bwd(ptr(qkv), ptr(o_in), ptr(g), ptr(lse_in), ptr(dqkv), ptr(delta), B, T, H, SCALE, code, layout, st),
                "gsl_attention_bwd")
        torch.cuda.synchronize()
        check_parts(dqkv.view, c["g"], TOL_G[dt], what)
        tensors = dict(qkv=qkv, o=o, lse=lse, o_in=o_in, lse_in=lse_in, d_o=g, dqkv=dqkv, delta=delta)
    else:
        c = cls_case("neg", B, T, H, dt)
        qin, q_cls = cls_inputs(c["qkv"], B, T, H, layout)
        qkv = Banded(tuple(qin.shape), dt, qin)
        qc = Banded((B, inner), dt, q_cls) if layout == 2 else None
        o, lse = Banded((B, inner), dt), Banded((B, H), F32)
        L.check(lib.gsl_attention_fwd_cls(ptr(qkv), ptr(qc), ptr(o), ptr(lse), B, T, H, SCALE, code, layout, st), "gsl_attention_fwd_cls")
        torch.cuda.synchronize()
        check_fwd(dict(c, tol_l=TOL_LSE[dt]), o.view, lse.view, dt, what)
        o_in, lse_in, g = Banded((B, inner), dt, o.view), Banded((B, H), F32, lse.view), Banded((B, inner), dt, c["d_cls"])
        dqkv = Banded(tuple(qin.shape), dt)
        dq = Banded((B, inner), dt) if layout == 2 else None
        L.check(lib.gsl_attention_bwd_cls(ptr(qkv), ptr(qc), ptr(o_in), ptr(g), ptr(lse_in), ptr(dqkv), ptr(dq), B, T, H, SCALE, code, layout,
                                          1, st), "gsl_attention_bwd_cls")
        torch.cuda.synchronize()
        got = cls_full((dqkv.view, dq.view) if layout == 2 else dqkv.view, B, T, H, layout, dt)
        check_parts(got, c["g"], TOL_G[dt], what)
        tensors = dict(qkv=qkv, o=o, lse=lse, o_in=o_in, lse_in=lse_in, d_o=g, dqkv=dqkv)
        if layout == 2:
            tensors.update(q_cls=qc, dq_cls=dq)
    for name, b in tensors.items():
        assert b.bands_intact(), (what, "bands of", name)
