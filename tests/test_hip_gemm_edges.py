"""The GEMM family (csrc/gemm.hip, gsl_lora_grad) at the edges of its kernels: the exact-integer probes of oracle/gemm_probes.py (a dropped
K tile, a row too many in a reduction, a store four columns off each change a compared element or a band:
tests/test_gemm_probes_host.py) at the smallest shapes that reach every kernel of the tile rule — each row asserts the tile
gsl_gemm_tile_choice names —, with N off every multiple of 8 and 64, operands and outputs as column blocks and row slices of larger
tensors, and guard bands (tests/guard_bands.py) around everything a kernel reads or writes.

Placements of every row: `contiguous` between bands; `padded` — A a column block (lda = K + 64), W the second column block of a matrix
twice as wide (ldw = 2 K), out / res / aux / out2 at column offset 8 of rows of N + 40 elements (rounded up to a multiple of 8 where the
entry asks for ldo % 8 == 0), once more with res aliased to out; `cls_rows` — out / res rows 7 N apart (8 N where ldo % 8 == 0 is required
and 7 N is not), the rows between them sentinel.

No tolerance of its own: the exact epilogues are compared with torch.equal against the float64 integer reference; the inexact ones (BIAS_GELU,
BIAS_GELU_G8 and its code tensor, MUL_G8, STORE_LN, STORE_QKV_HM_LN) must be bit-identical to the plain contiguous call of the same shape, which
tests/test_hip_ops.py holds to the reference. Every band must be intact and every input unchanged.

Findings this file was written against: ops.gemm_nt took any contiguous aux / out2 next to a row-sliced out although the kernels index both
with out's leading dimension (now refused, and strided ones accepted: test_aux_and_out2_share_the_row_stride_of_out); gsl_gemm_nt and
gsl_gemm_nt_lora did not check lda >= K, ldw >= K, ldo >= N (test_leading_dimensions_below_the_row_length_are_refused)."""
import functools

import pytest
import torch

from guard_bands import Banded
from oracle import gemm_probes as G

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
SEED, SITE = 77, 5
PLACEMENTS = ("contiguous", "padded", "cls_rows")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    from gslora_hip import ops as _ops
    from gslora_hip import _lib
    _lib.load()
    return _ops


def ident(v):
    return NAME.get(v, str(v))


@functools.lru_cache(maxsize=2)
def device_case(name):
    """A table row on the device: the float32 operands, the float64 accumulator and the dropout mask of (SEED, SITE) — built once,
    shared by every test of the row, never written to."""
    from gslora_hip import ops as _ops
    case = G.BY_NAME[name]
    d = {k: v.cuda() for k, v in G.make(case).items()}
    if case.kind == "lgrad":
        return case, d, None, None
    acc = G.accumulate(d) if case.kind == "gemm" else G.accumulate_lora(d)
    keep = _ops.dropout_mask(case.M * case.N, G.P_DROP, SEED, SITE, "cuda").reshape(case.M, case.N)
    return case, d, acc, keep


def same(got, ref, what):
    g = got.double()
    if not torch.equal(g, ref):
        bad = (g != ref).nonzero()
        i = tuple(bad[0].tolist())
        pytest.fail(f"{what}: {len(bad)} of {ref.numel()} elements differ, first at {i}: got {g[i].item()}, want {ref[i].item()}")


def intact(tensors, what):
    for n, b in tensors.items():
        if b is not None:
            assert b.bands_intact(), (what, "bands of" if not b.is_input else "input changed or bands of", n)


def up(x, m):
    return -(-x // m) * m


def out_kw(placement, N, ldo8):
    """Placement of out / res / aux / out2. ldo8: the entry asks for ldo % 8 == 0 (the 16-bit stream epilogues, mulgrad)."""
    if placement == "contiguous":      # (where the entry asks for ldo % 8 == 0 and N % 8 == 4: rows of N + 4, the closest a tensor of the entry's gets)
        return dict(ld=up(N, 8)) if ldo8 and N % 8 else {}
    if placement == "padded":
        return dict(ld=up(N + 40, 8 if ldo8 else 4), col0=8, pad_rows=2)
    return dict(ld=(8 if ldo8 and (7 * N) % 8 else 7) * N)


def place_in(src, dt, placement, kind):
    """An input operand. padded: A-like tensors are a column block at offset 32 of rows K + 64 long, W-like ones the second column block
    of rows 2 K long; both with two rows of NaN behind the last one."""
    if src is None:
        return None
    src = src.to(dt)
    K = src.shape[1]
    if placement != "padded" or kind is None:
        return Banded(src.shape, dt, src)
    if kind == "A":
        return Banded(src.shape, dt, src, ld=K + 64, col0=32, pad_rows=2)
    return Banded(src.shape, dt, src, ld=2 * K, col0=K, pad_rows=2)


def v(b):
    return None if b is None else b.view


def tile_of(L, case, dt, mode):
    if dt == F32:
        return getattr(L, "TILE_" + ("F32X3_MFMA" if mode == "x3" and case.tile == "F32_MFMA" else case.tile))
    return getattr(L, "TILE_" + ("RING64" if case.f32 else case.tile))      # the two f32 rows are 64x64-ring shapes in the 16-bit modes


# ---------------------------------------------------------------------------------------------------------------- gsl_gemm_nt
GEMM_ROWS = [c for c in G.TABLE if c.kind == "gemm"]
GEMM_PARAMS = ([(c.name, dt, None) for c in GEMM_ROWS for dt in (BF16, F16)]
               + [(c.name, F32, mode) for c in GEMM_ROWS if c.f32 for mode in (None, "x3")])


def stream_epi(L, dt, what):
    return {("bias_res", BF16): L.EPI_BIAS_RES_BF16, ("bias_res", F16): L.EPI_BIAS_RES_F16,
            ("patch", BF16): L.EPI_PATCH_BF16, ("patch", F16): L.EPI_PATCH_F16}[(what, dt)]


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("name,dt,mode", GEMM_PARAMS, ids=ident)
def test_gemm_nt_table(ops, name, dt, mode, placement):
    from gslora_hip import _lib as L
    case, d, acc, keep = device_case(name)
    M, N, K1, K2 = case.M, case.N, case.K1, case.K2
    what = f"{name} {NAME[dt]}{'x3' if mode else ''} {placement}"
    tile = ops.gemm_tile_choice(M, N, K1 + K2, dt, f32_mode=mode)
    print(f"{what}: tile {tile}")
    assert tile == tile_of(L, case, dt, mode), (what, "the tile rule moved: this row no longer runs the kernel it is named for")
    h16 = dt != F32
    A1, W1 = place_in(d["A1"], dt, placement, "A"), place_in(d["W1"], dt, placement, "W")
    A2, W2 = place_in(d.get("A2"), dt, placement, "A"), place_in(d.get("W2"), dt, placement, "W")
    bias, pos, cls = (Banded(d[k].shape, F32, d[k]) for k in ("bias", "pos", "cls"))
    inputs = dict(A1=A1, W1=W1, A2=A2, W2=W2, bias=bias, pos=pos, cls=cls)
    plain = dict(A1=d["A1"].to(dt), W1=d["W1"].to(dt), A2=None if not K2 else d["A2"].to(dt), W2=None if not K2 else d["W2"].to(dt))

    def call(out, epi, ops_in=None, **kw):
        o = ops_in or dict(A1=v(A1), W1=v(W1), A2=v(A2), W2=v(W2))
        ops.gemm_nt(o["A1"], o["W1"], out, epilogue=epi, A2=o["A2"], W2=o["W2"], f32_mode=mode, **kw)
        torch.cuda.synchronize()

    def exact(tag, epi, odt, ldo8=False, res_dt=None, aux=False, alias=False, **kw):
        okw = out_kw(placement, N, ldo8) if tag != "qkv_hm" else {}      # (STORE_QKV_HM: ldo == N)
        out = Banded((M, N), odt, **okw)
        extra = {}
        if res_dt is not None:
            if alias:
                out.view.copy_(d["res"].to(res_dt))
                kw["res"] = out.view
            else:
                extra["res"] = Banded((M, N), res_dt, d["res"].to(res_dt), **okw)
                kw["res"] = extra["res"].view
        if aux:
            extra["aux"] = Banded((M, N), dt, d["aux"].to(dt), **okw)
            kw["aux"] = extra["aux"].view
        call(out.view, epi, **kw)
        w = f"{what} {tag}{' res aliased to out' if alias else ''}"
        same(out.view, G.epilogue(tag, acc, d, keep if tag.endswith("_drop") else None), w)
        intact(dict(out=out, **extra), w)

    drop = dict(p_drop=G.P_DROP, seed=SEED, site=SITE)
    fb, fpc = dict(bias=bias.view), dict(bias=bias.view, pos=pos.view, cls=cls.view, T=G.PATCH_T)
    exact("store", L.EPI_STORE, dt, alpha=G.ALPHA)
    exact("store_f32", L.EPI_STORE_F32, F32, alpha=G.ALPHA)
    exact("mul", L.EPI_MUL, dt, aux=True, alpha=G.ALPHA)
    exact("patch", L.EPI_PATCH, F32, **fpc)
    for alias in ((False, True) if placement == "padded" else (False,)):
        exact("bias_res_f32", L.EPI_BIAS_RES_F32, F32, res_dt=F32, alias=alias, **fb)
        exact("bias_res_f32_drop", L.EPI_BIAS_RES_F32, F32, res_dt=F32, alias=alias, **fb, **drop)
        if h16:
            exact("bias_res_16", stream_epi(L, dt, "bias_res"), dt, ldo8=True, res_dt=dt, alias=alias, **fb)
            exact("bias_res_16_drop", stream_epi(L, dt, "bias_res"), dt, ldo8=True, res_dt=dt, alias=alias, **fb, **drop)
    if h16:
        exact("patch_16", stream_epi(L, dt, "patch"), dt, ldo8=True, **fpc)
        if N % 192 == 0 and M % G.PATCH_T == 0:
            exact("qkv_hm", L.EPI_STORE_QKV_HM, dt, alpha=G.ALPHA, T=G.PATCH_T)

    # ---- the inexact epilogues: bit-identical to the plain contiguous call of the same shape
    def pair(tag, epi, odt, second=None, qkv=False, **kw):
        """Runs the placed call and the plain one; `second`: dtype of an out2 placed like out."""
        okw = {} if qkv else out_kw(placement, N, False)
        out, ref = Banded((M, N), odt, **okw), torch.empty(M, N, device="cuda", dtype=odt)
        out2 = ref2 = None
        if second is not None:
            out2, ref2 = Banded((M, N), second, **okw), torch.empty(M, N, device="cuda", dtype=second)
        call(out.view, epi, out2=v(out2), **kw)
        call(ref, epi, ops_in=plain, out2=ref2, **kw)
        w = f"{what} {tag}"
        assert torch.equal(out.view, ref), (w, "differs from the contiguous call")
        if second is not None:
            assert torch.equal(out2.view, ref2), (w, "out2 differs from the contiguous call")
        intact(dict(out=out, out2=out2), w)
        return ref, ref2

    pair("bias_gelu", L.EPI_BIAS_GELU, dt, second=dt, **fb, **drop)
    mean = Banded((M,), F32, (torch.arange(M, device="cuda") % 7 - 3).float() / 8)
    rstd = Banded((M,), F32, 2.0 ** (torch.arange(M, device="cuda") % 3 - 1).float())
    c_n = Banded((N,), F32, (torch.arange(N, device="cuda") % 5 - 2).float())
    inputs.update(mean=mean, rstd=rstd, c=c_n)
    ln = dict(pos=mean.view, cls=rstd.view, aux=c_n.view, bias=bias.view)
    pair("store_ln", L.EPI_STORE_LN, dt, **ln)
    if h16 and N % 192 == 0 and M % G.PATCH_T == 0:
        pair("qkv_hm_ln", L.EPI_STORE_QKV_HM_LN, dt, qkv=True, T=G.PATCH_T, **ln)
    if h16 and N % 64 == 0:      # the 8-bit GELU' code tensor is slab-major and contiguous whatever ldo is: between bands
        okw = out_kw(placement, N, False)
        h, q = Banded((M, N), dt, **okw), Banded((M, N), torch.uint8)
        h0, q0 = torch.empty(M, N, device="cuda", dtype=dt), torch.empty(M, N, device="cuda", dtype=torch.uint8)
        call(h.view, L.EPI_BIAS_GELU_G8, out2=q.view, **fb, **drop)
        call(h0, L.EPI_BIAS_GELU_G8, ops_in=plain, out2=q0, **fb, **drop)
        assert torch.equal(h.view, h0) and torch.equal(q.view, q0), (what, "bias_gelu_g8 differs from the contiguous call")
        codes = Banded((M, N), torch.uint8, q0)
        o, o0 = Banded((M, N), dt, **okw), torch.empty(M, N, device="cuda", dtype=dt)
        call(o.view, L.EPI_MUL_G8, aux=codes.view, p_drop=G.P_DROP)
        call(o0, L.EPI_MUL_G8, ops_in=plain, aux=q0, p_drop=G.P_DROP)
        assert torch.equal(o.view, o0), (what, "mul_g8 differs from the contiguous call")
        intact(dict(h=h, q=q, codes=codes, o=o), what + " g8")
    intact(inputs, what)


# ---------------------------------------------------------------------------------------------------------------- gsl_gemm_nt_lora
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("dt", [BF16, F16], ids=ident)
@pytest.mark.parametrize("name", [c.name for c in G.TABLE if c.kind == "lora"])
def test_gemm_nt_lora_table(ops, name, dt, placement):
    from gslora_hip import _lib as L
    case, d, acc, keep = device_case(name)
    M, N, K = case.M, case.N, case.K1
    what = f"{name} {NAME[dt]} {placement}"
    tile = ops.gemm_tile_choice(M, N, K, dt, in_kernel_lora=True)
    print(f"{what}: tile {tile}")
    assert tile == getattr(L, "TILE_" + case.tile), (what, "the tile rule moved: this row no longer runs the kernel it is named for")
    A, W = place_in(d["A1"], dt, placement, "A"), place_in(d["W1"], dt, placement, "W")
    P, Q, bias = place_in(d["P"], dt, placement, None), place_in(d["Q"], dt, placement, None), Banded(d["bias"].shape, F32, d["bias"])
    t_ref = G.tout(d)

    def call(out, epi, tout, A_=None, W_=None, **kw):
        ops.gemm_nt_lora(v(A) if A_ is None else A_, v(W) if W_ is None else W_, P.view, Q.view, G.LORA_SCALE, tout, out, epilogue=epi, **kw)
        torch.cuda.synchronize()

    def exact(tag, epi, odt, ldo8=False, res_dt=None, aux=False, alias=False, **kw):
        okw = out_kw(placement, N, ldo8)
        out, tout = Banded((M, N), odt, **okw), Banded((M, 64), dt)
        extra = {}
        if res_dt is not None:
            if alias:
                out.view.copy_(d["res"].to(res_dt))
                kw["res"] = out.view
            else:
                extra["res"] = Banded((M, N), res_dt, d["res"].to(res_dt), **okw)
                kw["res"] = extra["res"].view
        if aux:
            extra["aux"] = Banded((M, N), dt, d["aux"].to(dt), **okw)
            kw["aux"] = extra["aux"].view
        call(out.view, epi, tout.view, **kw)
        w = f"{what} {tag}{' res aliased to out' if alias else ''}"
        same(out.view, G.epilogue_lora(tag, acc, d, keep if tag.endswith("_drop") else None), w)
        same(tout.view, t_ref, w + " tout")
        intact(dict(out=out, tout=tout, **extra), w)

    drop = dict(p_drop=G.P_DROP, seed=SEED, site=SITE)
    exact("store", L.EPI_STORE, dt)
    exact("mul", L.EPI_MUL, dt, aux=True)
    epi16 = L.EPI_BIAS_RES_BF16 if dt == BF16 else L.EPI_BIAS_RES_F16
    for alias in ((False, True) if placement == "padded" else (False,)):
        exact("bias_res_f32", L.EPI_BIAS_RES_F32, F32, res_dt=F32, alias=alias, bias=bias.view)
        exact("bias_res_16", epi16, dt, ldo8=True, res_dt=dt, alias=alias, bias=bias.view)
        exact("bias_res_16_drop", epi16, dt, ldo8=True, res_dt=dt, alias=alias, bias=bias.view, **drop)
    # BIAS_GELU: both outputs bit-identical to the plain contiguous call
    okw = out_kw(placement, N, False)
    out, out2, tout = Banded((M, N), dt, **okw), Banded((M, N), dt, **okw), Banded((M, 64), dt)
    ref, ref2 = torch.empty(M, N, device="cuda", dtype=dt), torch.empty(M, N, device="cuda", dtype=dt)
    call(out.view, L.EPI_BIAS_GELU, tout.view, out2=out2.view, bias=bias.view, **drop)
    call(ref, L.EPI_BIAS_GELU, None, A_=d["A1"].to(dt), W_=d["W1"].to(dt), out2=ref2, bias=bias.view, **drop)
    assert torch.equal(out.view, ref) and torch.equal(out2.view, ref2), (what, "bias_gelu differs from the contiguous call")
    same(tout.view, t_ref, what + " bias_gelu tout")
    intact(dict(out=out, out2=out2, tout=tout, A=A, W=W, P=P, Q=Q, bias=bias), what)


# ---------------------------------------------------------------------------------------------------------------- gsl_gemm_nt_lora_mulgrad
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("dt", [BF16, F16], ids=ident)
@pytest.mark.parametrize("name", [c.name for c in G.TABLE if c.kind == "mulgrad"])
def test_mulgrad_table(ops, name, dt, placement):
    """out, tout and the two fused reductions. G1 / G2 are views into gradient buckets with strides of their own: [N, r] rows 16 apart
    (padded) and [r, N]; both accumulate onto integers. U1 is the 16-column block at offset 16 of a 64-wide tensor in `padded`."""
    case, d, acc, _ = device_case(name)
    M, N, K, r = case.M, case.N, case.K1, case.r
    what = f"{name} {NAME[dt]} {placement}"
    okw = out_kw(placement, N, True)
    A, W = place_in(d["A1"], dt, placement, "A"), place_in(d["W1"], dt, placement, "W")
    P, Q = place_in(d["P"], dt, placement, None), place_in(d["Q"], dt, placement, None)
    aux, Y2 = Banded((M, N), dt, d["aux"].to(dt), **okw), Banded((M, N), dt, d["Y2"].to(dt), **okw)
    U1 = Banded((M, 16), dt, d["U1"].to(dt), **(dict(ld=64, col0=16, pad_rows=2) if placement == "padded" else {}))
    G1 = Banded((N, r), F32, d["G1_0"], **(dict(ld=16) if placement == "padded" else {}))
    G2 = Banded((r, N), F32, d["G2_0"].t())
    out, tout = Banded((M, N), dt, **okw), Banded((M, 64), dt)
    ops.gemm_nt_lora_mulgrad(A.view, W.view, P.view, Q.view, G.LORA_SCALE, tout.view, out.view, aux.view, U1.view, G1.view,
                             (G1.view.stride(0), 1), Y2.view, G2.view, (1, N), r, accumulate=True)
    torch.cuda.synchronize()
    o_ref, g1_ref, g2_ref = G.mulgrad(d, r)
    same(out.view, o_ref, what + " out")
    same(tout.view, G.tout(d), what + " tout")
    same(G1.view, g1_ref, what + " G1")
    same(G2.view.t(), g2_ref, what + " G2")
    intact(dict(out=out, tout=tout, A=A, W=W, P=P, Q=Q, aux=aux, Y2=Y2, U1=U1), what)
    assert G1.outside_intact() and G2.outside_intact(), (what, "a gradient store outside its view")


@pytest.mark.parametrize("dt", [BF16, F16], ids=ident)
def test_mulgrad_with_the_8bit_code_tensor_beside_a_padded_out(ops, dt):
    """aux_u8: aux is the slab-major code tensor of BIAS_GELU_G8 (N % 64 == 0), contiguous whatever ldo is. A padded out / Y2 with padded
    operands beside a contiguous code tensor: out, tout, G1 and G2 bit-identical to the all-contiguous call (which tests/test_hip_ops.py
    holds to the unfused form); the decoded multiplier is not an integer, so no exact reference here."""
    case = G.Case("mulgrad_u8", "mulgrad", 300, 320, 64, 0, 5, None, False)
    M, N, r = case.M, case.N, case.r
    d = {k: t.cuda() for k, t in G.make(case).items()}
    codes = torch.randint(0, 253, (M, N), generator=torch.Generator().manual_seed(11), dtype=torch.uint8).cuda()
    res = {}
    for placement in ("contiguous", "padded"):
        okw = out_kw(placement, N, True)
        A, W = place_in(d["A1"], dt, placement, "A"), place_in(d["W1"], dt, placement, "W")
        P, Q = place_in(d["P"], dt, placement, None), place_in(d["Q"], dt, placement, None)
        aux, Y2 = Banded((M, N), torch.uint8, codes), Banded((M, N), dt, d["Y2"].to(dt), **okw)
        U1 = Banded((M, 16), dt, d["U1"].to(dt), **(dict(ld=64, col0=16, pad_rows=2) if placement == "padded" else {}))
        G1, G2 = Banded((N, r), F32, d["G1_0"]), Banded((r, N), F32, d["G2_0"].t())
        out, tout = Banded((M, N), dt, **okw), Banded((M, 64), dt)
        ops.gemm_nt_lora_mulgrad(A.view, W.view, P.view, Q.view, G.LORA_SCALE, tout.view, out.view, aux.view, U1.view, G1.view, (r, 1),
                                 Y2.view, G2.view, (1, N), r, accumulate=True, p_drop=G.P_DROP)
        torch.cuda.synchronize()
        intact(dict(out=out, tout=tout, A=A, W=W, P=P, Q=Q, aux=aux, Y2=Y2, U1=U1), f"mulgrad u8 {NAME[dt]} {placement}")
        assert G1.outside_intact() and G2.outside_intact()
        assert out.unwritten() == 0 and torch.isfinite(out.view.float()).all()
        res[placement] = [t.view.clone() for t in (out, tout, G1, G2)]
    same(res["contiguous"][1], G.tout(d), "mulgrad u8 tout")
    for a, b, n in zip(res["contiguous"], res["padded"], ("out", "tout", "G1", "G2")):
        assert torch.equal(a, b), (NAME[dt], n, "padded call differs from the contiguous call")


# ---------------------------------------------------------------------------------------------------------------- gsl_lora_grad
LGRAD_PARAMS = [("lgrad_n132", F32), ("lgrad_n136", BF16), ("lgrad_n136", F16), ("lgrad_n136", F32),
                ("lgrad_n768", BF16), ("lgrad_n768", F16), ("lgrad_n768", F32)]


@pytest.mark.parametrize("placement", ("contiguous", "padded"))
@pytest.mark.parametrize("name,dt", LGRAD_PARAMS, ids=ident)
def test_lora_grad_table(ops, name, dt, placement):
    """Y a column block (padded), U at column offsets 0, r and 2 r of a 64-wide tensor, as the runner passes them; G accumulates onto
    integers, as [N, r] and as [r, N]."""
    case, d, _, _ = device_case(name)
    M, N, r = case.M, case.N, case.r
    what = f"{name} {NAME[dt]} {placement}"
    Y = Banded((M, N), dt, d["Y"].to(dt), **(dict(ld=N + 64, col0=32, pad_rows=2) if placement == "padded" else {}))
    U = Banded((M, 64), dt, d["U"].to(dt))
    for col in (0, r, 2 * r):
        ref = G.lora_grad(d, r, col)
        Ga, Gb = Banded((N, r), F32, d["G0"]), Banded((r, N), F32, d["G0"].t())
        ops.lora_grad(Y.view, U.view[:, col:], Ga.view, r, 1, r, accumulate=True)
        ops.lora_grad(Y.view, U.view[:, col:], Gb.view, 1, N, r, accumulate=True)
        torch.cuda.synchronize()
        same(Ga.view, ref, f"{what} U column {col} G [N, r]")
        same(Gb.view.t(), ref, f"{what} U column {col} G [r, N]")
        assert Ga.outside_intact() and Gb.outside_intact(), (what, "a gradient store outside its view")
    intact(dict(Y=Y, U=U), what)


@pytest.mark.parametrize("dt", [BF16, F16], ids=ident)
def test_lora_grad_batch_equals_the_single_launches(ops, dt):
    """A 256-column and a 768-column entry in one gsl_lora_grad_batch call: bit-identical to gsl_lora_grad on each, and exact."""
    entries, singles, keepers = [], [], []
    for e in G.make_lgrad_batch():
        r, (M, N) = e["r"], e["Y"].shape
        Y, U = Banded((M, N), dt, e["Y"].cuda().to(dt), ld=N + 64, col0=32, pad_rows=2), Banded((M, 64), dt, e["U"].cuda().to(dt))
        Gb, Gs = Banded((N, r), F32, e["G0"].cuda()), Banded((N, r), F32, e["G0"].cuda())
        assert ops.lora_grad_batchable(Y.view, U.view[:, 16:], r)
        entries.append((Y.view, U.view[:, 16:], Gb.view, r, 1, r, True))
        ops.lora_grad(Y.view, U.view[:, 16:], Gs.view, r, 1, r, accumulate=True)
        singles.append((Gb, Gs, G.lora_grad({k: t.cuda() for k, t in e.items() if k != "r"}, r, 16)))
        keepers += [Y, U]
    ops.lora_grad_batch(entries)
    torch.cuda.synchronize()
    for i, (Gb, Gs, ref) in enumerate(singles):
        same(Gs.view, ref, f"lora_grad entry {i} {NAME[dt]}")
        assert torch.equal(Gb.view, Gs.view), (i, "the batch differs from the single launch")
        assert Gb.outside_intact() and Gs.outside_intact()
    for b in keepers:
        assert b.bands_intact()


# ---------------------------------------------------------------------------------------------------------------- forced variants
@pytest.mark.parametrize("variant", ["1", "3", "8"])
@pytest.mark.parametrize("dt", [BF16, F16], ids=ident)
@pytest.mark.parametrize("name", ["ring64_direct_store", "ring64"])
def test_forced_tile_variants_on_the_ragged_shapes(ops, dev_lib, monkeypatch, name, dt, variant):
    """The development build's GSL_GEMM_VARIANT puts the two smallest ragged shapes on the 128x128, the 256x128 ring and the 8-phase kernel:
    one ragged tile each, N % 8 == 4 (fragment stores) and N % 64 == 0 (staged stores, and the 8-bit GELU' pair), padded placement."""
    from gslora_hip import _lib as L
    case, d, acc, keep = device_case(name)
    M, N = case.M, case.N
    monkeypatch.setenv("GSL_GEMM_VARIANT", variant)      # a knob of the development build only
    dev_lib(L)
    what = f"variant {variant} {name} {NAME[dt]}"
    A1, W1 = place_in(d["A1"], dt, "padded", "A"), place_in(d["W1"], dt, "padded", "W")
    A2, W2 = place_in(d.get("A2"), dt, "padded", "A"), place_in(d.get("W2"), dt, "padded", "W")
    bias = Banded(d["bias"].shape, F32, d["bias"])
    epi16 = L.EPI_BIAS_RES_BF16 if dt == BF16 else L.EPI_BIAS_RES_F16
    for tag, epi, odt, ldo8, kw in (("store", L.EPI_STORE, dt, False, dict(alpha=G.ALPHA)),
                                    ("mul", L.EPI_MUL, dt, False, dict(alpha=G.ALPHA)),
                                    ("bias_res_f32_drop", L.EPI_BIAS_RES_F32, F32, False, dict(p_drop=G.P_DROP, seed=SEED, site=SITE)),
                                    ("bias_res_16_drop", epi16, dt, True, dict(p_drop=G.P_DROP, seed=SEED, site=SITE))):
        okw = out_kw("padded", N, ldo8)
        out, extra = Banded((M, N), odt, **okw), {}
        if tag == "mul":
            extra["aux"] = Banded((M, N), dt, d["aux"].to(dt), **okw)
            kw["aux"] = extra["aux"].view
        if tag.startswith("bias_res"):
            extra["res"] = Banded((M, N), odt, d["res"].to(odt), **okw)
            kw.update(res=extra["res"].view, bias=bias.view)
        ops.gemm_nt(A1.view, W1.view, out.view, epilogue=epi, A2=v(A2), W2=v(W2), **kw)
        torch.cuda.synchronize()
        same(out.view, G.epilogue(tag, acc, d, keep if tag.endswith("_drop") else None), f"{what} {tag}")
        intact(dict(out=out, **extra), f"{what} {tag}")
    plain = dict(A2=None if not case.K2 else d["A2"].to(dt), W2=None if not case.K2 else d["W2"].to(dt))
    if N % 64 == 0:      # BIAS_GELU_G8 / MUL_G8 on these kernels' staged paths at ragged M: bit-identical to the contiguous call under the same variant
        # (rows of N + 48: the 256x128 ring and the 8-phase kernel stage this epilogue — and take GELU from the LDS table — where N and ldo are
        #  multiples of 16, and use the fragment path with the erf form elsewhere; the contiguous call has ldo = N = 192, so the padded one
        #  keeps ldo % 16 == 0. The fragment path at ldo = N + 40 is held to BIAS_GELU below.)
        okw, drop = dict(out_kw("padded", N, False), ld=up(N + 40, 16)), dict(p_drop=G.P_DROP, seed=SEED, site=SITE)
        h, q = Banded((M, N), dt, **okw), Banded((M, N), torch.uint8)
        h0, q0 = torch.empty(M, N, device="cuda", dtype=dt), torch.empty(M, N, device="cuda", dtype=torch.uint8)
        ops.gemm_nt(A1.view, W1.view, h.view, epilogue=L.EPI_BIAS_GELU_G8, A2=v(A2), W2=v(W2), bias=bias.view, out2=q.view, **drop)
        ops.gemm_nt(d["A1"].to(dt), d["W1"].to(dt), h0, epilogue=L.EPI_BIAS_GELU_G8, bias=bias.view, out2=q0, **plain, **drop)
        codes = Banded((M, N), torch.uint8, q0)
        o, o0 = Banded((M, N), dt, **okw), torch.empty(M, N, device="cuda", dtype=dt)
        ops.gemm_nt(A1.view, W1.view, o.view, epilogue=L.EPI_MUL_G8, A2=v(A2), W2=v(W2), aux=codes.view, p_drop=G.P_DROP)
        ops.gemm_nt(d["A1"].to(dt), d["W1"].to(dt), o0, epilogue=L.EPI_MUL_G8, aux=q0, p_drop=G.P_DROP, **plain)
        torch.cuda.synchronize()
        assert torch.equal(h.view, h0) and torch.equal(q.view, q0), (what, "bias_gelu_g8 differs from the contiguous call")
        assert torch.equal(o.view, o0), (what, "mul_g8 differs from the contiguous call")
        intact(dict(h=h, q=q, codes=codes, o=o), what + " g8")
        # ldo = N + 40 (a multiple of 8, not of 16): BIAS_GELU_G8 on the fragment path, whose first output is BIAS_GELU's bit for bit
        okw = out_kw("padded", N, False)
        hf, qf, hg = Banded((M, N), dt, **okw), Banded((M, N), torch.uint8), Banded((M, N), dt, **okw)
        ops.gemm_nt(A1.view, W1.view, hf.view, epilogue=L.EPI_BIAS_GELU_G8, A2=v(A2), W2=v(W2), bias=bias.view, out2=qf.view, **drop)
        ops.gemm_nt(A1.view, W1.view, hg.view, epilogue=L.EPI_BIAS_GELU, A2=v(A2), W2=v(W2), bias=bias.view, **drop)
        torch.cuda.synchronize()
        assert torch.equal(hf.view, hg.view), (what, "bias_gelu_g8 on the fragment path differs from bias_gelu")
        assert qf.unwritten() < M * N // 100 and int(qf.view.max()) <= 252, (what, "code tensor of the fragment path")
        intact(dict(h=hf, q=qf, h_gelu=hg), what + " g8 fragment path")
    # Did the knob take effect? The development build reads GSL_GEMM_VARIANT on every launch, after the tile rule; the results above are exact on
    # every kernel, so two side effects tell the kernels apart. (a) N <= 128: the compact [M, 16] second output of STORE exists on the 256x128
    # ring kernel alone, where the rule sends such a call — forced onto variant 1 or 8 it stays unwritten, on 3 it is written. (b) N % 8 == 0:
    # GSL_STORE_MODE=3 (no output store) acts in the staged copy-out of variants 3 and 8; the 64x64 ring kernel this shape runs by default
    # stores fragments and ignores it. Each variant is told apart on one of the two shapes; (1, N = 192) and (3, N = 68) have no such mark.
    if N <= 128:
        out, out2 = Banded((M, N), dt), Banded((M, 16), dt)
        ops.gemm_nt(A1.view, W1.view, out.view, A2=v(A2), W2=v(W2), alpha=G.ALPHA, out2=out2.view)
        torch.cuda.synchronize()
        ref = G.epilogue("store", acc, d)
        same(out.view, ref, what + " store with out2")
        if variant == "3":
            same(out2.view, ref[:, :16], what + " out2")
        else:
            assert out2.unwritten() == M * 16, (what, "GSL_GEMM_VARIANT did not take effect: the ring kernel wrote out2")
        intact(dict(out=out, out2=out2), what + " out2")
    elif variant != "1":
        monkeypatch.setenv("GSL_STORE_MODE", "3")
        out = Banded((M, N), dt)
        ops.gemm_nt(A1.view, W1.view, out.view, A2=v(A2), W2=v(W2), alpha=G.ALPHA)
        torch.cuda.synchronize()
        monkeypatch.delenv("GSL_STORE_MODE")
        assert out.unwritten() == M * N and out.bands_intact(), (what, "GSL_GEMM_VARIANT did not take effect: a fragment-path kernel stored the output")
    intact(dict(A1=A1, W1=W1, A2=A2, W2=W2, bias=bias), what)


# ---------------------------------------------------------------------------------------------------------------- what the wrappers and entries refuse
def test_aux_and_out2_share_the_row_stride_of_out(ops):
    """The kernels index the aux of EPI_MUL and the out2 of EPI_BIAS_GELU with out's leading dimension. ops.gemm_nt / gemm_nt_lora pass
    strided ones through (the padded placement of the table rows) and refuse a row stride that differs from out's, as for res."""
    from gslora_hip import _lib as L
    M, N, K = 16, 64, 64
    z = lambda *s, dt=BF16: torch.zeros(*s, device="cuda", dtype=dt)
    A, W, bias = z(M, K), z(N, K), z(N, dt=F32)
    wide = z(M, 2 * N)
    for out, other in ((wide[:, :N], z(M, N)), (z(M, N), wide[:, :N])):
        with pytest.raises(RuntimeError, match="row stride"):
            ops.gemm_nt(A, W, out, epilogue=L.EPI_MUL, aux=other)
        with pytest.raises(RuntimeError, match="row stride"):
            ops.gemm_nt(A, W, out, epilogue=L.EPI_BIAS_GELU, bias=bias, out2=other)
        with pytest.raises(RuntimeError, match="row stride"):
            ops.gemm_nt(A, W, out, epilogue=L.EPI_BIAS_RES_BF16, bias=bias, res=other)
        P, Q = z(16, K), z(N, 32)
        with pytest.raises(RuntimeError, match="row stride"):
            ops.gemm_nt_lora(A, W, P, Q, 1.0, None, out, epilogue=L.EPI_MUL, aux=other)
        with pytest.raises(RuntimeError, match="row stride"):
            ops.gemm_nt_lora(A, W, P, Q, 1.0, None, out, epilogue=L.EPI_BIAS_GELU, bias=bias, out2=other)
    with pytest.raises(RuntimeError, match="contiguous"):      # the 8-bit code tensor has a layout of its own
        ops.gemm_nt(A, W, z(M, N), epilogue=L.EPI_MUL_G8, aux=z(M, 2 * N, dt=torch.uint8)[:, :N])
    # ... in the gradient-fused form too: a uint8 column block whose row stride equals a padded out's would be read slab-major
    P, Q, U1, r = z(16, K), z(N, 32), z(M, 16), 4
    G1, G2 = z(N, r, dt=F32), z(r, N, dt=F32)
    args = lambda out, aux, Y2: (A, W, P, Q, 1.0, None, out, aux, U1, G1, (r, 1), Y2, G2, (1, N), r)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.gemm_nt_lora_mulgrad(*args(z(M, 2 * N)[:, :N], z(M, 2 * N, dt=torch.uint8)[:, :N], z(M, 2 * N)[:, :N]))
    with pytest.raises(RuntimeError, match="row stride"):      # a 16-bit aux is indexed with ldo
        ops.gemm_nt_lora_mulgrad(*args(z(M, 2 * N)[:, :N], z(M, N), z(M, 2 * N)[:, :N]))
    with pytest.raises(RuntimeError, match="row stride"):
        ops.gemm_nt_lora_mulgrad(*args(z(M, N), z(M, N), z(M, 2 * N)[:, :N]))


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=ident)
def test_leading_dimensions_below_the_row_length_are_refused(ops, dt):
    """gsl_gemm_nt and gsl_gemm_nt_lora: lda < K, ldw < K, ldo < N fail with an argument error before anything is launched (aligned
    values, so only the new check can refuse them)."""
    from gslora_hip import _lib as L
    lib, code, st = L.load(), ops.code(dt), ops._stream()
    M, N, K = 16, 64, 128
    A, W, out = (torch.zeros(M * K, device="cuda", dtype=dt), torch.zeros(N * K, device="cuda", dtype=dt),
                 torch.zeros(M * N, device="cuda", dtype=dt))
    p = lambda t: t.data_ptr()

    def gemm(lda, ldw, ldo, lda2=64, ldw2=64, K2=0):
        return lib.gsl_gemm_nt(p(A), lda, p(W), ldw, K, p(A) if K2 else None, lda2, p(W) if K2 else None, ldw2, K2, M, N, code, L.EPI_STORE, 1.0,
                               None, None, None, p(out), None, ldo, None, None, 0, 0.0, 0, 0, st)

    assert gemm(K, K, N) == 0
    for bad in (dict(lda=64), dict(ldw=64), dict(ldo=32), dict(K2=64, lda2=32), dict(K2=64, ldw2=32)):
        kw = dict(dict(lda=K, ldw=K, ldo=N), **bad)
        assert gemm(**kw) != 0, bad
        assert b"argument check failed" in lib.gsl_last_error(), bad
    if dt != F32:
        P, Q = torch.zeros(16 * K, device="cuda", dtype=dt), torch.zeros(N * 32, device="cuda", dtype=dt)

        def lora(lda, ldw, ldp, ldo):
            return lib.gsl_gemm_nt_lora(p(A), lda, p(W), ldw, K, p(P), ldp, p(Q), 32, 1.0, None, 0, M, N, code, L.EPI_STORE, None, None, None,
                                        p(out), None, ldo, 0.0, 0, 0, st)

        assert lora(K, K, K, N) == 0
        for bad in (dict(lda=64), dict(ldw=64), dict(ldp=64), dict(ldo=32)):
            assert lora(**dict(dict(lda=K, ldw=K, ldp=K, ldo=N), **bad)) != 0, bad
            assert b"argument check failed" in lib.gsl_last_error(), bad
    torch.cuda.synchronize()


def test_alpha_is_refused_where_not_every_kernel_applies_it(ops):
    """gsl_gemm_nt applies alpha in the STORE, STORE_F32 and MUL epilogues on every kernel; the staged residual, patch and table-GELU epilogues of
    the 8-phase kernel drop it while their fragment forms differ among themselves. So alpha != 1 is an argument error for BIAS_RES_*, PATCH* and
    BIAS_GELU*: the call names alpha and returns before anything is launched (out keeps its sentinel), the same call with alpha = 1 runs.
    Where alpha is applied, alpha = 2 doubles the alpha = 1 result: within one rounding of the output type (a factor 2 is exact, so the bound
    is the unit roundoff of the output format times the value)."""
    from gslora_hip import _lib as L
    M = N = K = 64
    T = 8
    g = torch.Generator(device="cuda").manual_seed(SEED)
    rnd = lambda *s, dt=BF16: torch.randn(*s, device="cuda", generator=g).to(dt)
    A, W, bias, pos, cls = rnd(M, K), rnd(N, K), rnd(N, dt=F32), rnd(T, N, dt=F32), rnd(N, dt=F32)
    stream = lambda dt: dict(bias=bias, res=rnd(M, N, dt=dt))
    patch = dict(bias=bias, pos=pos, cls=cls, T=T)
    refused = (("BIAS_RES_F32", F32, stream(F32)), ("BIAS_RES_BF16", BF16, stream(BF16)), ("BIAS_RES_F16", F16, stream(F16)),
               ("PATCH", F32, patch), ("PATCH_BF16", BF16, patch), ("PATCH_F16", F16, patch),
               ("BIAS_GELU", BF16, dict(bias=bias)), ("BIAS_GELU_G8", BF16, dict(bias=bias)))
    for name, odt, kw in refused:
        out = torch.full((M, N), 7.0, device="cuda", dtype=odt)
        with pytest.raises(RuntimeError, match="alpha"):
            ops.gemm_nt(A, W, out, epilogue=getattr(L, "EPI_" + name), alpha=2.0, **kw)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), (name, "a refused call wrote to out")
        ops.gemm_nt(A, W, out, epilogue=getattr(L, "EPI_" + name), alpha=1.0, **kw)      # the operands were valid: alpha alone was refused
        torch.cuda.synchronize()
        assert not bool((out == 7.0).all()), name
    for name, odt, kw in (("STORE", BF16, {}), ("STORE_F32", F32, {}), ("MUL", BF16, dict(aux=rnd(M, N)))):
        one, two = torch.zeros(M, N, device="cuda", dtype=odt), torch.zeros(M, N, device="cuda", dtype=odt)
        ops.gemm_nt(A, W, one, epilogue=getattr(L, "EPI_" + name), alpha=1.0, **kw)
        ops.gemm_nt(A, W, two, epilogue=getattr(L, "EPI_" + name), alpha=2.0, **kw)
        torch.cuda.synchronize()
        want = 2.0 * one.double()
        assert bool((want != 0).any()), name
        err = (two.double() - want).abs()
        bound = want.abs() * (torch.finfo(odt).eps / 2)
        print(f"alpha=2 {name}: max |err| {err.max().item():.3e}, max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
        assert bool((err <= bound).all()), (name, err.max().item())
