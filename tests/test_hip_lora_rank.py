"""gsl_lora_grad / gsl_lora_grad_batch above rank 16 (csrc/lora.hip: the R = 32 and R = 64 instantiations of the MFMA form, the chunked
VALU form, the reducers), exact: the small-integer operands of oracle/gemm_probes.py make every sum exact in f32, so every comparison is
torch.equal against the float64 reference G.lora_grad. Every tensor sits in guard bands (tests/guard_bands.py).

Shapes, the smallest that reach each form (every note is what gsl_lora_grad_plan answers: tests/test_lora_grad_plan_host.py,
test_shape_notes_of_the_rank_tests):
  MFMA form (16-bit operands, N % 256 == 0, M >= 64, 16-byte aligned U): (65, 256) a last split of one row, (700, 768) 22 row splits,
  (1300, 2048) 21 splits of two slabs — all three on the single-launch reduction (N * R >= 8192 outputs from R = 32 on) —, and
  (5153, 256) 162 splits, more than the single launch takes: the two-level reduction, level-1 slabs of 32 x 5 + 2 splits (r = 17 and 64).
  VALU form: (333, 132) f32 vector width 4, (333, 136) 16-bit vector width 8, (5, 256) M < 64, (700, 768) f32 with six splits — one
  reduce launch each —, and (4225, 8) 34 splits: the chunked form in front of the two-level reduction (r = 17).
The read rule of include/gslora_hip.h: above rank 16 the aligned MFMA form reads the 8-column chunks [0, 8 * ceil(r / 8)) of U, every
other form the columns [0, r), and no result depends on a column outside [0, r): U is a column block of a 64-wide tensor whose other
columns are NaN in one variant, up to the row end."""
import functools

import pytest
import torch

from guard_bands import Banded
from oracle import gemm_probes as G

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}


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


@functools.lru_cache(maxsize=None)
def operands(M, N):
    """The operands of one (M, N) on the device, built once with a 64-column G0 and never written to: rank r uses G0[:, :r]."""
    case = G.Case(f"lgrad_rank_{M}x{N}", "lgrad", M, N, 0, 0, 64, None, True)
    return {k: v.cuda() for k, v in G.make(case).items()}


def for_rank(d, r):
    return dict(Y=d["Y"], U=d["U"], G0=d["G0"][:, :r].contiguous())


def same(got, ref, what):
    g = got.double()
    if not torch.equal(g, ref):
        bad = (g != ref).nonzero()
        i = tuple(bad[0].tolist())
        pytest.fail(f"{what}: {len(bad)} of {ref.numel()} elements differ, first at {i}: got {g[i].item()}, want {ref[i].item()}")


def run_both_layouts(ops, Y, Uview, d, r, ref, what, gscale=None):
    """G as [N, r] and as [r, N], accumulating onto integers."""
    N = d["Y"].shape[1]
    Ga, Gb = Banded((N, r), F32, d["G0"]), Banded((r, N), F32, d["G0"].t())
    ops.lora_grad(Y.view, Uview, Ga.view, r, 1, r, accumulate=True, gscale=gscale)
    ops.lora_grad(Y.view, Uview, Gb.view, 1, N, r, accumulate=True, gscale=gscale)
    torch.cuda.synchronize()
    same(Ga.view, ref, f"{what} G [N, r]")
    same(Gb.view.t(), ref, f"{what} G [r, N]")
    assert Ga.outside_intact() and Gb.outside_intact(), (what, "a gradient store outside its view")
    return Ga.view.clone()


MFMA_SHAPES = [(65, 256), (700, 768), (1300, 2048)]
MFMA_RANKS = [17, 24, 32, 33, 48, 63, 64]


@pytest.mark.parametrize("r", MFMA_RANKS)
@pytest.mark.parametrize("dt", [BF16, F16], ids=ident)
@pytest.mark.parametrize("M,N", MFMA_SHAPES)
def test_mfma_form(ops, M, N, dt, r):
    mfma_form(ops, M, N, dt, r)


@pytest.mark.parametrize("r", [17, 64])
@pytest.mark.parametrize("dt", [BF16, F16], ids=ident)
def test_mfma_form_two_level_reduce(ops, dt, r):
    """162 row splits: lora_grad_reduce1_kernel over slabs of 32 splits, then lora_grad_reduce2_kernel, at R = 32 and R = 64."""
    from gslora_hip import _lib as L
    p = ops.lora_grad_plan_args(5153, 256, r, dt)
    assert (p.form, p.reduce, p.nsplit) == (L.LGRAD_MFMA, L.LGRAD_REDUCE_TWO_LEVEL, 162)
    mfma_form(ops, 5153, 256, dt, r)


def mfma_form(ops, M, N, dt, r):
    d = for_rank(operands(M, N), r)
    what = f"mfma {M}x{N} {NAME[dt]} r={r}"
    Y, U = Banded((M, N), dt, d["Y"].to(dt)), Banded((M, 64), dt, d["U"].to(dt))
    assert ops.lora_grad_batchable(Y.view, U.view, r)      # the shapes of the MFMA form
    run_both_layouts(ops, Y, U.view, d, r, G.lora_grad(d, r), what)
    assert Y.bands_intact() and U.bands_intact(), what


VALU_PARAMS = [(333, 132, F32), (333, 136, BF16), (333, 136, F16), (5, 256, BF16), (5, 256, F16), (5, 256, F32), (700, 768, F32)]


@pytest.mark.parametrize("r", [17, 32, 64])
@pytest.mark.parametrize("M,N,dt", VALU_PARAMS, ids=ident)
def test_valu_form(ops, M, N, dt, r):
    valu_form(ops, M, N, dt, r)


@pytest.mark.parametrize("dt", [BF16, F16], ids=ident)
def test_valu_form_two_level_reduce(ops, dt):
    """34 row splits of the chunked VALU form (two 16-column chunks): level-1 slabs of 32 and 2 splits."""
    from gslora_hip import _lib as L
    p = ops.lora_grad_plan_args(4225, 8, 17, dt)
    assert (p.form, p.reduce, p.nsplit, p.R) == (L.LGRAD_VALU, L.LGRAD_REDUCE_TWO_LEVEL, 34, 32)
    valu_form(ops, 4225, 8, dt, 17)


def valu_form(ops, M, N, dt, r):
    d = for_rank(operands(M, N), r)
    what = f"valu {M}x{N} {NAME[dt]} r={r}"
    Y, U = Banded((M, N), dt, d["Y"].to(dt)), Banded((M, 64), dt, d["U"].to(dt))
    run_both_layouts(ops, Y, U.view, d, r, G.lora_grad(d, r), what)
    assert Y.bands_intact() and U.bands_intact(), what


BLOCKS = [(0, 64), (32, 32), (16, 48), (40, 24), (42, 21), (31, 33)]      # (42, 21) and (31, 33): unaligned, the exact-r form


@pytest.mark.parametrize("nan_outside", [False, True], ids=["ternary_outside", "nan_outside"])
@pytest.mark.parametrize("col,r", BLOCKS)
@pytest.mark.parametrize("dt", [BF16, F16, F32], ids=ident)
@pytest.mark.parametrize("M,N", [(700, 768)])
def test_u_column_blocks_of_a_64_wide_tensor(ops, M, N, dt, col, r, nan_outside):
    """U = columns [col, col + r) of a 64-wide banded tensor (the last row and the row end included), Y a padded column block. With NaN
    in every other column of U the result is the same: no product depends on a column outside the block."""
    d = for_rank(operands(M, N), r)
    what = f"block {M}x{N} {NAME[dt]} col={col} r={r} nan={nan_outside}"
    Y = Banded((M, N), dt, d["Y"].to(dt), ld=N + 64, col0=32, pad_rows=2)
    u = d["U"].clone()
    if nan_outside:
        u[:, :col] = float("nan")
        u[:, col + r:] = float("nan")
    U = Banded((M, 64), dt, u.to(dt))
    run_both_layouts(ops, Y, U.view[:, col:], d, r, G.lora_grad(d, r, col), what)
    assert Y.bands_intact() and U.bands_intact(), what


@pytest.mark.parametrize("r", [32, 64])
@pytest.mark.parametrize("M,N,dt", [(700, 768, F16), (1300, 2048, F16), (333, 136, F16), (700, 768, F32)], ids=ident)
def test_gscale_is_divided_out_exactly(ops, M, N, dt, r):
    """gscale = {2^k, 2^-k} with operands scaled by 2^k: the unscaled result, exactly (the 1/S of a loss-scaled fp16 backward)."""
    d = for_rank(operands(M, N), r)
    k = 3
    gscale = torch.tensor([2.0 ** k, 2.0 ** -k], device="cuda")
    Y, U = Banded((M, N), dt, (d["Y"] * 2.0 ** k).to(dt)), Banded((M, 64), dt, d["U"].to(dt))
    run_both_layouts(ops, Y, U.view, d, r, G.lora_grad(d, r), f"gscale {M}x{N} {NAME[dt]} r={r}", gscale=gscale)


def batch_entries(dt, ranks):
    out = []
    for i, r in enumerate(ranks):
        M, N = ((700, 768), (65, 256), (1300, 2048))[i % 3]
        d = for_rank(operands(M, N), r)
        col = 0 if r > 32 else 16
        Y, U = Banded((M, N), dt, d["Y"].to(dt), ld=N + 64, col0=32, pad_rows=2), Banded((M, 64), dt, d["U"].to(dt))
        out.append((Y, U, col, r, d))
    return out


@pytest.mark.parametrize("ranks", [(8, 16, 32, 64), tuple([8, 16, 32, 64, 24, 48, 17] * 4)], ids=["one_chunk", "chunked_28"])
@pytest.mark.parametrize("dt", [BF16, F16], ids=ident)
def test_batch_of_mixed_ranks_equals_the_single_launches(ops, dt, ranks):
    """Entries of rank 8, 16, 32 and 64 (and more than 24 entries: the chunked path) in one gsl_lora_grad_batch call: bit-identical
    to gsl_lora_grad on each, and exact."""
    entries, checks = [], []
    for Y, U, col, r, d in batch_entries(dt, ranks):
        N = d["Y"].shape[1]
        Gb, Gs = Banded((N, r), F32, d["G0"]), Banded((N, r), F32, d["G0"])
        assert ops.lora_grad_batchable(Y.view, U.view[:, col:], r)
        entries.append((Y.view, U.view[:, col:], Gb.view, r, 1, r, True))
        ops.lora_grad(Y.view, U.view[:, col:], Gs.view, r, 1, r, accumulate=True)
        checks.append((Gb, Gs, G.lora_grad(d, r, col), Y, U))
    ops.lora_grad_batch(entries)
    torch.cuda.synchronize()
    for i, (Gb, Gs, ref, Y, U) in enumerate(checks):
        same(Gs.view, ref, f"single launch, entry {i} (r = {ranks[i]}) {NAME[dt]}")
        assert torch.equal(Gb.view, Gs.view), (i, ranks[i], "the batch differs from the single launch")
        assert Gb.outside_intact() and Gs.outside_intact()
        assert Y.bands_intact() and U.bands_intact()


@pytest.mark.parametrize("M,N,dt,r", [(700, 768, BF16, 32), (1300, 2048, F16, 64), (333, 136, F16, 33), (700, 768, F32, 64)], ids=ident)
def test_two_identical_calls_are_bit_identical(ops, M, N, dt, r):
    """Fixed summation order, no atomics: on non-integer operands (where the order shows) two calls give the same bits."""
    g = torch.Generator().manual_seed(5)
    Y = torch.randn(M, N, generator=g).cuda().to(dt)
    U = torch.randn(M, 64, generator=g).cuda().to(dt)
    outs = []
    for _ in range(2):
        Gv = torch.zeros(N, r, device="cuda")
        ops.lora_grad(Y, U, Gv, r, 1, r, accumulate=False)
        outs.append(Gv)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    ref = Y.double().t() @ U.double()[:, :r]
    assert (outs[0].double() - ref).abs().max() < 1e-3 * ref.abs().max()      # (the order-dependent operands are the kernel's, not garbage)


@pytest.mark.parametrize("r", [0, 65])
def test_ranks_outside_1_to_64_are_refused_before_any_launch(ops, r):
    from gslora_hip import _lib as L
    Y, U = torch.zeros(64, 256, device="cuda", dtype=BF16), torch.zeros(64, 128, device="cuda", dtype=BF16)
    Gv = torch.full((256, 128), 7.0, device="cuda")
    with pytest.raises(RuntimeError):
        ops.lora_grad(Y, U, Gv, 128, 1, r, accumulate=False)
    assert "r in [1,64]" in L.load().gsl_last_error().decode()
    assert not ops.lora_grad_batchable(Y, U, r)
    with pytest.raises(RuntimeError):
        ops.lora_grad_batch([(Y, U, Gv, 128, 1, r, False)])
    assert "r in [1,64]" in L.load().gsl_last_error().decode()
    torch.cuda.synchronize()
    assert bool((Gv == 7.0).all())
