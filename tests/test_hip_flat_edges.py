"""The flat-buffer kernels of csrc/lora.hip (group-lasso norms, AdamW, casts, packs) off their friendly sizes: tensors of 1 to 4099
elements that start off a 16-byte boundary with NaN in the gaps between them, more tensors and groups than the 64 lanes of the final
kernel, an empty and an all-zero group; element counts of 1, 255, 257 and one more than a grid sweep; transposes around the 32 x 32 tile;
packs with a second sweep. Every tensor sits between guard bands (tests/guard_bands.py): inputs between NaN, outputs in sentinel
buffers, tensors a kernel reads and writes (p, m, v, gradflat) checked with outside_intact().

Tolerances: the two of tests/test_hip_ops.py (1e-6 relative for the norms, 2e-6 for AdamW against torch.optim.AdamW on float64), the
rounding count 4 * 2^-24 (|grad| + |k flat|) for the group-norm backward (coef * scale / norm, the product, the add); everything else is exact."""
import numpy as np
import pytest
import torch

from guard_bands import NAN_SENTINEL, Banded, ptr
from oracle.norm_probes import E

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
NORM_RTOL, ADAMW_ATOL = 1e-6, 2e-6          # tests/test_hip_ops.py: test_group_norms_and_mask, test_adamw_matches_torch


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


def stream():
    return torch.cuda.current_stream().cuda_stream


def gen(seed):
    return torch.Generator().manual_seed(seed)


def relerr(a, b):
    return (a.double() - b).abs().max().item() / max(1e-12, b.abs().max().item())


# ---------------------------------------------------------------------------------------------------------------- group norms
NT, NG, EMPTY_GROUP, ZERO_TENSOR = 70, 67, 13, 41
NUMEL = (1, 3, 5, 7, 8, 30, 257, 4099)


def norm_layout():
    """70 tensors in 67 groups: group 13 has no tensor, tensor 41 (alone in its group) is all zero, four groups hold two tensors, tgroup is
    not sorted; gaps of 1 to 3 elements (NaN) between the tensors."""
    g = gen(11)
    numel = [NUMEL[t % len(NUMEL)] for t in range(NT)]
    off, toff = 0, []
    for t in range(NT):
        toff.append(off)
        off += numel[t] + 1 + t % 3
    groups = [q for q in range(NG) if q != EMPTY_GROUP]                       # 66 groups for 70 tensors
    others = [t for t in range(NT) if t != ZERO_TENSOR]
    order = [others[i] for i in torch.randperm(len(others), generator=g).tolist()]
    tgroup = [0] * NT
    zero_group = groups.pop(20)
    tgroup[ZERO_TENSOR] = zero_group
    for i, t in enumerate(order):
        tgroup[t] = groups[i % len(groups)]
    flat = torch.full((off,), float("nan"))
    inside = torch.zeros(off, dtype=torch.bool)
    for t in range(NT):
        flat[toff[t]:toff[t] + numel[t]] = 0.0 if t == ZERO_TENSOR else torch.randn(numel[t], generator=g) * (0.5 + t % 5)
        inside[toff[t]:toff[t] + numel[t]] = True
    return flat, inside, toff, numel, tgroup, zero_group


def norm_reference(flat, toff, numel, tgroup):
    ss = torch.stack([(flat[o:o + n].double() ** 2).sum() for o, n in zip(toff, numel)])
    gn, cn = torch.zeros(NG, dtype=torch.float64), torch.zeros(NG, dtype=torch.float64)
    for t, q in enumerate(tgroup):
        gn[q] += ss[t]
        cn[q] += ss[t].sqrt()
    return ss, gn.sqrt(), cn


def run_norms(flat_b, tabs, tau):
    from gslora_hip import _lib as L
    out = dict(ws=Banded((NT * L.NORM_SPLIT,), F32), tensor_sumsq=Banded((NT,), F32), group_norm=Banded((NG,), F32), cal_norm=Banded((NG,), F32),
               loss=Banded((1,), F32), mask=Banded((NG,), torch.uint8))
    L.check(L.load().gsl_group_norms_fwd(ptr(flat_b), ptr(tabs[0]), ptr(tabs[1]), ptr(tabs[2]), NT, NG, float(tau), ptr(out["ws"]), ptr(out["tensor_sumsq"]),
                                         ptr(out["group_norm"]), ptr(out["cal_norm"]), ptr(out["loss"]), ptr(out["mask"]), stream()), "gsl_group_norms_fwd")
    torch.cuda.synchronize()
    for n, b in list(out.items()) + [("flat", flat_b)] + [(f"table {i}", t) for i, t in enumerate(tabs)]:
        assert b.bands_intact(), n
    for n, b in out.items():
        assert b.unwritten() == 0, n
    return {n: b.view for n, b in out.items()}


def test_group_norms_on_unaligned_tensors_with_nan_gaps(ops):
    from gslora_hip import _lib as L
    flat, inside, toff, numel, tgroup, zero_group = norm_layout()
    off16 = sum(1 for o in toff if o % 4) / NT
    assert 0.6 < off16 < 0.9 and tgroup != sorted(tgroup) and EMPTY_GROUP not in tgroup and len(set(tgroup)) == NG - 1
    assert NT > 64 and NG > 64                       # the t += 64 and g += 64 loops of the final kernel
    flat_b = Banded(flat.shape, F32, flat)
    tabs = (Banded((NT,), torch.int64, torch.tensor(toff)), Banded((NT,), torch.int64, torch.tensor(numel)), Banded((NT,), torch.int32, torch.tensor(tgroup, dtype=torch.int32)))
    ss, gn, cn = (t.cuda() for t in norm_reference(flat, toff, numel, tgroup))
    out = run_norms(flat_b, tabs, 0.0)
    assert relerr(out["tensor_sumsq"], ss) < NORM_RTOL and relerr(out["group_norm"], gn) < NORM_RTOL and relerr(out["cal_norm"], cn) < NORM_RTOL
    assert relerr(out["loss"], gn.sum()[None]) < NORM_RTOL
    for q in (EMPTY_GROUP, zero_group):
        assert out["group_norm"][q] == 0 and out["cal_norm"][q] == 0 and out["mask"][q] == 0
    assert out["tensor_sumsq"][ZERO_TENSOR] == 0
    assert out["mask"].tolist() == (gn > 0.0).to(torch.uint8).tolist()
    srt = gn.sort().values
    lo, hi = float(srt[NG // 2]), float(srt[NG // 2 + 1])
    assert hi - lo > 4 * NORM_RTOL * hi               # the two neighbours are apart: tau midway decides every group the same way in f32
    tau = 0.5 * (lo + hi)
    out2 = run_norms(flat_b, tabs, tau)
    assert out2["mask"].tolist() == (gn > tau).to(torch.uint8).tolist() and 0 < int(out2["mask"].sum()) < NG
    # backward: gradflat += coef * scale * flat / ||group||; gaps untouched, zero groups add exactly 0
    grad0 = torch.randn(flat.shape, generator=gen(12))
    grad_b = Banded(flat.shape, F32, grad0)
    coef, scale = Banded((1,), F32, torch.tensor([2.0])), 0.3
    gn_b = Banded((NG,), F32, out["group_norm"])
    L.check(L.load().gsl_group_norms_bwd(ptr(flat_b), ptr(tabs[0]), ptr(tabs[1]), ptr(tabs[2]), NT, ptr(gn_b), ptr(coef), scale, ptr(grad_b), stream()),
            "gsl_group_norms_bwd")
    torch.cuda.synchronize()
    assert grad_b.outside_intact() and flat_b.bands_intact() and gn_b.bands_intact() and coef.bands_intact()
    got, grad0, inside = grad_b.view, grad0.cuda(), inside.cuda()
    assert torch.equal(got[~inside].view(torch.int32), grad0[~inside].view(torch.int32)), "a gap of gradflat changed"
    assert torch.isfinite(got[inside]).all()
    z = slice(toff[ZERO_TENSOR], toff[ZERO_TENSOR] + numel[ZERO_TENSOR])
    assert torch.equal(got[z], grad0[z])
    k = torch.zeros(flat.shape, dtype=torch.float64, device="cuda")
    for t in range(NT):
        nrm = float(out["group_norm"][tgroup[t]])        # the norm the call was given
        k[toff[t]:toff[t] + numel[t]] = 2.0 * float(np.float32(scale)) / nrm if nrm > 0 else 0.0
    add = k[inside] * flat.cuda().double()[inside]
    err = (got[inside].double() - (grad0[inside].double() + add)).abs()
    assert (err <= 4 * E * (grad0[inside].double().abs() + add.abs())).all(), float(err.max())


# ---------------------------------------------------------------------------------------------------------------- AdamW
@pytest.mark.parametrize("n", [1, 255, 257, 2048 * 256 + 3])
def test_adamw_sizes_around_a_block_and_beyond_one_sweep(ops, n):
    """Three steps against torch.optim.AdamW on float64 parameters; gsl_adamw_flat_dev bit-identical to the value form; nothing behind n written."""
    p0, g = torch.randn(n, generator=gen(1)), torch.randn(n, generator=gen(2))
    pt = torch.nn.Parameter(p0.double())
    opt = torch.optim.AdamW([pt], lr=1e-2, weight_decay=0.05, eps=1e-8)
    a = [Banded((n,), F32, t) for t in (p0, torch.zeros(n), torch.zeros(n))]
    b = [Banded((n,), F32, t) for t in (p0, torch.zeros(n), torch.zeros(n))]
    lr_dev, step_dev = torch.full((1,), 1e-2, device="cuda"), torch.zeros(1, device="cuda", dtype=torch.int64)
    for step in (1, 2, 3):
        pt.grad = g.double() * step
        opt.step()
        gb = Banded((n,), F32, g * step)
        ops.adamw_flat(a[0].view, gb.view, a[1].view, a[2].view, 1e-2, 0.9, 0.999, 1e-8, 0.05, step)
        step_dev.fill_(step)
        ops.adamw_flat_dev(b[0].view, gb.view, b[1].view, b[2].view, lr_dev, 0.9, 0.999, 1e-8, 0.05, step_dev)
        torch.cuda.synchronize()
        assert gb.bands_intact() and all(t.outside_intact() for t in a + b)
        assert (a[0].view.double().cpu() - pt.detach()).abs().max() < ADAMW_ATOL, step
        assert all(torch.equal(x.view, y.view) for x, y in zip(a, b)), (step, "device-step form differs")


# ---------------------------------------------------------------------------------------------------------------- casts
def cast(src, dt):
    from gslora_hip import _lib as L
    from gslora_hip import ops as O
    s, out = Banded(src.shape, F32, src), Banded(src.shape, dt, sentinel=NAN_SENTINEL[dt])      # (values over 46 decades: any finite sentinel is one of them)
    L.check(L.load().gsl_cast(ptr(s), ptr(out), src.numel(), O.code(dt), stream()), "gsl_cast")
    torch.cuda.synchronize()
    assert s.bands_intact() and out.bands_intact() and out.unwritten() == 0
    return out.view


def cast_values(n, dt):
    """Magnitudes over the range torch and the kernel must round alike: up to 3e38 for bf16 and f32, below the fp16 limit for fp16, down
    to the subnormals of the 16-bit type."""
    x = torch.randn(n, generator=gen(n))
    top = 4.0 if dt == F16 else 38.0
    return x * 10.0 ** (torch.rand(n, generator=gen(n + 1)) * (top + 8.0) - 8.0)


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=ident)
@pytest.mark.parametrize("n", [1, 257, 4096 * 256 + 5])
def test_cast_rounds_like_torch(ops, n, dt):
    x = cast_values(n, dt)
    x = x[(x.abs() < (65504.0 if dt == F16 else 3e38))]
    if x.numel() == 0:
        x = torch.tensor([0.3333])
    got = cast(x, dt)
    want = x.to(dt).cuda()
    assert torch.equal(got.view(torch.int16 if dt != F32 else torch.int32), want.view(torch.int16 if dt != F32 else torch.int32))


def test_cast_saturates_at_the_largest_finite_value_and_keeps_inf_and_nan(ops):
    """include/gslora_hip.h at gsl_cast: a finite f32 beyond the largest finite value of the 16-bit type becomes that value — +-65504 in fp16
    and +-0x7f7f = 3.3895e38 in bf16 (where round-to-nearest alone would give Inf) — while Inf and NaN stay Inf and NaN."""
    inf, nan = float("inf"), float("nan")
    got = cast(torch.tensor([65520.0, 1e6, -65520.0, -1e6, 65504.0, inf, -inf, nan, 3e38]), F16).float().cpu()
    assert got[:5].tolist() == [65504.0, 65504.0, -65504.0, -65504.0, 65504.0] and got[5:7].tolist() == [inf, -inf]
    assert got[7].isnan() and got[8] == 65504.0
    top = torch.tensor([0x7F7F], dtype=torch.int16).view(BF16).float().item()          # 3.3895e38
    src = torch.tensor([3.39e38, 3.396e38, 3.4e38, 3.4028234e38, -3.4e38, top, inf, -inf, nan])
    assert src[:5].to(BF16).float().abs().tolist() == [top, top, inf, inf, inf]         # what rounding to nearest alone gives
    got = cast(src, BF16).float().cpu()
    assert got[:6].tolist() == [top, top, top, top, -top, top] and got[6:8].tolist() == [inf, -inf] and got[8].isnan()


# ---------------------------------------------------------------------------------------------------------------- transpose, packs
@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=ident)
@pytest.mark.parametrize("R,C", [(1, 1), (31, 33), (32, 32), (33, 65), (40, 24)])
def test_transpose_cast_around_the_tile(ops, R, C, dt):
    from gslora_hip import _lib as L
    W = torch.randn(R, C, generator=gen(R * 100 + C))
    s, out = Banded((R, C), F32, W), Banded((C, R), dt)
    L.check(L.load().gsl_transpose_cast(ptr(s), ptr(out), R, C, ops.code(dt), stream()), "gsl_transpose_cast")
    torch.cuda.synchronize()
    assert s.bands_intact() and out.bands_intact() and out.unwritten() == 0
    assert torch.equal(out.view.cpu(), W.t().contiguous().to(dt))


def pack_reference(src, transposed, rows, cols, scale, rows_out, ld_out, dt):
    want = torch.zeros(rows_out, ld_out)
    want[:rows, :cols] = scale * (src.t() if transposed else src)
    return want.to(dt)


PACKS = [("rows", False, 8, 128, 0.5, 64, 160), ("transposed", True, 128, 8, 0.25, 136, 64), ("second_sweep", False, 60, 8190, 2.0, 64, 8200),
         ("transposed_ragged", True, 33, 5, 0.5, 40, 12)]


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=ident)
@pytest.mark.parametrize("name,transposed,rows,cols,scale,rows_out,ld_out", PACKS, ids=ident)
def test_pack_pad(ops, name, transposed, rows, cols, scale, rows_out, ld_out, dt):
    """out[i, j] = scale * in[i si + j sj] (a power-of-two scale: exact before the one rounding), zero beyond rows x cols."""
    src = torch.randn((cols, rows) if transposed else (rows, cols), generator=gen(rows + cols))
    s, out = Banded(src.shape, F32, src), Banded((rows_out, ld_out), dt)
    si, sj = (1, rows) if transposed else (cols, 1)
    ops.pack_pad(s.view, si, sj, rows, cols, rows_out, ld_out, dt, scale=scale, out=out.view)
    torch.cuda.synchronize()
    assert s.bands_intact() and out.bands_intact() and out.unwritten() == 0
    got = out.view.cpu()
    assert torch.equal(got, pack_reference(src, transposed, rows, cols, scale, rows_out, ld_out, dt))
    assert torch.count_nonzero(got[rows:]) == 0 and torch.count_nonzero(got[:, cols:]) == 0
    if name == "second_sweep":
        assert rows_out * ld_out > 2048 * 256


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=ident)
def test_pack_pad_batch_of_three_shapes(ops, dt):
    """Outputs of 16 x 8, 64 x 768 and 16 x 2048 in one call: bit-identical to the single packs, nothing written outside any of them."""
    geoms = [(True, 5, 8, 0.5, 16, 8), (False, 16, 768, 1.0, 64, 768), (False, 8, 2000, 0.125, 16, 2048)]     # transposed, rows, cols, scale, rows_out, ld_out
    srcs, outs, singles, entries = [], [], [], []
    for i, (tr, rows, cols, scale, ro, ld) in enumerate(geoms):
        src = torch.randn((cols, rows) if tr else (rows, cols), generator=gen(40 + i))
        s, o, one = Banded(src.shape, F32, src), Banded((ro, ld), dt), Banded((ro, ld), dt)
        si, sj = (1, rows) if tr else (cols, 1)
        ops.pack_pad(s.view, si, sj, rows, cols, ro, ld, dt, scale=scale, out=one.view)
        entries.append((s.view, si, sj, rows, cols, scale, o.view))
        srcs.append(s); outs.append(o); singles.append(one)
        assert torch.equal(one.view.cpu(), pack_reference(src, tr, rows, cols, scale, ro, ld, dt))
    table, mx = ops.pack_desc_table(entries, "cuda")
    assert mx == 64 * 768
    ops.pack_pad_batch(table, len(entries), mx, dt)
    torch.cuda.synchronize()
    for s, o, one in zip(srcs, outs, singles):
        assert s.bands_intact() and o.bands_intact() and o.unwritten() == 0
        assert torch.equal(o.view.view(torch.uint8), one.view.view(torch.uint8))
