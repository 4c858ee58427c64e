"""gsl_lora_grad / gsl_lora_grad_batch at ranks 1 - 16 (csrc/lora.hip), one row per path of the launch plan, exact.

The table is oracle/gemm_probes.py LGRAD_EDGES; tests/test_lora_grad_plan_host.py holds every row to the path it is named for, and each
test here asks gsl_lora_grad_plan again for the very tensors it passes. Operands are the small-integer probes of that module (Y and G0 in
[-4, 4], U ternary) with its edge_rows option: the first and the last row of every row split of the plan — and so of every level-1 slab —
hold no zero, so a dropped or doubled boundary row moves every element. |sums| <= 4 * 16385 + 4 < 2^24: every comparison is torch.equal
against the float64 reference G.lora_grad, no tolerance. Every tensor is Banded (tests/guard_bands.py): inputs between NaN, outputs in
sentinel buffers.

Placements: `contiguous`; `padded` — Y a column block (ld = N + 64, col0 = 32, two pad rows), U the columns from 16 on of a 64-wide
tensor, G as [N, r] rows 16 apart inside a bucket and as [r, N] inside wider rows, both accumulating onto integers; a third call stores
(accumulate = 0) into a sentinel buffer and must leave no element unwritten. The cls rows are Y rows 197 * ld apart.

Full-mantissa operands (random normal values rounded to the dtype; the integer probes have two or three mantissa bits and cannot see a
dropped low bit): each element against float64 on the rounded inputs under the bound every summation order satisfies,
|err| <= 1.01 * ((M - 1) * 2^-24 * sum_m |y u| + 2^-24 * |G0 + sum|): 16-bit products are exact in f32, the f32 form uses fmaf (one
rounding per term), the final add onto G0 rounds once; 1.01 covers the second-order terms ((M - 1) 2^-24 < 2e-4) and, for the f32 chain,
the M-th rounding of its first product (its shapes have M >= 300). The largest |err| / bound ratios are printed (RATIO lines) and recorded in
profiles/lora_grad_tests.md."""
import functools

import pytest
import torch

from guard_bands import Banded
from oracle import gemm_probes as G

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
PLACEMENTS = ("contiguous", "padded")
FAN = 32
CASES = [(c, dt) for c in G.LGRAD_EDGES for dt in ((F32,) if c.kind == "f32" else (BF16, F16))]
CASE_IDS = [f"{i}-{NAME[dt]}" for i, c in zip(G.LGRAD_EDGE_IDS, G.LGRAD_EDGES) for dt in ((F32,) if c.kind == "f32" else (BF16, F16))]


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


def case(M, N, r, kind="16"):
    return next(c for c in G.LGRAD_EDGES if (c.M, c.N, c.r, c.kind) == (M, N, r, kind))


@functools.lru_cache(maxsize=None)
def operands(M, N, *rps):
    """Device operands of one shape with the edge rows of the given rows-per-split; built once, shared, never written to."""
    return {k: v.cuda() for k, v in G.make_lgrad_edges(M, N, G.split_edge_rows(M, *rps)).items()}


def reference(d, r, col=0):
    return G.lora_grad(dict(d, G0=d["G0"][:, :r]), r, col)


def same(got, ref, what):
    g = got.double()
    if not torch.equal(g, ref):
        bad = (g != ref).nonzero()
        i = tuple(bad[0].tolist())
        pytest.fail(f"{what}: {len(bad)} of {ref.numel()} elements differ, first at {i}: got {g[i].item()}, want {ref[i].item()}")


def place_inputs(d, dt, placement, ystep=1, yscale=1.0):
    """-> (Y, U, column of U the call starts at)."""
    M, N = d["Y"].shape
    kw = dict(ld=N + 64, col0=32, pad_rows=2) if placement == "padded" else {}
    if ystep > 1:
        kw = dict(kw, ld=kw.get("ld", N), row_step=ystep)
    Y = Banded((M, N), dt, (d["Y"] * yscale).to(dt), **kw)
    U = Banded((M, 64), dt, d["U"].to(dt))
    return Y, U, (16 if placement == "padded" else 0)


def g_views(d, r, placement):
    """The two accumulating gradient views, onto the integers of G0: [N, r] (padded: rows 16 apart) and [r, N] (padded: inside wider rows);
    and the sentinel buffer of the storing call. -> [(banded, view as [N, r], gsn, gsj)]"""
    N = d["Y"].shape[1]
    g0 = d["G0"][:, :r]
    if placement == "padded":
        a, b = Banded((N, r), F32, g0, ld=16, pad_rows=1), Banded((r, N), F32, g0.t(), ld=N + 24, col0=8, pad_rows=1)
        s = Banded((N, r), F32, ld=16, pad_rows=1)
        return [(a, a.view, 16, 1), (b, b.view.t(), 1, N + 24), (s, s.view, 16, 1)]
    a, b, s = Banded((N, r), F32, g0), Banded((r, N), F32, g0.t()), Banded((N, r), F32)
    return [(a, a.view, r, 1), (b, b.view.t(), 1, N), (s, s.view, r, 1)]


def check_plan(ops, c, Y, U, col, r):
    from gslora_hip import _lib as L
    p = ops.lora_grad_plan(Y.view, U.view[:, col:], r)
    want = (getattr(L, "LGRAD_" + c.form), G.padded_rank(r), c.nsplit, c.rps, c.CG, getattr(L, "LGRAD_REDUCE_" + c.reduce))
    assert (p.form, p.R, p.nsplit, p.rps, p.CG, p.reduce) == want, (c, p)


def run_case(ops, c, dt, placement, gscale=None, yscale=1.0):
    d = operands(c.M, c.N, c.rps)
    what = f"{c.name} {c.M}x{c.N} r={c.r} {NAME[dt]} {placement}"
    Y, U, col = place_inputs(d, dt, placement, c.ystep, yscale)
    check_plan(ops, c, Y, U, col, c.r)
    ref = reference(d, c.r, col)
    views = g_views(d, c.r, placement)
    for i, (b, _, gsn, gsj) in enumerate(views):
        ops.lora_grad(Y.view, U.view[:, col:], b.view, gsn, gsj, c.r, accumulate=i < 2, gscale=gscale)
    torch.cuda.synchronize()
    (a, av, _, _), (b, bv, _, _), (s, sv, _, _) = views
    same(av, ref, f"{what} G [N, r]")
    same(bv, ref, f"{what} G [r, N]")
    same(sv, ref - d["G0"][:, :c.r].double(), f"{what} stored G")
    assert a.outside_intact() and b.outside_intact(), (what, "a gradient stored outside its view")
    assert s.bands_intact() and s.unwritten() == 0, (what, "the storing call: a store outside the view, or an element never written")
    assert Y.bands_intact() and U.bands_intact(), (what, "an input changed")


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("c,dt", CASES, ids=CASE_IDS)
def test_table_is_exact_in_both_placements(ops, c, dt, placement):
    run_case(ops, c, dt, placement)


GSCALE_ROWS = [(case(65, 256, 8), F16), (case(2049, 256, 8), F16), (case(130, 2048, 8), F16), (case(4225, 8, 3), F16), (case(4225, 4, 3, "f32"), F32)]


@pytest.mark.parametrize("c,dt", GSCALE_ROWS, ids=lambda v: NAME.get(v) or f"{v.name}-{v.M}x{v.N}")
def test_gscale_is_divided_out_exactly(ops, c, dt):
    """gscale = {2^3, 2^-3} with Y scaled by 2^3: the unscaled result, exactly — one row per reduce kernel (direct, two-level, one-launch;
    the batch reducer: test_batch_is_exact_in_one_call)."""
    gscale = torch.tensor([8.0, 0.125], device="cuda")
    run_case(ops, c, dt, "padded", gscale=gscale, yscale=8.0)


# ---------------------------------------------------------------------------------------------------------------- neighbouring adapters
def three_blocks(M, r, seed):
    """A 64-wide U whose first 3 r columns are three different ternary blocks (edge rows of 32-row splits without a zero), the rest zero."""
    g = torch.Generator().manual_seed(seed)
    u = torch.zeros(M, 64)
    u[:, :3 * r] = G.ternary(g, M, 3 * r)
    rows = torch.tensor(G.split_edge_rows(M, 32))
    u[rows, :3 * r] = torch.where(u[rows, :3 * r] != 0, u[rows, :3 * r], torch.ones(len(rows), 3 * r))
    assert not torch.equal(u[:, :r], u[:, r:2 * r]) and not torch.equal(u[:, r:2 * r], u[:, 2 * r:3 * r])
    return u.cuda()


@pytest.mark.parametrize("dt", [BF16, F16], ids=ident)
@pytest.mark.parametrize("r,form", [(8, "single"), (8, "batch"), (5, "single")])
def test_neighbouring_adapters_give_their_own_block(ops, r, form, dt):
    """U = v[:, g r:] of the 64-wide tensor the QKV adapters share (_bwd_qkv_lora): group g reads its neighbours' finite columns and
    gives exactly its own block's gradient. r = 8: aligned blocks on the MFMA form and in the batch; r = 5: blocks 1 and 2 start off a
    16-byte boundary and take the VALU form."""
    from gslora_hip import _lib as L
    M, N = 65, 256
    d = dict(operands(M, N, 32), U=three_blocks(M, r, 11 + r))
    Y, U = Banded((M, N), dt, d["Y"].to(dt), ld=N + 64, col0=32, pad_rows=2), Banded((M, 64), dt, d["U"].to(dt))
    outs = [Banded((N, r), F32, d["G0"][:, :r]) for _ in range(3)]
    if form == "batch":
        assert all(ops.lora_grad_batchable(Y.view, U.view[:, g * r:], r) for g in range(3))
        ops.lora_grad_batch([(Y.view, U.view[:, g * r:], outs[g].view, r, 1, r, True) for g in range(3)])
    else:
        for g in range(3):
            p = ops.lora_grad_plan(Y.view, U.view[:, g * r:], r)
            assert p.form == (L.LGRAD_MFMA if (g * r) % 8 == 0 else L.LGRAD_VALU), (g, p)
            ops.lora_grad(Y.view, U.view[:, g * r:], outs[g].view, r, 1, r, accumulate=True)
    torch.cuda.synchronize()
    refs = [reference(d, r, g * r) for g in range(3)]
    assert not torch.equal(refs[0], refs[1]) and not torch.equal(refs[1], refs[2])
    for g in range(3):
        same(outs[g].view, refs[g], f"group {g} r={r} {form} {NAME[dt]}")
        assert outs[g].outside_intact()
    assert Y.bands_intact() and U.bands_intact()


# ---------------------------------------------------------------------------------------------------------------- batch form
BATCH_SHAPES = [(M, N) for M in (1, 8, 33, 65, 2049) for N in (256, 768)]


def batch_setup(ops, shapes_ranks, dt, yscale=1.0, ystep_of=lambda i: 1):
    """Entries (Y padded, U from column 16) with mixed accumulate and both output layouts; the operands carry the edge rows of the batch
    plan and of the single call's. -> [(entry tuple, checks...)]"""
    plans = ops.lora_grad_batch_plan([(M, N, r) for M, N, r in shapes_ranks])
    out = []
    for i, ((M, N, r), p) in enumerate(zip(shapes_ranks, plans)):
        d = operands(M, N, *sorted({p.rps, 32}))
        kw = dict(ld=N + 64, col0=32, pad_rows=2)
        if ystep_of(i) > 1:
            kw["row_step"] = ystep_of(i)
        Y, U = Banded((M, N), dt, (d["Y"] * yscale).to(dt), **kw), Banded((M, 64), dt, d["U"].to(dt))
        acc, nr_layout = i % 2 == 0, i % 4 < 2
        g0 = d["G0"][:, :r]
        if acc:
            Gb = Banded((N, r), F32, g0, ld=16, pad_rows=1) if nr_layout else Banded((r, N), F32, g0.t(), ld=N + 24, col0=8, pad_rows=1)
        else:
            Gb = Banded((N, r), F32, ld=16, pad_rows=1) if nr_layout else Banded((r, N), F32, ld=N + 24, col0=8, pad_rows=1)
        gsn, gsj = (16, 1) if nr_layout else (1, N + 24)
        ref = reference(d, r, 16) - (0 if acc else g0.double())
        assert ops.lora_grad_batchable(Y.view, U.view[:, 16:], r)
        out.append(dict(entry=(Y.view, U.view[:, 16:], Gb.view, gsn, gsj, r, acc), Y=Y, U=U, G=Gb, acc=acc, nr=nr_layout, ref=ref, r=r, M=M, N=N,
                        d=d, gs=(gsn, gsj)))
    got = ops.lora_grad_batch_plan([e["entry"] for e in out])
    assert got == plans, "the plan of the tensors is the plan of the shapes"
    return out


def batch_check(entries, what):
    for i, e in enumerate(entries):
        Gb = e["G"]
        same(Gb.view if e["nr"] else Gb.view.t(), e["ref"], f"{what} entry {i} ({e['M']}x{e['N']} r={e['r']} acc={e['acc']})")
        if e["acc"]:
            assert Gb.outside_intact(), (what, i)
        else:
            assert Gb.bands_intact() and Gb.unwritten() == 0, (what, i)
        assert e["Y"].bands_intact() and e["U"].bands_intact(), (what, i)


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "gscale"])
@pytest.mark.parametrize("dt", [BF16, F16], ids=ident)
def test_batch_is_exact_in_one_call(ops, dt, scaled):
    """M in {1, 8, 33, 65, 2049} x N in {256, 768}, r in {3, 8, 16}, in one call: mixed accumulate, both output layouts, with and without
    gscale; where M >= 64 the single call gives the same bits."""
    shapes = [(M, N, (3, 8, 16)[(i + i // 3) % 3]) for i, (M, N) in enumerate(BATCH_SHAPES)]
    assert {(M, r) for M, _, r in shapes} >= {(1, 3), (1, 8), (8, 16), (2049, 3), (2049, 8)} and {r for _, _, r in shapes} == {3, 8, 16}
    gscale = torch.tensor([8.0, 0.125], device="cuda") if scaled else None
    entries = batch_setup(ops, shapes, dt, yscale=8.0 if scaled else 1.0)
    ops.lora_grad_batch([e["entry"] for e in entries], gscale=gscale)
    torch.cuda.synchronize()
    batch_check(entries, f"batch {NAME[dt]} scaled={scaled}")
    for i, e in enumerate(entries):
        if e["M"] < 64:
            continue
        N, r = e["N"], e["r"]
        g0 = e["d"]["G0"][:, :r]
        Gs = (Banded((N, r), F32, g0 if e["acc"] else torch.zeros_like(g0), ld=16, pad_rows=1) if e["nr"]
              else Banded((r, N), F32, (g0 if e["acc"] else torch.zeros_like(g0)).t(), ld=N + 24, col0=8, pad_rows=1))
        ops.lora_grad(e["Y"].view, e["U"].view[:, 16:], Gs.view, *e["gs"], r, accumulate=e["acc"], gscale=gscale)
        torch.cuda.synchronize()
        assert torch.equal(Gs.view, e["G"].view), (i, "the batch differs from the single call")


@pytest.mark.parametrize("dt", [BF16, F16], ids=ident)
def test_batch_of_25_entries_and_cls_row_stride(ops, dt):
    """25 entries: the 25th rides in the second launch pair. One M = 1 entry, and the 8 cls rows (Y rows 197 * ld apart) in each pair."""
    shapes = [((33, 256, 8), (65, 256, 3), (8, 768, 16), (8, 512, 8))[i % 4] for i in range(24)] + [(8, 512, 8)]
    shapes[5] = (1, 256, 8)
    cls = {3, 24}
    entries = batch_setup(ops, shapes, dt, ystep_of=lambda i: 197 if i in cls else 1)
    assert entries[3]["Y"].view.stride(0) == 197 * (512 + 64)
    ops.lora_grad_batch([e["entry"] for e in entries])
    torch.cuda.synchronize()
    batch_check(entries, f"batch of 25 {NAME[dt]}")


# ---------------------------------------------------------------------------------------------------------------- order and mantissa
def randn_operands(M, N, dt, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(M, N, generator=g).cuda().to(dt), torch.randn(M, 64, generator=g).cuda().to(dt), torch.randn(N, 16, generator=g).cuda())


@pytest.mark.parametrize("c,dt", [(case(2049, 256, 8), BF16), (case(2049, 256, 8), F16), (case(4225, 8, 3), BF16), (case(4225, 8, 3), F16),
                                  (case(4225, 4, 3, "f32"), F32)], ids=lambda v: NAME.get(v) or f"{v.name}-{v.M}x{v.N}")
def test_two_calls_give_the_same_bits(ops, c, dt):
    """Fixed summation order on both reduce levels: random operands (where the order shows), two calls, the same bits."""
    y, u, _ = randn_operands(c.M, c.N, dt, 5)
    Y, U = Banded((c.M, c.N), dt, y), Banded((c.M, 64), dt, u)
    check_plan(ops, c, Y, U, 0, c.r)
    outs = []
    for _ in range(2):
        Gv = Banded((c.N, c.r), F32)
        ops.lora_grad(Y.view, U.view, Gv.view, c.r, 1, c.r, accumulate=False)
        outs.append(Gv)
    torch.cuda.synchronize()
    assert torch.equal(outs[0].view.view(torch.int32), outs[1].view.view(torch.int32))
    assert outs[0].unwritten() == 0 and outs[0].bands_intact() and outs[1].bands_intact()


# name, M, N, r, dtypes. f32 operands run the VALU form at every shape. 16-bit only: the batch form, and the two 65- / 63-row shapes —
# they are where a dropped low mantissa bit of a 16-bit operand exceeds the bound most (the bound grows with M^2, the fault with sqrt(M)),
# and at M < 100 the f32 chain's M-th rounding is not within the 1.01.
MANTISSA = [("mfma_two_level", 2049, 768, 8, (BF16, F16, F32)), ("mfma_one_launch_many_splits", 2081, 512, 16, (BF16, F16, F32)),
            ("valu_cg128", 300, 520, 9, (BF16, F16, F32)), ("batch_entry", 2049, 256, 8, (BF16, F16)),
            ("mfma_one_row_tail", 65, 256, 8, (BF16, F16)), ("valu_cg128", 63, 256, 16, (BF16, F16))]
MANTISSA_CASES = [(n, M, N, r, dt) for n, M, N, r, dts in MANTISSA for dt in dts]


@pytest.mark.parametrize("name,M,N,r,dt", MANTISSA_CASES, ids=[f"{n}-{M}x{N}-r{r}-{NAME[dt]}" for n, M, N, r, dt in MANTISSA_CASES])
def test_full_mantissa_operands_hold_the_summation_bound(ops, name, M, N, r, dt):
    """See the module docstring for the bound."""
    from gslora_hip import _lib as L
    y, u, g0 = randn_operands(M, N, dt, 1000 + M + N)
    Y, U, Gv = Banded((M, N), dt, y), Banded((M, 64), dt, u), Banded((N, r), F32, g0[:, :r])
    if name == "batch_entry":
        ops.lora_grad_batch([(Y.view, U.view, Gv.view, r, 1, r, True)])
    else:
        c = case(M, N, r)
        p = ops.lora_grad_plan(Y.view, U.view, r)
        if dt == F32:
            assert p.form == L.LGRAD_VALU
        else:
            assert (p.form, p.reduce, p.nsplit) == (getattr(L, "LGRAD_" + c.form), getattr(L, "LGRAD_REDUCE_" + c.reduce), c.nsplit)
        ops.lora_grad(Y.view, U.view, Gv.view, r, 1, r, accumulate=True)
    torch.cuda.synchronize()
    yd, ud = y.double(), u.double()[:, :r]
    exact = g0[:, :r].double() + yd.t() @ ud
    mag = yd.abs().t() @ ud.abs()
    bound = 1.01 * ((M - 1) * 2.0 ** -24 * mag + 2.0 ** -24 * exact.abs())
    err = (Gv.view.double() - exact).abs()
    ratio = float((err / bound).max())
    print(f"RATIO lora_grad {name} {M}x{N} r={r} {NAME[dt]} {ratio:.4f}")
    assert bool((err <= bound).all()), (name, NAME[dt], ratio)
    assert Gv.outside_intact() and Y.bands_intact() and U.bands_intact()
