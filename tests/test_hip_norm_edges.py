"""The LayerNorm kernels (csrc/norm.hip: gsl_layernorm_fwd, gsl_layernorm_bwd, gsl_layernorm_fwd_lora) at their edges, on the probes of
oracle/norm_probes.py: every width, row counts around one block of four waves, a second grid-stride trip, every dtype instantiation of
the two dispatch chains, x / dres / dx as column blocks and cls rows of larger tensors, the compact dres, the dropout copy, the overflow
guard gmax (NaN and Inf included) and the argument checks.

Every tensor a kernel reads sits between NaN bands and every output in a sentinel buffer (tests/guard_bands.py): the bands must be intact,
the inputs unchanged and no output element left unwritten. Results are held per element to the float64 references under the bounds of
oracle/norm_probes.py (no tolerance of this file's own; tests/test_norm_probes_host.py shows on the CPU that an f32 restatement of the
kernels stays under them and that each fault model exceeds them), strided placements bit for bit to the contiguous call. Each comparison
prints its largest error / bound ratio (pytest -s; profiles/row_kernel_tests.md).

Findings this file was written against: gsl_layernorm_bwd's gmax took its maximum with fmaxf, which drops a NaN — a NaN gradient never
reached the guard and gsl_adamw_flat applied the step (test_gmax_turns_non_finite_and_adamw_skips_the_step); io_row_stride in (0, D) and
x_row_stride < D were accepted (test_forward_refusals, test_backward_refusals, test_forward_lora_refusals). Floating-point outputs use
the NaN sentinel of tests/guard_bands.py: the default 16-bit one is 203.25 in fp16, a value dx takes."""
import functools

import pytest
import torch

from guard_bands import NAN_SENTINEL, Banded, ptr
from oracle import norm_probes as N

pytestmark = pytest.mark.gpu

F32, BF16, F16 = N.F32, N.BF16, N.F16
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
T_CLS = N.CLS_T
SEED, SITE = 3, 9


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


@functools.lru_cache(maxsize=3)
def device_case(name, X):
    """A table row on the device (x rounded to X), built once, shared, never written to."""
    case = N.BY_NAME[name]
    return case, {k: v.cuda() for k, v in N.make(case, X).items()}


def Out(shape, dt):
    """An output buffer whose sentinel is a NaN with a payload: no result equals it by chance (0x5A5A is 203.25 in fp16, a value dx takes)."""
    return Banded(shape, dt, sentinel=NAN_SENTINEL[dt])


def place(src, dt, placement, D, pad=64):
    """(Banded input, row stride). colblock: a column block at offset 8 of rows D + pad long; cls: rows T_CLS * D apart."""
    src = src.to(dt)
    if placement == "colblock":
        return Banded(src.shape, dt, src, ld=D + pad, col0=8, pad_rows=1), D + pad
    if placement == "cls":
        return Banded(src.shape, dt, src, ld=D, row_step=T_CLS), T_CLS * D
    return Banded(src.shape, dt, src), D


def settled(bands, outputs=()):
    torch.cuda.synchronize()
    for n, b in bands.items():
        if b is not None:
            assert b.bands_intact(), ("input changed or bands of" if b.is_input else "bands of", n)
    for n in outputs:
        assert bands[n].unwritten() == 0, ("unwritten elements in", n)


def under(what, got, ref, bound):
    r = N.ratio(got, ref, bound)
    print(f"RATIO {what} {r:.3f}")
    assert r <= 1.0, (what, r)


def forward(ops, d, M, D, T, X, placement="contiguous", stats_only=False):
    from gslora_hip import _lib as L
    x, xs = place(d["x"], X, placement, D)
    t = dict(x=x, gamma=Banded((D,), F32, d["gamma"]), beta=Banded((D,), F32, d["beta"]),
             y=None if stats_only else Out((M, D), T), mean=Out((M,), F32), rstd=Out((M,), F32))
    L.check(L.load().gsl_layernorm_fwd(ptr(x), xs, ptr(t["gamma"]), ptr(t["beta"]), N.EPS, ptr(t["y"]), ptr(t["mean"]), ptr(t["rstd"]),
                                       M, D, ops.code(T), ops.code(X), stream()), "gsl_layernorm_fwd")
    settled(t, ("mean", "rstd") + (() if stats_only else ("y",)))
    return (None if stats_only else t["y"].view), t["mean"].view, t["rstd"].view


def check_forward(what, d, D, T, y, mean, rstd, rows=slice(None)):
    x = d["x"][rows]
    mean64, rstd64, y64 = N.forward(x, d["gamma"], d["beta"])
    under(f"{what} mean", mean[rows], mean64, N.bound_mean(x, D))
    under(f"{what} rstd", rstd[rows], rstd64, N.bound_rstd(x, rstd64, D))
    under(f"{what} y", y[rows], y64, N.bound_y(x, d["gamma"], rstd64, y64, D, T))


def backward(ops, d, mean, rstd, M, D, T, S, X, placement="contiguous", dres="dense", p_drop=0.0, drs=0, gmax=None, dy=None, dres_src=None):
    """dres: None, "dense", "compact" (dres_cls_T = T_CLS: the first ceil(M / T_CLS) rows of d["dres"]) or, with the cls placement,
    aliased to dx (in place). Returns (dx, dxb) views."""
    from gslora_hip import _lib as L
    x, xs = place(d["x"], X, placement, D)
    dy = d["dy"] if dy is None else dy
    dres_src = d["dres"] if dres_src is None else dres_src
    t = dict(x=x, dy=Banded((M, D), T, dy.to(T)), gamma=Banded((D,), F32, d["gamma"]), mean=Banded((M,), F32, mean), rstd=Banded((M,), F32, rstd),
             dxb=Out((M, D), T), dres=None)
    ios, cls_T, inplace = 0, 0, placement == "cls"
    if inplace:
        dx, ios = place(dres_src, S, "cls", D)                 # holds dres, updated in place
        p_dres = ptr(dx)
    else:
        dx = Out((M, D), S)
        if dres == "compact":
            t["dres"], cls_T = Banded(((M + T_CLS - 1) // T_CLS, D), S, dres_src[:(M + T_CLS - 1) // T_CLS].to(S)), T_CLS
        elif dres == "dense":
            t["dres"] = Banded((M, D), S, dres_src.to(S))
        p_dres = ptr(t["dres"])
    L.check(L.load().gsl_layernorm_bwd(ptr(t["dy"]), ptr(x), xs, ptr(t["gamma"]), ptr(t["mean"]), ptr(t["rstd"]), p_dres, ptr(dx), ios, ptr(t["dxb"]),
                                       M, D, ops.code(T), ops.code(S), ops.code(X), float(p_drop), SEED, SITE, int(drs), cls_T, gmax, stream()),
            "gsl_layernorm_bwd")
    settled(t, ("dxb",))
    if inplace:
        assert dx.outside_intact(), "dx in place: something outside its rows changed"
    else:
        assert dx.bands_intact() and dx.unwritten() == 0
    return dx.view, t["dxb"].view


def check_backward(what, ops, d, mean, rstd, D, T, S, dx, dxb, dres, p_drop=0.0, drs=0, rows=slice(None), dy=None):
    """dres: the float32 incoming stream gradient as the kernel saw it (rounded to S, dense), or None."""
    dy = (d["dy"] if dy is None else dy).to(T)[rows]
    ref, parts = N.backward(dy, d["x"][rows], d["gamma"], mean[rows], rstd[rows], None if dres is None else dres[rows], parts=True)
    under(f"{what} dx", dx[rows], ref, N.bound_dx(parts, ref, D, S))
    if not p_drop:
        return under(f"{what} dxb", dxb[rows], ref, N.bound_dx(parts, ref, D, T))
    M = dx.shape[0]
    keep = N.keep_rows(ops.dropout_mask(M * (drs or D), p_drop, SEED, SITE, "cuda"), M, D, drs or D)[rows].bool()
    assert 0 < int(keep.sum()) < keep.numel()
    got = dxb[rows]
    assert (got[~keep] == 0).all(), (what, "a dropped element of dxb is not exactly zero")
    ref2 = N.dropout_copy(ref, keep, p_drop)
    b = N.bound_dx(parts, ref2, D, T, scale=1.0 / (1.0 - p_drop))
    under(f"{what} dxb kept", got[keep], ref2[keep], b[keep])


def seen(t, dt):
    return t.to(dt).float()


# ---------------------------------------------------------------------------------------------------------------- widths x rows
@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=ident)
@pytest.mark.parametrize("M", N.SMALL_M)
@pytest.mark.parametrize("D", N.WIDTHS)
def test_every_width_around_one_block(ops, D, M, dt):
    """16-bit: operands, stream and x all of that type; f32: all f32."""
    what = f"d{D} m{M} {NAME[dt]}"
    case, d = device_case(f"d{D}_m{M}", dt)
    y, mean, rstd = forward(ops, d, M, D, dt, dt)
    check_forward(what, d, D, dt, y, mean, rstd)
    _, mean2, rstd2 = forward(ops, d, M, D, dt, dt, stats_only=True)
    assert torch.equal(mean, mean2) and torch.equal(rstd, rstd2), (what, "statistics-only call differs")
    dx, dxb = backward(ops, d, mean, rstd, M, D, dt, dt, dt)
    check_backward(what, ops, d, mean, rstd, D, dt, dt, dx, dxb, seen(d["dres"], dt))
    dx, dxb = backward(ops, d, mean, rstd, M, D, dt, dt, dt, dres=None)
    check_backward(what + " no dres", ops, d, mean, rstd, D, dt, dt, dx, dxb, None)


@pytest.mark.parametrize("dt", [F32, BF16], ids=ident)
@pytest.mark.parametrize("D", [64, 768])
def test_second_grid_stride_trip(ops, D, dt):
    """M = 8192 + 5: the rows behind the first trip of min(ceil(M / 4), 2048) blocks. Every row is compared."""
    what = f"trip2 d{D} {NAME[dt]}"
    case, d = device_case(f"trip2_d{D}", dt)
    M = case.M
    assert M > N.ROWS_PER_TRIP
    y, mean, rstd = forward(ops, d, M, D, dt, dt)
    check_forward(what, d, D, dt, y, mean, rstd)
    check_forward(what + " rows of trip 2", d, D, dt, y, mean, rstd, rows=slice(N.ROWS_PER_TRIP, M))
    dx, dxb = backward(ops, d, mean, rstd, M, D, dt, dt, dt)
    check_backward(what, ops, d, mean, rstd, D, dt, dt, dx, dxb, seen(d["dres"], dt))
    check_backward(what + " rows of trip 2", ops, d, mean, rstd, D, dt, dt, dx, dxb, seen(d["dres"], dt), rows=slice(N.ROWS_PER_TRIP, M))


# ---------------------------------------------------------------------------------------------------------------- instantiations
FWD = [(F16, F16), (F16, F32), (BF16, F16), (BF16, BF16), (BF16, F32), (F32, F32)]
BWD = [(F16, F16, F16), (F16, F16, F32), (F16, F32, F16), (F16, F32, F32), (BF16, BF16, F16), (BF16, F32, F16), (BF16, BF16, BF16),
       (BF16, BF16, F32), (BF16, F32, BF16), (BF16, F32, F32), (F32, F32, F32)]


def test_instantiation_lists_are_complete():
    assert len(FWD) == 6 and len(set(FWD)) == 6 and set(FWD) == set(N.FWD_INSTANCES)
    assert len(BWD) == 11 and len(set(BWD)) == 11 and set(BWD) == set(N.BWD_INSTANCES)


@pytest.mark.parametrize("T,X", FWD, ids=ident)
@pytest.mark.parametrize("D", [128, 256])
def test_forward_instantiations(ops, D, T, X):
    case, d = device_case(f"inst_d{D}", X)
    y, mean, rstd = forward(ops, d, case.M, D, T, X)
    check_forward(f"inst d{D} T={NAME[T]} X={NAME[X]}", d, D, T, y, mean, rstd)


@pytest.mark.parametrize("T,S,X", BWD, ids=ident)
@pytest.mark.parametrize("D", [128, 256])
def test_backward_instantiations(ops, D, T, S, X):
    case, d = device_case(f"inst_d{D}", X)
    M = case.M
    _, mean, rstd = forward(ops, d, M, D, T, X, stats_only=True)
    dx, dxb = backward(ops, d, mean, rstd, M, D, T, S, X)
    check_backward(f"inst d{D} T={NAME[T]} S={NAME[S]} X={NAME[X]}", ops, d, mean, rstd, D, T, S, dx, dxb, seen(d["dres"], S))


# ---------------------------------------------------------------------------------------------------------------- placements
@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=ident)
@pytest.mark.parametrize("placement", ["colblock", "cls"])
@pytest.mark.parametrize("D", [128, 256, 512, 1024])
def test_strided_placements_equal_the_contiguous_call(ops, D, placement, dt):
    """colblock: x a column block (rows of D + 64 elements, column offset 8). cls: x, dres and dx rows T D apart, dx updated in place
    (dres aliased to it), dy and dxb dense, dropout with drop_row_stride = T D."""
    what = f"d{D} {placement} {NAME[dt]}"
    M = 37
    case, d = device_case(f"d{D}_m{M}", dt)
    y0, mean0, rstd0 = forward(ops, d, M, D, dt, dt)
    y, mean, rstd = forward(ops, d, M, D, dt, dt, placement)
    assert torch.equal(y, y0) and torch.equal(mean, mean0) and torch.equal(rstd, rstd0), what
    check_forward(what, d, D, dt, y, mean, rstd)
    kw = dict(p_drop=N.P_DROP, drs=T_CLS * D) if placement == "cls" else {}
    dx0, dxb0 = backward(ops, d, mean, rstd, M, D, dt, dt, dt, **kw)
    dx, dxb = backward(ops, d, mean, rstd, M, D, dt, dt, dt, placement, **kw)
    assert torch.equal(dx, dx0) and torch.equal(dxb, dxb0), what
    check_backward(what, ops, d, mean, rstd, D, dt, dt, dx, dxb, seen(d["dres"], dt), **kw)


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=ident)
@pytest.mark.parametrize("D", [64, 128, 256, 768])
def test_compact_dres_equals_the_dense_zero_filled_call(ops, D, dt):
    what = f"d{D} compact {NAME[dt]}"
    M = 37
    case, d = device_case(f"d{D}_m{M}", dt)
    _, mean, rstd = forward(ops, d, M, D, dt, dt, stats_only=True)
    dense = N.expand_compact(d["dres"][:(M + T_CLS - 1) // T_CLS], M, T_CLS)
    dx0, dxb0 = backward(ops, d, mean, rstd, M, D, dt, dt, dt, dres_src=dense)
    dx, dxb = backward(ops, d, mean, rstd, M, D, dt, dt, dt, dres="compact")
    assert torch.equal(dx, dx0) and torch.equal(dxb, dxb0), what
    check_backward(what, ops, d, mean, rstd, D, dt, dt, dx, dxb, seen(dense, dt))


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=ident)
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("D", [128, 256, 512, 768, 1024])
def test_dropout_copy(ops, D, strided, dt):
    """p = 0.5 on the scalar (D = 128: one or two elements per lane) and the 4-wide counter path (D = 256 .. 1024: VEC = 4 from four
    elements per lane on, at each of its row lengths): dropped elements of dxb exactly 0, kept ones within the bound
    of 2 dx, dx itself unmasked."""
    what = f"d{D} drop {'T D' if strided else 'D'} {NAME[dt]}"
    M = 37
    case, d = device_case(f"d{D}_m{M}", dt)
    _, mean, rstd = forward(ops, d, M, D, dt, dt, stats_only=True)
    drs = T_CLS * D if strided else D
    dx, dxb = backward(ops, d, mean, rstd, M, D, dt, dt, dt, p_drop=N.P_DROP, drs=drs)
    dx0, _ = backward(ops, d, mean, rstd, M, D, dt, dt, dt)
    assert torch.equal(dx, dx0), (what, "dx is masked")
    check_backward(what, ops, d, mean, rstd, D, dt, dt, dx, dxb, seen(d["dres"], dt), p_drop=N.P_DROP, drs=drs)


# ---------------------------------------------------------------------------------------------------------------- gmax
GUARD_LIMIT = 65504.0            # adamw_kernel skips the update when not (*guard < 65504)


@functools.lru_cache(maxsize=1)
def gmax_case(ops):
    """trip2_d64 in fp16 with its statistics; dy an eighth of the table's, so that LN'(dy) on the rows of rstd = rsqrt(eps) stays two
    thousands and nothing exceeds the values the tests plant."""
    case, d = device_case("trip2_d64", F16)
    M, D = case.M, case.D
    d = dict(d, dy=d["dy"] * 0.125)
    _, mean, rstd = forward(ops, d, M, D, F16, F16, stats_only=True)
    return M, D, d, mean.clone(), rstd.clone()


def run_gmax(ops, dy=None, dres=None, x=None, gmax=None):
    M, D, d, mean, rstd = gmax_case(ops)
    d = dict(d, x=d["x"] if x is None else x)
    g = Banded((1,), F32, torch.zeros(1)) if gmax is None else gmax
    dx, _ = backward(ops, d, mean, rstd, M, D, F16, F16, F16, dy=dy, dres_src=dres, gmax=ptr(g))
    assert g.outside_intact()
    return g, dx


def test_gmax_reports_the_second_trip_and_keeps_the_maximum(ops):
    M, D, d, mean, rstd = gmax_case(ops)
    row = M - 1                                  # an outlier row (kind 6): rstd is small, so LN'(dy) stays far below the planted values
    assert row >= N.ROWS_PER_TRIP and row % len(N.ROW_KINDS) == 6
    dy = d["dy"].clone()
    dy[row, 5] = 30000.0
    g, dx = run_gmax(ops, dy=dy)
    ref = N.backward(seen(dy, F16), d["x"], d["gamma"], mean, rstd, seen(d["dres"], F16))
    assert float(ref.abs().max()) < 20000.0 and N.fault_gmax_first_trip(seen(dy, F16), ref) < 30000.0      # the probe is what it says
    assert float(g.view[0]) == 30000.0
    dres = d["dres"].clone()
    dres[row, 9] = 40000.0
    g2, dx = run_gmax(ops, dy=dy, dres=dres, gmax=g)      # |dx| is taken on the f32 value, before the store rounds it
    ref, parts = N.backward(seen(dy, F16), d["x"], d["gamma"], mean, rstd, seen(dres, F16), parts=True)
    b = N.bound_dx(parts, ref, D, F32)
    i = ref.abs().argmax()
    assert i == row * D + 9 and abs(float(g.view[0]) - float(ref.abs().flatten()[i])) <= float(b.flatten()[i])
    top = float(g.view[0])
    run_gmax(ops, gmax=g)                                 # a maximum, not the last value
    assert float(g.view[0]) == top


@pytest.mark.parametrize("where", ["nan_dy", "nan_dres", "nan_x", "inf_dy"])
def test_gmax_turns_non_finite_and_adamw_skips_the_step(ops, where):
    """A NaN in dy (a first-trip row held by the last wave of its block), in dres only, in x only, and +Inf in dy: the guard must fail
    adamw_kernel's predicate *guard < 65504, and gsl_adamw_flat under it must leave p, m, v as they are."""
    M, D, d, mean, rstd = gmax_case(ops)
    row = 43
    assert row % 4 == 3 and row < N.ROWS_PER_TRIP
    t = {k: d[k].clone() for k in ("dy", "dres", "x")}
    t[where[4:]][row, 17] = float("inf") if where == "inf_dy" else float("nan")
    g, dx = run_gmax(ops, dy=t["dy"], dres=t["dres"], x=t["x"])
    assert not dx[row].float().isfinite().all()
    seen_max = float(g.view[0])
    assert not (seen_max < GUARD_LIMIT), (where, seen_max)
    n = 1000
    gen = torch.Generator().manual_seed(5)
    p, grad, m, v = (Banded((n,), F32, torch.randn(n, generator=gen).abs()) for _ in range(4))
    before = [b.view.clone() for b in (p, m, v)]
    ops.adamw_flat(p.view, grad.view, m.view, v.view, 1e-2, 0.9, 0.999, 1e-8, 0.05, 1, guard=g.view)
    torch.cuda.synchronize()
    assert all(torch.equal(b.view, a) for b, a in zip((p, m, v), before)) and grad.bands_intact()
    assert p.outside_intact() and m.outside_intact() and v.outside_intact()


# ---------------------------------------------------------------------------------------------------------------- gsl_layernorm_fwd_lora
LORA_CASES = [c for c in N.TABLE if c.kind == "lora"]


def forward_lora(ops, d, case, placement, ldp=None, xs=None):
    from gslora_hip import _lib as L
    M, D = case.M, case.D
    x, stride = place(d["x"], BF16, placement, D, pad=8)
    P = Banded((16, D), BF16, d["P"].to(BF16), ld=D + 8)            # exactly 16 rows between the bands: a read of row 16 is a NaN
    t = dict(x=x, P=P, gamma=Banded((D,), F32, d["gamma"]), beta=Banded((D,), F32, d["beta"]), y=Out((M, D), BF16),
             mean=Out((M,), F32), rstd=Out((M,), F32), u=Out((M, 64), BF16))
    alpha = 1.0 / case.r
    L.check(L.load().gsl_layernorm_fwd_lora(ptr(x), stride if xs is None else xs, ptr(t["gamma"]), ptr(t["beta"]), N.EPS, ptr(t["y"]), ptr(t["mean"]),
                                            ptr(t["rstd"]), M, D, ptr(P), D + 8 if ldp is None else ldp, alpha, ptr(t["u"]), stream()),
            "gsl_layernorm_fwd_lora")
    settled(t, ("y", "u", "mean", "rstd"))
    return t["y"].view, t["mean"].view, t["rstd"].view, t["u"].view, alpha


@pytest.mark.parametrize("placement", ["contiguous", "colblock", "cls"])
@pytest.mark.parametrize("case", LORA_CASES, ids=lambda c: c.name)
def test_layernorm_fwd_lora(ops, case, placement):
    """colblock: x_row_stride = D + 8; cls: T D. P is a column block (ldp = D + 8) of exactly 16 rows in every case."""
    what = f"{case.name} {placement}"
    D, r = case.D, case.r
    _, d = device_case(case.name, BF16)
    y, mean, rstd, u, alpha = forward_lora(ops, d, case, placement)
    check_forward(what, d, D, BF16, y, mean, rstd)
    assert torch.count_nonzero(u[:, 16:]) == 0 and torch.count_nonzero(u[:, r:16]) == 0, what
    under(f"{what} u", u[:, :16], *N.lora_u(y, d["P"], alpha, D))       # from the bf16 rows the kernel itself wrote


# ---------------------------------------------------------------------------------------------------------------- refusals
def refused(ops, entry, call, outs):
    with pytest.raises(RuntimeError, match=rf"\): {entry}: "):              # the library's own message names the entry
        call()
    torch.cuda.synchronize()
    for n, b in outs.items():
        assert b.bands_intact() and b.unwritten() == b.rows * b.cols, (entry, "wrote", n)


def fwd_args(ops, M=5, D=128, T=F32, X=F32, xs=None, ld=None):
    x = Banded((M, ld or D), X, torch.ones(M, ld or D))
    outs = dict(y=Out((M, D), T), mean=Out((M,), F32), rstd=Out((M,), F32))
    g, b = Banded((max(D, 64),), F32, torch.ones(max(D, 64))), Banded((max(D, 64),), F32, torch.ones(max(D, 64)))
    return [ptr(x), D if xs is None else xs, ptr(g), ptr(b), N.EPS, ptr(outs["y"]), ptr(outs["mean"]), ptr(outs["rstd"]), M, D, ops.code(T), ops.code(X),
            stream()], outs, (x, g, b)


@pytest.mark.parametrize("why,kw", [("width 192", dict(D=192)), ("x_row_stride % 4", dict(xs=130, ld=132)), ("16-bit x, f32 operands", dict(X=BF16)),
                                    ("bf16 x, fp16 operands", dict(T=F16, X=BF16)), ("x_row_stride < D", dict(xs=64))])
def test_forward_refusals(ops, why, kw):
    from gslora_hip import _lib as L
    args, outs, keep = fwd_args(ops, **kw)
    refused(ops, "gsl_layernorm_fwd", lambda: L.check(L.load().gsl_layernorm_fwd(*args), "gsl_layernorm_fwd"), outs)


def bwd_args(ops, M=7, D=128, T=F32, S=F32, X=F32, xs=None, ios=0, cls_T=0, dres="own", ld=None):
    ins = [Banded((M, D), T, torch.ones(M, D)), Banded((M, ld or D), X, torch.ones(M, ld or D)), Banded((max(D, 64),), F32, torch.ones(max(D, 64))),
           Banded((M,), F32, torch.zeros(M)), Banded((M,), F32, torch.ones(M)), Banded((M, D), S, torch.ones(M, D))]
    outs = dict(dx=Out((M, D), S), dxb=Out((M, D), T))
    p_dres = {"own": ptr(ins[5]), "null": None, "alias": ptr(outs["dx"])}[dres]
    return [ptr(ins[0]), ptr(ins[1]), D if xs is None else xs, ptr(ins[2]), ptr(ins[3]), ptr(ins[4]), p_dres, ptr(outs["dx"]), ios, ptr(outs["dxb"]), M, D,
            ops.code(T), ops.code(S), ops.code(X), 0.0, SEED, SITE, 0, cls_T, None, stream()], outs, ins


@pytest.mark.parametrize("why,kw", [("width 192", dict(D=192)), ("x_row_stride % 4", dict(xs=130, ld=132)), ("16-bit x, f32 operands", dict(X=F16)),
                                    ("bf16 x, fp16 operands", dict(T=F16, X=BF16)), ("stream bf16, operands fp16", dict(T=F16, S=BF16)),
                                    ("stream fp16, operands f32", dict(S=F16)), ("compact dres NULL", dict(cls_T=7, dres="null")),
                                    ("compact dres aliased to dx", dict(cls_T=7, dres="alias")), ("0 < io_row_stride < D", dict(ios=64)),
                                    ("x_row_stride < D", dict(xs=64))])
def test_backward_refusals(ops, why, kw):
    from gslora_hip import _lib as L
    args, outs, keep = bwd_args(ops, **kw)
    refused(ops, "gsl_layernorm_bwd", lambda: L.check(L.load().gsl_layernorm_bwd(*args), "gsl_layernorm_bwd"), outs)


@pytest.mark.parametrize("why,kw", [("width 256", dict(D=256)), ("ldp < D", dict(ldp=504)), ("x_row_stride < D", dict(xs=256))])
def test_forward_lora_refusals(ops, why, kw):
    from gslora_hip import _lib as L
    M, D = 5, kw.get("D", 512)
    ins = [Banded((M, D), BF16, torch.ones(M, D)), Banded((D,), F32, torch.ones(D)), Banded((D,), F32, torch.ones(D)), Banded((16, D), BF16, torch.ones(16, D))]
    outs = dict(y=Out((M, D), BF16), mean=Out((M,), F32), rstd=Out((M,), F32), u=Out((M, 64), BF16))
    args = [ptr(ins[0]), kw.get("xs", D), ptr(ins[1]), ptr(ins[2]), N.EPS, ptr(outs["y"]), ptr(outs["mean"]), ptr(outs["rstd"]), M, D, ptr(ins[3]),
            kw.get("ldp", D), 1.0, ptr(outs["u"]), stream()]
    refused(ops, "gsl_layernorm_fwd_lora", lambda: L.check(L.load().gsl_layernorm_fwd_lora(*args), "gsl_layernorm_fwd_lora"), outs)
