"""The LayerNorm probes of oracle/norm_probes.py, checked on the CPU for every row of the table tests/test_hip_norm_edges.py runs:

(a) an f32 restatement of the kernels' summation order (oracle/norm_probes.py emulate_*) stays under every bound, with slack where the
    output is f32 (a 16-bit store adds up to the half ulp the bound grants it, so those ratios come close to 1); the largest ratios are
    printed (pytest -s) and recorded in profiles/row_kernel_tests.md;
(b) every fault model exceeds a bound or breaks a guard band, on every row it applies to: an element dropped from the mean, 1/D of the
    neighbouring width, row m read at stride D, the second grid-stride trip skipped, dres added on every row in compact mode, the dropout
    counter row * D, the S and X casts swapped, gmax without the second trip's rows;
(c) the dropout copy's reference gives what tests/test_hip_ops.py expects on that file's shapes, and the instantiation lists hold the
    6 and 11 combinations the argument checks of gsl_layernorm_fwd / gsl_layernorm_bwd accept.

Pure torch / numpy: no GPU and no library."""
import functools
import itertools

import pytest
import torch

from guard_bands import BAND, SENTINEL, Banded
from oracle import norm_probes as N

F32, BF16, F16 = N.F32, N.BF16, N.F16
PLAIN = [c.name for c in N.TABLE if c.kind != "lora"]
LORA = [c.name for c in N.TABLE if c.kind == "lora"]
SAMPLE = 71            # rows of a second-trip case the emulation runs on (the last ones: every row kind, the rows behind the first trip)


@functools.lru_cache(maxsize=4)
def built(name, xdtype=F32):
    """(case, inputs) with at most SAMPLE rows (the emulation and the bounds are per row)."""
    case = N.BY_NAME[name]
    d = N.make(case, xdtype)
    if case.M > SAMPLE:
        d = {k: (v[-SAMPLE:] if v.shape[0] == case.M else v) for k, v in d.items()}
    return case, d


def stored(t, dtype):
    return t.to(dtype).double()


def fwd_ratios(d, D, out, T):
    mean64, rstd64, y64 = N.forward(d["x"], d["gamma"], d["beta"])
    mu, rs, y = out
    return dict(mean=N.ratio(mu, mean64, N.bound_mean(d["x"], D)), rstd=N.ratio(rs, rstd64, N.bound_rstd(d["x"], rstd64, D)),
                y=N.ratio(stored(y, T), y64, N.bound_y(d["x"], d["gamma"], rstd64, y64, D, T)))


@pytest.mark.parametrize("T,X", N.FWD_INSTANCES, ids=str)
@pytest.mark.parametrize("name", PLAIN)
def test_emulated_forward_and_backward_stay_under_the_bounds(name, T, X):
    case, d = built(name, X)
    D = case.D
    out = N.emulate_forward(d["x"], d["gamma"], d["beta"], D)
    r = fwd_ratios(d, D, out, T)
    dy = d["dy"].to(T).float()
    for S in sorted({F32, T}, key=str):
        dres = d["dres"].to(S).float()
        ref, parts = N.backward(dy, d["x"], d["gamma"], out[0], out[1], dres, parts=True)
        dx = N.emulate_backward(dy, d["x"], d["gamma"], out[0], out[1], dres, D)
        r[f"dx[{S}]"] = N.ratio(stored(dx, S), ref, N.bound_dx(parts, ref, D, S))
        r[f"dxb[{S}]"] = N.ratio(stored(dx, T), ref, N.bound_dx(parts, ref, D, T))
    print(f"{name} T={T} X={X}: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    # slack where the bound is all summation (the f32 forward); a store's own rounding — 16 bits, or the f32 add of a dres that dwarfs
    # LN'(dy) on an outlier row — can use the half ulp the bound grants it in full
    slack = {"mean", "rstd"} | ({"y"} if T == F32 else set())
    for k, v in r.items():
        assert v < (0.5 if k in slack else 1.0), (k, r)


@pytest.mark.parametrize("name", LORA)
def test_emulated_lora_forward_stays_under_the_bf16_bounds(name):
    case, d = built(name, BF16)
    r = fwd_ratios(d, case.D, N.emulate_forward_lora(d["x"], d["gamma"], d["beta"], case.D), BF16)
    print(f"{name}: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert r["mean"] < 1.0 and r["rstd"] < 1.0 and r["y"] < 1.0, r


# ---------------------------------------------------------------------------------------------------------------- fault models
@pytest.mark.parametrize("fault", [N.fault_dropped_element, N.fault_inv_d], ids=lambda f: f.__name__)
@pytest.mark.parametrize("name", PLAIN)
def test_a_wrong_mean_exceeds_the_bounds(name, fault):
    case, d = built(name)
    r = fwd_ratios(d, case.D, fault(d, case.D), F32)
    assert r["mean"] > 1.0 and r["y"] > 1.0, r
    r16 = fwd_ratios(d, case.D, fault(d, case.D), BF16)      # the widest bound any test uses
    assert r16["mean"] > 1.0 and (r16["y"] > 1.0 or r16["rstd"] > 1.0), r16


@pytest.mark.parametrize("placement", ["colblock", "cls"])
@pytest.mark.parametrize("name", [n for n in PLAIN if 1 < N.BY_NAME[n].M <= 37])
def test_a_row_read_at_stride_d_exceeds_the_bounds(name, placement):
    case, d = built(name)
    M, D = case.M, case.D
    kw = dict(ld=D + 64, col0=8, pad_rows=1) if placement == "colblock" else dict(ld=D, row_step=N.CLS_T)
    b = Banded((M, D), F32, d["x"], device="cpu", **kw)
    assert torch.equal(b.view, d["x"])
    x_bad = N.fault_row_stride(b.buf, BAND + b.col0, M, D)
    assert torch.equal(x_bad[0], d["x"][0])
    r = fwd_ratios(d, D, N.emulate_forward(x_bad, d["gamma"], d["beta"], D), F32)
    assert r["mean"] > 1.0 and r["y"] > 1.0, r


@pytest.mark.parametrize("name", [c.name for c in N.TABLE if c.kind == "trip2"])
def test_a_skipped_second_trip_leaves_the_sentinel_and_misses_gmax(name):
    case = N.BY_NAME[name]
    d = N.make(case)
    M, D = case.M, case.D
    y = N.emulate_forward(d["x"], d["gamma"], d["beta"], D)[2]
    out = Banded((M, D), F32, device="cpu")
    sent = torch.tensor([SENTINEL[4][1]], dtype=torch.int32).view(F32)
    out.view.copy_(N.fault_trip_skipped(y, sent))
    assert out.unwritten() == 5 * D and out.bands_intact()
    mean64, rstd64, y64 = N.forward(d["x"], d["gamma"], d["beta"])
    assert N.ratio(out.view, y64, N.bound_y(d["x"], d["gamma"], rstd64, y64, D, BF16)) > 1.0
    dy = d["dy"].clone()
    dy[N.ROWS_PER_TRIP + 2, 5] = 1000.0
    dx = N.backward(dy, d["x"], d["gamma"], mean64, rstd64)
    assert N.fault_gmax_first_trip(dy, dx) < N.gmax_reference(dy, dx)


@pytest.mark.parametrize("name", ["d128_m37", "d256_m37"])
def test_dres_on_every_row_of_the_compact_form_exceeds_the_bound(name):
    case, d = built(name)
    M, D, T = case.M, case.D, N.CLS_T
    mean64, rstd64, _ = N.forward(d["x"], d["gamma"], d["beta"])
    dres_c = d["dres"][:(M + T - 1) // T]
    ref, parts = N.backward(d["dy"], d["x"], d["gamma"], mean64, rstd64, N.expand_compact(dres_c, M, T), parts=True)
    bad = N.fault_dres_every_row(N.backward(d["dy"], d["x"], d["gamma"], mean64, rstd64), dres_c, T)
    assert N.ratio(bad, ref, N.bound_dx(parts, ref, D, BF16)) > 1.0
    assert N.ratio(ref, ref, N.bound_dx(parts, ref, D, F32)) == 0.0


@pytest.mark.parametrize("name", ["d128_m37", "d512_m37"])
def test_the_dropout_counter_of_dense_rows_breaks_the_strided_copy(name):
    case, d = built(name)
    M, D, T = case.M, case.D, N.CLS_T
    flat = N.dropout_keep(M * T * D, N.P_DROP, 3, 9)
    keep, bad = N.keep_rows(flat, M, D, T * D), N.fault_drop_counter(flat, M, D)
    mean64, rstd64, _ = N.forward(d["x"], d["gamma"], d["beta"])
    dx, parts = N.backward(d["dy"], d["x"], d["gamma"], mean64, rstd64, parts=True)
    ref, got = N.dropout_copy(dx, keep), N.dropout_copy(dx, bad)
    assert torch.equal(keep[0], bad[0]) and not torch.equal(keep, bad)
    assert (got[keep == 0] != 0).any()                                            # a dropped element that is not exactly zero
    assert N.ratio(got, ref, N.bound_dx(parts, ref, D, BF16, scale=2.0)) > 1.0


@pytest.mark.parametrize("T,S,X", [t for t in N.BWD_INSTANCES if t[1] != t[2]], ids=str)
@pytest.mark.parametrize("name", ["inst_d128", "inst_d256"])
def test_swapped_stream_and_x_casts_exceed_the_bound(name, T, S, X):
    case, d = built(name, X)
    M, D = case.M, case.D
    mean64, rstd64, _ = N.forward(d["x"], d["gamma"], d["beta"])
    dy, dres = d["dy"].to(T).float(), d["dres"].to(S).float()
    ref, parts = N.backward(dy, d["x"], d["gamma"], mean64, rstd64, dres, parts=True)
    x_bad, dres_bad = N.fault_swapped_casts(d["x"].to(X), d["dres"].to(S), M, D, X, S)
    bad = N.backward(dy, x_bad, d["gamma"], mean64, rstd64, dres_bad)
    assert N.ratio(bad, ref, N.bound_dx(parts, ref, D, BF16)) > 1.0


# ---------------------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("D", [64, 128, 512, 768])
def test_dropout_copy_reference_is_what_the_op_tests_expect(D):
    """tests/test_hip_ops.py test_layernorm: dxb == grad * keep * 2 with keep = dropout_mask(M * D).reshape(M, D), M = 37, seed 3, site 9;
    test_layernorm_bwd_strided_inplace: keep = dropout_mask(B T D).view(B, T, D)[:, 0] at (B, T, D) = (5, 7, 128)."""
    M = 37
    dx = torch.randn(M, D, generator=torch.Generator().manual_seed(D)).double()
    flat = N.dropout_keep(M * D, 0.5, 3, 9)
    assert torch.equal(N.dropout_copy(dx, N.keep_rows(flat, M, D, D)), dx * flat.reshape(M, D).double() * 2)
    assert 0.4 < flat.float().mean() < 0.6
    B, T, D2 = 5, 7, 128
    flat = N.dropout_keep(B * T * D2, 0.5, 3, 9)
    assert torch.equal(N.keep_rows(flat, B, D2, T * D2), flat.view(B, T, D2)[:, 0])


def test_instantiation_lists_are_what_the_argument_checks_accept():
    types = (F32, BF16, F16)
    okx = lambda T, X: X == F32 or (X in (BF16, F16) and T == BF16) or (X == F16 and T == F16)
    fwd = {(T, X) for T, X in itertools.product(types, types) if okx(T, X)}
    bwd = {(T, S, X) for T, S, X in itertools.product(types, types, types) if okx(T, X) and (S == F32 or (S == T and T != F32))}
    assert len(N.FWD_INSTANCES) == 6 and set(N.FWD_INSTANCES) == fwd
    assert len(N.BWD_INSTANCES) == 11 and set(N.BWD_INSTANCES) == bwd


def test_table_reaches_what_it_is_named_for():
    assert {c.D for c in N.TABLE if c.kind == "small"} == set(N.WIDTHS) and all(N.npl(D) * 64 == D for D in N.WIDTHS)
    assert all(c.M > N.ROWS_PER_TRIP for c in N.TABLE if c.kind == "trip2")
    assert N.BY_NAME["lora_trip2"].M > N.LORA_ROWS_PER_TRIP
    d = N.make(N.BY_NAME["d64_m37"])
    assert (d["x"][3] == 3.0).all() and (d["x"][4] == torch.tensor(-1234.567)).all() and d["x"][6].abs().max() > 100
    h = N.make(N.BY_NAME["d64_m37"], F16)["x"]
    assert torch.equal(h, h.half().float()) and not torch.equal(h, d["x"])
