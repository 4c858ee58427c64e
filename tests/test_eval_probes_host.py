"""The evaluation probes of oracle/eval_probes.py, checked on the CPU for the cases tests/test_hip_eval_edges.py runs:

(a) the two restatements of calculate_roc — the kernels' integer algorithm (counts_model + select_model) and the float-accuracy route
    (roc_restatement) — agree bit for bit on every (P, F) x Tn x threshold order, and each of the fault models differs from them: a
    fold boundary one pair late, <= for <, the last arg-max for the first, a chunk's tail dropped;
(b) the inputs hold what the device test relies on (NaN, +Inf, distances equal to a threshold, the four issame bytes, a duplicate
    threshold, tied train maxima at 44, 45 and 300 in the hand-built tables);
(c) an f32 restatement of verif_pair_dist_kernel in its lane and summation order stays under the bounds of E.bound_*, and the two
    fault models (the columns behind the last whole 64 dropped, rows read D apart where ld was passed) exceed them. The largest
    ratios are printed (pytest -s) and recorded in profiles/eval_kernel_tests.md;
(d) the class-statistics references on the label sets of the device test.

Pure torch / numpy: no GPU and no library."""
import numpy as np
import pytest
import torch

from oracle import eval_probes as E


def same_bits(a, b):
    return a.dtype == b.dtype == np.float64 and a.tobytes() == b.tobytes()


def both(d, same, thr, F):
    c, t = E.counts_model(d, same, thr, F)
    return E.select_model(c, t, thr), E.roc_restatement(d, same, thr, F)


@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("Tn", E.TNS)
@pytest.mark.parametrize("P,F", E.FOLD_CASES)
def test_the_two_restatements_agree_bit_for_bit(P, F, Tn, order):
    d, same = E.fold_inputs(P, F)
    thr = E.thresholds_of(Tn, order)
    a, b = both(d, same, thr, F)
    for x, y, name in zip(a, b, ("accuracy", "best", "tpr", "fpr")):
        assert same_bits(x, y), (name, P, F, Tn, order)


def test_the_fold_inputs_hold_their_edges():
    for P, F in E.FOLD_CASES:
        d, same = E.fold_inputs(P, F)
        assert np.isnan(d).any() and np.isinf(d).any() and d.dtype == np.float32 and same.dtype == np.uint8
        assert set(same.tolist()) == {0, 1, 2, 255} or P < 12
        for Tn in E.TNS:
            for order in ("sorted", "shuffled"):
                thr = E.thresholds_of(Tn, order)
                assert len(thr) == Tn and thr.dtype == np.float64 and (Tn == 1 or len(set(thr.tolist())) == Tn - 1)
                assert (d.astype(np.float64)[:, None] == thr[None, :]).any()
                if Tn > 5:
                    c = np.float32(0.01)
                    assert {0.25, 0.5, float(c), float(np.nextafter(c, np.float32(0))), float(np.nextafter(c, np.float32(1)))} <= set(thr.tolist())
        assert (np.sort(E.thresholds_of(400, "shuffled")) == E.thresholds_of(400, "sorted")).all()
        assert (E.thresholds_of(400, "shuffled") != E.thresholds_of(400, "sorted")).any()
    from util import verification as V
    assert [b - a for a, b in V.fold_bounds(8195, 2)] == [4098, 4097] and [b - a for a, b in V.fold_bounds(12289, 3)] == [4097, 4096, 4096]


@pytest.mark.parametrize("fault,P,F", [("bound_late", 8195, 2), ("bound_late", 603, 10), ("le", 7, 7), ("le", 603, 10), ("le", 8195, 2),
                                       ("chunk_tail", 8195, 2), ("chunk_tail", 12289, 3)])
def test_count_fault_models_differ(fault, P, F):
    d, same = E.fold_inputs(P, F)
    thr = E.thresholds_of(400, "sorted")
    c, t = E.counts_model(d, same, thr, F)
    cf, tf = E.counts_fault(d, same, thr, F, fault)
    assert not (np.array_equal(c, cf) and np.array_equal(t, tf)), (fault, P, F)
    assert any(not same_bits(x, y) for x, y in zip(E.select_model(c, t, thr), E.select_model(cf, tf, thr)))
    if fault == "chunk_tail":      # the pairs behind a fold's first 4096: 2 and 1 of them, and 1, 0, 0
        assert (c - cf).sum() > 0 and np.array_equal(t, tf)


@pytest.mark.parametrize("F", [2, 3])
def test_hand_built_tables_tie_at_44_45_300_and_the_first_wins(F):
    counts, tot = E.select_tables(F)
    thr = E.thresholds_of(400, "shuffled")
    for f in range(F):
        tr = counts.sum(0) - counts[f]
        num = tr[:, 0] + (tot[:, 1].sum() - tot[f, 1]) - tr[:, 1]
        assert np.flatnonzero(num == num.max()).tolist() == [44, 45, 300]
    assert (counts[:, :, 0] <= tot[:, None, 0]).all() and (counts[:, :, 1] <= tot[:, None, 1]).all() and (counts >= 0).all()
    if F == 3:
        assert tot[1, 0] == 0 and tot[2, 1] == 0
    acc, best, tpr, fpr = E.select_model(counts, tot, thr)
    assert (best == thr[44]).all() and thr[44] != thr[45] and thr[44] != thr[300]
    assert (E.select_model(counts, tot, thr, last_argmax=True)[1] == thr[300]).all()


# ---------------------------------------------------------------------------------------------------------------- pair distances
DIST_CASES = [(P, D) for D in E.DIST_D for P in E.DIST_P] + list(E.DIST_EXTRA)


def dist_ratios(e0, e1, out, plain, D):
    dist64, n64, pn64, xn64 = E.pair_dist_ref(e0, e1, plain)
    dist, nemb, pn, xn = out
    if plain:
        return dict(dist=E.ratio(dist, dist64, E.bound_dist(e0.double(), e1.double(), D, plain=True)))
    return dict(dist=E.ratio(dist, dist64, E.bound_dist(n64[0::2], n64[1::2], D)), nemb=E.ratio(nemb, n64, E.bound_nemb(n64, D)),
                pair_norm=E.ratio(pn, pn64, E.bound_pair_norm(pn64, D)),
                xnorm=E.ratio(xn.reshape(1), xn64.reshape(1), E.bound_xnorm(xn64, D).reshape(1)))


@pytest.mark.parametrize("P,D", DIST_CASES)
def test_emulated_pair_distances_stay_under_the_bounds(P, D):
    e0, e1 = E.pair_inputs(P, D)
    r = dist_ratios(e0, e1, E.emulate_pair_dist(e0, e1), False, D)
    r["plain"] = dist_ratios(e0[:P], e1[:P], E.emulate_pair_dist(e0[:P], e1[:P], plain=True), True, D)["dist"]      # the rows the device test takes
    dist, nemb, _, _ = E.emulate_pair_dist(e0, e1)
    assert torch.equal(E.emulate_pair_dist(nemb[0::2], nemb[1::2], plain=True)[0], dist)      # the plain form on nemb: the same bits
    if P >= 3:
        assert not nemb[2].any() and not nemb[-1].any()
    print(f"HOST P={P} D={D}: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    for k, v in r.items():
        assert v < 0.5, (k, r)            # worst-case linear counts: a correct kernel uses less than half


@pytest.mark.parametrize("P,D", [(P, D) for P, D in DIST_CASES if D % 64 and D > 64 or D in (1, 63)])
def test_dropped_tail_columns_exceed_the_bound(P, D):
    e0, e1 = E.pair_inputs(P, D)
    r = dist_ratios(e0, e1, E.emulate_pair_dist(*E.fault_tail_columns(e0, e1)), False, D)
    assert r["dist"] > 1.0 or r["nemb"] > 1.0, r
    assert r["pair_norm"] > 1.0 and r["xnorm"] > 1.0
    if P > 1 or D > 1:      # (P = 1, D = 1: the plain pair may be a - a = 0)
        a, b = E.fault_tail_columns(e0[0::2], e1[0::2])
        assert dist_ratios(e0[0::2], e1[0::2], E.emulate_pair_dist(a, b, plain=True), True, D)["dist"] > 1.0


@pytest.mark.parametrize("P,D", [(3, 64), (5, 65), (9, 1), (4, 1024)])
def test_rows_read_at_stride_d_exceed_the_bound(P, D):
    e0, e1 = E.pair_inputs(P, D)
    ld = D + 24

    def placed(t):
        buf = torch.full((t.shape[0] * ld + 8,), float("nan"))
        buf.as_strided(t.shape, (ld, 1), 8).copy_(t)
        return E.fault_row_stride(buf, 8, t.shape[0], D)
    r = dist_ratios(e0, e1, E.emulate_pair_dist(placed(e0), placed(e1)), False, D)
    assert r["dist"] > 1.0 and r["nemb"] > 1.0 and r["xnorm"] > 1.0, r


# ---------------------------------------------------------------------------------------------------------------- class statistics
def test_embed_labels_and_the_sequential_sum():
    for B in (1024, 1025, 2049):
        y = E.embed_labels(B, 5, cls=2)
        assert np.flatnonzero((y == 2).numpy()).tolist() == [i for i in (1022, 1023, 1024, 1025) if i < B]
        assert y[3] == -1 and y[7] == 5 and y[11] == 2 ** 32 + 3 and y.dtype == torch.int64
        sums, cnt = torch.zeros(5, 3), torch.zeros(5, dtype=torch.long)
        emb = torch.randn(B, 3, generator=torch.Generator().manual_seed(B))
        assert E.embed_sum_ref(sums, cnt, emb, y) == 3 and int(cnt.sum()) == B - 3 and int(cnt[2]) == min(4, B - 1022)
        want = torch.zeros(3)
        for i in np.flatnonzero((y == 2).numpy()):
            want += emb[i]
        assert torch.equal(sums[2], want)
    lo = torch.tensor([[1.0, float("nan"), 3.0], [2.0, 2.0, 1.0], [0.0, 1.0, 5.0]])
    cnt, hit, conf, bad = E.class_stats_ref(lo, torch.tensor([1, 0, 7]), 3)
    assert cnt.tolist() == [1, 1, 0] and hit.tolist() == [1, 1, 0] and bad == 1 and int(conf[1, 1]) == 1 and int(conf[0, 0]) == 1
