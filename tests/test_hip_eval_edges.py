"""The evaluation kernels at their edges, on the probes of oracle/eval_probes.py: csrc/verif.hip (gsl_verif_fold_counts, gsl_verif_select,
gsl_verif_pair_dist) and csrc/classstat.hip (gsl_class_stats, gsl_class_embed_sum), through the C ABI.

Every tensor a kernel reads sits between bands (NaN for floats, 0x5A bytes, 0x5A5A... integers: a leaked issame byte is a "same", a leaked
label is out of range, a leaked logit ranks highest) and every output in a sentinel buffer (tests/guard_bands.py): bands intact, inputs
unchanged, no output element left unwritten; the counters and sums a kernel accumulates into are checked with outside_intact().

Paths reached.
 * Fold counts: folds of 4098 / 4097 and 4097 / 4096 / 4096 pairs (a second trip of the VERIF_CHUNK = 4096 staging loop holding 2, 1
   and 1 pairs), P = F, the ragged 603 / 10; Tn = 1, 255, 256, 257, 400 (one and two workgroups of thresholds); thresholds sorted and
   shuffled with a duplicate; distances that are NaN, +Inf and exactly equal to a threshold (0.25, 0.5, np.float32(0.01) and its f32
   neighbours); issame bytes 0, 1, 2, 255. Integer-exact against E.counts_model, f64 bit-exact against E.select_model
   (tests/test_eval_probes_host.py holds both against a second restatement of calculate_roc and shows the fault models differ).
 * Select on hand-built tables: train maxima tied at t = 44, 45 and 300 (inside one thread's stride and across threads; the first must
   win), a fold without a same pair, one without a different pair, F = 2.
 * Pair distances: D = 1, 63, 64, 65, 130, 1024 x P = 1, 3, 4, 5, 9 and P = 300, D = 8 (the strided f64 partials of the xnorm kernel), both
   modes, ld = D and a column block at offset 8 of rows D + 24 long, a zero row and an e0 = -e1 row, nemb on and off. Held per pair to
   float64 under the bounds of oracle/eval_probes.py (no tolerance of this file's own; the host test shows an f32 restatement of the
   kernel under them and the fault models above them). Each comparison prints its largest error / bound ratio (pytest -s;
   profiles/eval_kernel_tests.md). The plain mode on the written nemb gives the flip-sum distances bit for bit.
 * Class statistics: C = 1, 63, 64, 65, 129 x B = 1, 5 with the logits a column block (ld = C + 24), ties, NaN, -Inf rows and a label
   outside the classes. Class embedding sums: B = 1024, 1025, 2049 (the CSUM_CHUNK = 1024 boundary: one class sits on rows 1022 .. 1025),
   D = 255, 256, 257 (the 256-column workgroup), ld = D + 8, labels -1, C and 2^32 + 3, two calls accumulating: bit-equal to the
   sequential f32 host loop.

Findings this file was written against: none in the kernels — every case passed as written."""
import functools

import numpy as np
import pytest
import torch

from guard_bands import NAN_SENTINEL, Banded, ptr
from oracle import eval_probes as E

pytestmark = pytest.mark.gpu

F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    from gslora_hip import _lib
    return _lib.load()


def check(rc, what):
    from gslora_hip import _lib
    _lib.check(rc, what)


def stream():
    return torch.cuda.current_stream().cuda_stream


def Out32(shape):
    return Banded(shape, F32, sentinel=NAN_SENTINEL[F32])


def settled(ins, outs, rw=()):
    torch.cuda.synchronize()
    for n, b in ins.items():
        assert b.bands_intact(), ("input changed:", n)
    for n, b in outs.items():
        assert b.bands_intact(), ("a store outside", n)
        assert b.unwritten() == 0, ("unwritten elements in", n)
    for n, b in rw:
        assert b.outside_intact(), ("a store outside", n)


def under(what, got, ref, bound):
    r = E.ratio(got.cpu(), ref, bound)
    print(f"RATIO {what} {r:.3f}")
    assert r <= 1.0, (what, r)


# ---------------------------------------------------------------------------------------------------------------- fold counts, select
@functools.lru_cache(maxsize=2)
def fold_case(P, F):
    return E.fold_inputs(P, F)


@functools.lru_cache(maxsize=4)
def fold_model(P, F, Tn, order):
    d, same = fold_case(P, F)
    thr = E.thresholds_of(Tn, order)
    counts, tot = E.counts_model(d, same, thr, F)
    return thr, counts, tot, E.select_model(counts, tot, thr)


def run_select(lib, counts, tot, thr, F, Tn):
    """counts / tot: banded int32 inputs. Returns (accuracy, best, tpr, fpr) as float64 numpy."""
    xn = Banded((1,), F32, torch.tensor([1.25]))
    out = Banded((2 * F + 2 * Tn + 1,), F64)
    check(lib.gsl_verif_select(ptr(counts), ptr(tot), ptr(thr), Tn, F, ptr(xn), ptr(out), stream()), "gsl_verif_select")
    settled(dict(counts=counts, tot=tot, thr=thr, xnorm=xn), dict(out=out))
    o = out.view.cpu().numpy()
    assert o[-1] == 1.25
    return o[:F], o[F:2 * F], o[2 * F:2 * F + Tn], o[2 * F + Tn:2 * F + 2 * Tn]


@pytest.mark.parametrize("order", ["sorted", "shuffled"])
@pytest.mark.parametrize("Tn", E.TNS)
@pytest.mark.parametrize("P,F", E.FOLD_CASES)
def test_fold_counts_and_select_equal_the_model(lib, P, F, Tn, order):
    d, same = fold_case(P, F)
    thr_np, want_c, want_t, want_sel = fold_model(P, F, Tn, order)
    dist, iss = Banded((P,), F32, torch.from_numpy(d)), Banded((P,), U8, torch.from_numpy(same))
    thr = Banded((Tn,), F64, torch.from_numpy(thr_np))
    counts, tot = Banded((F * Tn * 2,), I32), Banded((F * 2,), I32)
    check(lib.gsl_verif_fold_counts(ptr(dist), ptr(iss), P, ptr(thr), Tn, F, ptr(counts), ptr(tot), stream()), "gsl_verif_fold_counts")
    settled(dict(dist=dist, issame=iss, thr=thr), dict(counts=counts, fold_tot=tot))
    got_c, got_t = counts.view.cpu().numpy().reshape(F, Tn, 2), tot.view.cpu().numpy().reshape(F, 2)
    assert np.array_equal(got_c, want_c), np.argwhere(got_c != want_c)[:4]
    assert np.array_equal(got_t, want_t)
    cin, tin = Banded((F * Tn * 2,), I32, counts.view), Banded((F * 2,), I32, tot.view)
    got = run_select(lib, cin, tin, thr, F, Tn)
    for g, w, name in zip(got, want_sel, ("accuracy", "best_thresholds", "tpr", "fpr")):
        assert g.dtype == np.float64 and g.tobytes() == w.tobytes(), (name, P, F, Tn, order)


@pytest.mark.parametrize("F", [2, 3])
def test_select_ties_and_empty_classes_on_hand_built_tables(lib, F):
    """The train numerator is maximal at t = 44, 45 and 300 in every fold: the first wins. F = 3: fold 1 has no same pair (tpr term 0),
    fold 2 no different pair (fpr term 0)."""
    Tn = 400
    c_np, t_np = E.select_tables(F, Tn)
    thr_np = E.thresholds_of(Tn, "shuffled")
    counts = Banded((F * Tn * 2,), I32, torch.from_numpy(c_np.astype(np.int32)).flatten())
    tot = Banded((F * 2,), I32, torch.from_numpy(t_np.astype(np.int32)).flatten())
    thr = Banded((Tn,), F64, torch.from_numpy(thr_np))
    got = run_select(lib, counts, tot, thr, F, Tn)
    want = E.select_model(c_np, t_np, thr_np)
    for g, w, name in zip(got, want, ("accuracy", "best_thresholds", "tpr", "fpr")):
        assert g.tobytes() == w.tobytes(), (name, F)
    assert (got[1] == thr_np[44]).all() and thr_np[44] not in (thr_np[45], thr_np[300])


# ---------------------------------------------------------------------------------------------------------------- pair distances
DIST_CASES = [(P, D) for D in E.DIST_D for P in E.DIST_P] + list(E.DIST_EXTRA)


def rows_in(t, placement, D):
    """(Banded input, ld). colblock: a column block at offset 8 of rows D + 24 long, between NaN bands."""
    if placement == "colblock":
        return Banded(t.shape, F32, t, ld=D + 24, col0=8, pad_rows=1), D + 24
    return Banded(t.shape, F32, t), D


def pair_dist(lib, a, b, P, D, placement, mode, want_nemb=False):
    from gslora_hip import _lib as L
    e0, ld = rows_in(a, placement, D)
    e1, _ = rows_in(b, placement, D)
    outs = dict(dist=Out32((P,)))
    if mode == L.VERIF_FLIP_SUM:
        outs.update(xnorm=Out32((1,)), pair_norm=Out32((P,)))
        if want_nemb:
            outs["nemb"] = Out32((2 * P, D))
    check(lib.gsl_verif_pair_dist(ptr(e0), ptr(e1), ld, P, D, mode, ptr(outs["dist"]), ptr(outs.get("xnorm")), ptr(outs.get("pair_norm")),
                                  ptr(outs.get("nemb")), stream()), "gsl_verif_pair_dist")
    settled(dict(e0=e0, e1=e1), outs)
    return outs


@pytest.mark.parametrize("placement", ["contiguous", "colblock"])
@pytest.mark.parametrize("P,D", DIST_CASES)
def test_pair_distances_stay_under_the_f64_bounds(lib, P, D, placement):
    from gslora_hip import _lib as L
    what = f"P={P} D={D} {placement}"
    e0, e1 = E.pair_inputs(P, D)
    dist64, n64, pn64, xn64 = E.pair_dist_ref(e0, e1)
    o = pair_dist(lib, e0, e1, P, D, placement, L.VERIF_FLIP_SUM, want_nemb=True)
    under(f"{what} dist", o["dist"].view, dist64, E.bound_dist(n64[0::2], n64[1::2], D))
    under(f"{what} nemb", o["nemb"].view, n64, E.bound_nemb(n64, D))
    under(f"{what} pair_norm", o["pair_norm"].view, pn64, E.bound_pair_norm(pn64, D))
    under(f"{what} xnorm", o["xnorm"].view, xn64.reshape(1), E.bound_xnorm(xn64, D).reshape(1))
    if P >= 3:
        assert not o["nemb"].view[2].any() and not o["nemb"].view[-1].any()      # the zero row and the e0 = -e1 row: exactly 0
    # nemb off: the same distances and norms
    o2 = pair_dist(lib, e0, e1, P, D, placement, L.VERIF_FLIP_SUM)
    for k in ("dist", "xnorm", "pair_norm"):
        assert torch.equal(o2[k].view, o[k].view), (what, k)
    # the plain mode on the written nemb (rows 2p against 2p + 1: row stride 2 D): the flip-sum distances bit for bit
    plain = Out32((P,))
    nemb = Banded((2 * P, D), F32, o["nemb"].view)
    check(lib.gsl_verif_pair_dist(ptr(nemb), ptr(nemb) + 4 * D, 2 * D, P, D, L.VERIF_PLAIN, ptr(plain), None, None, None, stream()),
          "gsl_verif_pair_dist")
    settled(dict(nemb=nemb), dict(dist=plain))
    assert torch.equal(plain.view, o["dist"].view), what
    # the plain mode on given rows
    a, b = e0[:P], e1[:P]
    op = pair_dist(lib, a, b, P, D, placement, L.VERIF_PLAIN)
    under(f"{what} plain", op["dist"].view, E.pair_dist_ref(a, b, plain=True)[0], E.bound_dist(a.double(), b.double(), D, plain=True))


# ---------------------------------------------------------------------------------------------------------------- class statistics
def stats_batch(B, C):
    """Logits rounded to one decimal (ties), row 1 tied between its first and last column, row 2 with a NaN in the middle below larger
    numbers, row 3 all equal, row 4 all -Inf; labels: hits on the even rows, a miss on row 1, a label outside the classes on row 3."""
    g = torch.Generator().manual_seed(100 * B + C)
    lo = (torch.randn(B, C, generator=g) * 2).mul(10).round().div(10)
    if B > 1:
        lo[1, 0] = lo[1, C - 1] = 9.0
        lo[2, C // 2] = float("nan")
        lo[3, :] = 1.0
        lo[4, :] = float("-inf")
    pred = torch.max(lo, 1)[1]
    y = pred.clone()
    if B > 1:
        y[1] = C - 1
        y[3] = C
    return lo, y


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 129])
def test_class_stats_on_a_column_block(lib, C, B):
    lo, y = stats_batch(B, C)
    logits = Banded((B, C), F32, lo, ld=C + 24, col0=8, pad_rows=1)
    labels = Banded((B,), I64, y)
    cnt, hit, bad = (Banded((n,), I64, torch.zeros(n, dtype=I64)) for n in (C, C, 1))
    conf = Banded((C * C,), I32, torch.zeros(C * C, dtype=I32))
    for _ in range(2):      # the counters persist
        check(lib.gsl_class_stats(ptr(logits), C + 24, ptr(labels), B, C, ptr(cnt), ptr(hit), ptr(bad), ptr(conf), stream()), "gsl_class_stats")
    settled(dict(logits=logits, labels=labels), {}, rw=(("count", cnt), ("hit", hit), ("bad", bad), ("confusion", conf)))
    wc, wh, wm, wb = E.class_stats_ref(lo, y, C)
    assert torch.equal(cnt.view.cpu(), 2 * wc) and torch.equal(hit.view.cpu(), 2 * wh) and int(bad.view[0]) == 2 * wb
    assert torch.equal(conf.view.cpu().long().view(C, C), 2 * wm)
    if B > 1:
        assert wb == 1 and int(wh.sum()) == (4 if C == 1 else 3) and (C == 1 or int(wm[C - 1, 0]) == 1)      # row 1: the first of the tied columns, a miss


@pytest.mark.parametrize("D", [255, 256, 257])
@pytest.mark.parametrize("B", [1024, 1025, 2049])
def test_class_embed_sum_around_the_label_chunk_and_the_column_block(lib, B, D):
    C, cls = 5, 2
    want, wcnt, wbad = torch.zeros(C, D), torch.zeros(C, dtype=I64), 0
    sums = Banded((C, D), F32, torch.zeros(C, D))
    cnt, bad = Banded((C,), I64, torch.zeros(C, dtype=I64)), Banded((1,), I64, torch.zeros(1, dtype=I64))
    for call in range(2):      # two calls accumulate into the same sum / count
        emb_t = torch.randn(B, D, generator=torch.Generator().manual_seed(B + D + call))
        y = E.embed_labels(B, C, cls, seed=call)
        emb, labels = Banded((B, D), F32, emb_t, ld=D + 8), Banded((B,), I64, y)
        check(lib.gsl_class_embed_sum(ptr(emb), D + 8, ptr(labels), B, D, C, ptr(sums), ptr(cnt), ptr(bad), stream()), "gsl_class_embed_sum")
        settled(dict(emb=emb, labels=labels), {}, rw=(("sum", sums), ("count", cnt), ("bad", bad)))
        wbad += E.embed_sum_ref(want, wcnt, emb_t, y)
        assert sums.view.cpu().numpy().tobytes() == want.numpy().tobytes(), (B, D, call)
        assert torch.equal(cnt.view.cpu(), wcnt) and int(bad.view[0]) == wbad == 3 * (call + 1)
    assert int(wcnt[cls]) == 2 * min(4, B - 1022)
