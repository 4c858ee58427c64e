"""Probes, references, bounds and fault models of the evaluation kernels: csrc/verif.hip (gsl_verif_pair_dist, gsl_verif_fold_counts,
gsl_verif_select) and csrc/classstat.hip (gsl_class_stats, gsl_class_embed_sum). tests/test_eval_probes_host.py on the CPU,
tests/test_hip_eval_edges.py on the device, tests/test_verification_host.py for the two count models against the recorded reference.

Fold counts and selection are integer arithmetic followed by IEEE f64 divisions: the models give the kernels' outputs bit for bit.
  counts_model / select_model      the kernels' own algorithm in numpy (per-fold integer counts; train counts = totals minus the fold's;
                                   first arg-max of the integer train numerator)
  roc_restatement                  the reference's calculate_roc a second way: boolean masks of the train and test pairs, FLOAT accuracies
                                   per threshold, np.argmax, np.mean over the folds. It shares only V.fold_bounds with the models.
  fault models                     counts_fault(): a fold boundary one pair late, <= for <, the pairs of a fold behind its last whole chunk
                                   of CHUNK dropped; select_model(last_argmax=True).

Pair distances are f32 sums: a per-pair bound against float64, from the kernel's operation order (verif_pair_dist_kernel). With
e = 2^-24, n = ceil(D / 64) elements per lane and 6 butterfly levels:
  s = e0 + e1                      one rounding: e |s|
  ||s||                            n products of s (2 e each from s, e their own), n - 1 adds, 6 levels, all terms >= 0: (n + 8) e relative
                                   on the sum of squares; the square root halves it and adds its own e
  nemb = s / ||s||                 rho = ((n + 8) / 2 + 3) e relative: s, the norm, the division          -> bound_nemb
  df = n0 - n1                     delta = rho (|n0| + |n1|) + e |df|
  dist = sum df^2                  sum (2 |df| delta + delta^2) + (n + 7) e dist: the squares' roundings, n - 1 adds, 6 levels
                                   -> bound_dist; in plain mode the rows are given: delta = e |df|
  pair_norm                        four norms of given rows ((n + 6) / 2 + 1) e each, three adds: ((n + 6) / 2 + 4) e relative
  xnorm                            the f64 sum of the f32 pair norms over 4 P, rounded to f32: one more e               -> bound_xnorm
A zero row and a row with e0 = -e1 give s = 0 exactly, norm 0 -> 1, nemb = 0 exactly. emulate_pair_dist() restates the kernel in f32
torch in its lane and summation order; fault_tail_columns() / fault_row_stride() are the two fault models.

Class statistics are integers (class_stats_ref: torch.max's first arg-max, NaN highest); the class embedding sums are sequential f32
adds in row order (embed_sum_ref), bit for bit."""
import numpy as np
import torch

from oracle.norm_probes import _seq, _wave_sum, ratio      # noqa: F401  (the xor butterfly and the ratio rule are the LayerNorm probes')

E = 2.0 ** -24
CHUNK = 4096             # csrc/verif.hip VERIF_CHUNK
CSUM_CHUNK = 1024        # csrc/classstat.hip

FOLD_CASES = ((8195, 2), (12289, 3), (7, 7), (603, 10))      # (P, F)
TNS = (1, 255, 256, 257, 400)
DIST_D = (1, 63, 64, 65, 130, 1024)
DIST_P = (1, 3, 4, 5, 9)
DIST_EXTRA = ((300, 8),)                                     # (P, D): the strided f64 partials of verif_xnorm_kernel


# ---------------------------------------------------------------------------------------------------------------- fold counts, selection
def counts_model(dist32, issame, thresholds, F):
    """gsl_verif_fold_counts in numpy: (counts [F, Tn, 2], fold_tot [F, 2])."""
    from util import verification as V
    d = dist32.astype(np.float32).astype(np.float64)
    same = issame.astype(bool)
    counts, tot = np.zeros((F, len(thresholds), 2), np.int64), np.zeros((F, 2), np.int64)
    for f, (a, b) in enumerate(V.fold_bounds(len(d), F)):
        acc = d[a:b, None] < np.asarray(thresholds)[None, :]
        counts[f, :, 0] = (acc & same[a:b, None]).sum(0)
        counts[f, :, 1] = (acc & ~same[a:b, None]).sum(0)
        tot[f] = same[a:b].sum(), (~same[a:b]).sum()
    return counts, tot


def select_model(counts, tot, thresholds, last_argmax=False):
    """gsl_verif_select in numpy: accuracy [F], best_thresholds [F], tpr [Tn], fpr [Tn]. last_argmax: the fault model."""
    F, Tn = counts.shape[:2]
    acc, best = np.zeros(F), np.zeros(F)
    all_c, all_d = counts.sum(0), tot[:, 1].sum()
    for f in range(F):
        tr = all_c - counts[f]
        num = tr[:, 0] + (all_d - tot[f, 1]) - tr[:, 1]
        bi = int(np.argmax(num))      # first maximum
        if last_argmax:
            bi = Tn - 1 - int(np.argmax(num[::-1]))
        best[f] = thresholds[bi]
        acc[f] = float(counts[f, bi, 0] + tot[f, 1] - counts[f, bi, 1]) / float(tot[f].sum())
    tpr, fpr = np.zeros(Tn), np.zeros(Tn)
    for f in range(F):      # fold order, as np.mean(axis=0) adds the rows
        tpr += 0.0 if tot[f, 0] == 0 else counts[f, :, 0].astype(np.float64) / float(tot[f, 0])
        fpr += 0.0 if tot[f, 1] == 0 else counts[f, :, 1].astype(np.float64) / float(tot[f, 1])
    return acc, best, tpr / F, fpr / F


def roc_restatement(dist32, issame, thresholds, F):
    """accuracy [F], best_thresholds [F], tpr [Tn], fpr [Tn] by the reference's own route: per fold a boolean train / test split of all
    pairs, per threshold the float train accuracy over the whole train set, np.argmax, the test rates at every threshold and the test
    accuracy at the chosen one, np.mean over the folds."""
    from util import verification as V
    dist = np.asarray(dist32, np.float32).astype(np.float64)
    actual = np.asarray(issame) != 0
    thresholds = np.asarray(thresholds, np.float64)
    P, Tn = len(dist), len(thresholds)

    def rates(thr, d, a):
        said = np.less(d, thr)
        tp, fp = np.sum(said & a), np.sum(said & ~a)
        tn, fn = np.sum(~said & ~a), np.sum(~said & a)
        tpr = 0.0 if tp + fn == 0 else float(tp) / float(tp + fn)
        fpr = 0.0 if fp + tn == 0 else float(fp) / float(fp + tn)
        return tpr, fpr, float(tp + tn) / d.size

    tprs, fprs, acc, best = np.zeros((F, Tn)), np.zeros((F, Tn)), np.zeros(F), np.zeros(F)
    for f, (a, b) in enumerate(V.fold_bounds(P, F)):
        test = np.zeros(P, bool)
        test[a:b] = True
        train_acc = np.array([rates(t, dist[~test], actual[~test])[2] for t in thresholds])
        bi = np.argmax(train_acc)
        for i, t in enumerate(thresholds):
            tprs[f, i], fprs[f, i], _ = rates(t, dist[test], actual[test])
        best[f] = thresholds[bi]
        acc[f] = rates(thresholds[bi], dist[test], actual[test])[2]
    return acc, best, np.mean(tprs, 0), np.mean(fprs, 0)


def counts_fault(dist32, issame, thresholds, F, fault):
    """counts_model with one fault: "bound_late" (every fold boundary but the ends one pair late), "le" (<= for <), "chunk_tail" (the pairs
    of a fold behind its last whole CHUNK are never staged)."""
    from util import verification as V
    d = np.asarray(dist32, np.float32).astype(np.float64)
    same = np.asarray(issame) != 0
    thr = np.asarray(thresholds)[None, :]
    P = len(d)
    counts, tot = np.zeros((F, len(thresholds), 2), np.int64), np.zeros((F, 2), np.int64)
    for f, (a, b) in enumerate(V.fold_bounds(P, F)):
        if fault == "bound_late":
            a, b = a + (a > 0), b + (b < P)
        tot[f] = same[a:b].sum(), (~same[a:b]).sum()
        if fault == "chunk_tail" and b - a > CHUNK:
            b = a + (b - a) // CHUNK * CHUNK
        acc = (d[a:b, None] <= thr) if fault == "le" else (d[a:b, None] < thr)
        counts[f, :, 0] = (acc & same[a:b, None]).sum(0)
        counts[f, :, 1] = (acc & ~same[a:b, None]).sum(0)
    return counts, tot


def thresholds_of(Tn, order, seed=0):
    """Tn f64 thresholds: 0.25, 0.5, np.float32(0.01) and its two f32 neighbours (as far as Tn goes), the rest a grid over [0, 4); one
    duplicate (the last entry repeats the first) when Tn > 1. order: "sorted" or "shuffled"."""
    c = np.float32(0.01)
    special = [0.25, 0.5, float(c), float(np.nextafter(c, np.float32(0))), float(np.nextafter(c, np.float32(1)))][:Tn]
    rest = Tn - len(special)
    thr = np.array(special + list(np.arange(rest) * (4.0 / max(rest, 1)) + 0.003), np.float64)
    if Tn > 1:
        thr[-1] = thr[0]
    thr = np.sort(thr)
    if order == "shuffled":
        thr = thr[np.random.RandomState(seed + Tn).permutation(Tn)]
    return thr


def fold_inputs(P, F, seed=0):
    """(dist f32 [P], issame uint8 [P]): distances over [0, 4) with NaN, +Inf, and values exactly equal to thresholds_of()'s specials
    spread over every fold (both chunks of a long fold); issame bytes 0, 1, 2 and 255."""
    r = np.random.RandomState(1000 * P + F + seed)
    d = (r.rand(P) * 4.0).astype(np.float32)
    c = np.float32(0.01)
    special = np.array([0.25, 0.5, c, np.nextafter(c, np.float32(0)), np.nextafter(c, np.float32(1)), np.nan, np.inf], np.float32)
    at = r.permutation(P)[:max(P // 3, min(P, len(special)))]
    d[at] = special[np.arange(len(at)) % len(special)]
    d[-1] = 0.25                                           # the last pair of the last fold (the tail of its last chunk)
    same = np.array([0, 1, 2, 255], np.uint8)[r.randint(0, 4, P)]
    return d, same


def select_tables(F, Tn=400, at=(44, 45, 300)):
    """Hand-built (counts [F, Tn, 2], fold_tot [F, 2]) whose train numerator has its maximum exactly at `at` in every fold: 44 and 300
    belong to one thread of verif_select_kernel (stride 256), 45 to its neighbour; the first must win. F = 3: fold 1 holds no same pair,
    fold 2 no different pair."""
    S = np.zeros(Tn, np.int64)
    S[list(at)] = 1
    counts, tot = np.zeros((F, Tn, 2), np.int64), np.zeros((F, 2), np.int64)
    if F == 2:
        tot[:] = (9, 8)
        counts[0, :, 0], counts[0, :, 1] = 5 + 3 * S, 2
        counts[1, :, 0], counts[1, :, 1] = 4, 6 - 2 * S
    else:
        assert F == 3
        tot[0], tot[1], tot[2] = (9, 8), (0, 10), (6, 0)
        counts[0, :, 0], counts[0, :, 1] = 5 + 3 * S, 2
        counts[1, :, 1] = 7 - 2 * S
        counts[2, :, 0] = 4 + S
    return counts, tot


# ---------------------------------------------------------------------------------------------------------------- pair distances
def npl(D):
    return -(-D // 64)


def pair_inputs(P, D, seed=0):
    """e0, e1 f32 [2P, D] ~ N(0, 1) with rows scaled 1, 30, 1/30 in turn; from P = 3 on row 2 of e0 and e1 is zero and e1 = -e0 on the last
    row (pairs 1 and P - 1 hold a zero normalised row each; P = 1 has its one pair ordinary)."""
    g = torch.Generator().manual_seed(7919 * P + D + seed)
    scale = torch.tensor([1.0, 30.0, 1.0 / 30.0])[torch.arange(2 * P) % 3][:, None]
    e0, e1 = torch.randn(2 * P, D, generator=g) * scale, torch.randn(2 * P, D, generator=g) * scale
    if P >= 3:
        e0[2], e1[2] = 0.0, 0.0
        e1[-1] = -e0[-1]
    return e0, e1


def pair_dist_ref(e0, e1, plain=False):
    """float64: (dist [P], nemb [2P, D] or None, pair_norm [P] or None, xnorm or None)."""
    a, b = e0.double(), e1.double()
    if plain:
        return ((a - b) ** 2).sum(1), None, None, None
    s = a + b
    nrm = s.norm(dim=1, keepdim=True)
    n = s / torch.where(nrm == 0, torch.ones_like(nrm), nrm)
    rown = a.norm(dim=1) + b.norm(dim=1)
    pn = rown[0::2] + rown[1::2]
    return ((n[0::2] - n[1::2]) ** 2).sum(1), n, pn, pn.sum() / (4 * pn.numel())


def rho(D):
    return ((npl(D) + 8) / 2 + 3) * E


def bound_nemb(nemb64, D):
    return rho(D) * nemb64.abs()


def bound_dist(n0, n1, D, plain=False):
    """n0, n1 float64 [P, D]: the two rows of every pair (normalised ones in flip-sum mode, the given ones in plain mode)."""
    df = (n0 - n1).abs()
    delta = E * df if plain else rho(D) * (n0.abs() + n1.abs()) + E * df
    return (2 * df * delta + delta * delta).sum(1) + (npl(D) + 7) * E * (df * df).sum(1)


def bound_pair_norm(pn64, D):
    return ((npl(D) + 6) / 2 + 4) * E * pn64


def bound_xnorm(xn64, D):
    return ((npl(D) + 6) / 2 + 5) * E * xn64


def _lanes(t):
    """[R, D] -> [R, n, 64]: [.., v, lane] = column lane + 64 v, zeros behind D."""
    R, D = t.shape
    n = npl(D)
    return torch.cat([t.float(), torch.zeros(R, n * 64 - D)], 1).view(R, n, 64)


def emulate_pair_dist(e0, e1, plain=False):
    """verif_pair_dist_kernel (+ verif_xnorm_kernel) in f32 torch: (dist, nemb, pair_norm, xnorm), the last three None in plain mode."""
    D = e0.shape[1]
    a, b = _lanes(e0), _lanes(e1)
    if plain:
        df = a - b
        return _wave_sum(_seq(df * df)), None, None, None
    t = a + b
    na, nb, ns = (torch.sqrt(_wave_sum(_seq(v * v))) for v in (a, b, t))
    n = t / torch.where(ns == 0, torch.ones_like(ns), ns)[:, None, None]
    pn = ((na[0::2] + nb[0::2]) + na[1::2]) + nb[1::2]
    df = n[0::2] - n[1::2]
    xn = (pn.double().sum() / (4.0 * pn.numel())).float()
    return _wave_sum(_seq(df * df)), n.reshape(n.shape[0], -1)[:, :D], pn, xn


def fault_tail_columns(e0, e1):
    """The columns behind the last whole 64 dropped (a loop over D / 64 whole passes)."""
    D = e0.shape[1]
    keep = D // 64 * 64
    e0, e1 = e0.clone(), e1.clone()
    e0[:, keep:], e1[:, keep:] = 0.0, 0.0
    return e0, e1


def fault_row_stride(buf, first, rows, D):
    """Row m read at first + m D of the flat buffer that holds the rows ld apart."""
    return buf.as_strided((rows, D), (D, 1), first)


# ---------------------------------------------------------------------------------------------------------------- class statistics
def class_stats_ref(logits, labels, C):
    """(count [C], hit [C], confusion [C, C], bad) of one batch: torch.max's first arg-max (NaN highest), labels outside [0, C) in bad."""
    pred = torch.max(logits, 1)[1]
    ok = (labels >= 0) & (labels < C)
    y, p = labels[ok], pred[ok]
    return (torch.bincount(y, minlength=C), torch.bincount(y[p == y], minlength=C), torch.bincount(y * C + p, minlength=C * C).view(C, C),
            int((~ok).sum()))


def embed_sum_ref(sums, count, emb, labels):
    """One f32 row add per sample with a label in [0, C), in sample order, on top of sums / count. Returns the skipped rows."""
    C, bad = sums.shape[0], 0
    for e, c in zip(emb, labels.tolist()):
        if 0 <= c < C:
            sums[c] += e
            count[c] += 1
        else:
            bad += 1
    return bad


def embed_labels(B, C, cls, seed=0):
    """int64 labels [B] over [0, C), C >= 2: class `cls` exactly on rows 1022 .. 1025 (as far as B goes: the rows around the first
    CSUM_CHUNK boundary), the other rows on the other classes; rows 3, 7 and 11 (as far as B goes) hold -1, C and 2^32 + 3."""
    r = np.random.RandomState(B + C + seed)
    other = np.array([c for c in range(C) if c != cls])
    y = other[r.randint(0, len(other), B)]
    y[[i for i in (1022, 1023, 1024, 1025) if i < B]] = cls
    for i, v in ((3, -1), (7, C), (11, 2 ** 32 + 3)):
        if i < B - 1:
            y[i] = v
    return torch.from_numpy(y.astype(np.int64))
