"""Pair verification (LFW-style ROC / accuracy / TAR@FAR) on the HIP path — the reference's `util/verification.py`
(calculate_roc :37-113, calculate_accuracy :116-134, calculate_val :137-184, calculate_val_far :187-195, evaluate :198-212) with the same
names, signatures and return values, on device tensors.

Every operation on more than a handful of scalars runs in libgslora_hip.so (csrc/verif.hip): the squared distances, the per-fold /
per-threshold decision counts, the first-arg-max threshold selection and the fold means. The host reads the results once. Embeddings are
torch tensors on the GPU; CPU tensors and numpy arrays raise, like every other entry of the product. `actual_issame` is a host sequence
(list / numpy, as the reference's callers pass it) or a device tensor.

What differs from the reference, on purpose:
  * `pca > 0` raises NotImplementedError (an sklearn PCA fit per fold on the host is outside the HIP path).
  * The folds are sklearn's `KFold(n_splits, shuffle=False)` restated (`fold_bounds`): contiguous, the first `P % F` folds one pair longer;
    `P < nrof_folds` (and `nrof_folds < 2`) raise ValueError as sklearn does.
  * `calculate_val`'s `interp1d(far_train, thresholds, kind="slinear")` is restated (`slinear`) instead of importing scipy. far_train
    holds repeated values on every real pair set (a few dozen distinct false-accept rates over 400 thresholds); a current scipy refuses
    them ("Expect x to not have duplicates"), so the reference's calculate_val only ran on older ones, whose order-1 B-spline is the
    rule kept here: stable sort by x; between two distinct x values the line from the LAST point of the left one to the FIRST point of the right
    one; exactly at a repeated x the last of its points (right-continuous).
"""
import numpy as np
import torch

THRESHOLDS = np.arange(0, 4, 0.01)      # evaluate's grid (:200), passed to the kernels unchanged (f64)


def fold_bounds(nrof_pairs, nrof_folds):
    """[(start, stop)] of the test folds of sklearn's KFold(n_splits=nrof_folds, shuffle=False) on nrof_pairs samples."""
    P, F = int(nrof_pairs), int(nrof_folds)
    if F < 2:
        raise ValueError(f"k-fold cross-validation requires at least one train/test split by setting n_splits=2 or more, got n_splits={F}.")
    if F > P:
        raise ValueError(f"Cannot have number of splits n_splits={F} greater than the number of samples: n_samples={P}.")
    base, rem = divmod(P, F)
    out, start = [], 0
    for f in range(F):
        stop = start + base + (1 if f < rem else 0)
        out.append((start, stop))
        start = stop
    return out


def slinear(x, y, x_new):
    """interp1d(x, y, kind="slinear")(x_new) for one x_new (see the module docstring for repeated x). ValueError outside [min x, max x],
    as interp1d's bounds_error."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    order = np.argsort(x, kind="mergesort")
    x, y = x[order], y[order]
    x_new = float(x_new)
    if x_new < x[0] or x_new > x[-1]:
        raise ValueError(f"A value ({x_new}) in x_new is outside the interpolation range [{x[0]}, {x[-1]}].")
    hi = int(np.searchsorted(x, x_new, side="right"))      # first point with x > x_new
    lo = hi - 1                                            # last point with x <= x_new
    if hi == len(x) or x[lo] == x_new:
        return float(y[lo])
    # the order-1 B-spline on the knots (x[lo], x[hi]): c0 * (x1 - t) / (x1 - x0) + c1 * (t - x0) / (x1 - x0)
    x0, x1 = x[lo], x[hi]
    return float(y[lo] * ((x1 - x_new) / (x1 - x0)) + y[hi] * ((x_new - x0) / (x1 - x0)))


def _device_f32(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"gs-lora_amd verification: {what} must be a torch tensor on a ROCm GPU; the metric runs in libgslora_hip.so "
                           "and has no CPU fallback")
    return t if t.dtype == torch.float32 else t.float()


def _issame_dev(actual_issame, device, n=None):
    if isinstance(actual_issame, torch.Tensor):
        t = actual_issame.to(device=device).ne(0).to(torch.uint8)
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(actual_issame).astype(bool).astype(np.uint8))).to(device)
    t = t.reshape(-1)
    return t.contiguous() if n is None else t[:n].contiguous()


def _thresholds_dev(thresholds, device):
    th = np.ascontiguousarray(np.atleast_1d(np.asarray(thresholds, dtype=np.float64)))
    return th, torch.from_numpy(th).to(device)


def roc_from_dist(thresholds, dist, actual_issame, nrof_folds=10, xnorm=None):
    """calculate_roc behind its distances: dist [P] f32 on the device -> (tpr [Tn], fpr [Tn], accuracy [F], best_thresholds [F], xnorm) as
    numpy f64 (xnorm a float, 0.0 if not given). Two launches and one host read."""
    from gslora_hip import ops
    dist = _device_f32(dist, "dist").contiguous()
    F = int(nrof_folds)
    fold_bounds(dist.numel(), F)      # sklearn's argument errors
    same = _issame_dev(actual_issame, dist.device, dist.numel())
    if same.numel() != dist.numel():
        raise ValueError(f"{dist.numel()} pairs but {same.numel()} issame flags")
    th, th_dev = _thresholds_dev(thresholds, dist.device)
    counts, tot = ops.verif_fold_counts(dist, same, th_dev, F)
    out = ops.verif_select(counts, tot, th_dev, xnorm).cpu().numpy()
    Tn = th.size
    return out[2 * F:2 * F + Tn], out[2 * F + Tn:2 * F + 2 * Tn], out[:F], out[F:2 * F], float(out[2 * F + 2 * Tn])


def calculate_roc(thresholds, embeddings1, embeddings2, actual_issame, nrof_folds=10, pca=0):
    """:return: tpr [Tn], fpr [Tn], accuracy [nrof_folds], best_thresholds [nrof_folds] (numpy f64), as the reference."""
    if pca != 0:
        raise NotImplementedError("gs-lora_amd verification: pca > 0 (an sklearn PCA fit per fold, on the host) is outside the HIP path")
    from gslora_hip import ops
    e1, e2 = _device_f32(embeddings1, "embeddings1"), _device_f32(embeddings2, "embeddings2")
    assert e1.shape[0] == e2.shape[0]
    assert e1.shape[1] == e2.shape[1]
    nrof_pairs = min(len(actual_issame), e1.shape[0])
    dist = ops.verif_sq_dist(e1, e2)[:nrof_pairs]
    tpr, fpr, accuracy, best_thresholds, _ = roc_from_dist(thresholds, dist, actual_issame, nrof_folds)
    return tpr, fpr, accuracy, best_thresholds


def _counts_one_fold(thresholds, dist, actual_issame):
    """(true accepts [Tn], false accepts [Tn], n_same, n_diff) of the whole set, as Python / numpy integers."""
    from gslora_hip import ops
    dist = _device_f32(dist, "dist").contiguous().reshape(-1)
    same = _issame_dev(actual_issame, dist.device)
    if same.numel() != dist.numel():
        raise ValueError(f"{dist.numel()} distances but {same.numel()} issame flags")
    _, th_dev = _thresholds_dev(thresholds, dist.device)
    counts, tot = ops.verif_fold_counts(dist, same, th_dev, 1)
    counts, tot = counts.cpu().numpy(), tot.cpu().numpy()
    return counts[0, :, 0], counts[0, :, 1], int(tot[0, 0]), int(tot[0, 1])


def calculate_accuracy(threshold, dist, actual_issame):
    """:return: tpr, fpr, acc of `dist < threshold` against actual_issame (dist: device tensor)."""
    ta, fa, n_same, n_diff = _counts_one_fold(threshold, dist, actual_issame)
    tp, fp = int(ta[0]), int(fa[0])
    fn, tn = n_same - tp, n_diff - fp
    tpr = 0 if (tp + fn == 0) else float(tp) / float(tp + fn)
    fpr = 0 if (fp + tn == 0) else float(fp) / float(fp + tn)
    acc = float(tp + tn) / (n_same + n_diff)
    return tpr, fpr, acc


def calculate_val_far(threshold, dist, actual_issame):
    """:return: val (true accept rate), far (false accept rate); a set without same or without different pairs divides by zero, as the reference."""
    ta, fa, n_same, n_diff = _counts_one_fold(threshold, dist, actual_issame)
    return float(ta[0]) / float(n_same), float(fa[0]) / float(n_diff)


def far_thresholds(counts, fold_tot, thresholds, far_target):
    """calculate_val's per-fold threshold (:165-175) from the count kernel's integers: counts [F, Tn, 2], fold_tot [F, 2] (host arrays).
    TRAIN false accepts / different pairs of a fold = the totals minus the fold's."""
    counts, fold_tot = np.asarray(counts, dtype=np.int64), np.asarray(fold_tot, dtype=np.int64)
    th = np.asarray(thresholds, dtype=np.float64)
    fa_all, nd_all = counts[:, :, 1].sum(0), int(fold_tot[:, 1].sum())
    out = np.zeros(counts.shape[0])
    for f in range(counts.shape[0]):
        n_diff = nd_all - int(fold_tot[f, 1])
        far_train = np.array([float(v) / float(n_diff) for v in (fa_all - counts[f, :, 1])])      # ZeroDivisionError as the reference
        out[f] = slinear(far_train, th, far_target) if np.max(far_train) >= far_target else 0.0
    return out


def val_far_of_folds(counts_at_fold_thr, fold_tot):
    """(val_mean, val_std, far_mean) from counts [F, F, 2] taken at the F per-fold thresholds: fold f reads entry [f, f] (:177-184)."""
    c2, tot = np.asarray(counts_at_fold_thr, dtype=np.int64), np.asarray(fold_tot, dtype=np.int64)
    F = c2.shape[0]
    val = np.array([float(c2[f, f, 0]) / float(tot[f, 0]) for f in range(F)])
    far = np.array([float(c2[f, f, 1]) / float(tot[f, 1]) for f in range(F)])
    return np.mean(val), np.std(val), np.mean(far)


def val_from_dist(thresholds, dist, actual_issame, far_target, nrof_folds=10):
    """calculate_val behind its distances. Two launches of the count kernel (the grid, then each fold's interpolated threshold) and two host reads;
    the interpolation between them is host arithmetic on <= Tn integers per fold."""
    from gslora_hip import ops
    dist = _device_f32(dist, "dist").contiguous()
    F = int(nrof_folds)
    fold_bounds(dist.numel(), F)
    same = _issame_dev(actual_issame, dist.device, dist.numel())
    th, th_dev = _thresholds_dev(thresholds, dist.device)
    counts, tot = ops.verif_fold_counts(dist, same, th_dev, F)
    tot = tot.cpu().numpy()
    fold_thr = far_thresholds(counts.cpu().numpy(), tot, th, far_target)
    c2, _ = ops.verif_fold_counts(dist, same, torch.from_numpy(fold_thr).to(dist.device), F)
    return val_far_of_folds(c2.cpu().numpy(), tot)


def calculate_val(thresholds, embeddings1, embeddings2, actual_issame, far_target, nrof_folds=10):
    """:return: val_mean, val_std, far_mean at the per-fold thresholds whose TRAIN false-accept rate is far_target."""
    from gslora_hip import ops
    e1, e2 = _device_f32(embeddings1, "embeddings1"), _device_f32(embeddings2, "embeddings2")
    assert e1.shape[0] == e2.shape[0]
    assert e1.shape[1] == e2.shape[1]
    nrof_pairs = min(len(actual_issame), e1.shape[0])
    dist = ops.verif_sq_dist(e1, e2)[:nrof_pairs]
    return val_from_dist(thresholds, dist, actual_issame, far_target, nrof_folds)


def evaluate(embeddings, actual_issame, nrof_folds=10, pca=0):
    """embeddings [2P, D]: the normalised embeddings, rows 2p and 2p + 1 = pair p. :return: tpr, fpr, accuracy, best_thresholds."""
    if pca != 0:
        raise NotImplementedError("gs-lora_amd verification: pca > 0 (an sklearn PCA fit per fold, on the host) is outside the HIP path")
    emb = _device_f32(embeddings, "embeddings")
    return calculate_roc(THRESHOLDS, emb[0::2], emb[1::2], np.asarray(actual_issame.cpu() if isinstance(actual_issame, torch.Tensor)
                                                                       else actual_issame), nrof_folds=nrof_folds, pca=pca)
