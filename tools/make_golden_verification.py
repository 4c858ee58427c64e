"""Golden fixture of the face-verification metric, from the REAL reference (util/verification.py and util/utils.py perform_val, imported
unmodified through oracle.make_golden.install_shims) on the deterministic recipe of oracle/recipe.py. Runs only where the reference
sources, sklearn and scipy are available (the build machine); the tests read the arrays alone.

    python tools/make_golden_verification.py

writes tests/golden/verification_small.npz (arrays only):

  the model case — the reference ViT_face of cfg_small2 (CosFace, eval mode = merged non-zero LoRA B) on N_PAIRS synthetic pairs
  (verif_pairs below; the tests rebuild the same images from the recipe), through the real perform_val with batch size 50:
    pair_seed                    seed of the pair set: the first one for which no reference distance lies within MIN_GAP of a threshold
    emb0, emb1 [2P, D] f32       what the backbone returned for the images / the flipped images
    dist [P] f64, issame [P]     the reference's distances (f64 arithmetic on the f32 embeddings) and the pair flags
    min_gap                      min |dist - threshold| over all pairs and thresholds (>= MIN_GAP by construction)
    acc_mean, acc_std, xnorm, thr_mean, tpr, fpr, accuracy, best_thresholds      perform_val's outputs and evaluate's behind them
    val_1e-1, val_1e-2 [3]       calculate_val(far_target) = (val_mean, val_std, far_mean)
  metric cases `<case>::{dist32, issame, folds, tpr, fpr, accuracy, best_thresholds}` for case in model (the distances above rounded to
  f32), p603_f10, p50_f5, nosame (a fold without a same pair), ties (tied train accuracies): calculate_roc's outputs recomputed from
  EXACTLY the f32 distances stored (see roc_of_dist).
  slinear::{x, y, xnew, out}     scipy's interp1d(kind="slinear") on strictly increasing x (ragged rows padded with NaN)
  kfold::{pf, bounds}            sklearn KFold(shuffle=False) test-fold bounds for a sweep of (P, F)

Two things are adapted AROUND the reference's code, neither inside it:
  * calculate_roc holds a stray pdb.set_trace() (:70-72); pdb.set_trace is replaced by a no-op for the run.
  * calculate_val's interp1d(far_train, thresholds, kind="slinear") is refused by a current scipy whenever far_train repeats a value
    ("Expect x to not have duplicates") — which it does on every pair set. The run hands scipy's real interp1d the two points that bracket
    the target under the rule older scipy versions implemented (last point of the left x value, first point of the right one; see
    util/verification.py), so the interpolation arithmetic is still scipy's.
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import recipe  # noqa: E402
from oracle.make_golden import REF, build_reference_model, install_shims  # noqa: E402

N_PAIRS = 120
MIN_GAP = 1e-4
BATCH = 50
THRESHOLDS = np.arange(0, 4, 0.01)


def verif_pairs(cfg, n_pairs, seed):
    """uint8 images [2 * n_pairs, 3, S, S] and issame [n_pairs]: an identity is a colour, an image of it 0.6 * colour + 0.4 * noise. Even
    pairs: two images of one identity; odd pairs: two identities. Pure recipe arithmetic. The model is fed the BYTE VALUES as floats
    (0 .. 255, what load_bin hands perform_val, util/utils.py:38-57): the recipe's random network moves its embedding little with the
    input, and on ToTensor()-range images every distance falls below the second threshold."""
    S = cfg["image_size"]

    def image(ident, k):
        base = recipe.uniform(f"verif_id{ident}", (3, 1, 1), seed, 0.1, 0.9)
        if k:      # the second image of an identity: its colour moved by 0.08 per channel, so that same pairs keep clear of threshold 0
            base = base + 0.08 * np.sign(recipe.uniform(f"verif_twin{ident}", (3, 1, 1), seed, -1.0, 1.0))
        noise = recipe.uniform(f"verif_noise{ident}_{k}", (3, S, S), seed, 0.0, 1.0)
        return np.floor((0.6 * base + 0.4 * noise) * 255.0).clip(0, 255).astype(np.uint8)

    imgs, issame = [], []
    for p in range(n_pairs):
        if p % 2 == 0:
            imgs += [image(p, 0), image(p, 1)]
        else:
            imgs += [image(p, 0), image(n_pairs + p, 0)]
        issame.append(p % 2 == 0)
    return np.stack(imgs), np.array(issame)


class _NoSquare:
    """numpy with square() = identity: calculate_roc(dist[:, None], zeros) then takes np.sum(np.square(dist - 0), 1) = dist exactly."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def square(x):
        return x


def roc_of_dist(RV, dist32, issame, folds):
    """The real calculate_roc on given distances: embeddings1 = the f32 distances as one f64 column, embeddings2 = 0."""
    d = np.asarray(dist32, dtype=np.float32).astype(np.float64)[:, None]
    RV.np = _NoSquare()
    try:
        tpr, fpr, acc, best = RV.calculate_roc(THRESHOLDS, d, np.zeros_like(d), np.asarray(issame), nrof_folds=folds)
    finally:
        RV.np = np
    return dict(dist32=np.asarray(dist32, dtype=np.float32), issame=np.asarray(issame, dtype=np.uint8), folds=np.int64(folds), tpr=tpr, fpr=fpr,
                accuracy=acc, best_thresholds=best)


def bracket_interp1d(real_interp1d):
    def interp1d(x, y, kind="linear"):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        order = np.argsort(x, kind="mergesort")
        x, y = x[order], y[order]

        def f(x_new):
            hi = int(np.searchsorted(x, x_new, side="right"))
            lo = hi - 1
            if hi == len(x) or x[lo] == x_new:
                return np.float64(y[lo])
            return real_interp1d(x[[lo, hi]], y[[lo, hi]], kind=kind)(x_new)
        return f
    return interp1d


def synthetic_cases(RV):
    out = {}
    g = np.random.RandomState(20240)

    def two_clusters(P, p_same=0.5):
        same = g.rand(P) < p_same
        d = np.where(same, g.normal(0.7, 0.35, P), g.normal(1.9, 0.45, P)).clip(0.0, 3.999)
        return d.astype(np.float32), same

    d, s = two_clusters(603)
    out["p603_f10"] = roc_of_dist(RV, d, s, 10)
    d, s = two_clusters(50)
    out["p50_f5"] = roc_of_dist(RV, d, s, 5)
    d, s = two_clusters(120)
    s[24:36] = False      # fold 2 of 10 holds no same pair: tpr takes the `0 if tp + fn == 0` branch
    d[24:36] = g.normal(1.9, 0.45, 12).clip(0, 3.999).astype(np.float32)
    out["nosame"] = roc_of_dist(RV, d, s, 10)
    # ties: perfectly separable distances with a wide empty band — every threshold inside the band has the same (maximal) train accuracy
    s = np.arange(60) % 2 == 0
    d = np.where(s, 0.30 + 0.004 * np.arange(60), 2.20 + 0.004 * np.arange(60)).astype(np.float32)
    out["ties"] = roc_of_dist(RV, d, s, 6)
    return out


def slinear_cases():
    from scipy import interpolate
    g = np.random.RandomState(7)
    n_max, rows = 40, []
    for _ in range(24):
        n = int(g.randint(2, n_max + 1))
        x = np.cumsum(g.rand(n) + 1e-3)
        y = g.rand(n) * 4
        xn = x[0] + (x[-1] - x[0]) * g.rand() if g.rand() < 0.8 else x[int(g.randint(0, n))]
        rows.append((x, y, xn, float(interpolate.interp1d(x, y, kind="slinear")(xn))))
    X = np.full((len(rows), n_max), np.nan)
    Y = np.full((len(rows), n_max), np.nan)
    for i, (x, y, _, _) in enumerate(rows):
        X[i, :len(x)], Y[i, :len(y)] = x, y
    return dict(x=X, y=Y, xnew=np.array([r[2] for r in rows]), out=np.array([r[3] for r in rows]))


def kfold_cases():
    from sklearn.model_selection import KFold
    pf, bounds = [], []
    for P in list(range(2, 41)) + [50, 120, 603, 6000, 6007]:
        for F in (2, 3, 5, 6, 7, 10):
            if F > P:
                continue
            pf.append((P, F))
            for _, test in KFold(n_splits=F, shuffle=False).split(np.arange(P)):
                assert np.array_equal(test, np.arange(test[0], test[-1] + 1))
                bounds.append((test[0], test[-1] + 1))
    return dict(pf=np.array(pf, dtype=np.int64), bounds=np.array(bounds, dtype=np.int64))


def model_case(RV, RU):
    cfg = recipe.cfg_small2()
    model = build_reference_model(cfg, recipe.make_state(cfg))
    model.eval()
    outs = []
    model.register_forward_hook(lambda m, i, o: outs.append(o.detach().numpy().copy()))
    seen = {}
    real_evaluate = RU.evaluate

    def spy(embeddings, issame, nrof_folds=10, pca=0):
        seen["emb"] = np.array(embeddings)
        seen["roc"] = real_evaluate(embeddings, issame, nrof_folds, pca)
        return seen["roc"]

    RU.evaluate = spy
    try:
        for seed in range(1, 400):
            u8, issame = verif_pairs(cfg, N_PAIRS, seed)
            x = torch.tensor(u8.astype(np.float32))
            del outs[:]
            with torch.no_grad():
                with contextlib.redirect_stdout(io.StringIO()):
                    res = RU.perform_val(False, "cpu", cfg["dim"], BATCH, model, [x, x.flip(3)], list(issame), 10)
            e = seen["emb"]
            dist = np.sum(np.square(e[0::2] - e[1::2]), 1)
            gap = float(np.min(np.abs(dist[:, None] - THRESHOLDS[None, :])))
            print(f"seed {seed}: min gap {gap:.2e}, accuracy {res[0]:.4f}, dist same {dist[0::2].mean():.3f} / different {dist[1::2].mean():.3f}")
            if gap >= MIN_GAP:
                break
        else:
            raise SystemExit("no seed qualifies")
    finally:
        RU.evaluate = real_evaluate
    nb = -(-2 * N_PAIRS // BATCH)
    assert len(outs) == 2 * nb
    tpr, fpr, accuracy, best = seen["roc"]
    out = dict(pair_seed=np.int64(seed), emb0=np.concatenate(outs[:nb]).astype(np.float32), emb1=np.concatenate(outs[nb:]).astype(np.float32),
               dist=dist, issame=issame.astype(np.uint8), min_gap=np.float64(gap), acc_mean=np.float64(res[0]), acc_std=np.float64(res[1]),
               xnorm=np.float64(res[2]), thr_mean=np.float64(res[3]), tpr=tpr, fpr=fpr, accuracy=accuracy, best_thresholds=best)
    real_interp1d = RV.interpolate.interp1d
    try:
        RV.calculate_val(THRESHOLDS, e[0::2], e[1::2], issame, 1e-1, 10)
        print("calculate_val ran with scipy's interp1d as is")
    except ValueError as exc:
        print("calculate_val with scipy's interp1d as is:", exc)

    class _Interp:
        def __getattr__(self, name):
            return getattr(sys.modules["scipy.interpolate"], name)
    shim = _Interp()
    shim.interp1d = bracket_interp1d(real_interp1d)
    RV.interpolate = shim
    try:
        for name, far in (("val_1e-1", 1e-1), ("val_1e-2", 1e-2)):
            out[name] = np.array(RV.calculate_val(THRESHOLDS, e[0::2], e[1::2], issame, far, 10), dtype=np.float64)
            print(name, out[name])
    finally:
        RV.interpolate = sys.modules["scipy.interpolate"]
    return out, roc_of_dist(RV, dist.astype(np.float32), issame, 10)


def main():
    install_shims()
    import pdb
    pdb.set_trace = lambda *a, **k: None      # the stray breakpoint of calculate_roc (:70-72)
    torch.manual_seed(0)
    torch.set_num_threads(8)
    from util import verification as RV
    from util import utils as RU
    assert RV.__file__.startswith(REF) and RU.__file__.startswith(REF), (RV.__file__, RU.__file__)      # the reference's, not the product's
    res, model_metric = model_case(RV, RU)
    for k in ("tpr", "fpr", "accuracy", "best_thresholds"):      # rounding the distances to f32 moved no decision
        assert np.array_equal(model_metric[k], res[k]), k
    cases = dict(model=model_metric, **synthetic_cases(RV))
    for case, d in cases.items():
        res.update({f"{case}::{k}": v for k, v in d.items()})
        print(case, "accuracy", d["accuracy"], "best", d["best_thresholds"])
    res.update({f"slinear::{k}": v for k, v in slinear_cases().items()})
    res.update({f"kfold::{k}": v for k, v in kfold_cases().items()})
    path = os.path.join(ROOT, "tests", "golden", "verification_small.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
