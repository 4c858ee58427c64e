"""Face verification, host side (no GPU): the restated pieces of util/verification.py against the real sklearn / scipy / reference
results recorded in tests/golden/verification_small.npz (tools/make_golden_verification.py), and the C ABI of the three metric entry points.

The kernels themselves run in tests/test_hip_verification.py. Here the numpy model of their integer arithmetic (oracle/eval_probes.py:
counts_model, select_model — contiguous folds, strict
(double)dist < thr, train counts = totals minus the fold's, first arg-max of the integer train numerator, f64 divisions on the integers)
is held against the reference's outputs bit for bit: it pins the algorithm the kernels implement and guards the fixture."""
import os
import re

import numpy as np
import pytest
import torch

from oracle.eval_probes import counts_model, select_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["model", "p603_f10", "p50_f5", "nosame", "ties"]
THRESHOLDS = np.arange(0, 4, 0.01)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "verification_small.npz"))


def test_fold_bounds_are_sklearns_kfold(gold):
    from util import verification as V
    pf, bounds = gold["kfold::pf"], gold["kfold::bounds"]
    assert len(pf) > 200
    i = 0
    for P, F in pf:
        got = V.fold_bounds(P, F)
        assert got == [tuple(b) for b in bounds[i:i + F].tolist()], (P, F)
        i += F
    assert i == len(bounds)
    with pytest.raises(ValueError, match="greater than the number of samples"):
        V.fold_bounds(9, 10)
    with pytest.raises(ValueError, match="n_splits=2 or more"):
        V.fold_bounds(9, 1)


def test_slinear_is_scipys_on_strictly_increasing_points(gold):
    from util import verification as V
    X, Y, xn, want = (gold[f"slinear::{k}"] for k in ("x", "y", "xnew", "out"))
    for x, y, t, w in zip(X, Y, xn, want):
        n = int(np.sum(~np.isnan(x)))
        got = V.slinear(x[:n], y[:n], t)
        # both sides evaluate the same line through two f64 points; the forms may round differently by a few ulp of the values (<= 4)
        assert abs(got - w) <= 8 * np.finfo(np.float64).eps * 4.0, (got, w)
        perm = np.random.RandomState(n).permutation(n)      # interp1d sorts its points
        assert V.slinear(x[:n][perm], y[:n][perm], t) == got
    with pytest.raises(ValueError, match="outside the interpolation range"):
        V.slinear([0.0, 1.0], [0.0, 1.0], 1.5)


def test_slinear_rule_for_repeated_x():
    from util import verification as V
    x = [0.0, 0.0, 0.0, 0.2, 0.2, 0.6, 1.0, 1.0]
    y = [0.00, 0.01, 0.02, 0.03, 0.04, 0.05, 0.06, 0.07]
    assert V.slinear(x, y, 0.0) == 0.02 and V.slinear(x, y, 0.2) == 0.04 and V.slinear(x, y, 1.0) == 0.07
    assert abs(V.slinear(x, y, 0.1) - 0.025) < 1e-15      # from the LAST point at 0.0 to the FIRST at 0.2
    assert abs(V.slinear(x, y, 0.4) - 0.045) < 1e-15


@pytest.mark.parametrize("case", CASES)
def test_integer_count_algorithm_reproduces_the_reference_bit_for_bit(gold, case):
    d, same, F = gold[f"{case}::dist32"], gold[f"{case}::issame"], int(gold[f"{case}::folds"])
    counts, tot = counts_model(d, same, THRESHOLDS, F)
    acc, best, tpr, fpr = select_model(counts, tot, THRESHOLDS)
    for name, got in (("accuracy", acc), ("best_thresholds", best), ("tpr", tpr), ("fpr", fpr)):
        want = gold[f"{case}::{name}"]
        assert got.dtype == np.float64 and want.dtype == np.float64
        assert np.array_equal(got, want), (case, name, np.abs(got - want).max())


def test_the_fixture_holds_the_cases_it_is_meant_to(gold):
    assert (len(gold["p603_f10::dist32"]), int(gold["p603_f10::folds"])) == (603, 10)      # ragged folds: 603 = 3 * 61 + 7 * 60
    assert (len(gold["model::dist32"]), int(gold["model::folds"])) == (120, 10)
    assert (len(gold["p50_f5::dist32"]), int(gold["p50_f5::folds"])) == (50, 5)
    _, tot = counts_model(gold["nosame::dist32"], gold["nosame::issame"], THRESHOLDS, int(gold["nosame::folds"]))
    assert (tot[:, 0] == 0).any()      # a fold without a same pair
    c, t = counts_model(gold["ties::dist32"], gold["ties::issame"], THRESHOLDS, int(gold["ties::folds"]))
    tr = c.sum(0) - c[0]
    num = tr[:, 0] + (t[:, 1].sum() - t[0, 1]) - tr[:, 1]
    assert (num == num.max()).sum() > 1      # tied train accuracies: the first one must win
    assert float(gold["min_gap"]) >= 1e-4
    d, th = gold["dist"], THRESHOLDS
    assert np.isclose(np.abs(d[:, None] - th[None, :]).min(), float(gold["min_gap"]), rtol=0, atol=1e-15)
    assert np.array_equal(gold["model::dist32"], d.astype(np.float32))


@pytest.mark.parametrize("far", ["1e-1", "1e-2"])
def test_calculate_val_host_arithmetic_against_the_reference(gold, far):
    """far_thresholds (the slinear step on the counts) + val_far_of_folds on the numpy count model == the reference's calculate_val."""
    from util import verification as V
    d, same = gold["model::dist32"], gold["model::issame"]
    counts, tot = counts_model(d, same, THRESHOLDS, 10)
    thr = V.far_thresholds(counts, tot, THRESHOLDS, float(far))
    c2, _ = counts_model(d, same, thr, 10)
    got = np.array(V.val_far_of_folds(c2, tot))
    assert np.array_equal(got, gold[f"val_{far}"]), (got, gold[f"val_{far}"])


def test_header_signatures_and_exports_hold_the_three_entry_points():
    from gslora_hip import _lib
    new = {"gsl_verif_pair_dist", "gsl_verif_fold_counts", "gsl_verif_select"}
    header = open(os.path.join(ROOT, "include", "gslora_hip.h")).read()
    declared = set(re.findall(r"\b(gsl_[a-z0-9_]+)\s*\(", header)) - {"gsl_dropout_keep"}
    assert new <= declared and declared == set(_lib.SIGNATURES)
    for name in new:      # prototype arity == binding arity
        proto = re.search(r"GSL_API int " + name + r"\(([^;]*)\);", header).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name]), name
    assert "gsl_*" in open(os.path.join(ROOT, "gs-lora_amd", "csrc", "exports.map")).read()
    lib = _lib.load()
    for name in new:
        assert hasattr(lib, name)
    # argument checks come before any launch (no GPU needed)
    assert lib.gsl_verif_pair_dist(None, None, 0, 1, 1, 0, None, None, None, None, None) == -1 and b"gsl_verif_pair_dist" in lib.gsl_last_error()
    assert lib.gsl_verif_fold_counts(None, None, 10, None, 400, 10, None, None, None) == -1
    assert lib.gsl_verif_select(None, None, None, 400, 10, None, None, None) == -1


def test_verification_refuses_host_inputs_pca_and_too_few_pairs():
    from util import verification as V
    from util.utils import perform_val, buffer_val      # noqa: F401
    e = torch.zeros(20, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.evaluate(e, [True] * 10, nrof_folds=5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.evaluate(e.numpy(), [True] * 10, nrof_folds=5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.calculate_val(THRESHOLDS, e[0::2], e[1::2], [True] * 10, 1e-2, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.calculate_accuracy(0.5, torch.zeros(10), [True] * 10)
    with pytest.raises(NotImplementedError, match="pca"):
        V.evaluate(e, [True] * 10, nrof_folds=5, pca=4)
    assert buffer_val("lfw", 0.9, 0.01, 20.0, 1.2, None, 7) == {"lfw_Accuracy": 0.9, "lfw_Std": 0.01, "lfw_XNorm": 20.0, "lfw_Best_Threshold": 1.2}


def test_driver_verification_is_off_by_default_and_builds_load_bin_shaped_pairs():
    import driver_cl
    assert driver_cl.get_args([]).verify_pairs == 0 and driver_cl.get_args(["--verify_pairs", "64"]).verify_pairs == 64
    (x, xf), issame = driver_cl.synthetic_pairs(10, 6, 48, seed=3)
    assert x.shape == (20, 3, 48, 48) and torch.equal(xf, x.flip(3)) and issame == [p % 2 == 0 for p in range(10)]
    assert x.dtype == torch.float32 and 0.0 <= float(x.min()) and float(x.max()) <= 1.0
    (u, _), _ = driver_cl.synthetic_pairs(10, 6, 48, seed=3, u8=True)
    assert u.dtype == torch.uint8 and torch.equal(u.float() / 255.0, x)
