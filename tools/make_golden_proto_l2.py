"""Golden fixtures of the l2 prototype distance and of precision@k, from the REAL reference (imported unmodified through
oracle.make_golden.install_shims) on the deterministic recipe of oracle/recipe.py. Runs only where the reference sources are checked out
(the build machine); the tests read the arrays alone.

    python tools/make_golden_proto_l2.py                         # all three fixtures
    python tools/make_golden_proto_l2.py topk_small              # one of them
    python tools/make_golden_proto_l2.py --out DIR [tags ...]    # into another directory (tests/test_proto_l2_host.py regenerates there)

Writes tests/golden/:
  proto_l2_small2_b3.npz       cfg_small2, CosFace: the keys of small2_b3.npz / arcface_small2_b3.npz (tools/make_golden_heads.model_case) with
                               the reference's get_prototype_loss(..., distance="l2") in the total loss; losses1[4:6] are the two l2 means.
                               `hyper_*` hold the loss hyper-parameters of losses1 / grad1 (BND_pro is chosen below so that the prototype hinge
                               is ACTIVE there; total_inactive / grad_inactive use BND = 5, BND_pro = INACTIVE_BND_PRO: both hinges inactive)
  proto_l2_small6_engine.npz   cfg_small6, CosFace: three steps of engine_cl.train_one_epoch + torch AdamW (keys as arcface_small6_engine.npz)
  topk_small.npz               logits [37, 23], labels, and the reference's train_accuracy for topk = (1, 5) and (5, 1, 3): `ret_*` is what
                               the reference returns for the tuple (its first entry, util/utils.py:368), `perk_*` the value of every k
                               (the reference asked for one k at a time)

The reference's engine and the hand-written total loss call the module-level engine_cl.get_prototype_loss with its default distance; the
generator binds that name to a wrapper that passes distance="l2" while a case runs. No reference text is edited.
"""
import contextlib
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import recipe  # noqa: E402
from oracle import make_golden as MG  # noqa: E402
from oracle.make_golden import HYPER, install_shims  # noqa: E402
import make_golden_heads as H  # noqa: E402

# The l2 distance of a recipe embedding from a recipe prototype is O(1) per element, far above the KL fixtures' BND_pro = 2: with that bound
# the forget hinge would be inactive in losses1 as well. L2_BND_PRO is set above the forget batch's l2 mean so that grad1 carries the hinge's
# gradient; model_case() asserts both states.
L2_BND_PRO = 4.0
INACTIVE_BND_PRO = 0.1


@contextlib.contextmanager
def l2_prototype_loss():
    """engine_cl.get_prototype_loss bound to distance="l2" (the engine and make_golden_heads.total_loss look the name up at call time)."""
    import engine_cl
    orig = engine_cl.get_prototype_loss
    engine_cl.get_prototype_loss = functools.partial(orig, distance="l2")
    try:
        yield orig
    finally:
        engine_cl.get_prototype_loss = orig


@contextlib.contextmanager
def hyper(**kw):
    """The generators of tools/make_golden_heads.py read the module-level HYPER dict; the l2 fixtures run them with another BND_pro."""
    saved = dict(HYPER)
    HYPER.update(kw)
    try:
        yield
    finally:
        HYPER.clear()
        HYPER.update(saved)


def model_case(tag, out):
    cfg = recipe.cfg_small2()
    with l2_prototype_loss(), hyper(BND_pro=L2_BND_PRO):
        assert H.HYPER is MG.HYPER and H.HYPER["BND_pro"] == L2_BND_PRO
        H.model_case(tag, cfg, "CosFace", 3, out)
    path = os.path.join(out, f"{tag}.npz")
    res = dict(np.load(path))
    l2_f = float(res["losses1"][4])
    assert INACTIVE_BND_PRO < l2_f < L2_BND_PRO, f"the forget l2 mean {l2_f} must lie between the inactive and the active bound"
    res.update({f"hyper_{k}": np.float64(v) for k, v in dict(HYPER, BND_pro=L2_BND_PRO).items()})
    H.save(out, tag, res)


def engine_case(tag, out):
    with l2_prototype_loss(), hyper(BND_pro=L2_BND_PRO):
        H.engine_case(tag, recipe.cfg_small6(), "CosFace", 2, out)
    path = os.path.join(out, f"{tag}.npz")
    res = dict(np.load(path))
    res.update({f"hyper_{k}": np.float64(v) for k, v in dict(HYPER, BND_pro=L2_BND_PRO).items()})
    H.save(out, tag, res)


TOPKS = {"1_5": (1, 5), "5_1_3": (5, 1, 3)}


def topk_inputs(B=37, C=23, seed=20240):
    """Seeded logits without ties; row i carries the label whose logit has rank i mod 8, so every k of the fixture sees hits and misses."""
    rng = np.random.RandomState(seed)
    logits = rng.permutation(B * C).reshape(B, C).astype(np.float32) / np.float32(B * C) * np.float32(8.0) - np.float32(4.0)
    order = np.argsort(-logits, axis=1, kind="stable")
    labels = order[np.arange(B), np.arange(B) % 8].astype(np.int64)
    return logits, labels


@contextlib.contextmanager
def view_as_in_the_reference_s_torch():
    """train_accuracy calls correct[:k].view(-1) on the comparison of a TRANSPOSED index tensor (util/utils.py:360-365). The torch the
    reference was written for returned that comparison contiguous, so the view was legal; a current torch keeps the transposed strides and
    raises for k > 1. While the reference function runs, a view torch refuses falls back to reshape (same elements, same order)."""
    orig = torch.Tensor.view

    def view(self, *shape, **kw):
        try:
            return orig(self, *shape, **kw)
        except RuntimeError:
            return self.reshape(*shape)
    torch.Tensor.view = view
    try:
        yield
    finally:
        torch.Tensor.view = orig


def topk_case(tag, out):
    from util import utils as rutil
    logits, labels = topk_inputs()
    lo, y = torch.tensor(logits), torch.tensor(labels)
    res = {"logits": logits, "labels": labels}
    with view_as_in_the_reference_s_torch():
        for name, ks in TOPKS.items():
            res[f"topk_{name}"] = np.array(ks, dtype=np.int64)
            res[f"ret_{name}"] = rutil.train_accuracy(lo, y, topk=ks).numpy().copy()
            res[f"perk_{name}"] = np.array([rutil.train_accuracy(lo, y, topk=(k,)).item() for k in ks], dtype=np.float32)
            assert res[f"ret_{name}"] == res[f"perk_{name}"][0]
    H.save(out, tag, res)


CASES = {
    "proto_l2_small2_b3": model_case,
    "proto_l2_small6_engine": engine_case,
    "topk_small": topk_case,
}


def main():
    install_shims()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    args = sys.argv[1:]
    out = os.path.join(ROOT, "tests", "golden")
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    for tag, run in CASES.items():
        if not args or tag in args:
            run(tag, out)


if __name__ == "__main__":
    main()
