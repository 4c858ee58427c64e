"""Golden fixture of the per-class evaluation, from the REAL reference (imported unmodified through oracle.make_golden.install_shims) on the
deterministic recipe of oracle/recipe.py. Runs only where the reference sources are checked out (the build machine); the tests read the
arrays alone and rebuild the inputs from the recipe (stats_inputs / proto_inputs below, restated in tests/test_hip_class_stats.py).

    python tools/make_golden_class_stats.py [--out DIR]

Writes tests/golden/class_stats_small.npz (cfg_small2, eval mode; the Softmax head: under the CosFace margin, 22.4 on the label's logit, the
untrained recipe model predicts no label at all, and a table of zeros pins little — with the linear head 6 of 48 predictions are correct):
  (a) stats_*   the reference's per-class evaluation, test/test_own.py:99-143. Those statements live inside the script's main(), behind
                its data set and checkpoint loading, so the generator reads exactly those lines from the reference's file at run time and
                executes them around the real model, a seeded synthetic loader and the names they use (model, testloader, DEVICE,
                NUM_CLASS, args.batch_size). No reference text is restated here.
                  stats_labels [48]   the loader's labels (every class occurs: the reference divides by each class's total; 48 = 8 batches
                                      of 6: the reference's loop indexes range(batch_size) and needs full batches)
                  stats_total / stats_correct [12] f64   class_total / class_correct as the reference leaves them
                  stats_accuracy f64  its overall accuracy          stats_lines [12] str   the lines of its class_accuracy40.txt
  (b) proto_*   util.utils.calculate_prototypes of the reference (:502-549) on 23 images in batches of 5 (ragged tail), classes of unequal
                frequency, class PROTO_ABSENT absent:  proto_labels [23], proto_keys, proto_vals [len(keys), dim]
No row of the reference's logits in (a) has a tied maximum, and every row's best logit leads the second by more than MIN_GAP, ten times
the f32 parity bar of the forward (both asserted below): the arg-max is unambiguous; tie rules are tested on constructed rows against torch.
"""
import contextlib
import io
import os
import sys
import tempfile
import textwrap
import types
from unittest import mock

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import recipe  # noqa: E402
from oracle.make_golden import REF, install_shims  # noqa: E402
import make_golden_heads as H  # noqa: E402

TAG = "class_stats_small"
STATS_N, STATS_BATCH = 48, 6
PROTO_N, PROTO_BATCH, PROTO_ABSENT = 23, 5, 7
HEAD = "Softmax"
MIN_GAP = 1e-3
REF_LINES = (99, 143)      # test/test_own.py: overall accuracy, the per-class loop, the text file


def stats_inputs(cfg):
    """48 images and labels; the first num_class labels are 0 .. num_class - 1, so every class occurs, the rest are the recipe's draw."""
    x = recipe.make_images(cfg, STATS_N, seed=500, tag="cs_x")
    y = recipe.make_labels(cfg, STATS_N, seed=500, tag="cs_y")
    y[:cfg["num_class"]] = np.arange(cfg["num_class"])
    return x, y


def proto_inputs(cfg):
    """23 images; labels of unequal frequency with class PROTO_ABSENT re-labelled as class 3."""
    x = recipe.make_images(cfg, PROTO_N, seed=600, tag="cp_x")
    y = recipe.make_labels(cfg, PROTO_N, seed=600, tag="cp_y")
    y[y == PROTO_ABSENT] = 3
    return x, y


def reference_per_class(model, loader, num_class, batch_size):
    """Run lines REF_LINES of the reference's test/test_own.py around `model` and `loader`; returns (the names they leave, the file's lines)."""
    with open(os.path.join(REF, "test", "test_own.py")) as f:
        src = f.readlines()[REF_LINES[0] - 1:REF_LINES[1]]
    code = textwrap.dedent("".join(src))
    assert "class_accuracy40.txt" in code and "class_total" in code and "torch.max" in code, "the reference's per-class block moved"
    ns = dict(torch=torch, model=model, testloader=loader, DEVICE=torch.device("cpu"), NUM_CLASS=num_class,
              args=types.SimpleNamespace(batch_size=batch_size))
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as d:
        os.chdir(d)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                exec(compile(code, "test_own.py[99:143]", "exec"), ns)
            with open("class_accuracy40.txt") as f:
                lines = f.read().split("\n")
        finally:
            os.chdir(cwd)
    assert lines[-1] == "" and len(lines) == num_class + 1
    return ns, lines[:-1]


def case(out):
    from util import utils as rutil
    cfg = recipe.cfg_small2()
    model = H.build_reference(cfg, HEAD, H.head_state(cfg, HEAD))
    model.eval()
    res = {}
    # ---- (a) per-class evaluation
    x, y = stats_inputs(cfg)
    assert STATS_N % STATS_BATCH == 0 and sorted(set(y.tolist())) == list(range(cfg["num_class"]))
    ds = torch.utils.data.TensorDataset(torch.tensor(x), torch.tensor(y))
    loader = torch.utils.data.DataLoader(ds, batch_size=STATS_BATCH, shuffle=False, drop_last=False)
    with torch.no_grad():
        logits = torch.cat([model(xb, yb.long())[0] for xb, yb in loader])
    top2 = torch.topk(logits, 2, dim=1).values
    assert not torch.isnan(logits).any() and (top2[:, 0] - top2[:, 1] > MIN_GAP).all(), "a row of the reference's logits has a (nearly) tied maximum"
    ns, lines = reference_per_class(model, loader, cfg["num_class"], STATS_BATCH)
    total, correct = np.array(ns["class_total"], dtype=np.float64), np.array(ns["class_correct"], dtype=np.float64)
    assert total.sum() == STATS_N == ns["total"] and correct.sum() == ns["correct"] and 0 < ns["correct"] < STATS_N
    assert len(set(total.tolist())) > 1, "classes of unequal frequency"
    res.update(stats_labels=y, stats_total=total, stats_correct=correct, stats_accuracy=np.float64(ns["accuracy"]),
               stats_lines=np.array(lines), stats_batch=np.int64(STATS_BATCH))
    # ---- (b) prototypes
    x, y = proto_inputs(cfg)
    ds = torch.utils.data.TensorDataset(torch.tensor(x), torch.tensor(y))
    with mock.patch.object(rutil, "DataLoader", torch.utils.data.DataLoader):
        protos = rutil.calculate_prototypes(model, ds, batch_size=PROTO_BATCH, device="cpu")
    keys = sorted(protos)
    assert PROTO_ABSENT not in keys and len(keys) > 3 and len(set(np.bincount(y).tolist())) > 2
    res.update(proto_labels=y, proto_keys=np.array(keys, dtype=np.int64), proto_vals=np.stack([protos[k].numpy() for k in keys]).astype(np.float32),
               proto_batch=np.int64(PROTO_BATCH), proto_absent=np.int64(PROTO_ABSENT))
    H.save(out, TAG, res)


def main():
    install_shims()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    args = sys.argv[1:]
    out = os.path.join(ROOT, "tests", "golden")
    if "--out" in args:
        out = args[args.index("--out") + 1]
    case(out)


if __name__ == "__main__":
    main()
