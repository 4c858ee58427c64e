"""Golden fixture of the SCRUB baseline, from the REAL reference (baselines/SCRUBtrain.py and util/sgda_utils.py imported unmodified through
oracle.make_golden.install_shims) on the deterministic recipe of oracle/recipe.py. Runs only where the reference sources are checked out
(the build machine); the tests read the arrays alone.

    python tools/make_golden_scrub.py                # tests/golden/scrub_small.npz
    python tools/make_golden_scrub.py --out DIR      # into another directory

scrub_small.npz (cfg_small(lora_rank=0), CosFace, the --only_ffn trainability rule of train/train_own_forget_cl.py:432-439, dropout 0):
ONE call of the real train_one_superepoch_SCRUB with a forget loader and a remain loader of one batch each (3 and 2 images: the recipe's
forget batch of seed 40 and the first two remain images of that seed), so 5 x 2 + 5 = 15 steps; the teacher is a deep copy of the initial
model in eval() (train_own_forget_cl.py:440-443), the averaged copy torch's AveragedModel with beta = 0.1 (:445-450); torch.optim.AdamW in
timm's grouping at lr = 1e-4, weight decay 0.05; kd_T = 2, sgda_gamma = 0.99, sgda_alpha = 0.001. Once with sgda_smoothing = 0 (tag `s0`)
and once with 0.1 (tag `s1`). Per tag:
  forget::<tag> [5, 2]    (kd, total) the loop fed its meters on the max steps (a recording AverageMeter: the loop resets its meters in place)
  remain::<tag> [10, 3]   (kd, CE, total) on the min steps, in order
  forget64::<tag>, remain64::<tag>   the same trajectory with the reference model, its copies and the batches in float64
  final::<tag>::<name>    every trainable tensor after step 15 (f32 run)
  final_diff::<tag>::<name>  (f64 run - f32 run) of that tensor per element, stored as float32: |.| is the recorded deviation, and
                             final + final_diff is the f64 run's tensor to about 1e-11 (half the bytes of storing it in float64)
  swa_is_final::<tag>     the averaged copy's tensors after update_parameters equal the student's (its first update is a copy): asserted here
and `trainable`, `y_forget`, `y_remain`, `hyper` (lr, wd, kd_T, gamma, alpha, smoothing of s1). No reference text is copied or edited.
"""
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import recipe  # noqa: E402
from oracle.make_golden import install_shims  # noqa: E402
import make_golden_ffn_train as F  # noqa: E402
import make_golden_heads as H  # noqa: E402

LR, WD, KD_T, GAMMA, ALPHA, SMOOTHING, BETA, SEED = 1e-4, 0.05, 2.0, 0.99, 0.001, 0.1, 0.1, 40


class InDouble(torch.nn.Module):
    """The reference loop hands its model `inputs.float()`: the float64 run casts the batch back up in front of the reference model."""

    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, x, y):
        return self.m(x.double(), y)


def run(smoothing, double):
    from baselines.SCRUBtrain import train_one_superepoch_SCRUB
    from util import utils as rutil

    class Recording(rutil.AverageMeter):
        def __init__(self):
            super().__init__()
            self.seen = []

        def update(self, val, n=1):
            self.seen.append(float(val))
            super().update(val, n)

    cfg = recipe.cfg_small(lora_rank=0)
    model = F.build_reference(cfg, F.state_without_lora(cfg))
    names = F.only_ffn_trainable(model)
    if double:
        model = model.double()
    teacher = copy.deepcopy(model)
    student = InDouble(model) if double else model
    teacher = InDouble(teacher) if double else teacher
    teacher.eval()
    swa = torch.optim.swa_utils.AveragedModel(student, avg_fn=lambda avg, new, n: avg * (1.0 - BETA) + new * BETA)
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    no_decay = [p for n, p in named if p.ndim <= 1 or n.endswith(".bias")]
    decay = [p for n, p in named if not (p.ndim <= 1 or n.endswith(".bias"))]
    opt = torch.optim.AdamW([dict(params=no_decay, weight_decay=0.0), dict(params=decay, weight_decay=WD)], lr=LR, eps=1e-8, betas=(0.9, 0.999))
    x_r, y_r, x_f, y_f = H.batches(cfg, 3, SEED)
    forget, remain = [(x_f, y_f)], [(x_r[:2], y_r[:2])]
    m = {k: Recording() for k in ("losses_CE", "losses_total_forget", "losses_total_remain", "losses_kd_remain", "losses_kd_forget")}
    out = train_one_superepoch_SCRUB(
        student=student, teacher=teacher, swa_model=swa, data_loader_forget=forget, remain_loader=remain, criterion=torch.nn.CrossEntropyLoss(),
        optimizer=opt, device=torch.device("cpu"), superepoch=0, batch=0, task_i=0, testloader_forget=None, testloader_remain=None,
        forget_acc_before=0.0, highest_H_mean=0.0, cfg=dict(lr_decay_rate=0.1, lr_decay_epochs=100, sgda_learning_rate=LR), kd_T=KD_T,
        sgda_smoothing=smoothing, sgda_gamma=GAMMA, sgda_alpha=ALPHA, **m)
    assert out[0] == 15 and len(m["losses_kd_forget"].seen) == 5 and len(m["losses_CE"].seen) == 10
    assert all(torch.equal(a, b) for a, b in zip(swa.parameters(), student.parameters())), "the first update_parameters is a copy"
    return dict(names=names, forget=np.array([m["losses_kd_forget"].seen, m["losses_total_forget"].seen], dtype=np.float64).T.copy(),
                remain=np.array([m["losses_kd_remain"].seen, m["losses_CE"].seen, m["losses_total_remain"].seen], dtype=np.float64).T.copy(),
                final={n: p.detach().clone() for n, p in named}, y_forget=y_f.numpy().copy(), y_remain=y_r[:2].numpy().copy())


def scrub_case(tag, out):
    res = {"hyper": np.array([LR, WD, KD_T, GAMMA, ALPHA, SMOOTHING], dtype=np.float64)}
    for name, smoothing in (("s0", 0.0), ("s1", SMOOTHING)):
        a, b = run(smoothing, False), run(smoothing, True)
        res.update(trainable=np.array(a["names"]), y_forget=a["y_forget"], y_remain=a["y_remain"])
        res[f"forget::{name}"], res[f"remain::{name}"] = a["forget"], a["remain"]
        res[f"forget64::{name}"], res[f"remain64::{name}"] = b["forget"], b["remain"]
        res[f"swa_is_final::{name}"] = np.bool_(True)
        for n in a["names"]:
            res[f"final::{name}::{n}"] = a["final"][n].numpy().copy()
            res[f"final_diff::{name}::{n}"] = (b["final"][n] - a["final"][n].double()).float().numpy().copy()
    H.save(out, tag, res)


def main():
    install_shims()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    args = sys.argv[1:]
    out = os.path.join(ROOT, "tests", "golden")
    if "--out" in args:
        out = args[args.index("--out") + 1]
    scrub_case("scrub_small", out)


if __name__ == "__main__":
    main()
