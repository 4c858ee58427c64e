"""Golden fixtures of the LwF / DER / DER++ / FDR baselines, from the REAL reference (baselines/Lwftrain.py, DERtrain.py, FDRtrain.py imported
unmodified through oracle.make_golden.install_shims) on the deterministic recipe of oracle/recipe.py. Runs only where the reference sources
are checked out (the build machine); the tests read the arrays alone.

    python tools/make_golden_distill.py                # tests/golden/distill_small*.npz, tests/golden/distill_signatures.json
    python tools/make_golden_distill.py --out DIR      # into another directory

Set-up (cfg_small(lora_rank=0), CosFace, the --only_ffn trainability rule of train/train_own_forget_cl.py:432-439, dropout 0): ONE call of the
real loop per tag; the forget loader has 3 batches of 3 images (the recipe's forget batches of seeds 40, 41, 42), the remain loader 3 batches
of 2 images (the first two remain images of those seeds), so a call is 3 steps and DER++'s draws cross the prefetcher's restart in the middle
of step 2 and at the end of step 3; torch.optim.AdamW in timm's grouping at lr = 1e-4, weight decay 0.05; the reference's default lambdas
(util/args.py:273-295). Tags are <method>_<teacher>: method lwf | der | derpp | fdr; teacher `copy` (a deep copy of the student: the
driver's real case, the first step's distance is exactly 0) or `far` (the copy with every FFN weight matrix multiplied element-wise by
recipe.uniform("far::" + name, shape, 77, 0.7, 1.3)). Every recorded distance of a `far` run is asserted to be above 1e-2.

distill_small.npz (all tags):
  meters::<tag> [3, k]      what the loop fed its meters per step, in the order of METERS[method] (a recording AverageMeter: the loop resets
                            its meters in place); meters64::<tag> the same from a run with model, teacher and batches in float64
  labels::<tag> [.]         the labels of every batch the loop handed the student, in order (recorded by a wrapper around the model): per
                            step forget, remain (, DER++'s second remain batch)
  trainable, hyper (lr, wd, Lwf_lambda_kd, Lwf_lambda_remain, Lwf_T, DER_lambda, DER_plus_lambda, FDR_lambda)
distill_small_<method>.npz (one file per method: a committed file stays below 1 MiB):
  grad::<tag>::<name>       the gradient the last step left on every trainable tensor (p.grad after the loop returned), both teachers
  grad_diff::<tag>::<name>  (f64 run - f32 run) of it, stored as float32
  final::<tag>::<name>, final_diff::<tag>::<name>   every trainable tensor after the last step and its f64 - f32 difference — for the `far`
                            teacher only (one AdamW step at this rate moves a weight by 1e-4: the weights cannot tell gradient magnitudes
                            apart, the gradients above are what holds them; the `copy` runs' weights would double the files for nothing)
distill_signatures.json: parameter names, defaults and return arity of the three reference functions (names only). No reference text is
copied or edited.
"""
import copy
import inspect
import json
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
from make_golden_scrub import InDouble  # noqa: E402

LR, WD, SEEDS = 1e-4, 0.05, (40, 41, 42)
LWF_KD, LWF_REMAIN, LWF_T, DER_LAMBDA, DER_PLUS_LAMBDA, FDR_LAMBDA = 0.5, 1.0, 2.0, 0.1, 0.1, 0.1      # util/args.py:273-295
METERS = {"lwf": ("losses_CE", "losses_KD", "losses_remain", "losses_total"), "der": ("losses_CE", "losses_DER", "losses_total"),
          "derpp": ("losses_CE", "losses_DER", "losses_total"), "fdr": ("losses_CE", "losses_FDR", "losses_total")}
REG_COLUMN = {"der": 1, "derpp": 1, "fdr": 1}
FAR_SEED, FAR_LO, FAR_HI = 77, 0.7, 1.3


def far_scale(name, shape):
    """The element-wise factor of the `far` teacher's FFN weight matrix `name`."""
    return recipe.uniform("far::" + name, tuple(shape), FAR_SEED, FAR_LO, FAR_HI)


def loaders(cfg):
    forget, remain = [], []
    for s in SEEDS:
        x_r, y_r, x_f, y_f = H.batches(cfg, 3, s)
        forget.append((x_f, y_f))
        remain.append((x_r[:2], y_r[:2]))
    return forget, remain


class Seen(torch.nn.Module):
    """Records the labels of every batch the loop hands the student, in order; `double`: casts the batch up in front of a float64 model
    (the reference loop hands its model `inputs.float()`)."""

    def __init__(self, m, double):
        super().__init__()
        self.m, self.double, self.labels = m, double, []

    def forward(self, x, y):
        self.labels.append(y.numpy().copy())
        return self.m(x.double() if self.double else x, y)


def run(method, far, double):
    from baselines.DERtrain import train_one_epoch_DER
    from baselines.FDRtrain import train_one_epoch_FDR
    from baselines.Lwftrain import train_one_epoch_Lwf
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
    teacher = copy.deepcopy(model)
    if far:
        with torch.no_grad():
            for n, p in teacher.named_parameters():
                if "fn.fn.net" in n and n.endswith("weight"):
                    p.mul_(torch.tensor(far_scale(n, p.shape)))
    if double:
        model, teacher = model.double(), teacher.double()
    student = Seen(model, double)
    teacher = InDouble(teacher) if double else teacher
    teacher.eval()
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    no_decay = [p for n, p in named if p.ndim <= 1 or n.endswith(".bias")]
    decay = [p for n, p in named if not (p.ndim <= 1 or n.endswith(".bias"))]
    opt = torch.optim.AdamW([dict(params=no_decay, weight_decay=0.0), dict(params=decay, weight_decay=WD)], lr=LR, eps=1e-8, betas=(0.9, 0.999))
    forget, remain = loaders(cfg)
    m = {k: Recording() for k in METERS[method]}
    common = dict(student_model=student, teacher_model=teacher, data_loader_cl_forget=forget, remain_loader=remain, criterion=torch.nn.CrossEntropyLoss(),
                  optimizer=opt, device=torch.device("cpu"), epoch=0, batch=0, task_i=0, testloader_forget=None, testloader_remain=None,
                  forget_acc_before=0.0, highest_H_mean=0.0, cfg={}, **m)
    if method == "lwf":
        out = train_one_epoch_Lwf(lambda_kd=LWF_KD, lambda_remain=LWF_REMAIN, temperature=LWF_T, **common)
    elif method in ("der", "derpp"):
        out = train_one_epoch_DER(lambda_der=DER_LAMBDA, plus=method == "derpp", lambda_der_plus=DER_PLUS_LAMBDA, **common)
    else:
        out = train_one_epoch_FDR(reg_lambda=FDR_LAMBDA, **common)
    assert out[0] == len(forget) and all(len(m[k].seen) == len(forget) for k in m)
    return dict(names=names, meters=np.array([m[k].seen for k in METERS[method]], dtype=np.float64).T.copy(), n_out=len(out),
                final={n: p.detach().clone() for n, p in named}, grad={n: p.grad.detach().clone() for n, p in named},
                labels=np.concatenate(student.labels))


def signatures():
    from baselines.DERtrain import train_one_epoch_DER
    from baselines.FDRtrain import train_one_epoch_FDR
    from baselines.Lwftrain import train_one_epoch_Lwf
    res = {}
    for fn, arity in ((train_one_epoch_Lwf, 6), (train_one_epoch_DER, 5), (train_one_epoch_FDR, 5)):
        sig = inspect.signature(fn)
        res[fn.__name__] = dict(parameters=list(sig.parameters), returns=arity,
                                defaults={n: p.default for n, p in sig.parameters.items() if p.default is not inspect.Parameter.empty})
    return res


def lwf_zero():
    """The reference's L_old_kd_loss on CPU tensors of 2 and 1000 classes: value and the largest gradient element."""
    from baselines.Lwftrain import L_old_kd_loss
    rec = []
    for C in (2, 1000):
        g = torch.Generator().manual_seed(C)
        p = (3.0 * torch.randn(4, C, generator=g)).requires_grad_(True)
        v = L_old_kd_loss(p, 3.0 * torch.randn(4, C, generator=g), temperature=LWF_T)
        v.backward()
        rec.append([C, float(v), float(p.grad.abs().max())])
    return np.array(rec, dtype=np.float64)


def main():
    install_shims()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    args = sys.argv[1:]
    out = os.path.join(ROOT, "tests", "golden")
    if "--out" in args:
        out = args[args.index("--out") + 1]
    res = {"hyper": np.array([LR, WD, LWF_KD, LWF_REMAIN, LWF_T, DER_LAMBDA, DER_PLUS_LAMBDA, FDR_LAMBDA], dtype=np.float64), "lwf_zero": lwf_zero()}
    arity = {}
    for method in METERS:
        per = {}
        for teacher in ("copy", "far"):
            tag = f"{method}_{teacher}"
            a, b = run(method, teacher == "far", False), run(method, teacher == "far", True)
            arity[method] = a["n_out"]
            res.update(trainable=np.array(a["names"]))
            res[f"meters::{tag}"], res[f"meters64::{tag}"], res[f"labels::{tag}"] = a["meters"], b["meters"], a["labels"]
            if teacher == "far" and method in REG_COLUMN:
                assert (a["meters"][:, REG_COLUMN[method]] > 1e-2).all(), (tag, a["meters"])
            if teacher == "copy" and method in REG_COLUMN:
                assert a["meters"][0, REG_COLUMN[method]] == 0.0, (tag, a["meters"])
            if method == "lwf":
                assert (a["meters"][:, 1] == 0.0).all() and (b["meters"][:, 1] == 0.0).all(), "the reference's KD is an exact 0"
            for n in a["names"]:
                per[f"grad::{tag}::{n}"] = a["grad"][n].numpy().copy()
                per[f"grad_diff::{tag}::{n}"] = (b["grad"][n] - a["grad"][n].double()).float().numpy().copy()
                if teacher == "far":
                    per[f"final::{tag}::{n}"] = a["final"][n].numpy().copy()
                    per[f"final_diff::{tag}::{n}"] = (b["final"][n] - a["final"][n].double()).float().numpy().copy()
        H.save(out, f"distill_small_{method}", per)
    H.save(out, "distill_small", res)
    sig = signatures()
    assert [sig[k]["returns"] for k in sig] == [arity["lwf"], arity["der"], arity["fdr"]]
    with open(os.path.join(out, "distill_signatures.json"), "w") as f:
        json.dump(sig, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
