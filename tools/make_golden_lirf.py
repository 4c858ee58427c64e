#!/usr/bin/env python
"""Fixtures of the LIRF baseline from the REAL reference: baselines/LIRFtrain.train_one_epoch_LIRF on the real ViT_face_low / ViT_face_up,
imported unmodified through oracle.make_golden.install_shims (run where the reference checkout is available):

    python tools/make_golden_lirf.py                # tests/golden/lirf_<cfg>.npz, lirf_<cfg>_<teacher>_<kind>.npz, lirf_signatures.json

Set-up (tests/test_hip_lirf.py restates it): recipe.cfg_small2(lora_rank=0) (depth 3: the odd split) and recipe.cfg_small(lora_rank=0)
(depth 2: one block each side), CosFace, dropout 0; the four half networks filled from one full state dict with strict=False; the
reference's --only_ffn rule (names containing fn.fn.net) applied to the real student_low BEFORE the real loop is called — the reference's
LIRF branch leaves all of student_low trainable, full-weight training is not on the HIP path; AdamW at 1e-4 / weight decay 0.05 in timm's
grouping (no decay for biases); the forget loader 3 x 3 images and the remain loader 3 x 2 (seeds 40 - 42); split = num_class // 2, T = 2,
alpha = 0.5. Teachers `copy` (the checkpoint itself) and `far` (every FFN weight matrix, lower blocks included, scaled element-wise by
recipe.uniform("far::" + name, shape, 77, 0.7, 1.3)); an f32 and an f64 run of each.

Recorded per tag <teacher>: the per-step meters [CE, AT, KP, PT_RE, total, REPLAY] of both runs; the last step's gradients and (far
teacher) the final weights of the trainable tensors with their f64 - f32 differences, one file per teacher and kind so that every file
stays below the size limit; the teacher's and the student's at() tables of step 1.
lirf_signatures.json: parameter names, defaults and return arity of the three loop functions and the state-dict key names of the two
half networks (names only). No reference text is stored.
"""
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

LR, WD, SEEDS = 1e-4, 0.05, (40, 41, 42)
LIRF_T, ALPHA = 2.0, 0.5
METERS = ("losses_CE", "losses_AT", "kd_lossesKP", "losses_pt_re", "losses_total", "losses_remain")
FAR_SEED, FAR_LO, FAR_HI = 77, 0.7, 1.3
CFGS = {"small2": lambda: recipe.cfg_small2(lora_rank=0), "small": lambda: recipe.cfg_small(lora_rank=0)}


def kwargs_of(cfg):
    return dict(loss_type="CosFace", GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
                dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], dropout=0.0, emb_dropout=0.0, lora_rank=0)


def far_state(state):
    return {n: (v * recipe.uniform("far::" + n, tuple(v.shape), FAR_SEED, FAR_LO, FAR_HI) if ("fn.fn.net" in n and n.endswith("weight")) else v)
            for n, v in state.items()}


class InDouble(torch.nn.Module):
    """The float64 run: the loop hands a lower half the f32 batch; cast it up in front of the float64 model."""

    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, x):
        return self.m(x.double())


class Tap(torch.nn.Module):
    """Keeps the mid streams a lower half returned, in order."""

    def __init__(self, m):
        super().__init__()
        self.m, self.mids = m, []

    def forward(self, x):
        out = self.m(x)
        self.mids.append(out.detach().clone())
        return out


def loaders(cfg):
    forget, remain = [], []
    for s in SEEDS:
        x_r, y_r, x_f, y_f = H.batches(cfg, 3, s)
        forget.append((x_f, y_f))
        remain.append((x_r[:2], y_r[:2]))
    return forget, remain


def run(cfg, far, double):
    from baselines.LIRFtrain import at, train_one_epoch_LIRF
    from util import utils as rutil
    from vit_pytorch_face import ViT_face_low, ViT_face_up

    class Recording(rutil.AverageMeter):
        def __init__(self):
            super().__init__()
            self.seen = []

        def update(self, val, n=1):
            self.seen.append(float(val))
            super().update(val, n)

    state = F.state_without_lora(cfg)
    t_state = far_state(state) if far else state
    load = lambda m, st: (m.load_state_dict({k: torch.tensor(v) for k, v in st.items()}, strict=False), m)[1]
    student, deposit = load(ViT_face_low(**kwargs_of(cfg)), state), load(ViT_face_low(**kwargs_of(cfg)), state)
    t_low, t_up = load(ViT_face_low(**kwargs_of(cfg)), t_state), load(ViT_face_up(**kwargs_of(cfg)), t_state)
    for m in (t_low, t_up):
        for p in m.parameters():
            p.requires_grad = False
    for n, p in student.named_parameters():      # the --only_ffn rule on the real student_low
        p.requires_grad = "fn.fn.net" in n
    names = [n for n, p in student.named_parameters() if p.requires_grad]
    if double:
        student, deposit, t_low, t_up = student.double(), deposit.double(), t_low.double(), t_up.double()
    named = [(n, p) for n, p in student.named_parameters() if p.requires_grad]
    no_decay = [p for n, p in named if p.ndim <= 1 or n.endswith(".bias")]
    decay = [p for n, p in named if not (p.ndim <= 1 or n.endswith(".bias"))]
    opt = torch.optim.AdamW([dict(params=no_decay, weight_decay=0.0), dict(params=decay, weight_decay=WD)], lr=LR, eps=1e-8, betas=(0.9, 0.999))
    wrap = (lambda m: Tap(InDouble(m))) if double else Tap
    s_tap, t_tap = wrap(student), wrap(t_low)
    d_in = InDouble(deposit) if double else deposit
    forget, remain = loaders(cfg)
    m = {k: Recording() for k in METERS}
    split = cfg["num_class"] // 2
    out = train_one_epoch_LIRF(s_tap, d_in, t_tap, t_up, forget, remain, torch.nn.CrossEntropyLoss(), opt, torch.device("cpu"), 0, 0,
                               *(m[k] for k in METERS), "0", None, None, 0.0, 0.0, dict(PER_FORGET_CLS=split, LIRF_T=LIRF_T, LIRF_alpha=ALPHA))
    assert out[0] == len(forget) and all(len(m[k].seen) == len(forget) for k in m)
    meters = np.array([m[k].seen for k in METERS], dtype=np.float64).T.copy()
    # the student's taps alternate forget / remain mids; the teacher's are the forget mids
    s_mids, t_mids = s_tap.mids[0::2], t_tap.mids
    under = []
    for a_s, a_t in zip(s_mids, t_mids):
        for mid in (a_s, a_t):
            raw = torch.nn.functional.normalize(mid.double().pow(2).mean(1).view(mid.size(0), -1))
            if far:
                assert float(((raw - 0.005).abs() / 0.005).min()) > 1e-3, "an at() entry sits on the 0.005 threshold"
            under.append(float((raw < 0.005).double().mean()))
    print(f"  at() entries under the threshold: {max(under):.4f} at most (per step and network)")
    return dict(names=names, meters=meters, n_out=len(out), final={n: p.detach().clone() for n, p in named},
                grad={n: p.grad.detach().clone() for n, p in named}, at_s=at(s_mids[0].clone()).numpy().copy(), at_t=at(t_mids[0].clone()).numpy().copy())


def signatures():
    from baselines.LIRFtrain import eval_data_LIRF, evaluate_LIRF, train_one_epoch_LIRF
    from vit_pytorch_face import ViT_face_low, ViT_face_up
    res = {}
    for fn, arity in ((train_one_epoch_LIRF, 8), (eval_data_LIRF, 1), (evaluate_LIRF, 1)):
        sig = inspect.signature(fn)
        res[fn.__name__] = dict(parameters=list(sig.parameters), returns=arity,
                                defaults={n: p.default for n, p in sig.parameters.items() if p.default is not inspect.Parameter.empty})
    for name, cfg in (("depth2", recipe.cfg_small(lora_rank=0)), ("depth3", recipe.cfg_small2(lora_rank=0))):
        for cls in (ViT_face_low, ViT_face_up):
            res[f"{cls.__name__}::{name}"] = list(cls(**kwargs_of(cfg)).state_dict().keys())
            sig = inspect.signature(cls.__init__)
            res[f"{cls.__name__}::init"] = dict(parameters=[n for n in sig.parameters if n != "self"],
                                                defaults={n: p.default for n, p in sig.parameters.items() if p.default is not inspect.Parameter.empty})
    return res


def main():
    install_shims()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    args = sys.argv[1:]
    out = os.path.join(ROOT, "tests", "golden")
    if "--out" in args:
        out = args[args.index("--out") + 1]
    for name, make in CFGS.items():
        cfg = make()
        res, per = {"hyper": np.array([LR, WD, LIRF_T, ALPHA, cfg["num_class"] // 2], dtype=np.float64)}, {}
        for teacher in ("copy", "far"):
            print(f"[golden] lirf {name} {teacher}")
            a, b = run(cfg, teacher == "far", False), run(cfg, teacher == "far", True)
            assert a["n_out"] == 8
            res.update(trainable=np.array(a["names"]))
            res[f"meters::{teacher}"], res[f"meters64::{teacher}"] = a["meters"], b["meters"]
            res[f"at_s::{teacher}"], res[f"at_t::{teacher}"] = a["at_s"], a["at_t"]
            if teacher == "far":
                assert (a["meters"][:, 1] > 0).all() and (b["meters"][:, 1] > 0).all(), ("AT > 0 at every step", a["meters"])
            else:
                assert a["meters"][0, 1] == 0.0 and b["meters"][0, 1] == 0.0, ("a copied teacher: AT of step 1 is an exact 0", a["meters"])
            for n in a["names"]:
                per[f"grad::{teacher}::{n}"] = a["grad"][n].numpy().copy()
                per[f"grad_diff::{teacher}::{n}"] = (b["grad"][n] - a["grad"][n].double()).float().numpy().copy()
                if teacher == "far":
                    per[f"final::{teacher}::{n}"] = a["final"][n].numpy().copy()
                    per[f"final_diff::{teacher}::{n}"] = (b["final"][n] - a["final"][n].double()).float().numpy().copy()
        H.save(out, f"lirf_{name}", res)
        # one file per teacher and kind: every committed file stays below the size limit
        for kind, teacher in sorted({tuple(k.split("::")[:2]) for k in per}):
            H.save(out, f"lirf_{name}_{teacher}_{kind}", {k: v for k, v in per.items() if k.startswith(f"{kind}::{teacher}::")})
    with open(os.path.join(out, "lirf_signatures.json"), "w") as f:
        json.dump(signatures(), f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
