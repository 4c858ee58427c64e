"""Golden fixtures of the regularisation baselines (L2 / EWC / MAS), from the REAL reference (imported unmodified through
oracle.make_golden.install_shims) on the deterministic recipe of oracle/recipe.py. Runs only where the reference sources are checked out
(the build machine); the tests read the arrays alone.

    python tools/make_golden_reg_baselines.py                           # both fixtures
    python tools/make_golden_reg_baselines.py importance_small          # one of them
    python tools/make_golden_reg_baselines.py --out DIR [tags ...]      # into another directory

Writes tests/golden/ (both on cfg_small(lora_rank=0), CosFace, the --only_ffn trainability rule of train/train_own_forget_cl.py:432-439):
  importance_small.npz
        The importance loops of train_own_forget_cl.py:1444-1512 (EWC) and :1524-1561 (MAS) over a loader of two batches, 3 and 2 images
        (the recipe's remain batches of seeds 0 and 1). The loops are closures inside the reference's main(), so they cannot be imported:
        the reference's MODEL in eval() and torch's CrossEntropyLoss (its LOSS) run here under torch autograd, and the accumulation is stated
        in this file's own words — omega += grad ** 2 * len(batch) / len(loader) for EWC, omega += |grad| / len(loader) for MAS, with
        the MAS objective mean(logits ** 2). `grad_ewc::b::name`, `grad_mas::b::name`: the per-batch gradients; `ewc::name`, `mas::name`:
        the importance from zeros; `ewc_online::name`: a second EWC pass over the same loader (the model has not moved: the same
        gradients) started from `ewc::name`, the reference's --online; `batch_sizes`, `y::b`.
  reg_epoch_small_engine.npz
        The real engine_cl.train_one_epoch_regularzation (engine_cl.py:463-568) over a loader of six batches of 2 images with
        torch.optim.AdamW in timm's grouping and TWO terms: term 0 the EWC importance of importance_small with the initial weights as
        task_param, term 1 an identity (L2) importance whose task_param is the initial weights shifted by SHIFT. `steps` [5, 3]: the
        (CE, regularisation, total) the engine fed its meters in steps 1-5 (a recording AverageMeter; the engine re-binds fresh meters at
        its display in step 5); `returned` [3, 4]: (val, avg, sum, count) of the three meters it returns (they hold step 6); `batch`: the
        returned batch count; `final::*`: every trainable tensor after step 6; `y1..y6`, `hyper_lr`, `hyper_wd`, `reg_lambda`, `shift`.
No reference text is copied or edited.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import recipe  # noqa: E402
from oracle.make_golden import HYPER, install_shims  # noqa: E402
import make_golden_ffn_train as F  # noqa: E402
import make_golden_heads as H  # noqa: E402

REG_LAMBDA = 4.0      # the L2 term alone is 33e3 * SHIFT^2 = 3.3 at the first step, times lambda about a third of the cross-entropy
SHIFT = 0.01
SIZES = (3, 2)


def model_and_names():
    cfg = recipe.cfg_small(lora_rank=0)
    model = F.build_reference(cfg, F.state_without_lora(cfg))
    return cfg, model, F.only_ffn_trainable(model)


def importance_pass(model, cfg, seeds, objective):
    """-> (per-batch gradients [{name: array}], labels). objective(logits, y) -> the scalar the pass differentiates."""
    model.eval()
    grads, labels = [], []
    for size, seed in zip(SIZES, seeds):
        x, y, _, _ = H.batches(cfg, size, seed)
        outputs, _ = model(x.float(), y)
        loss = objective(outputs, y)
        model.zero_grad()
        loss.backward()
        grads.append({n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
        labels.append(y.numpy().copy())
    model.train()
    return grads, labels


def accumulate(omega, grads, kind):
    n_batches = len(grads)
    for size, g in zip(SIZES, grads):
        for n, om in omega.items():
            if n in g:
                if kind == "ewc":
                    om += g[n] ** 2 * size / n_batches
                else:
                    om += g[n].abs() / n_batches
    return omega


def ewc_importance(model, cfg, names):
    ce = torch.nn.CrossEntropyLoss()
    g, y = importance_pass(model, cfg, (0, 1), lambda o, t: ce(o, t))
    zeros = {n: torch.zeros_like(p) for n, p in model.named_parameters() if n in names}
    return accumulate(zeros, g, "ewc"), g, y


def importance_case(tag, out):
    cfg, model, names = model_and_names()
    ce = torch.nn.CrossEntropyLoss()
    ewc, g_ewc, y = ewc_importance(model, cfg, names)
    g_mas, _ = importance_pass(model, cfg, (0, 1), lambda o, t: o.pow(2).mean())
    mas = accumulate({n: torch.zeros_like(v) for n, v in ewc.items()}, g_mas, "mas")
    g_ewc2, _ = importance_pass(model, cfg, (0, 1), lambda o, t: ce(o, t))
    assert all(torch.equal(a[n], b[n]) for a, b in zip(g_ewc, g_ewc2) for n in names)
    online = accumulate({n: v.clone() for n, v in ewc.items()}, g_ewc2, "ewc")
    assert model.training
    res = {"trainable": np.array(names), "batch_sizes": np.array(SIZES, dtype=np.int64)}
    for b in range(len(SIZES)):
        res[f"y::{b}"] = y[b]
        for n in names:
            res[f"grad_ewc::{b}::{n}"] = g_ewc[b][n].numpy().copy()
            res[f"grad_mas::{b}::{n}"] = g_mas[b][n].numpy().copy()
    for n in names:
        res[f"ewc::{n}"], res[f"mas::{n}"], res[f"ewc_online::{n}"] = ewc[n].numpy().copy(), mas[n].numpy().copy(), online[n].numpy().copy()
    H.save(out, tag, res)


def epoch_case(tag, out, n_steps=6):
    import engine_cl
    from util import utils as rutil

    class Recording(rutil.AverageMeter):
        def __init__(self):
            super().__init__()
            self.seen = []

        def update(self, val, n=1):
            self.seen.append(float(val))
            super().update(val, n)

    cfg, model, names = model_and_names()
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    no_decay = [p for n, p in named if p.ndim <= 1 or n.endswith(".bias")]
    decay = [p for n, p in named if not (p.ndim <= 1 or n.endswith(".bias"))]
    opt = torch.optim.AdamW([dict(params=no_decay, weight_decay=0.0), dict(params=decay, weight_decay=HYPER["wd"])], lr=HYPER["lr"], eps=1e-8,
                            betas=(0.9, 0.999))
    ewc, _, _ = ewc_importance(model, cfg, names)
    terms = {0: {"importance": ewc, "task_param": {n: p.clone().detach() for n, p in named}},
             1: {"importance": {n: p.clone().detach().fill_(1) for n, p in named}, "task_param": {n: p.clone().detach() + SHIFT for n, p in named}}}
    loader, res = [], {"trainable": np.array(names), "hyper_lr": np.float64(HYPER["lr"]), "hyper_wd": np.float64(HYPER["wd"]),
                       "reg_lambda": np.float64(REG_LAMBDA), "shift": np.float64(SHIFT)}
    for s in range(n_steps):
        x, y, _, _ = H.batches(cfg, 2, 10 + s)
        loader.append((x, y))
        res[f"y{s + 1}"] = y.numpy().copy()
    meters = [Recording(), Recording(), Recording()]
    batch, _, m_ce, m_reg, m_total = engine_cl.train_one_epoch_regularzation(
        model=model, criterion=torch.nn.CrossEntropyLoss(), data_loader_cl_forget=loader, optimizer=opt, device=torch.device("cpu"), epoch=0,
        batch=0, reg_lambda=REG_LAMBDA, regularization_terms=terms, losses_CE=meters[0], losses_regularization=meters[1],
        losses_total=meters[2], task_i=0, testloader_forget=None, testloader_remain=None, forget_acc_before=0.0, highest_H_mean=0.0, cfg={})
    assert batch == n_steps and all(len(m.seen) == 5 for m in meters)
    res["steps"] = np.array([m.seen for m in meters], dtype=np.float64).T.copy()
    res["returned"] = np.array([[m.val, m.avg, m.sum, m.count] for m in (m_ce, m_reg, m_total)], dtype=np.float64)
    res["batch"] = np.int64(batch)
    res.update({f"final::{n}": p.detach().numpy().copy() for n, p in named})
    H.save(out, tag, res)


CASES = {"importance_small": importance_case, "reg_epoch_small_engine": epoch_case}


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
