#!/usr/bin/env python
"""driver_reg — the build's counterpart of the reference's regularisation baselines (train/train_own_forget_cl.py:1411-1692, the "CL
baselines" branch of its task loop): L2, EWC and MAS on the FFN weights, the comparison rows of the paper's table against GS-LoRA.

Per task (run_tasks):
  task 0: back up task_param (:1416-1420) and compute the importance on the first remain set (:1423-1569) -> regularization_terms[0]
  epochs of engine_reg.train_one_epoch_regularzation on the task's forget loader with reg_lambda = --l2_lambda | --ewc_lambda | --mas_lambda
  back up task_param again (:1629-1633); unless it was the last task, compute the importance on the NEXT task's remain set (:1637-1680)
  and store it as regularization_terms[task + 1] — or, with --online, as regularization_terms[0], the accumulation continuing IN PLACE
  from the previous importance (:1448-1449, :1681-1685)
  evaluate forget / remain accuracy; one JSON record per task in <outdir>/reg_report.jsonl

Data are synthetic device-resident tensors as in driver_cl.py (the reference's ImageFolder splitting is out of scope).

    python gs-lora_amd/driver_reg.py --small --num_class 20 --per_forget_cls 4 --num_tasks 2 --epochs 1 --ewc

The model is built WITHOUT LoRA and the reference's --only_ffn rule (:432-439) is ALWAYS applied: the two FFN linears of every block train,
the `loss` head trains with --ffn_open (:426), every other backbone weight stays frozen — those do not train on the HIP path (DESIGN.md
section 9).
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import torch  # noqa: E402

import engine_cl  # noqa: E402
import engine_reg  # noqa: E402
from driver_common import (add_common_args, append_record, build_ffn_model, eval_cfg, eval_task, geometry, mark_only_ffn_as_trainable,  # noqa: E402, F401
                           meter_averages, outdir, synthetic_task_data)
from gslora_hip.optim import create_optimizer, create_scheduler  # noqa: E402
from util.utils import AverageMeter  # noqa: E402

NO_GPU = "gs-lora_amd driver_reg: no ROCm GPU is visible; the regularisation baselines run on the HIP path, which has no CPU fallback"


def get_args(argv=None):
    """The subset of the reference's util/args.py the baselines read (same names, types and defaults), plus driver_cl's synthetic-data and
    model switches."""
    p = argparse.ArgumentParser(description="L2 / EWC / MAS baselines on the FFN weights. The --only_ffn trainability rule of the reference is "
                                            "always applied: no other backbone weight trains on the HIP path.")
    kind = p.add_mutually_exclusive_group(required=True)
    kind.add_argument("--l2", default=False, action="store_true", help="identity importance (util/args.py:205)")
    kind.add_argument("--ewc", default=False, action="store_true", help="squared gradients of the criterion (util/args.py:211)")
    kind.add_argument("--MAS", default=False, action="store_true", help="absolute gradients of mean(logits^2) (util/args.py:215)")
    p.add_argument("--l2_lambda", type=float, default=0.1)
    p.add_argument("--ewc_lambda", type=float, default=0.1)
    p.add_argument("--mas_lambda", type=float, default=0.1)
    p.add_argument("--online", default=False, action="store_true", help="keep ONE term and accumulate its importance across tasks")
    p.add_argument("--epochs", type=int, default=2)
    p.add_argument("--min_lr", type=float, default=1e-5)
    p.add_argument("--sched", default="cosine")
    p.add_argument("--warmup_epochs", type=int, default=0)
    p.add_argument("--warmup_lr", type=float, default=1e-6)
    p.add_argument("--cooldown_epochs", type=int, default=10)
    add_common_args(p)
    return p.parse_args(argv)


def kind_of(args):
    return ("l2", args.l2_lambda) if args.l2 else ("ewc", args.ewc_lambda) if args.ewc else ("mas", args.mas_lambda)


def backup(model):
    """:1416-1420 / :1629-1633"""
    return {n: p.clone().detach() for n, p in model.named_parameters() if p.requires_grad}


def run_tasks(model, args, task_data, dev, out):
    """task_data(task_i) -> dict(loader_f: the task's forget training loader, loader_imp: the remain loader the importance of THIS task's
    term is computed on, te_f, te_r: test loaders, info). -> (report, regularization_terms)"""
    from gslora_hip import reg
    kind, reg_lambda = kind_of(args)
    criterion = torch.nn.CrossEntropyLoss()
    cfg = eval_cfg(out, args.net)
    evaluate = lambda loader, tag: engine_cl.eval_data(model, loader, dev, tag)
    terms, report = {}, []
    model.train()                                                                    # :1412
    path = os.path.join(out, "reg_report.jsonl")
    for task_i in range(args.num_tasks):
        td = task_data(task_i)
        skipped = 0
        if task_i == 0:                                                              # :1414-1569
            task_param = backup(model)
            importance = reg.calculate_importance(model, td["loader_imp"], kind, criterion=criterion, device=dev)
            skipped += importance.skipped
            terms[0] = {"importance": importance, "task_param": task_param}
        optimizer = create_optimizer(args, model)
        scheduler, _ = create_scheduler(args, optimizer)
        forget_before, remain_before = eval_task(evaluate, td, task_i, "before")
        model.train()
        batch, best_h = 0, 0.0
        m = dict(losses_CE=AverageMeter(), losses_regularization=AverageMeter(), losses_total=AverageMeter())
        epochs = []
        for epoch in range(args.epochs):                                             # :1580-1627
            scheduler.step(epoch)
            batch, best_h, m["losses_CE"], m["losses_regularization"], m["losses_total"] = engine_reg.train_one_epoch_regularzation(
                model=model, criterion=criterion, data_loader_cl_forget=td["loader_f"], optimizer=optimizer, device=dev, epoch=epoch,
                batch=batch, reg_lambda=reg_lambda, regularization_terms=terms, task_i=task_i, testloader_forget=td["te_f"],
                testloader_remain=td["te_r"], highest_H_mean=best_h, forget_acc_before=forget_before, cfg=cfg, **m)
            epochs.append(meter_averages(m))
        task_param = backup(model)                                                   # :1629-1633
        if task_i < args.num_tasks - 1:                                              # :1637-1690: the NEXT task's remain set
            nxt = task_data(task_i + 1)
            online = args.online and len(terms) > 0
            importance = reg.calculate_importance(model, nxt["loader_imp"], kind, criterion=criterion, device=dev,
                                                  prior=terms[0]["importance"] if online and kind != "l2" else None)
            skipped += importance.skipped
            terms[0 if online else task_i + 1] = {"importance": importance, "task_param": task_param}
        forget_after, remain_after = eval_task(evaluate, td, task_i, "after")
        model.train()
        last = terms[max(terms)]["importance"]
        rec = dict(task=task_i, kind=kind, reg_lambda=reg_lambda, online=bool(args.online), steps=batch, n_terms=len(terms), epochs=epochs,
                   importance_sum=float(sum(v.double().sum() for v in last.values())), skipped_importance_batches=skipped,
                   forget_before=forget_before, forget_after=forget_after, remain_before=remain_before, remain_after=remain_after,
                   **td.get("info", {}))
        append_record(path, report, rec, f"{kind} lambda={reg_lambda} terms={len(terms)} steps={batch}")
    return report, terms


def main(argv=None):
    args = get_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError(NO_GPU)
    torch.manual_seed(args.seed)
    dev = torch.device("cuda")
    geo = geometry(args.small)
    out = outdir(args, "gslora_reg_")
    model = build_ffn_model(args, geo, dev)
    task_data = synthetic_task_data(args, geo["image_size"], dev, remain_key="loader_imp")      # (the split of :1639-1643)
    report, terms = run_tasks(model, args, task_data, dev, out)
    return report, out, (model, terms)


if __name__ == "__main__":
    main()
