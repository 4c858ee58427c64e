#!/usr/bin/env python
"""driver_scrub — the build's counterpart of the reference's SCRUB baseline (train/train_own_forget_cl.py:440-451 the teacher and the
averaged copy, :843-879 the meters and the optimizer, :1236-1285 the superepoch loop), a comparison row of the paper's table against GS-LoRA.

Per task (run_tasks):
  teacher = copy.deepcopy(model).eval() with every parameter frozen; swa_model = torch.optim.swa_utils.AveragedModel(model, avg_fn) with
  beta = 0.1 (:445-450), used as torch makes it: it is never run, and its one update per superepoch is torch ops
  --SCRUB_superepoch calls of baselines.SCRUBtrain.train_one_superepoch_SCRUB on the task's forget and remain loaders
  evaluate forget / remain accuracy; one JSON record per task in <outdir>/scrub_report.jsonl

Data are synthetic device-resident tensors as in driver_reg.py (the reference's ImageFolder splitting is out of scope).

    python gs-lora_amd/driver_scrub.py --small --num_class 20 --per_forget_cls 4 --num_tasks 2 --SCRUB_superepoch 1

The model is built WITHOUT LoRA and the reference's --only_ffn rule (:432-439) is ALWAYS applied, as in driver_reg.py: the two FFN linears of
every block train, the `loss` head trains with --ffn_open, every other backbone weight stays frozen (DESIGN.md sections 9 and 9m).
The optimizer is create_optimizer's FusedAdamW: with the reference's default --opt adamw none of its three SCRUB branches (sgd / adam /
rmsp, :860-879) matches, so the timm AdamW built before stays. Those three values are refused with that explanation.
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import torch  # noqa: E402

import engine_cl  # noqa: E402
from driver_common import (add_common_args, append_record, build_ffn_model, eval_cfg, eval_task, frozen_copy, geometry, meter_averages,  # noqa: E402
                           outdir, synthetic_task_data)
from gslora_hip.optim import create_optimizer  # noqa: E402
from util.utils import AverageMeter  # noqa: E402

NO_GPU = "gs-lora_amd driver_scrub: no ROCm GPU is visible; the SCRUB baseline runs on the HIP path, which has no CPU fallback"
SCRUB_OPTS = ("sgd", "adam", "rmsp")
BETA = 0.1      # :445


def get_args(argv=None):
    """The subset of the reference's util/args.py SCRUB reads (same names, types and defaults), plus driver_reg's synthetic-data and model
    switches. --opt sgd | adam | rmsp (the reference's SCRUB-only optimizers, :860-879) are refused: FusedAdamW is the optimizer here."""
    p = argparse.ArgumentParser(description="The SCRUB baseline on the FFN weights. The --only_ffn trainability rule of the reference is always "
                                            "applied: no other backbone weight trains on the HIP path.")
    p.add_argument("--SCRUB", default=True, action="store_true", help="always on (util/args.py:241)")
    p.add_argument("--sgda_smoothing", default=0.0, type=float, help="weight of the distance to the averaged copy")
    p.add_argument("--sgda_gamma", default=0.99, type=float, help="weight of the cross-entropy on the min steps")
    p.add_argument("--sgda_alpha", default=0.001, type=float, help="weight of the distillation KL on the min steps")
    p.add_argument("--SCRUB_superepoch", default=10, type=int, help="superepochs per task")
    p.add_argument("--kd_T", default=2.0, type=float, help="distillation temperature")
    p.add_argument("--scrub_decay_epoch", default=100, type=int, help="inner epoch behind which the rate decays")
    add_common_args(p)
    args = p.parse_args(argv)
    if args.opt.lower() in SCRUB_OPTS:
        p.error(f"--opt {args.opt}: the reference builds torch's SGD / Adam / RMSprop for SCRUB only under --opt sgd | adam | rmsp; with its "
                "default --opt adamw none of those branches matches and the timm AdamW stays, which is the optimizer of this build "
                "(FusedAdamW). The three torch optimizers are not on the HIP path.")
    return args


def scrub_cfg(args, out):
    """config.py:107-110 on top of what evaluate reads."""
    return {**eval_cfg(out, args.net), "lr_decay_rate": 0.1, "lr_decay_epochs": args.scrub_decay_epoch, "sgda_learning_rate": args.lr}


def make_teacher_and_average(model, dev):
    """:440-451"""
    # an exponential moving average: the new weights enter with BETA, the running average keeps the rest
    ema = lambda avg, new, n: avg * (1.0 - BETA) + new * BETA
    return frozen_copy(model, dev), torch.optim.swa_utils.AveragedModel(model, avg_fn=ema).to(dev)


def run_tasks(model, args, task_data, dev, out):
    """task_data(task_i) -> dict(loader_f, loader_r: the task's forget and remain training loaders, te_f, te_r: test loaders, info).
    -> report"""
    from baselines.SCRUBtrain import train_one_superepoch_SCRUB
    criterion = torch.nn.CrossEntropyLoss()
    cfg = scrub_cfg(args, out)
    evaluate = lambda loader, tag: engine_cl.eval_data(model, loader, dev, tag)
    report = []
    path = os.path.join(out, "scrub_report.jsonl")
    for task_i in range(args.num_tasks):
        td = task_data(task_i)
        teacher, swa_model = make_teacher_and_average(model, dev)
        optimizer = create_optimizer(args, model)
        forget_before, remain_before = eval_task(evaluate, td, task_i, "before")
        model.train()
        batch, best_h = 0, 0.0
        m = dict(losses_CE=AverageMeter(), losses_total_forget=AverageMeter(), losses_total_remain=AverageMeter(), losses_kd_remain=AverageMeter(),
                 losses_kd_forget=AverageMeter())
        superepochs = []
        for epoch in range(args.SCRUB_superepoch):                                   # :1248-1285
            (batch, best_h, m["losses_CE"], m["losses_total_forget"], m["losses_total_remain"], m["losses_kd_forget"], m["losses_kd_remain"],
             swa_model) = train_one_superepoch_SCRUB(
                student=model, teacher=teacher, swa_model=swa_model, data_loader_forget=td["loader_f"], remain_loader=td["loader_r"],
                criterion=criterion, optimizer=optimizer, device=dev, superepoch=epoch, batch=batch, task_i=task_i, testloader_forget=td["te_f"],
                testloader_remain=td["te_r"], highest_H_mean=best_h, forget_acc_before=forget_before, cfg=cfg, kd_T=args.kd_T,
                sgda_smoothing=args.sgda_smoothing, sgda_gamma=args.sgda_gamma, sgda_alpha=args.sgda_alpha, **m)
            superepochs.append(meter_averages(m))
        forget_after, remain_after = eval_task(evaluate, td, task_i, "after")
        model.train()
        rec = dict(task=task_i, steps=batch, superepochs=superepochs, kd_T=args.kd_T, sgda_smoothing=args.sgda_smoothing,
                   sgda_gamma=args.sgda_gamma, sgda_alpha=args.sgda_alpha, n_averaged=int(swa_model.n_averaged.item()),
                   forget_before=forget_before, forget_after=forget_after, remain_before=remain_before, remain_after=remain_after,
                   **td.get("info", {}))
        append_record(path, report, rec, f"SCRUB steps={batch}")
    return report


def main(argv=None):
    args = get_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError(NO_GPU)
    torch.manual_seed(args.seed)
    dev = torch.device("cuda")
    geo = geometry(args.small)
    out = outdir(args, "gslora_scrub_")
    model = build_ffn_model(args, geo, dev)
    report = run_tasks(model, args, synthetic_task_data(args, geo["image_size"], dev), dev, out)
    return report, out, model


if __name__ == "__main__":
    main()
