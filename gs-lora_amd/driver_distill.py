#!/usr/bin/env python
"""driver_distill — the build's counterpart of the reference's LwF, DER, DER++ and FDR baselines (train/train_own_forget_cl.py:440-443 the
teacher, :1286-1409 the three epoch loops), comparison rows of the paper's table against GS-LoRA.

Per task (run_tasks):
  teacher = copy.deepcopy(model).eval() with every parameter frozen (:440-443)
  --epochs calls of baselines.Lwftrain.train_one_epoch_Lwf / DERtrain.train_one_epoch_DER / FDRtrain.train_one_epoch_FDR on the task's
  forget and remain loaders
  evaluate forget / remain accuracy; one JSON record per task in <outdir>/distill_report.jsonl

Data are synthetic device-resident tensors as in driver_scrub.py (the reference's ImageFolder splitting is out of scope).

    python gs-lora_amd/driver_distill.py --method derpp --small --num_class 20 --per_forget_cls 4 --num_tasks 2 --epochs 1

--method lwf | der | derpp | fdr stands for the reference's --Lwf, --Der, --Der --DER_plus and --FDR; the lambdas and --Lwf_T keep the
reference's names and defaults (util/args.py:273-295). The model is built WITHOUT LoRA and the reference's --only_ffn rule (:432-439) is
ALWAYS applied, as in driver_scrub.py: the two FFN linears of every block train, the `loss` head trains with --ffn_open, every other backbone
weight stays frozen (DESIGN.md sections 9 and 9n). LwF's distillation term is the reference's L_old_kd_loss as it ships: an exact zero
(baselines/Lwftrain.py), so an LwF run never runs its teacher.
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

NO_GPU = "gs-lora_amd driver_distill: no ROCm GPU is visible; the distillation baselines run on the HIP path, which has no CPU fallback"
METHODS = ("lwf", "der", "derpp", "fdr")
METERS = {"lwf": ("losses_CE", "losses_KD", "losses_total", "losses_remain"), "der": ("losses_CE", "losses_DER", "losses_total"),
          "derpp": ("losses_CE", "losses_DER", "losses_total"), "fdr": ("losses_CE", "losses_FDR", "losses_total")}


def get_args(argv=None):
    """The subset of the reference's util/args.py the three loops read (same names, types and defaults), plus driver_scrub's synthetic-data
    and model switches."""
    p = argparse.ArgumentParser(description="The LwF / DER / DER++ / FDR baselines on the FFN weights. The --only_ffn trainability rule of the "
                                            "reference is always applied: no other backbone weight trains on the HIP path.")
    p.add_argument("--method", required=True, choices=METHODS, help="lwf: --Lwf; der: --Der; derpp: --Der --DER_plus; fdr: --FDR")
    p.add_argument("--Lwf_T", default=2, type=float, help="temperature for Lwf")
    p.add_argument("--Lwf_lambda_kd", default=0.5, type=float, help="lambda kd for Lwf")
    p.add_argument("--Lwf_lambda_remain", default=1, type=float, help="lambda remain for Lwf")
    p.add_argument("--DER_lambda", default=0.1, type=float, help="lambda for DER")
    p.add_argument("--DER_plus_lambda", default=0.1, type=float, help="lambda for DER_plus")
    p.add_argument("--FDR_lambda", default=0.1, type=float, help="lambda for FDR")
    p.add_argument("--epochs", default=1, type=int, help="epochs over the forget loader per task")
    add_common_args(p)
    args = p.parse_args(argv)
    if args.method == "lwf" and args.num_class < 2:
        p.error("--method lwf needs --num_class >= 2: the reference's L_old_kd_loss is NaN for one class")
    return args


make_teacher = frozen_copy      # :440-443


def one_epoch(args, common, m):
    """One call of the method's loop; the meters of `m` are replaced by the ones the loop returns, as the reference's driver does."""
    if args.method == "lwf":
        from baselines.Lwftrain import train_one_epoch_Lwf
        batch, best_h, m["losses_CE"], m["losses_KD"], m["losses_remain"], m["losses_total"] = train_one_epoch_Lwf(
            lambda_kd=args.Lwf_lambda_kd, lambda_remain=args.Lwf_lambda_remain, temperature=args.Lwf_T, **common, **m)
    elif args.method in ("der", "derpp"):
        from baselines.DERtrain import train_one_epoch_DER
        batch, best_h, m["losses_CE"], m["losses_DER"], m["losses_total"] = train_one_epoch_DER(
            lambda_der=args.DER_lambda, plus=args.method == "derpp", lambda_der_plus=args.DER_plus_lambda, **common, **m)
    else:
        from baselines.FDRtrain import train_one_epoch_FDR
        batch, best_h, m["losses_CE"], m["losses_FDR"], m["losses_total"] = train_one_epoch_FDR(reg_lambda=args.FDR_lambda, **common, **m)
    return batch, best_h


def run_tasks(model, args, task_data, dev, out):
    """task_data(task_i) -> dict(loader_f, loader_r: the task's forget and remain training loaders, te_f, te_r: test loaders, info).
    -> report"""
    criterion = torch.nn.CrossEntropyLoss()
    cfg = eval_cfg(out, args.net)
    evaluate = lambda loader, tag: engine_cl.eval_data(model, loader, dev, tag)
    report = []
    path = os.path.join(out, "distill_report.jsonl")
    for task_i in range(args.num_tasks):
        td = task_data(task_i)
        teacher = make_teacher(model, dev)
        optimizer = create_optimizer(args, model)
        forget_before, remain_before = eval_task(evaluate, td, task_i, "before")
        model.train()
        batch, best_h = 0, 0.0
        m = {k: AverageMeter() for k in METERS[args.method]}
        epochs = []
        for epoch in range(args.epochs):
            common = dict(student_model=model, teacher_model=teacher, data_loader_cl_forget=td["loader_f"], remain_loader=td["loader_r"],
                          criterion=criterion, optimizer=optimizer, device=dev, epoch=epoch, batch=batch, task_i=task_i,
                          testloader_forget=td["te_f"], testloader_remain=td["te_r"], highest_H_mean=best_h, forget_acc_before=forget_before, cfg=cfg)
            batch, best_h = one_epoch(args, common, m)
            epochs.append(meter_averages(m))
        forget_after, remain_after = eval_task(evaluate, td, task_i, "after")
        model.train()
        rec = dict(task=task_i, method=args.method, steps=batch, epochs=epochs, forget_before=forget_before, forget_after=forget_after,
                   remain_before=remain_before, remain_after=remain_after, **td.get("info", {}))
        append_record(path, report, rec, f"{args.method} steps={batch}")
    return report


def main(argv=None):
    args = get_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError(NO_GPU)
    torch.manual_seed(args.seed)
    dev = torch.device("cuda")
    geo = geometry(args.small)
    out = outdir(args, "gslora_distill_")
    model = build_ffn_model(args, geo, dev)
    report = run_tasks(model, args, synthetic_task_data(args, geo["image_size"], dev), dev, out)
    return report, out, model


if __name__ == "__main__":
    main()
