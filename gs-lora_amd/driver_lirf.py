#!/usr/bin/env python
"""driver_lirf — the build's counterpart of the reference's LIRF baseline (train/train_own_forget_cl.py:330-422 the four half networks,
:1191-1240 the epoch loop), the last comparison row of the paper's table against GS-LoRA.

Per task (run_tasks):
  teacher_low, teacher_up (frozen, eval), student_low and deposit_low are filled from ONE full ViT_face state dict with strict=False
  (:389-399); the student's half of the previous task is the next task's checkpoint
  --epochs calls of baselines.LIRFtrain.train_one_epoch_LIRF on the task's forget and remain loaders
  eval_data_LIRF forget / remain accuracy; one JSON record per task in <outdir>/lirf_report.jsonl

Data are synthetic device-resident tensors as in driver_distill.py (the reference's ImageFolder splitting is out of scope).

    python gs-lora_amd/driver_lirf.py --small --num_class 20 --per_forget_cls 4 --num_tasks 2 --epochs 1 --LIRF_T 2

--LIRF_T and --LIRF_alpha keep the reference's names, types and defaults (util/args.py:237-238). The models are built WITHOUT LoRA and the
reference's --only_ffn rule is ALWAYS applied to student_low: the two FFN linears of its blocks train, every other weight stays frozen
(the reference's LIRF branch leaves all of student_low trainable; full-weight training is not on the HIP path: DESIGN.md section 9o).
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import torch  # noqa: E402

from driver_common import (add_common_args, append_record, eval_cfg, eval_task, geometry, mark_only_ffn_as_trainable, meter_averages,  # noqa: E402
                           model_keywords, outdir, synthetic_task_data)
from gslora_hip.optim import create_optimizer  # noqa: E402
from util.utils import AverageMeter, count_trainable_parameters  # noqa: E402

NO_GPU = "gs-lora_amd driver_lirf: no ROCm GPU is visible; the LIRF baseline runs on the HIP path, which has no CPU fallback"
METERS = ("losses_CE", "losses_AT", "kd_lossesKP", "losses_pt_re", "losses_total", "losses_remain")


def get_args(argv=None):
    """The subset of the reference's util/args.py the LIRF loop reads (same names, types and defaults), plus driver_distill's
    synthetic-data and model switches."""
    p = argparse.ArgumentParser(description="The LIRF baseline on the FFN weights of the student's lower half. The --only_ffn trainability "
                                            "rule of the reference is always applied: no other weight trains on the HIP path.")
    p.add_argument("--LIRF_T", default=10, type=float, help="lambda for LIRF")
    p.add_argument("--LIRF_alpha", default=0.1, type=float, help="lambda for LIRF")
    p.add_argument("--epochs", default=1, type=int, help="epochs over the forget loader per task")
    p.add_argument("--vit_depth", type=int, default=None, help="transformer depth (default 6, 3 with --small); the halves split at depth // 2")
    add_common_args(p, net=False, ffn=False)
    args = p.parse_args(argv)
    if not 0 < args.per_forget_cls < args.num_class:
        p.error("--per_forget_cls is the column at which LIRF cuts the logits: it must lie inside (0, num_class)")
    if args.vit_depth is not None and args.vit_depth < 2:
        p.error("--vit_depth must be at least 2: the lower half holds depth // 2 blocks")
    return args


def mark_student(student_low):
    """The reference's --only_ffn rule on the student's half: names containing fn.fn.net train. -> their names"""
    return mark_only_ffn_as_trainable(student_low)


def make_halves(kw, state, dev, dtype):
    """:330-422 — four half networks from one full state dict; the teachers frozen and in eval()."""
    from vit_pytorch_face import ViT_face_low, ViT_face_up
    nets = dict(teacher_low=ViT_face_low(**kw), teacher_up=ViT_face_up(**kw), student_low=ViT_face_low(**kw), deposit_low=ViT_face_low(**kw))
    for m in nets.values():
        res = m.load_state_dict(state, strict=False)
        assert not res.missing_keys, res.missing_keys
        m.to(dev).set_compute_dtype(dtype)
    for k in ("teacher_low", "teacher_up", "deposit_low"):
        for p in nets[k].parameters():
            p.requires_grad_(False)
    nets["teacher_low"].eval()
    nets["teacher_up"].eval()
    nets["deposit_low"].train()
    return nets


def run_tasks(kw, state, args, task_data, dev, out):
    """task_data(task_i) -> dict(loader_f, loader_r, te_f, te_r, info). state: the full ViT_face checkpoint. -> (report, the last student)"""
    from baselines.LIRFtrain import eval_data_LIRF, train_one_epoch_LIRF
    criterion = torch.nn.CrossEntropyLoss()
    cfg = {**eval_cfg(out, "VIT"), "PER_FORGET_CLS": args.per_forget_cls, "LIRF_T": args.LIRF_T, "LIRF_alpha": args.LIRF_alpha}
    report, nets = [], None
    path = os.path.join(out, "lirf_report.jsonl")
    for task_i in range(args.num_tasks):
        td = task_data(task_i)
        nets = make_halves(kw, state, dev, args.dtype)
        student, up = nets["student_low"], nets["teacher_up"]
        names = mark_student(student)
        print("trainable parameters:", count_trainable_parameters(student), f"({len(names)} tensors)")
        optimizer = create_optimizer(args, student)
        evaluate = lambda loader, tag: eval_data_LIRF(student, up, loader, dev, tag)
        forget_before, remain_before = eval_task(evaluate, td, task_i, "before")
        batch, best_h = 0, 0.0
        m = {k: AverageMeter() for k in METERS}
        epochs = []
        for epoch in range(args.epochs):
            out_ = train_one_epoch_LIRF(nets["student_low"], nets["deposit_low"], nets["teacher_low"], up, td["loader_f"], td["loader_r"], criterion,
                                        optimizer, dev, epoch, batch, *(m[k] for k in METERS), str(task_i), td["te_f"], td["te_r"], forget_before,
                                        best_h, cfg)
            batch, best_h = out_[0], out_[1]
            m = dict(zip(METERS, out_[2:]))
            epochs.append(meter_averages(m))
        forget_after, remain_after = eval_task(evaluate, td, task_i, "after")
        student.train()
        rec = dict(task=task_i, method="lirf", steps=batch, epochs=epochs, forget_before=forget_before, forget_after=forget_after,
                   remain_before=remain_before, remain_after=remain_after, best_H_mean=best_h, **td.get("info", {}))
        append_record(path, report, rec, f"lirf steps={batch}")
        # the next task starts from this task's student: its lower blocks replace the checkpoint's
        state = {**state, **{k: v.detach().clone() for k, v in student.state_dict().items() if k.startswith("transformer.layers.")}}
    return report, nets


def main(argv=None):
    from vit_pytorch_face import ViT_face
    args = get_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError(NO_GPU)
    torch.manual_seed(args.seed)
    dev = torch.device("cuda")
    geo = geometry(args.small, args.vit_depth)
    out = outdir(args, "gslora_lirf_")
    kw = model_keywords(args, geo)
    state = {k: v.detach().clone() for k, v in ViT_face(**kw).state_dict().items()}      # stands for the pretrained checkpoint
    report, nets = run_tasks(kw, state, args, synthetic_task_data(args, geo["image_size"], dev), dev, out)
    return report, out, nets


if __name__ == "__main__":
    main()
