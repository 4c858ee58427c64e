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
import copy
import json
import os
import random
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import torch  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

import engine_cl  # noqa: E402
from driver_reg import mark_only_ffn_as_trainable  # noqa: E402
from gslora_hip.optim import create_optimizer  # noqa: E402
from util.utils import AverageMeter, count_trainable_parameters  # noqa: E402

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
    p.add_argument("--ffn_open", default=False, action="store_true", help="train the `loss` head too (train_own_forget_cl.py:426)")
    p.add_argument("--only_ffn", default=True, action="store_true",
                   help="always on: the FFN linears (names containing fn.fn.net) are the backbone weights that train on the HIP path")
    p.add_argument("--num_class", type=int, default=100)
    p.add_argument("--num_tasks", type=int, default=4)
    p.add_argument("--per_forget_cls", type=int, default=20)
    p.add_argument("--batch_size", type=int, default=48)
    p.add_argument("--samples_per_class", type=int, default=8)
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--weight_decay", type=float, default=0.05)
    p.add_argument("--opt", default="adamw")
    p.add_argument("--opt_eps", type=float, default=1e-8)
    p.add_argument("--opt_betas", default=None)
    p.add_argument("--dropout", type=float, default=0.1)
    p.add_argument("--dtype", default=os.environ.get("GSLORA_DTYPE", "fp16"), help="fp16 | bf16 | fp32 | fp32x3")
    p.add_argument("--small", action="store_true", help="shrunken model (48 px, dim 128, depth 3) for tests")
    p.add_argument("-n", "--net", default="VIT", choices=["VIT", "VITs"])
    p.add_argument("--head", default="CosFace", choices=["CosFace", "ArcFace", "Softmax"])
    p.add_argument("--outdir", default=None)
    p.add_argument("--seed", type=int, default=1337)
    args = p.parse_args(argv)
    if args.method == "lwf" and args.num_class < 2:
        p.error("--method lwf needs --num_class >= 2: the reference's L_old_kd_loss is NaN for one class")
    return args


def make_teacher(model, dev):
    """:440-443"""
    teacher = copy.deepcopy(model).to(dev).eval()
    for p in teacher.parameters():
        p.requires_grad_(False)
    return teacher


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
    cfg = {"DATA_ROOT": "./data/synthetic/", "MULTI_GPU": False, "WORK_PATH": out, "BACKBONE_NAME": args.net}
    report = []
    path = os.path.join(out, "distill_report.jsonl")
    for task_i in range(args.num_tasks):
        td = task_data(task_i)
        teacher = make_teacher(model, dev)
        optimizer = create_optimizer(args, model)
        forget_before = engine_cl.eval_data(model, td["te_f"], dev, f"forget-{task_i}-before")
        remain_before = engine_cl.eval_data(model, td["te_r"], dev, f"remain-{task_i}-before")
        model.train()
        batch, best_h = 0, 0.0
        m = {k: AverageMeter() for k in METERS[args.method]}
        epochs = []
        for epoch in range(args.epochs):
            common = dict(student_model=model, teacher_model=teacher, data_loader_cl_forget=td["loader_f"], remain_loader=td["loader_r"],
                          criterion=criterion, optimizer=optimizer, device=dev, epoch=epoch, batch=batch, task_i=task_i,
                          testloader_forget=td["te_f"], testloader_remain=td["te_r"], highest_H_mean=best_h, forget_acc_before=forget_before, cfg=cfg)
            batch, best_h = one_epoch(args, common, m)
            epochs.append({k: (v.avg if v.count else None) for k, v in m.items()})
        forget_after = engine_cl.eval_data(model, td["te_f"], dev, f"forget-{task_i}-after")
        remain_after = engine_cl.eval_data(model, td["te_r"], dev, f"remain-{task_i}-after")
        model.train()
        rec = dict(task=task_i, method=args.method, steps=batch, epochs=epochs, forget_before=forget_before, forget_after=forget_after,
                   remain_before=remain_before, remain_after=remain_after, **td.get("info", {}))
        report.append(rec)
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(f"[task {task_i}] {args.method} steps={batch} forget {forget_before:.1f}->{forget_after:.1f}  remain {remain_before:.1f}->{remain_after:.1f}")
    return report


def main(argv=None):
    import driver_cl
    from vit_pytorch_face import ViT_face, ViTs_face
    args = get_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError(NO_GPU)
    torch.manual_seed(args.seed)
    dev = torch.device("cuda")
    geo = (dict(image_size=48, patch_size=8, dim=128, depth=3, heads=2, mlp_dim=256) if args.small else
           dict(image_size=112, patch_size=8, dim=512, depth=6, heads=8, mlp_dim=2048))
    out = args.outdir or tempfile.mkdtemp(prefix="gslora_distill_")
    os.makedirs(out, exist_ok=True)
    kw = dict(loss_type=args.head, GPU_ID=[0], num_class=args.num_class, dropout=args.dropout, emb_dropout=args.dropout, lora_rank=0, **geo)
    model = ViTs_face(ac_patch_size=12, pad=4, **kw) if args.net == "VITs" else ViT_face(**kw)
    names = mark_only_ffn_as_trainable(model, args.ffn_open)
    print("trainable parameters:", count_trainable_parameters(model), f"({len(names)} tensors)")
    model = model.to(dev).set_compute_dtype(args.dtype)
    order = list(range(args.num_class))
    random.seed(args.seed)
    random.shuffle(order)
    x_all, y_all = driver_cl.synthetic_dataset(args.num_class, args.samples_per_class, geo["image_size"], args.seed)
    x_te, y_te = driver_cl.synthetic_dataset(args.num_class, 2, geo["image_size"], args.seed + 1)
    x_all, y_all, x_te, y_te = x_all.to(dev), y_all.to(dev), x_te.to(dev), y_te.to(dev)      # device-resident: the loaders index on the GPU
    num_first = args.num_class - args.per_forget_cls

    def subset(x, y, classes):
        m = torch.isin(y, torch.tensor(classes, device=y.device))
        return torch.utils.data.TensorDataset(x[m], y[m])

    def task_data(task_i):
        en1 = num_first - task_i * args.per_forget_cls
        en2 = en1 + args.per_forget_cls
        remain_cls, forget_cls = order[:en1], order[en1:en2]
        gen = torch.Generator().manual_seed(args.seed + task_i)
        mk = lambda ds, bs, sh: DataLoader(ds, batch_size=bs, shuffle=sh, generator=gen if sh else None, drop_last=False)
        return dict(loader_f=mk(subset(x_all, y_all, forget_cls), args.batch_size, True),
                    loader_r=mk(subset(x_all, y_all, remain_cls), args.batch_size, True),
                    te_f=mk(subset(x_te, y_te, forget_cls), 5 * args.batch_size, False),
                    te_r=mk(subset(x_te, y_te, remain_cls), 5 * args.batch_size, False), info=dict(forget_cls=forget_cls))

    report = run_tasks(model, args, task_data, dev, out)
    return report, out, model


if __name__ == "__main__":
    main()
