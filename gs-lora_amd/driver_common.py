"""What the drivers share: the model geometry, the class split of a task, and — for the baseline drivers (driver_reg, driver_scrub,
driver_distill, driver_lirf) — the common arguments, the --only_ffn trainability rule, the frozen teacher copy, the model without LoRA, the
device-resident synthetic task loaders, the evaluation around a task and the task record. Plain functions: every driver keeps its own
get_args, run_tasks and main."""
import copy
import json
import os
import random
import tempfile

import torch
from torch.utils.data import DataLoader, TensorDataset


def geometry(small, depth=None):
    """ViT_face's geometry keywords: the paper's 112 px / dim 512 / depth 6 model, or with `small` the shrunken one the tests run."""
    geo = (dict(image_size=48, patch_size=8, dim=128, depth=3, heads=2, mlp_dim=256) if small else
           dict(image_size=112, patch_size=8, dim=512, depth=6, heads=8, mlp_dim=2048))
    if depth is not None:
        geo["depth"] = depth
    return geo


def task_classes(order, num_class, per_forget_cls, task_i):
    """train_own_forget_cl.py:539-545 (st1 = 0, st2 = en1): task i forgets the last per_forget_cls classes of `order` that are not yet
    forgotten, the ones in front of them remain. -> (remain_cls, forget_cls)"""
    en1 = num_class - per_forget_cls - task_i * per_forget_cls
    return order[:en1], order[en1:en1 + per_forget_cls]


def add_common_args(p, net=True, ffn=True):
    """The options every baseline driver declares with one meaning. net: -n / --net; ffn: --ffn_open / --only_ffn."""
    if ffn:
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
    if net:
        p.add_argument("-n", "--net", default="VIT", choices=["VIT", "VITs"])
    p.add_argument("--head", default="CosFace", choices=["CosFace", "ArcFace", "Softmax"])
    p.add_argument("--outdir", default=None)
    p.add_argument("--seed", type=int, default=1337)


def mark_only_ffn_as_trainable(model, ffn_open=False):
    """train_own_forget_cl.py:425-439: requires_grad = "fn.fn.net" in name, or ("loss" in name and --ffn_open). -> the names that train"""
    names = []
    for name, param in model.named_parameters():
        param.requires_grad = "fn.fn.net" in name or (ffn_open and "loss" in name)
        if param.requires_grad:
            names.append(name)
    return names


def frozen_copy(model, dev):
    """train_own_forget_cl.py:440-443: the teacher — a deep copy in eval() with every parameter frozen."""
    teacher = copy.deepcopy(model).to(dev).eval()
    for p in teacher.parameters():
        p.requires_grad_(False)
    return teacher


def model_keywords(args, geo):
    return dict(loss_type=args.head, GPU_ID=[0], num_class=args.num_class, dropout=args.dropout, emb_dropout=args.dropout, lora_rank=0, **geo)


def build_ffn_model(args, geo, dev):
    """ViT_face / ViTs_face WITHOUT LoRA, the --only_ffn rule applied, on `dev` in args.dtype."""
    from util.utils import count_trainable_parameters
    from vit_pytorch_face import ViT_face, ViTs_face
    kw = model_keywords(args, geo)
    model = ViTs_face(ac_patch_size=12, pad=4, **kw) if args.net == "VITs" else ViT_face(**kw)
    names = mark_only_ffn_as_trainable(model, args.ffn_open)
    print("trainable parameters:", count_trainable_parameters(model), f"({len(names)} tensors)")
    return model.to(dev).set_compute_dtype(args.dtype)


def outdir(args, prefix):
    out = args.outdir or tempfile.mkdtemp(prefix=prefix)
    os.makedirs(out, exist_ok=True)
    return out


def eval_cfg(out, net):
    """What the loops' evaluate reads of the reference's cfg."""
    return {"DATA_ROOT": "./data/synthetic/", "MULTI_GPU": False, "WORK_PATH": out, "BACKBONE_NAME": net}


def subset(x, y, classes):
    """driver_cl.subset on device-resident tensors."""
    m = torch.isin(y, torch.tensor(classes, device=y.device))
    return TensorDataset(x[m], y[m])


def synthetic_task_data(args, image_size, dev, remain_key="loader_r"):
    """-> task_data(task_i) -> dict(loader_f, <remain_key>: the task's forget and remain training loaders, te_f, te_r: test loaders, info)
    over driver_cl's synthetic images, device-resident: the loaders index on the GPU."""
    import driver_cl
    order = list(range(args.num_class))
    random.seed(args.seed)
    random.shuffle(order)
    x_all, y_all = (t.to(dev) for t in driver_cl.synthetic_dataset(args.num_class, args.samples_per_class, image_size, args.seed))
    x_te, y_te = (t.to(dev) for t in driver_cl.synthetic_dataset(args.num_class, 2, image_size, args.seed + 1))

    def task_data(task_i):
        remain_cls, forget_cls = task_classes(order, args.num_class, args.per_forget_cls, task_i)
        gen = torch.Generator().manual_seed(args.seed + task_i)
        mk = lambda ds, bs, sh: DataLoader(ds, batch_size=bs, shuffle=sh, generator=gen if sh else None, drop_last=False)
        return {"loader_f": mk(subset(x_all, y_all, forget_cls), args.batch_size, True),
                remain_key: mk(subset(x_all, y_all, remain_cls), args.batch_size, True),
                "te_f": mk(subset(x_te, y_te, forget_cls), 5 * args.batch_size, False),
                "te_r": mk(subset(x_te, y_te, remain_cls), 5 * args.batch_size, False), "info": dict(forget_cls=forget_cls)}

    return task_data


def eval_task(evaluate, td, task_i, when):
    """evaluate(loader, tag) -> accuracy. -> (forget, remain) accuracy on the task's test loaders; when: "before" | "after"."""
    return evaluate(td["te_f"], f"forget-{task_i}-{when}"), evaluate(td["te_r"], f"remain-{task_i}-{when}")


def meter_averages(meters):
    return {k: (v.avg if v.count else None) for k, v in meters.items()}


def append_record(path, report, rec, what):
    """One task's record: into `report`, as a line of the JSONL file at `path`, and on the terminal behind `what`."""
    report.append(rec)
    with open(path, "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(f"[task {rec['task']}] {what} forget {rec['forget_before']:.1f}->{rec['forget_after']:.1f}  "
          f"remain {rec['remain_before']:.1f}->{rec['remain_after']:.1f}")
