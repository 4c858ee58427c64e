#!/usr/bin/env python
"""driver_probe — the build's counterpart of the reference's linear-probe driver (train/backbone_forget_main.py): after a forgetting
run, freeze everything but the classifier head (:596-600, the parameters whose name contains "loss"), retrain that head with plain
cross-entropy on a mix of forget and remain images (:649-670) and report forget / remain accuracy before training and after every
epoch (:637-638 and the per-epoch eval_data calls): can a fresh linear layer read the forgotten identities back out of the backbone's
features? The baseline drivers expose the same capability as --ffn_open (train_own_forget_cl.py:426).

Data are synthetic tensors as in driver_cl.py (the reference's ImageFolder splitting and subset sampling are out of scope).

    python gs-lora_amd/driver_probe.py --small --num_class 20 --per_forget_cls 4 --epochs 2

On the HIP path the step is gslora_hip.step.head_probe_step: the train-mode forward without saved activations, the CE kernels, one
gsl_head_wgrad launch and the fused AdamW.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import torch  # noqa: E402
from torch.utils.data import ConcatDataset, DataLoader  # noqa: E402

import engine_cl  # noqa: E402
from gslora_hip.optim import create_optimizer, create_scheduler  # noqa: E402
from gslora_hip.step import MeterQueue, head_probe_step  # noqa: E402
from util.utils import AverageMeter, count_trainable_parameters  # noqa: E402


class ProbeMeterQueue(MeterQueue):
    """MeterQueue over head_probe_step's [loss, prec1 %] packs (backbone_forget_main.py:664-665: both weighted with the batch size)."""
    ORDER = ("losses", "top1")
    WEIGHT = ("r", "r")


def mark_only_head_as_trainable(model):
    """backbone_forget_main.py:596-600, verbatim rule: requires_grad = ("loss" in name). -> the names that train"""
    names = []
    for name, param in model.named_parameters():
        param.requires_grad = "loss" in name
        if param.requires_grad:
            names.append(name)
    return names


def run_probe(model, args, loaders, dev):
    """model: a ViT_face / ViTs_face on `dev` (it is modified in place: pass a copy to keep the original).
    args: epochs, lr, min_lr, weight_decay and the optimizer / scheduler fields create_optimizer / create_scheduler read.
    loaders: dict(train=combined forget + remain loader, te_f=forget test loader, te_r=remain test loader).
    -> dict(trainable, forget_before, remain_before, forget_acc [per epoch], remain_acc [per epoch], losses [per-epoch average],
            top1 [per-epoch average], lrs, steps)"""
    names = mark_only_head_as_trainable(model)
    print("learnable_parameters", count_trainable_parameters(model), names)
    criterion = torch.nn.CrossEntropyLoss()
    optimizer = create_optimizer(args, model)
    scheduler, _ = create_scheduler(args, optimizer)
    model.train()                                                                    # :631
    forget_before = engine_cl.eval_data(model, loaders["te_f"], dev, "forget-probe-before")   # :637-638
    remain_before = engine_cl.eval_data(model, loaders["te_r"], dev, "remain-probe-before")
    rec = dict(trainable=names, forget_before=forget_before, remain_before=remain_before, forget_acc=[], remain_acc=[], losses=[], top1=[],
               lrs=[], steps=0)
    queue = ProbeMeterQueue()
    for epoch in range(args.epochs):                                                 # :643
        scheduler.step(epoch)                                                        # :645
        rec["lrs"].append(optimizer.param_groups[0]["lr"])
        model.train()
        meters = dict(losses=AverageMeter(), top1=AverageMeter())
        for inputs, labels in loaders["train"]:                                      # :649-670
            inputs, labels = inputs.to(dev), labels.to(dev).long()
            queue.push(head_probe_step(model, optimizer, criterion, inputs, labels), inputs.size(0), inputs.size(0))
            rec["steps"] += 1
        queue.flush(meters)                                                          # the epoch's one host read of the meters
        rec["losses"].append(meters["losses"].avg)
        rec["top1"].append(meters["top1"].avg)
        rec["forget_acc"].append(engine_cl.eval_data(model, loaders["te_f"], dev, f"forget-probe-{epoch}", rec["steps"]))
        rec["remain_acc"].append(engine_cl.eval_data(model, loaders["te_r"], dev, f"remain-probe-{epoch}", rec["steps"]))
        print(f"[probe epoch {epoch}] loss {meters['losses'].avg:.4f} prec@1 {meters['top1'].avg:.2f}  "
              f"forget {forget_before:.1f}->{rec['forget_acc'][-1]:.1f}  remain {remain_before:.1f}->{rec['remain_acc'][-1]:.1f}")
    model.train()
    return rec


def probe_loaders(x_tr, y_tr, x_te, y_te, forget_cls, remain_cls, batch_size, seed):
    """The combined training loader (forget + remain images, shuffled: the reference's combined_loader_train) and the two test loaders over
    synthetic tensors, built as driver_cl builds its loaders."""
    from driver_cl import subset
    gen = torch.Generator().manual_seed(seed)
    train = DataLoader(ConcatDataset([subset(x_tr, y_tr, forget_cls), subset(x_tr, y_tr, remain_cls)]), batch_size=batch_size, shuffle=True,
                       generator=gen)
    return dict(train=train, te_f=DataLoader(subset(x_te, y_te, forget_cls), batch_size=5 * batch_size),
                te_r=DataLoader(subset(x_te, y_te, remain_cls), batch_size=5 * batch_size))


def main(argv=None):
    import random

    import driver_cl
    from driver_common import geometry, task_classes
    from vit_pytorch_face import ViT_face, ViTs_face
    args = driver_cl.get_args(argv)
    torch.manual_seed(args.seed)
    dev = torch.device("cuda")
    geo = geometry(args.small)
    kw = dict(loss_type=args.head, GPU_ID=[0], num_class=args.num_class, dropout=args.dropout, emb_dropout=args.dropout, lora_rank=args.lora_rank, **geo)
    model = (ViTs_face(ac_patch_size=12, pad=4, **kw) if args.net == "VITs" else ViT_face(**kw)).to(dev).set_compute_dtype(args.dtype)
    if args.u8_input:
        model.set_input_norm("totensor")
    order = list(range(args.num_class))
    random.seed(args.seed)
    random.shuffle(order)
    remain_cls, forget_cls = task_classes(order, args.num_class, args.per_forget_cls, 0)
    x_tr, y_tr = driver_cl.synthetic_dataset(args.num_class, args.samples_per_class, geo["image_size"], args.seed, u8=args.u8_input)
    x_te, y_te = driver_cl.synthetic_dataset(args.num_class, 2, geo["image_size"], args.seed + 1, u8=args.u8_input)
    loaders = probe_loaders(x_tr, y_tr, x_te, y_te, forget_cls, remain_cls, args.batch_size, args.seed)
    return run_probe(model, args, loaders, dev), model


if __name__ == "__main__":
    main()
