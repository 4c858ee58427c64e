#!/usr/bin/env python
"""Cost of the linear probe (a trainable classifier head), one process, one build. Prints one JSON line; profiles/head_probe.md holds the
numbers of the last run.

  (a) kernel   one gsl_head_wgrad launch at B = 1024, C = 100, D = 512 for the three head kinds, against torch eager computing the same
               gradient from the same device tensors (F.normalize, F.linear, the margin on the label column, autograd backward to W; the
               forward is part of the eager sample because autograd needs its graph, the kernel needs none). HIP events around one call,
               5 warm-up and 20 timed calls each, the two alternating call by call; median and minimum in microseconds.
  (b) step     head_probe_step on ViT-P8S8 (112 px, depth 6, dim 512, CosFace-100, LoRA r = 8 frozen, dropout 0.1) at batch 1024 in fp16,
               against the train-mode forward alone under no_grad at the same batch and dtype; same alternation; the ratio is reported.

    python tools/bench_head_probe.py [--warmup 5] [--iters 20] [--step-iters 10] [--batch 1024]

Exits non-zero when the kernel's median is above eager's for any kind (no margin is granted).
"""
import argparse
import json
import math
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gs-lora_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

GEO = dict(image_size=112, patch_size=8, dim=512, depth=6, heads=8, mlp_dim=2048, lora_rank=8)
S, M = 64.0, 0.5


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3      # microseconds


def alternate(fns, warmup, iters):
    """fns: name -> callable. Every round runs each once, the order flipping from round to round. -> name -> [us]"""
    names = list(fns)
    for _ in range(warmup):
        for n in names:
            fns[n]()
    torch.cuda.synchronize()
    out = {n: [] for n in names}
    for r in range(iters):
        for n in (names if r % 2 == 0 else names[::-1]):
            out[n].append(timed(fns[n]))
    return out


def summary(samples):
    return {"median_us": round(statistics.median(samples), 2), "min_us": round(min(samples), 2)}


def eager_head_grad(kind, emb, W, bias, dl, label):
    """d (logits . dl) / d W (and bias) by torch eager + autograd: the reference's head forward (vit_face.py:181-207, 117-141, 47-50)."""
    W = W.detach().requires_grad_(True)
    if kind == "linear":
        b = bias.detach().requires_grad_(True)
        logits = F.linear(emb, W, b)
        return torch.autograd.grad(logits, (W, b), dl)
    cos = F.linear(F.normalize(emb), F.normalize(W))
    onehot = torch.zeros_like(cos).scatter_(1, label.view(-1, 1), 1.0)
    if kind == "cosface":
        logits = S * (cos - 0.35 * onehot)
    else:
        sine = torch.sqrt((1.0 - cos * cos).clamp(min=0.0))
        phi = cos * math.cos(M) - sine * math.sin(M)
        phi = torch.where(cos > math.cos(math.pi - M), phi, cos - math.sin(math.pi - M) * M)
        logits = S * (onehot * phi + (1.0 - onehot) * cos)
    return torch.autograd.grad(logits, (W,), dl)


def bench_kernel(args):
    from gslora_hip import ops
    B, C, D = 1024, 100, 512
    g = torch.Generator().manual_seed(0)
    emb = torch.randn(B, D, generator=g).cuda()
    bound = math.sqrt(6.0 / (C + D))
    W = ((torch.rand(C, D, generator=g) * 2 - 1) * bound).cuda()
    bias = torch.zeros(C).cuda()
    dl = torch.randn(B, C, generator=g).cuda()
    label = torch.randint(0, C, (B,), generator=g).cuda()
    cos_y = F.linear(F.normalize(emb), F.normalize(W))[torch.arange(B, device="cuda"), label].contiguous()
    res = {}
    for kind in ("cosface", "arcface", "linear"):
        dW = torch.empty(C, D, device="cuda")
        db = torch.empty(C, device="cuda") if kind == "linear" else None
        hip = lambda: ops.head_wgrad(dl, emb, W, kind, cos_s=S, m=M, label=label, cos_y=cos_y, bias=kind == "linear", dW=dW, dbias=db)
        eager = lambda: eager_head_grad(kind, emb, W, bias, dl, label)
        t = alternate({"gsl_head_wgrad": hip, "torch_eager": eager}, args.warmup, args.iters)
        want = eager()[0]
        err = ((dW - want).abs() / want.abs().clamp(min=1.0)).max().item()
        res[kind] = {k: summary(v) for k, v in t.items()}
        res[kind]["max_err_over_bar"] = round(err / 1e-4, 4)
        res[kind]["not_slower"] = res[kind]["gsl_head_wgrad"]["median_us"] <= res[kind]["torch_eager"]["median_us"]
    return res


def bench_step(args):
    from gslora_hip.optim import create_optimizer
    from gslora_hip.step import head_probe_step
    from vit_pytorch_face import ViT_face
    torch.manual_seed(1337)
    m = ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=100, dropout=0.1, emb_dropout=0.1, **GEO)
    for n, p in m.named_parameters():      # train/backbone_forget_main.py:596-600
        p.requires_grad = "loss" in n
    m = m.cuda().set_compute_dtype("fp16").train()
    opt = create_optimizer(SimpleNamespace(opt="adamw", lr=1e-3, weight_decay=0.05, opt_eps=1e-8, opt_betas=None), m)
    crit = torch.nn.CrossEntropyLoss()
    x = torch.rand(args.batch, 3, GEO["image_size"], GEO["image_size"], device="cuda")
    y = torch.randint(0, 100, (args.batch,), device="cuda")

    def fwd():
        with torch.no_grad():
            m(x, y)

    t = alternate({"probe_step": lambda: head_probe_step(m, opt, crit, x, y), "forward_no_grad": fwd}, 3, args.step_iters)
    res = {k: {"median_ms": round(statistics.median(v) / 1e3, 3), "min_ms": round(min(v) / 1e3, 3)} for k, v in t.items()}
    res["ratio_step_over_forward"] = round(res["probe_step"]["median_ms"] / res["forward_no_grad"]["median_ms"], 4)
    res["batch"] = args.batch
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step-iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1024)
    args = ap.parse_args()
    kernel = bench_kernel(args)
    print(json.dumps({"kernel_B1024_C100_D512": kernel, "step_fp16": bench_step(args)}))
    slower = [k for k, r in kernel.items() if not r["not_slower"]]
    if slower:      # no margin: one launch stands against torch's chain of launches
        sys.exit(f"gsl_head_wgrad is SLOWER than torch eager for: {', '.join(slower)}")


if __name__ == "__main__":
    main()
