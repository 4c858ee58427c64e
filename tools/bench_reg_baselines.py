#!/usr/bin/env python
"""Cost of the regularisation baselines' kernels (libgslora_reg.so) and of the batched regulariser in the FFN-training step. Prints one JSON
line per part and a markdown table; profiles/reg_baselines.md holds the numbers of the last run. Not part of bench.py.

  acc    gsr_importance_acc at n = 1 Mi and 16 Mi f32 elements, both kinds: HIP events around `--launches` back-to-back launches after a
         warm-up, median of `--iters` rounds; achieved GB/s against the 12 bytes per element the kernel must move (omega read and written,
         the gradient read).
  step   one ffn_reg_step (gslora_hip.step) on ViT-P8S8 (112 px, depth 6, dim 512, mlp 2048, CosFace, lora_rank = 0, dropout 0.1, fp16;
         FFN linears and the head train: 25 tensors) at batch 8 and batch 512 with 1 and with 4 regularisation terms, the terms passed as a
         gslora_hip.reg.RegTerms (two launches forward, one backward) against the reference's dict (two forward and one backward per term
         and tensor: the path before RegTerms existed), same process, same model and optimizer. Blocks of `--block` steps (host clock around
         a block that ends in a device synchronise) alternate between the two forms, the order flipping from round to round; per form the
         median block time per step, and for the dict form its spread (max - min over its blocks). Requirement: in every cell the RegTerms
         median is not above the dict median by more than the dict spread.

    python tools/bench_reg_baselines.py [--parts acc,step] [--iters 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gs-lora_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

GEO = dict(image_size=112, patch_size=8, dim=512, depth=6, heads=8, mlp_dim=2048)


def part_acc(args):
    import torch
    from gslora_hip import _lib_reg as LR
    rows = []
    for n in (1 << 20, 1 << 24):
        omega, g = torch.zeros(n, device="cuda"), torch.randn(n, device="cuda")
        for kind, name in ((LR.EWC, "ewc"), (LR.MAS, "mas")):
            for _ in range(3):
                LR.importance_acc(omega, g, kind, 3, 7)
            times = []
            for _ in range(args.iters):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.launches):
                    LR.importance_acc(omega, g, kind, 3, 7)
                b.record()
                b.synchronize()
                times.append(a.elapsed_time(b) * 1e-3 / args.launches)
            t = statistics.median(times)
            rows.append(dict(part="acc", n=n, kind=name, us=t * 1e6, gb_per_s=12.0 * n / t / 1e9, min_us=min(times) * 1e6, max_us=max(times) * 1e6))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def part_step(args):
    import torch
    from gslora_hip import reg
    from gslora_hip.optim import create_optimizer
    from gslora_hip.step import ffn_reg_step
    from types import SimpleNamespace
    from vit_pytorch_face import ViT_face
    torch.manual_seed(0)
    m = ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=100, dropout=0.1, emb_dropout=0.1, lora_rank=0, **GEO)
    for n, p in m.named_parameters():
        p.requires_grad = "fn.fn.net" in n or "loss" in n
    m = m.to("cuda").set_compute_dtype(args.dtype).train()
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    opt = create_optimizer(SimpleNamespace(opt="adamw", lr=1e-5, weight_decay=0.05, opt_eps=1e-8, opt_betas=None), m)
    crit = torch.nn.CrossEntropyLoss()
    rows = []
    for batch in (8, 512):
        x = torch.rand(batch, 3, GEO["image_size"], GEO["image_size"], device="cuda")
        y = torch.randint(0, 100, (batch,), device="cuda")
        block = args.block if batch == 8 else max(2, args.block // 8)
        for n_terms in (1, 4):
            terms = {k: {"importance": {n: torch.rand_like(p) for n, p in named}, "task_param": {n: p.detach().clone() for n, p in named}}
                     for k in range(n_terms)}
            forms = {"dict": terms, "RegTerms": reg.RegTerms(m, terms, 0.1)}

            def run(form):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(block):
                    ffn_reg_step(m, opt, crit, x, y, regularization_terms=forms[form], reg_lambda=0.1)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / block
            for form in forms:      # warm-up of both forms at this shape
                run(form)
            times = {f: [] for f in forms}
            for it in range(args.iters):
                for form in (list(forms) if it % 2 == 0 else list(forms)[::-1]):
                    times[form].append(run(form))
            d, r = statistics.median(times["dict"]), statistics.median(times["RegTerms"])
            spread = max(times["dict"]) - min(times["dict"])
            rows.append(dict(part="step", batch=batch, terms=n_terms, tensors=len(named), block=block, dict_ms=d * 1e3, regterms_ms=r * 1e3,
                             dict_spread_ms=spread * 1e3, regterms_spread_ms=(max(times["RegTerms"]) - min(times["RegTerms"])) * 1e3,
                             ratio=d / r, ok=bool(r <= d + spread)))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="acc,step")
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--block", type=int, default=40)
    ap.add_argument("--dtype", default="fp16")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("tools/bench_reg_baselines.py measures on a ROCm GPU; none is visible (no fallback)")
    rows = []
    for part in args.parts.split(","):
        rows += {"acc": part_acc, "step": part_step}[part](args)
    print("\n| n | kind | time / launch (us) | GB/s of 12 B per element |\n|---|---|---|---|")
    for r in rows:
        if r["part"] == "acc":
            print(f"| {r['n']} | {r['kind']} | {r['us']:.1f} | {r['gb_per_s']:.0f} |")
    print("\n| batch | terms | dict (ms / step) | RegTerms (ms / step) | dict spread (ms) | dict / RegTerms | not above dict + spread |\n|---|---|---|---|---|---|---|")
    for r in rows:
        if r["part"] == "step":
            print(f"| {r['batch']} | {r['terms']} | {r['dict_ms']:.3f} | {r['regterms_ms']:.3f} | {r['dict_spread_ms']:.3f} | {r['ratio']:.2f} | {r['ok']} |")
    return 0 if all(r.get("ok", True) for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
