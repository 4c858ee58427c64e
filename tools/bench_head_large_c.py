#!/usr/bin/env python
"""Cost of the head at large class counts, one process, one build. Prints one JSON line; profiles/head_large_c.md holds the numbers of
the last run. Not part of bench.py.

  (a) kernels  gsl_head_fwd (CosFace, logits) and gsl_head_bwd (f32, and the fp16 loss-scaled form: gscale given) at B = 1024, D = 512,
               T = 1 for C in 1000, 1024 (the per-image kernels), 1025, 2048, 10 572, 93 431 (the class-tiled kernels), each beside torch's
               f32 matmul on the same device tensors (e-hat @ Wn.T for the forward, dl @ Wn for the backward: the products alone, without
               the pool / LayerNorm / margin / LayerNorm-backward work the entry points also do), and gsl_head_wgrad at the same C.
               HIP events around one call, warm-up, then timed rounds in which the candidates alternate; median and minimum in microseconds.
  (b) step     gs_lora_step on ViT-P8S8 (112 px, depth 6, dim 512, CosFace, LoRA r = 8, dropout 0.1, fp16) at batch 512 + 512 — bench.py's
               config 2 — with num_class = 10 572 against num_class = 100, alternating.

  (c) probe    head_probe_step (head only trainable, the same model, fp16) at batch 512 with num_class = 100 and 10 572, alternating
               (--probe-step): the step whose backward is the one gsl_head_wgrad launch.

    python tools/bench_head_large_c.py [--warmup 5] [--iters 20] [--step-iters 8] [--no-step] [--probe-step] [--classes 1000,1024,...]
    python tools/bench_head_large_c.py --wgrad-acceptance NEW1.json,NEW2.json PARENT1.json,PARENT2.json

Every run also reports head_wgrad over the tiled head_bwd f32 of the same run ("wgrad_over_head_bwd_f32"): two kernels of equal FLOPs.

The acceptance rule of the tiled kernels is evaluated and printed ("acceptance"): time(C) <= time_old(1024) * C / 1024 for the forward and the
backward at C = 2048 and 10 572, and fp16 loss-scaled backward < 1.25 x the plain one at C = 10 572. Exits non-zero when it does not hold.

The class-tiled weight gradient is judged against the PARENT build, not against a rule inside one library: run the tool several times on one
box, whole runs alternating between the two libraries (GSLORA_HIP_LIB, the way tools/ab_libs.sh compares builds), keep each run's JSON line,
and hand the files to --wgrad-acceptance (no GPU needed). With the mean of the runs' medians: head_wgrad at C = 10 572 and 93 431 takes at
most HALF the parent's time, at C = 1025 and 2048 it is not slower, and the C <= 1024 rows are reported. Exits non-zero when it does not hold.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gs-lora_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

GEO = dict(image_size=112, patch_size=8, dim=512, depth=6, heads=8, mlp_dim=2048, lora_rank=8)
B, D, S, M = 1024, 512, 64.0, 0.35


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
    return {"median_us": round(statistics.median(samples), 1), "min_us": round(min(samples), 1)}


def bench_kernels(args, C):
    from gslora_hip import ops
    g = torch.Generator().manual_seed(C)
    x = torch.randn(B, D, generator=g).cuda()
    gamma, beta = torch.ones(D).cuda(), torch.zeros(D).cuda()
    W = torch.randn(C, D, generator=g).cuda()
    Wn = ops.cosface_prep(W)
    label = torch.randint(0, C, (B,), generator=g).cuda()
    dl = (torch.randn(B, C, generator=g) * 1e-3).cuda()
    logits, emb, mean, rstd = ops.head_fwd(x, B, 1, D, gamma, beta, 1e-5, Wn, label, S, M)
    en = F.normalize(emb)
    gscale = torch.zeros(4, device="cuda")
    bwd = lambda dt, gs: ops.head_bwd(dl, None, x, B, 1, D, gamma, mean, rstd, emb, Wn, S, dt, compact=True, gscale=gs)
    iters = args.iters if C <= 20000 else max(4, args.iters // 4)
    t = alternate({"head_fwd": lambda: ops.head_fwd(x, B, 1, D, gamma, beta, 1e-5, Wn, label, S, M),
                   "torch_fwd_matmul": lambda: en @ Wn.T,
                   "head_bwd_f32": lambda: bwd(torch.float32, None),
                   "head_bwd_fp16_scaled": lambda: bwd(torch.float16, gscale),
                   "torch_bwd_matmul": lambda: dl @ Wn,
                   "head_wgrad": lambda: ops.head_wgrad(dl, emb, W, "cosface", cos_s=S)}, args.warmup, iters)
    res = {k: summary(v) for k, v in t.items()}
    # the two agree (a sanity check of what was timed, not a tolerance test)
    want = (en @ Wn.T) * S
    want[torch.arange(B, device="cuda"), label] -= S * M
    res["logits_vs_torch_max_abs"] = round((want - logits).abs().max().item(), 7)
    res["path"] = "tiled" if C > ops.HEAD_TILED_C else "per-image"
    res["wgrad_over_head_bwd_f32"] = round(res["head_wgrad"]["median_us"] / res["head_bwd_f32"]["median_us"], 3)
    return res


def bench_step(args):
    from gslora_hip.optim import FusedAdamW
    from gslora_hip.step import gs_lora_step
    import loralib as lora
    from vit_pytorch_face import ViT_face
    crit = torch.nn.CrossEntropyLoss()
    hy = dict(beta=0.15, alpha=1e-2, BND=105.0)
    runs = {}
    for C in (100, 10572):
        torch.manual_seed(1337)
        m = ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=C, dropout=0.1, emb_dropout=0.1, **GEO)
        lora.mark_only_lora_as_trainable(m)
        m = m.cuda().set_compute_dtype("fp16").train()
        opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=0.05, eps=1e-8)
        n = args.batch
        data = [torch.rand(n, 3, 112, 112, device="cuda"), torch.randint(0, C - C // 5, (n,), device="cuda"),
                torch.rand(n, 3, 112, 112, device="cuda"), torch.randint(C - C // 5, C, (n,), device="cuda")]
        runs[f"num_class_{C}"] = (lambda m=m, opt=opt, data=data: gs_lora_step(m, opt, crit, *data, **hy))
    t = alternate(runs, 3, args.step_iters)
    res = {k: {"median_ms": round(statistics.median(v) / 1e3, 3), "min_ms": round(min(v) / 1e3, 3)} for k, v in t.items()}
    res["ratio_10572_over_100"] = round(res["num_class_10572"]["median_ms"] / res["num_class_100"]["median_ms"], 4)
    res["batch"] = f"{args.batch} + {args.batch}"
    return res


def bench_probe_step(args):
    from gslora_hip.optim import create_optimizer
    from gslora_hip.step import head_probe_step
    from types import SimpleNamespace
    from vit_pytorch_face import ViT_face
    crit = torch.nn.CrossEntropyLoss()
    runs = {}
    for C in (100, 10572):
        torch.manual_seed(1337)
        m = ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=C, dropout=0.1, emb_dropout=0.1, **GEO)
        for n, p in m.named_parameters():      # train/backbone_forget_main.py:596-600
            p.requires_grad = "loss" in n
        m = m.cuda().set_compute_dtype("fp16").train()
        opt = create_optimizer(SimpleNamespace(opt="adamw", lr=1e-3, weight_decay=0.05, opt_eps=1e-8, opt_betas=None), m)
        x, y = torch.rand(args.batch, 3, 112, 112, device="cuda"), torch.randint(0, C, (args.batch,), device="cuda")
        runs[f"num_class_{C}"] = (lambda m=m, opt=opt, x=x, y=y: head_probe_step(m, opt, crit, x, y))
    t = alternate(runs, 3, args.step_iters)
    res = {k: {"median_ms": round(statistics.median(v) / 1e3, 3), "min_ms": round(min(v) / 1e3, 3)} for k, v in t.items()}
    res["batch"] = args.batch
    return res


def wgrad_acceptance(new_files, parent_files):
    """Mean over the runs of a library of head_wgrad's median, per C; new / parent. -> (table, missed)"""
    def load(files):
        runs = [json.loads(open(f).read().strip().splitlines()[-1])["kernels_B1024_D512"] for f in files.split(",")]
        return {C: statistics.mean(r[C]["head_wgrad"]["median_us"] for r in runs) for C in runs[0] if all(C in r for r in runs)}, runs
    new, new_runs = load(new_files)
    old, _ = load(parent_files)
    out, missed = {}, []
    for C in sorted(set(new) & set(old), key=int):
        ratio = new[C] / old[C]
        bwd = statistics.mean(r[C]["head_bwd_f32"]["median_us"] for r in new_runs)
        out[C] = {"new_us": round(new[C], 1), "parent_us": round(old[C], 1), "new_over_parent": round(ratio, 4),
                  "new_over_head_bwd_f32": round(new[C] / bwd, 3)}
        bound = 0.5 if int(C) in (10572, 93431) else 1.0 if int(C) in (1025, 2048) else None
        if bound is not None:
            out[C]["bound"] = bound
            if ratio > bound:
                missed.append(f"C={C}: {ratio:.3f} > {bound}")
    return out, missed


def acceptance(k):
    """time(C) <= time_old(1024) * C / 1024, no margin; the loss-scaled backward below 1.25 x the plain one at 10 572 classes."""
    out = {}
    if "1024" not in k:
        return out
    for what in ("head_fwd", "head_bwd_f32"):
        old = k["1024"][what]["median_us"]
        for C in (2048, 10572):
            if str(C) in k:
                out[f"{what}_C{C}_over_linear_extrapolation_of_1024"] = round(k[str(C)][what]["median_us"] / (old * C / 1024), 4)
    if "10572" in k:
        out["fp16_scaled_over_f32_bwd_C10572"] = round(k["10572"]["head_bwd_fp16_scaled"]["median_us"] / k["10572"]["head_bwd_f32"]["median_us"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step-iters", type=int, default=8)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--classes", default="1000,1024,1025,2048,10572,93431")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--probe-step", action="store_true")
    ap.add_argument("--wgrad-acceptance", nargs=2, metavar=("NEW_JSONS", "PARENT_JSONS"))
    args = ap.parse_args()
    if args.wgrad_acceptance:
        table, missed = wgrad_acceptance(*args.wgrad_acceptance)
        print(json.dumps({"head_wgrad_new_against_parent": table}))
        sys.exit(f"acceptance missed: {', '.join(missed)}" if missed else 0)
    kernels = {str(C): bench_kernels(args, C) for C in map(int, args.classes.split(","))}
    acc = acceptance(kernels)
    out = {"kernels_B1024_D512": kernels, "acceptance": acc}
    if not args.no_step:
        out["step_config2_fp16"] = bench_step(args)
    if args.probe_step:
        out["probe_step_fp16"] = bench_probe_step(args)
    print(json.dumps(out))
    bad = [k for k, v in acc.items() if (v >= 1.25 if k.startswith("fp16") else v > 1.0)]
    if bad:
        sys.exit(f"acceptance missed: {', '.join(bad)}")


if __name__ == "__main__":
    main()
