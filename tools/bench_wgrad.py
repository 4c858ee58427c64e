#!/usr/bin/env python
"""Cost of the weight-gradient GEMM gst_wgrad and of the FFN-training step. Prints one JSON line per part; profiles/ffn_wgrad.md holds the
numbers of the last run. Not part of bench.py.

  kernels  fp16 and bf16 at M = 201 728 (1024 images x 197 tokens), (N, K) = (2048, 512) and (512, 2048):
             (a) gst_wgrad (dW and db);
             (b) the only route of the product library alone: gsl_lora_grad with r = 64 over the 64-column blocks of the narrower operand
                 (it re-reads the wide operand once per block: 8 times).
           HIP events around one call, warm-up, then timed rounds in which the candidates alternate (order flipping from round to round) on one
           box; median and minimum in microseconds, and the ratio of (a) to the floor max(bytes / 5.5 TB/s, FLOPs / 1.85 PFLOP/s) (the delivered
           rates of DESIGN.md section 13; bytes = both operands once + the output once). Acceptance: (a) < (b) at both shapes and both formats.
  step     one ffn_reg_step (gslora_hip.step) on ViT-P8S8 (112 px, depth 6, dim 512, mlp 2048, CosFace, lora_rank = 0, dropout 0.1, fp16) at
           batch 512 with an L2 term, and beside it what three of its parts cost on their own: the twelve gst_wgrad calls at the step's
           shapes, the re-casts of the twelve FFN weights into their [N, K] and [K, N] operand copies, and optimizer.step() (one AdamW launch
           per tensor).

    python tools/bench_wgrad.py [--warmup 3] [--iters 10] [--parts kernels,step]

Each part runs in a child process of its own under a time limit; a part that fails or runs out of time ends the run (nothing more is started).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gs-lora_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

GEO = dict(image_size=112, patch_size=8, dim=512, depth=6, heads=8, mlp_dim=2048)
M_FULL = 1024 * 197
HBM, PEAK = 5.5e12, 1.85e15
LIMITS = {"kernels": 300, "step": 300}


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3      # microseconds


def alternate(fns, warmup, iters):
    names = list(fns)
    for _ in range(warmup):
        for n in names:
            fns[n]()
    out = {n: [] for n in names}
    for it in range(iters):
        for n in (names if it % 2 == 0 else names[::-1]):
            out[n].append(timed(fns[n]))
    return out


def summary(ts):
    return {"median_us": round(statistics.median(ts), 1), "min_us": round(min(ts), 1)}


def part_kernels(args):
    import torch
    from gslora_hip import _lib_train as LT
    from gslora_hip import ops
    res = {"part": "kernels", "M": M_FULL, "rows": []}
    ok = True
    for name, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        for N, K in ((2048, 512), (512, 2048)):
            g = torch.Generator(device="cuda").manual_seed(1)
            Y = torch.randn(M_FULL, N, device="cuda", generator=g).to(dt)
            X = torch.randn(M_FULL, K, device="cuda", generator=g).to(dt)
            dW, db = torch.empty(N, K, device="cuda"), torch.empty(N, device="cuda")
            ws = torch.empty(LT.wgrad_ws_elems(M_FULL, N, K, dt), device="cuda")
            blocks = torch.empty(N, K, device="cuda")

            def block_route():
                if K <= N:      # the narrower operand is X: dW[:, k0:k0+64] = Y^T X[:, k0:k0+64]
                    for k0 in range(0, K, 64):
                        ops.lora_grad(Y, X[:, k0:k0 + 64], blocks[:, k0:], K, 1, 64, accumulate=False)
                else:           # the narrower operand is Y: dW[n0:n0+64, :] = (X^T Y[:, n0:n0+64])^T
                    for n0 in range(0, N, 64):
                        ops.lora_grad(X, Y[:, n0:n0 + 64], blocks[n0:], 1, K, 64, accumulate=False)
            t = alternate({"wgrad": lambda: LT.wgrad(Y, X, dW, db, ws=ws), "blocks": block_route}, args.warmup, args.iters)
            diff = (dW - blocks).abs().max().item() / dW.abs().max().item()
            floor = max((M_FULL * (N + K) * 2 + N * K * 4) / HBM, 2.0 * M_FULL * N * K / PEAK) * 1e6
            a, b = summary(t["wgrad"]), summary(t["blocks"])
            ok = ok and a["median_us"] < b["median_us"]
            res["rows"].append({"dtype": name, "N": N, "K": K, "plan": LT.wgrad_plan(M_FULL, N, K, dt), "wgrad": a, "blocks_r64": b,
                                "floor_us": round(floor, 1), "wgrad_over_floor": round(a["median_us"] / floor, 2),
                                "blocks_over_wgrad": round(b["median_us"] / a["median_us"], 2), "max_rel_diff": diff})
            del Y, X, ws
    res["acceptance"] = ok
    print(json.dumps(res), flush=True)
    return 0 if ok else 1


def part_step(args):
    from types import SimpleNamespace
    import torch
    from gslora_hip import _lib_train as LT
    from gslora_hip import ops
    from gslora_hip.optim import create_optimizer
    from gslora_hip.step import ffn_reg_step
    from vit_pytorch_face import ViT_face
    B = 512
    torch.manual_seed(0)
    m = ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=100, dropout=0.1, emb_dropout=0.1, lora_rank=0, **GEO)
    for n, p in m.named_parameters():
        p.requires_grad = "fn.fn.net" in n or "loss" in n
    m = m.to("cuda").set_compute_dtype("fp16").train()
    opt = create_optimizer(SimpleNamespace(opt="adamw", lr=1e-4, weight_decay=0.05, opt_eps=1e-8, opt_betas=None), m)
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    terms = {0: {"importance": {n: None for n, _ in named}, "task_param": {n: p.detach().clone() for n, p in named}}}
    x = torch.rand(B, 3, 112, 112, device="cuda")
    y = torch.randint(0, 100, (B,), device="cuda")
    crit = torch.nn.CrossEntropyLoss()
    dt, D, mlp, T = torch.float16, GEO["dim"], GEO["mlp_dim"], 197
    shapes = [(B * T, D, mlp), (B * T, mlp, D)] * (GEO["depth"] - 1) + [(B, D, mlp), (B, mlp, D)]
    ops_ = {s: (torch.randn(s[0], s[1], device="cuda").to(dt), torch.randn(s[0], s[2], device="cuda").to(dt)) for s in set(shapes)}
    outs = {s: (torch.empty(s[1], s[2], device="cuda"), torch.empty(s[1], device="cuda")) for s in set(shapes)}
    ws = torch.empty(max(LT.wgrad_ws_elems(*s, dt) for s in set(shapes)), device="cuda")
    weights = [lin.weight.detach() for _, ff in m.transformer.layers for lin in (ff.fn.fn.net[0], ff.fn.fn.net[3])]

    def wgrads():
        for s in shapes:
            LT.wgrad(*ops_[s], *outs[s], ws=ws)

    def recasts():
        for w in weights:
            ops.cast(w, dt)
            ops.transpose_cast(w, dt)
    step = lambda: ffn_reg_step(m, opt, crit, x, y, regularization_terms=terms, reg_lambda=1.0)
    step()      # (gives every parameter its gradient: optimizer.step() alone is timed on them)
    t = alternate({"step": step, "wgrad_x12": wgrads, "recast_x12": recasts, "adamw": lambda: opt.step()}, args.warmup, args.iters)
    res = {"part": "step", "batch": B, "dtype": "fp16", **{k: summary(v) for k, v in t.items()}}
    tot = res["step"]["median_us"]
    res["share"] = {k: round(res[k]["median_us"] / tot, 3) for k in ("wgrad_x12", "recast_x12", "adamw")}
    res["loss_scale"] = m.runner().loss_scale_report()
    print(json.dumps(res), flush=True)
    return 0


PARTS = {"kernels": part_kernels, "step": part_step}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--parts", default="kernels,step")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return PARTS[args.child](args)
    for part in args.parts.split(","):      # a fresh process per part, each under its own time limit; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--child", part, "--warmup", str(args.warmup), "--iters", str(args.iters)]
        try:
            rc = subprocess.run(cmd, timeout=LIMITS[part]).returncode
        except subprocess.TimeoutExpired:
            print(f"[bench_wgrad] {part}: no result within {LIMITS[part]} s; stopping", flush=True)
            return 124
        if rc != 0:
            print(f"[bench_wgrad] {part}: exit {rc}; stopping", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
