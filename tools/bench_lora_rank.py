#!/usr/bin/env python
"""Cost of LoRA ranks above 16, one process, one box. Prints one JSON line; profiles/lora_rank.md holds the numbers of the last run. Not
part of bench.py.

  (a) reductions  gsl_lora_grad at the config-2 shapes (M = 201 728 token rows; N = 2048 and 512; fp16 operands) at r = 32 and r = 64:
                  the one launch of the R = 32 / 64 instantiation ("new") against the same result without it ("blocks"): ceil(r / 16)
                  calls of the rank-16 kernel over 16-column blocks of U, each of which streams Y again. --baseline-lib names the library
                  the rank-16 calls go to (the parent commit's libgslora_hip.so; default: this build's, whose rank-16 instantiation is the
                  same code). The rank-16 call alone is timed beside them. HIP events around one result, warm-up, then rounds in which the
                  candidates alternate; median and minimum in microseconds, and the achieved rate over the bytes of Y and of the r columns
                  of U. Exits non-zero unless "new" is faster than "blocks" at both ranks and both N.
  (b) step        gs_lora_step on ViT-P8S8 (112 px, depth 6, dim 512, CosFace-100, dropout 0.1, fp16) at batch 512 + 512 — bench.py's
                  config 2 — at r = 8, 16, 32, 64, alternating. Above rank 16 the step runs the two-launch K-segment GEMMs and four unfused
                  reductions per block.

    python tools/bench_lora_rank.py [--warmup 3] [--iters 15] [--step-iters 6] [--no-step] [--baseline-lib PATH] [--rows 201728]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gs-lora_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

GEO = dict(image_size=112, patch_size=8, dim=512, depth=6, heads=8, mlp_dim=2048)


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


def open_lib(path):
    """A second libgslora_hip.so (the baseline's), with the two signatures this tool calls."""
    from gslora_hip import _lib as L
    lib = ctypes.CDLL(path)
    for name in ("gsl_lora_grad", "gsl_lora_grad_ws_elems"):
        fn = getattr(lib, name)
        fn.argtypes = L.SIGNATURES[name]
        fn.restype = ctypes.c_long if name.endswith("ws_elems") else ctypes.c_int
    return lib


def bench_reductions(args, N, base):
    from gslora_hip import _lib as L
    new = L.load()
    M, F16 = args.rows, L.F16
    g = torch.Generator().manual_seed(N)
    Y = (torch.randn(M, N, generator=g) * 0.05).cuda().half()
    U = (torch.randn(M, 64, generator=g) * 0.05).cuda().half()
    stream = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(max(new.gsl_lora_grad_ws_elems(M, N, 64), base.gsl_lora_grad_ws_elems(M, N, 16), 1 << 22), device="cuda")

    def call(lib, col, r, G):
        rc = lib.gsl_lora_grad(Y.data_ptr(), N, U.data_ptr() + 2 * col, 64, G.data_ptr() + 4 * col, 64, 1, M, N, r, F16, 0, ws.data_ptr(),
                               None, stream)
        assert rc == 0, (rc, r, col)
    res = {}
    for r in (32, 64):
        Gn, Gb = torch.zeros(N, 64, device="cuda"), torch.zeros(N, 64, device="cuda")
        t = alternate({"new": lambda: call(new, 0, r, Gn),
                       "blocks": lambda: [call(base, c, min(16, r - c), Gb) for c in range(0, r, 16)],
                       "rank16": lambda: call(base, 0, 16, Gb)}, args.warmup, args.iters)
        call(new, 0, r, Gn)
        [call(base, c, min(16, r - c), Gb) for c in range(0, r, 16)]
        torch.cuda.synchronize()
        out = {}
        for k, v in t.items():
            cols = 16 if k == "rank16" else r
            nbytes = 2.0 * M * N * (1 if k != "blocks" else -(-r // 16)) + 2.0 * M * cols
            med = statistics.median(v)
            out[k] = {"median_us": round(med, 1), "min_us": round(min(v), 1), "TB_per_s": round(nbytes / med / 1e6, 3)}
        out["new_over_blocks"] = round(out["new"]["median_us"] / out["blocks"]["median_us"], 4)
        out["same_bits_as_blocks"] = bool(torch.equal(Gn[:, :r], Gb[:, :r]))      # (what was timed computes the same sums; fp16 x fp16 products are exact in f32, the order differs)
        out["max_abs_diff_vs_blocks"] = float((Gn[:, :r] - Gb[:, :r]).abs().max())
        res[f"r{r}"] = out
    return res


def bench_step(args):
    from gslora_hip.optim import FusedAdamW
    from gslora_hip.step import gs_lora_step
    import loralib as lora
    from vit_pytorch_face import ViT_face
    crit = torch.nn.CrossEntropyLoss()
    hy = dict(beta=0.15, alpha=1e-2, BND=105.0)
    n, C = args.batch, 100
    torch.manual_seed(1337)
    data = [torch.rand(n, 3, 112, 112, device="cuda"), torch.randint(0, 80, (n,), device="cuda"),
            torch.rand(n, 3, 112, 112, device="cuda"), torch.randint(80, C, (n,), device="cuda")]
    runs = {}
    for r in (8, 16, 32, 64):
        torch.manual_seed(1337)
        m = ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=C, dropout=0.1, emb_dropout=0.1, lora_rank=r, **GEO)
        lora.mark_only_lora_as_trainable(m)
        m = m.cuda().set_compute_dtype("fp16").train()
        opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=0.05, eps=1e-8)
        runs[f"r{r}"] = (lambda m=m, opt=opt: gs_lora_step(m, opt, crit, *data, **hy))
    t = alternate(runs, 3, args.step_iters)
    res = {k: {"median_ms": round(statistics.median(v) / 1e3, 3), "min_ms": round(min(v) / 1e3, 3)} for k, v in t.items()}
    for r in (8, 32, 64):
        res[f"r{r}_over_r16"] = round(res[f"r{r}"]["median_ms"] / res["r16"]["median_ms"], 4)
    res["batch"] = f"{n} + {n}"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--step-iters", type=int, default=6)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--rows", type=int, default=201728)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    from gslora_hip import _lib as L
    base = open_lib(args.baseline_lib) if args.baseline_lib else L.load()
    out = {"reductions_fp16": {f"N{N}": bench_reductions(args, N, base) for N in (2048, 512)}, "rows": args.rows,
           "baseline_lib": args.baseline_lib or "this build"}
    if not args.no_step:
        out["step_config2_fp16"] = bench_step(args)
    print(json.dumps(out))
    bad = [f"{n} {r}" for n, d in out["reductions_fp16"].items() for r, v in d.items() if v["new_over_blocks"] >= 1.0]
    if bad:
        sys.exit(f"the one launch is not faster than the rank-16 blocks at: {', '.join(bad)}")


if __name__ == "__main__":
    main()
