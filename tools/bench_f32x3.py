#!/usr/bin/env python
"""The fp32x3 mode (GSL_F32X3: f32 tensors, the GEMMs' products as three bf16 pieces on the bf16 matrix cores) against the exact-f32 mode, on the
same device in one call, old and new alternating after warm-up. Sections (all by default; profiles/f32x3.md is written from this output):

  --accuracy   error of both GEMM kernels against a float64 product on the shapes and operand families of tests/test_hip_f32x3.py
  --gemm       the six GEMM shapes of the config-2 step (M = 201 728 rows): time and TF/s on the algorithmic 2 M N K count, x3 against the
               exact-f32 MFMA kernel, and the share of the 16 / 6 ceiling
  --step       python bench.py --dtype fp32 against --dtype fp32x3 (child processes, alternating)
  --eval       engine_cl.eval_data images/s with EVAL_DTYPE fp32 against fp32x3, batches of 5 x 512, on an fp16-trained config-2 model

python tools/bench_f32x3.py [--accuracy] [--gemm] [--step] [--eval] [--out FILE.json]      (GSLORA_HIP_LIB selects a build)"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gs-lora_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

M_STEP = 201728      # rows of the config-2 step: (512 remain + 512 forget) images x 197 tokens
# name, K1, K2, N, epilogue: the FFN GEMMs carry their LoRA segment (K2 = 64: rank 8 zero padded), as the f32 step runs them
GEMMS = (("QKV", 512, 0, 1536, "store"), ("out-proj (bias + residual)", 512, 0, 512, "res"), ("FFN1 (bias + GELU, 2 outputs)", 512, 64, 2048, "gelu"),
         ("FFN2 (bias + residual)", 2048, 64, 512, "res"), ("FFN2-dX (x GELU')", 512, 64, 2048, "mul"), ("FFN1-dX", 2048, 64, 512, "store"))
ACC_SHAPES = ((64, 128, 64, 0), (130, 192, 64, 64), (394, 384, 128, 0), (256, 512, 512, 64))


def operands(family, rows, K, seed):
    g = torch.Generator().manual_seed(seed)
    if family == "uniform":
        return torch.rand(rows, K, generator=g) * 2 - 1
    return torch.randn(rows, K, generator=g) * torch.exp(4 * torch.randn(rows, K, generator=g))


def accuracy():
    from gslora_hip import _lib as L, ops
    rows = []
    for M, N, K1, K2 in ACC_SHAPES:
        for fam in ("uniform", "wide"):
            A, W = operands(fam, M, K1 + K2, 1), operands(fam, N, K1 + K2, 2)
            a64, w64 = A.double().numpy(), W.double().numpy()
            ref, scale = a64 @ w64.T, np.abs(a64) @ np.abs(w64).T
            err = lambda o: float((np.abs(o - ref) / scale).max())
            Ad, Wd = A.cuda(), W.cuda()
            seg = dict(A2=Ad[:, K1:].contiguous(), W2=Wd[:, K1:].contiguous()) if K2 else {}
            out = {}
            for mode in (None, "x3"):
                o = torch.empty(M, N, device="cuda")
                ops.gemm_nt(Ad[:, :K1].contiguous(), Wd[:, :K1].contiguous(), o, epilogue=L.EPI_STORE_F32, f32_mode=mode, **seg)
                out[mode] = err(o.double().cpu().numpy())
            e5 = err(ops.f32x3_product_reference(A.numpy(), W.numpy(), ops.F32X3_FIVE))
            e6 = err(ops.f32x3_product_reference(A.numpy(), W.numpy()))
            rows.append(dict(M=M, N=N, K1=K1, K2=K2, family=fam, e_f32=out[None], e_x3=out["x3"], e_five_host=e5, e_six_host=e6,
                             x3_over_f32=out["x3"] / out[None], x3_over_five=out["x3"] / e5))
            print(f"accuracy ({M},{N},{K1},{K2}) {fam:8s}: e_f32 {out[None]:.2e}  e_x3 {out['x3']:.2e}  (x3 / f32 {out['x3'] / out[None]:.2f}, x3 / five {out['x3'] / e5:.3f};"
                  f" host six {e6:.1e}, five {e5:.1e})", flush=True)
    return rows


def gemm(reps=6):
    from gslora_hip import _lib as L, ops
    torch.manual_seed(0)
    rows, M = [], M_STEP
    for name, K1, K2, N, epi in GEMMS:
        A, W = torch.randn(M, K1, device="cuda"), torch.randn(N, K1, device="cuda") * K1 ** -0.5
        seg = dict(A2=torch.randn(M, K2, device="cuda"), W2=torch.randn(N, K2, device="cuda") * 0.1) if K2 else {}
        out, bias = torch.empty(M, N, device="cuda"), torch.randn(N, device="cuda")
        extra = {"store": {}, "gelu": dict(epilogue=L.EPI_BIAS_GELU, bias=bias, out2=torch.empty(M, N, device="cuda")),
                 "res": dict(epilogue=L.EPI_BIAS_RES_F32, bias=bias, res=torch.randn(M, N, device="cuda")),
                 "mul": dict(epilogue=L.EPI_MUL, aux=torch.randn(M, N, device="cuda"))}[epi]
        run = lambda mode: ops.gemm_nt(A, W, out, f32_mode=mode, **seg, **extra)
        for mode in (None, "x3", None, "x3"):
            run(mode)
        torch.cuda.synchronize()
        ms = {None: [], "x3": []}
        for _ in range(reps):      # alternating, one event pair per launch
            for mode in (None, "x3"):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); run(mode); b.record(); torch.cuda.synchronize()
                ms[mode].append(a.elapsed_time(b))
        flop = 2.0 * M * N * (K1 + K2)
        t32, t3 = float(np.median(ms[None])), float(np.median(ms["x3"]))
        rows.append(dict(name=name, M=M, N=N, K1=K1, K2=K2, f32_ms=t32, x3_ms=t3, f32_tfs=flop / t32 / 1e9, x3_tfs=flop / t3 / 1e9, speedup=t32 / t3,
                         share_of_ceiling=(t32 / t3) / (16 / 6), f32_ms_all=ms[None], x3_ms_all=ms["x3"]))
        print(f"gemm {name:32s} N={N:5d} K={K1}+{K2}: f32 {t32:7.3f} ms {flop / t32 / 1e9:6.1f} TF/s | x3 {t3:7.3f} ms {flop / t3 / 1e9:6.1f} TF/s | x {t32 / t3:.2f}"
              f" = {100 * (t32 / t3) / (16 / 6):.0f} % of 16/6", flush=True)
        del A, W, seg, out, extra
        torch.cuda.empty_cache()
    return rows


def step(steps, warmup, rounds=2):
    res = {"fp32": [], "fp32x3": []}
    for _ in range(rounds):
        for dt in ("fp32", "fp32x3"):
            p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--dtype", dt],
                               capture_output=True, text=True, timeout=900)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode or not line:
                raise RuntimeError(f"bench.py --dtype {dt} failed ({p.returncode}): {p.stderr[-2000:]}")
            j = json.loads(line[-1])
            res[dt].append(dict(ms_per_step=j["ms_per_step"], images_per_s=j["value"]))
            print(f"step --dtype {dt}: {j['ms_per_step']} ms/step, {j['value']} images/s", flush=True)
    return res


def evaluation(n_batches=3):
    """bench.py's eval leg with the two f32 evaluation dtypes: the config-2 model in its default training mode, 5 x 512 images per batch."""
    import contextlib
    import io
    import bench
    import engine_cl
    dev = torch.device("cuda:0")
    model = bench.build_model("fp16", 0.1, dev)
    g = torch.Generator().manual_seed(4242)
    Be = 5 * 512
    batch = ((torch.randint(0, 256, (Be, 3, 112, 112), generator=g, dtype=torch.uint8).float() / 255.0).to(dev), torch.randint(0, 100, (Be,), generator=g).to(dev))
    saved, res = engine_cl.EVAL_DTYPE, {"fp32": [], "fp32x3": []}
    try:
        for rnd in range(3):      # round 0 = warm-up of both (operand caches, eval-mode merge)
            for ev in ("fp32", "fp32x3"):
                engine_cl.EVAL_DTYPE = ev
                with contextlib.redirect_stdout(io.StringIO()):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    acc = engine_cl.eval_data(model, [batch] * (1 if rnd == 0 else n_batches), dev, "bench", 0)      # (.item() at its end = the sync)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                if rnd:
                    res[ev].append(dict(images_per_s=n_batches * Be / dt, accuracy=acc))
                    print(f"eval EVAL_DTYPE={ev}: {n_batches * Be / dt:9.1f} images/s (accuracy {acc:.3f})", flush=True)
    finally:
        engine_cl.EVAL_DTYPE = saved
    assert model.compute_mode == "fp16"
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for s in ("accuracy", "gemm", "step", "eval"):
        ap.add_argument("--" + s, action="store_true")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/bench_f32x3.py measures on the GPU; there is none here")
    every = not (args.accuracy or args.gemm or args.step or args.eval)
    out = {"device": torch.cuda.get_device_name(0), "lib": os.environ.get("GSLORA_HIP_LIB", "product")}
    if every or args.accuracy:
        out["accuracy"] = accuracy()
    if every or args.gemm:
        out["gemm"] = gemm()
    if every or args.eval:
        out["eval"] = evaluation()
    if every or args.step:
        out["step"] = step(args.steps, args.warmup)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1)
