#!/usr/bin/env python
"""bench.py — forgetting-step images/sec of the GS-LoRA step on MI355X (BASELINE.json metric).

  python bench.py --gpus N --steps K --warmup W [--scaling weak|strong] [--config 2|4|5] [--dump-outputs DIR] [--full]

N > 1: one process per GPU over RCCL. Either the driver launches the ranks (`python -m torch.distributed.run --nproc-per-node N
bench.py --gpus N ...`: RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* come from the environment) or, when WORLD_SIZE is not set,
bench.py launches them itself through torch.distributed.run on 127.0.0.1. The process group must have exactly N ranks, otherwise
the run fails.

Workload (config.workload): BASELINE.json configs[1] — ViT-P8S8 depth 6, 112 px, LoRA r=8 on both FFN linears, CosFace-100 head,
per-GPU batch 512 remain + 512 forget images resident in HBM (weak scaling; `--scaling strong` keeps the GLOBAL batch at 512 + 512),
16-bit speed mode (--dtype fp16, the default: IEEE fp16 MFMA operands; bf16: the same kernels on bf16 operands), dropout 0.1 / emb-dropout 0.1 (the reference's training setting), prototype term on, FusedAdamW (lr 1e-2, wd 0.05).
One "step" = the engine_cl.train_one_epoch loop body (2 forwards, 5 loss terms, backward, packed scalar all-reduce + gradient
all-reduce when N > 1, AdamW). Prints ONE JSON line on rank 0.

--config selects the BASELINE.json configuration (default 2, the one the metric is quoted on); the same JSON contract for all:
  2  ViT-P8S8 d6 r=8, per-GPU batch 512 + 512, dropout 0.1, eager launches (GPU-bound)                      [configs[1]]
  4  ViT-B/16 224 px r=16 (ModifiedViT, 100-way linear head), per-GPU batch 48 + 48 (scripts/run_cl_forget_image.sh:15: -b 48),
     dropout 0 (torchvision default), the step replayed as HIP-graph segments (what the engines pick below 256 images)   [configs[3]]
  5  few-shot GS-LoRA++: ViT-P8S8 d6 r=8, per-GPU batch 4 + 4, BND_pro 50, pro_f_weight 0.017 (scripts/run_cl_forget.sh:223-235),
     HIP-graph replay (launch-bound regime)                                                                  [configs[4]]

A plain run does only what the headline needs: set-up, warm-up, the timed steps, --dump-outputs, the JSON line (for eager configs its
`roofline` comes from HIP events around launches inside the timed region, at no extra run). `--full` adds the legs that run after the
timed region: the CPU baseline (config 2), the bf16 `secondary` leg (config 2, fp16), the `eval` leg, the LayerNorm / attention
`memory_bound_kernels` steps (eager configs) and, for graph-replayed configs, the 3 eager steps whose per-kernel HIP-event timings give
their `roofline` (a replay makes no Python launch to bracket; the kernels are the same). The --no-* options drop single legs of --full.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "gs-lora_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0   # dense MFMA bf16, /opt/skills/guides/MI355X_MICROARCH.md
PEAK_HBM_GBS = 8000.0       # HBM3E, same guide
FULL = dict(image_size=112, patch_size=8, dim=512, depth=6, heads=8, mlp_dim=2048, num_class=100, lora_rank=8)
HYPER = dict(lr=1e-2, wd=0.05, beta=0.15, alpha=1e-4, BND=105.0, BND_pro=18.0, pro_f=0.01, pro_r=0.01)
# minimal necessary FLOPs per image (2 m n k, no recompute, no dW of frozen weights)
FLOP_IMG_ALG = 15.646e9
# what this path executes: the head pools the cls token and everything behind a block's attention is token-wise, so in the LAST block
# only the cls query's attention output and the cls rows of out-proj / LayerNorm / FFN are ever consumed. Its backward (one generic-layer
# backward, 1.43065 GFLOP/img) and the forward behind its QKV projection (QK^T + PV 0.07948, out-proj 0.10328, FFN 0.82628, LoRA
# 0.01614 = 1.02518 GFLOP/img) shrink to 1/197 of their rows. Exact (no output of the model depends on the skipped rows); the
# fractions of the MFMA peak below are quoted on section 8(d)'s ALGORITHMIC count, the executed count is carried beside it.
FLOP_IMG_EXEC = FLOP_IMG_ALG - (1.43065e9 + 1.02518e9) * (196.0 / 197.0)
T_TOK = 197
# ViT-B/16 r=16: fwd 35.707 + bwd 35.385 GFLOP/img algorithmic; executed: the last block's backward (1/12 of 11 generic-layer
# backwards ~ 3.2 GFLOP/img) and the forward behind its QKV projection (QK^T + PV 0.119, out-proj 0.232, FFN + LoRA 1.878 = 2.229) on 1/197 of the rows
VITB = dict(image_size=224, patch_size=16, dim=768, depth=12, heads=12, mlp_dim=3072, num_class=100, lora_rank=16)
FLOP_IMG_ALG_VITB = 71.09e9
FLOP_IMG_EXEC_VITB = FLOP_IMG_ALG_VITB - (35.385e9 / 11.0 + 2.229e9) * (196.0 / 197.0)
CONFIGS = {
    2: dict(model="vitp8s8", batch=512, dropout=0.1, graph=False, BND_pro=18.0, pro_f=0.01, pro_r=0.01, rank=8,
            name="BASELINE configs[1]: ViT-P8S8 depth-6 CASIA-100-shaped single-task forget step, LoRA r=8"),
    4: dict(model="vitb16", batch=48, dropout=0.0, graph=True, BND_pro=18.0, pro_f=0.05, pro_r=0.05, rank=16,
            name="BASELINE configs[3]: ViT-B/16 224px ImageNet100-shaped forget step, LoRA r=16, 100-way linear head"),
    5: dict(model="vitp8s8", batch=4, dropout=0.1, graph=True, BND_pro=50.0, pro_f=0.017, pro_r=0.01, rank=8,
            name="BASELINE configs[4]: few-shot + prototype-regularised GS-LoRA++ step, ViT-P8S8 depth-6, LoRA r=8"),
}


def build_model(dtype, dropout, device):
    import loralib as lora
    from vit_pytorch_face import ViT_face
    torch.manual_seed(1337)
    m = ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=FULL["num_class"], image_size=FULL["image_size"],
                 patch_size=FULL["patch_size"], dim=FULL["dim"], depth=FULL["depth"], heads=FULL["heads"],
                 mlp_dim=FULL["mlp_dim"], dropout=dropout, emb_dropout=dropout, lora_rank=FULL["lora_rank"])
    lora.mark_only_lora_as_trainable(m)
    with torch.no_grad():   # non-trivial adapters (B != 0) so the LoRA paths do real work
        for n, p in m.named_parameters():
            if "lora_B" in n:
                p.normal_(0.0, 0.02)
    return m.to(device).set_compute_dtype(dtype).train()


def build_vitb16(dtype, rank, device):
    """ModifiedViT over the torchvision-named ViT-B/16 parameter tree, LoRA r on both FFN linears (replace_ffn_with_lora), 100-way head."""
    import loralib as lora
    from util.utils import replace_ffn_with_lora
    from vit_pytorch_face import ModifiedViT
    from vit_pytorch_face.modified_VIT import vit_b_16
    torch.manual_seed(1337)
    m = replace_ffn_with_lora(ModifiedViT(vit_b_16(num_classes=100)), rank=rank)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("lora_B"):
                p.normal_(0, 0.02)
        m.heads.head.weight.normal_(0, 0.02)
    lora.mark_only_lora_as_trainable(m)
    return m.to(device).set_compute_dtype(dtype).train()


def host_cpu():
    """(physical cores visible to this process, CPU model string)"""
    model, cores = "unknown", set()
    try:
        phys = core = None
        for line in open("/proc/cpuinfo"):
            k, _, v = line.partition(":")
            k, v = k.strip(), v.strip()
            if k == "model name":
                model = v
            elif k == "physical id":
                phys = v
            elif k == "core id":
                core = v
            elif not k and phys is not None:
                cores.add((phys, core))
                phys = core = None
        if phys is not None:
            cores.add((phys, core))
    except OSError:
        pass
    n_phys = len(cores) or (os.cpu_count() or 1)
    try:
        n_phys = min(n_phys, len(os.sched_getaffinity(0)))
    except AttributeError:
        pass
    return max(1, n_phys), model


def cpu_baseline(batch=16, steps=3, dropout=0.1, sweep=(16, 32, 64)):
    """SURVEY.md 8(d) / BASELINE.md section 3: the build's CPU restatement of the reference step (oracle port; the reference's Python
    cannot travel to the GPU box) timed on the host cores: fp32, B = 16 + 16, full-size model, dropout 0.1 ON (torch's own Bernoulli
    dropout at the reference's 19 sites, as the reference trains), 1 warm-up + `steps` timed. `value` is at torch.set_num_threads(physical
    cores) as 8(d) specifies; a 32-image step does not feed that many threads, so the best of a short thread sweep (1 warm-up + 2 timed
    steps each) is carried beside it — THAT is the figure to hold a GPU / CPU ratio against."""
    from oracle import gslora_oracle as O
    from oracle import recipe
    cfg = recipe.cfg_full()
    cores, model = host_cpu()
    xr = torch.tensor(recipe.make_images(cfg, batch, seed=1)); yr = torch.tensor(recipe.make_labels(cfg, batch, seed=1, hi=80))
    xf = torch.tensor(recipe.make_images(cfg, batch, seed=2)); yf = torch.tensor(recipe.make_labels(cfg, batch, seed=2, lo=80))
    proto = torch.tensor(recipe.make_prototypes(cfg))
    hy = dict(beta=HYPER["beta"], alpha=HYPER["alpha"], BND=HYPER["BND"], BND_pro=HYPER["BND_pro"], pro_f_weight=HYPER["pro_f"],
              pro_r_weight=HYPER["pro_r"], wd=HYPER["wd"], dropout=dropout)

    def run(threads, nsteps):
        torch.set_num_threads(threads)
        st, opt, times = recipe.make_state(cfg), None, []
        for s in range(nsteps + 1):
            t0 = time.perf_counter()
            _, _, new_st, opt = O.train_step(st, cfg, xr, yr, xf, yf, hy, opt_state=opt, step=s + 1, lr=HYPER["lr"], proto=proto)
            st = {k: v.numpy() for k, v in new_st.items()}
            if s:
                times.append(time.perf_counter() - t0)
        return sorted(times)[len(times) // 2]
    t = run(cores, steps)
    sw = {}
    for th in sorted(set(x for x in sweep if x < cores)):
        sw[str(th)] = round(2 * batch / run(th, 2), 3)
    best = max([(v, k) for k, v in sw.items()] + [(round(2 * batch / t, 3), str(cores))])
    return {"value": round(2 * batch / t, 3), "unit": "images/s", "cores": cores, "kind": "port",
            "thread_sweep": sw, "best_of_sweep": {"value": best[0], "threads": int(best[1])},
            "sample": f"oracle train_step (fp32 torch CPU, dropout {dropout}), ViT-P8S8 d6 r8, B={batch}+{batch}, median of {steps} timed steps "
                      f"after 1 warm-up, {t:.2f} s/step, {cores} threads = physical cores visible, CPU: {model}; thread sweep = images/s at "
                      f"fewer threads (1 warm-up + 2 timed steps each)"}


def self_launch(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks through torch.distributed.run (one process per GPU)."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd)


class StubWorkload:
    """GSL_BENCH_STUB=1 (tests/test_bench_launch.py): a CPU stand-in step under gloo, so that the launch / process-group / barrier /
    max-over-ranks / JSON plumbing of this file is exercised where no GPU exists. Never measured, never used by the driver."""
    device_type = "cpu"

    def __init__(self, args, rank, world, dev):
        self.B = args.batch
        self.w = torch.ones(64, 64)

    def step(self):
        self.w = torch.tanh(self.w @ self.w * 1e-3)
        if dist.is_initialized():
            dist.all_reduce(self.w)
        return self.w.reshape(-1)[:8].clone()

    def outputs(self, pack):
        return {"meters": pack, "w": self.w}

    def profile(self):
        return {}


class GsLoraWorkload:
    device_type = "cuda"

    def __init__(self, args, rank, world, dev):
        from gslora_hip.optim import FusedAdamW
        from gslora_hip.step import GraphedStep, gs_lora_step
        self.args, self.B = args, args.batch
        B, C = self.B, CONFIGS[args.config]
        vitb = C["model"] == "vitb16"
        self.model = build_vitb16(args.dtype, C["rank"], dev) if vitb else build_model(args.dtype, args.dropout, dev)
        self.opt = FusedAdamW([p for p in self.model.parameters() if p.requires_grad], lr=HYPER["lr"], weight_decay=HYPER["wd"], eps=1e-8)
        self.crit = crit = torch.nn.CrossEntropyLoss()
        g = torch.Generator(device="cpu").manual_seed(1337 + rank)
        import random
        order = list(range(100)); random.seed(1337); random.shuffle(order)
        if vitb:      # [B, 3, 224, 224] normalised by the ImageNet mean / std (train_own_forget_cl.py:138-146)
            mean, std = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1), torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
            mk_img = lambda: (((torch.randint(0, 256, (B, 3, 224, 224), generator=g, dtype=torch.uint8).float() / 255.0) - mean) / std).to(dev)
            dim = VITB["dim"]
        else:
            mk_img = lambda: (torch.randint(0, 256, (B, 3, 112, 112), generator=g, dtype=torch.uint8).float() / 255.0).to(dev)
            dim = FULL["dim"]
        self.x_r, self.x_f = mk_img(), mk_img()
        self.y_r = torch.tensor(order[:80])[torch.randint(0, 80, (B,), generator=g)].to(dev)
        self.y_f = torch.tensor(order[80:])[torch.randint(0, 20, (B,), generator=g)].to(dev)
        self.proto = torch.randn(100, dim, generator=g).to(dev)
        self.graph = bool(args.graph)
        self.eager = lambda *a, **k: gs_lora_step(self.model, self.opt, crit, *a, **k)
        self.stepper = GraphedStep(self.model, self.opt, crit) if args.graph else self.eager
        self.kw = dict(beta=HYPER["beta"], alpha=HYPER["alpha"], BND=HYPER["BND"], use_structure=True, group_type="block", use_prototype=True,
                       proto_table=self.proto, w_f=C["pro_f"], w_r=C["pro_r"], BND_pro=C["BND_pro"])

    def step(self, eager=False):
        return (self.eager if eager else self.stepper)(self.x_r, self.y_r, self.x_f, self.y_f, **self.kw)

    def outputs(self, pack):
        """What a caller of the step receives: the 8 meters it returns, and in place the updated trainable (LoRA) parameters and the
        gradients the update was computed from."""
        out = {"meters": pack}
        for n, p in self.model.named_parameters():
            if p.requires_grad:
                out["param." + n] = p
                if p.grad is not None:
                    out["grad." + n] = p.grad
        return out

    def eval_leg(self, n_batches):
        """engine_cl.eval_data (reference engine_cl.py:318-346) on a synthetic test loader shaped like the reference's: batches of
        5 x batch images (train/train_own_forget_cl.py:737-750), device resident, labels passed (margin logits). Timed OUTSIDE the step
        metric's region, in both evaluation dtypes: "fp32" = the engines' default (the reference's arithmetic, whatever mode the model
        trains in), "fp16" / "bf16" = the two 16-bit operand formats (GSLORA_EVAL_DTYPE=fp16 | bf16 | model). One untimed batch first (operand caches of the evaluation dtype, eval-mode merge)."""
        import engine_cl
        dev = self.x_r.device
        g = torch.Generator(device="cpu").manual_seed(4242)
        Be = 5 * self.B
        shape = (Be,) + tuple(self.x_r.shape[1:])
        batch = ((torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).float() / 255.0).to(dev), torch.randint(0, 100, (Be,), generator=g).to(dev))
        out, saved = {}, engine_cl.EVAL_DTYPE
        import contextlib
        import io
        try:
            for name, ev in (("fp32", "fp32"), ("fp16", "fp16"), ("bf16", "bf16")):
                engine_cl.EVAL_DTYPE = ev
                with contextlib.redirect_stdout(io.StringIO()):
                    engine_cl.eval_data(self.model, [batch], dev, "warm-up", 0)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    acc = engine_cl.eval_data(self.model, [batch] * n_batches, dev, "bench", 0)      # (.item() at its end = the sync)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                out[name] = {"images_per_s": round(n_batches * Be / dt, 1), "ms_per_batch": round(1e3 * dt / n_batches, 2), "accuracy": acc}
        finally:
            engine_cl.EVAL_DTYPE = saved
            self.model.train()
        return {"what": "engine_cl.eval_data, eval mode (LoRA merged), margin logits + top-1 on the device, one host read per call",
                "batch": Be, "batches_timed": n_batches, "default_dtype": saved, **out}

    def adopt_static_inputs(self):
        """HIP-graph replay reads the batch from static buffers. The synthetic batch is device resident, so after the capture it simply
        lives IN those buffers (as a prefetcher's H2D copy would put it there): no per-step staging copy inside the timed region."""
        get = getattr(self.stepper, "static_inputs", None)
        bufs = get(self.x_r, self.y_r, self.x_f, self.y_f, **self.kw) if get else None
        if bufs is not None:
            self.x_r, self.y_r, self.x_f, self.y_f = bufs
        return bufs is not None


def kernel_roofline(name, what, recs, flops_of, bytes_of):
    """Live numbers of one GEMM family: HIP-event duration of every launch in the timed region (events recorded on the stream the
    kernel is launched on), algorithmic FLOPs / bytes per launch from the launch's own shape."""
    durs = [a.elapsed_time(b) for a, b, *_ in recs]
    mmax = max(r[2] for r in recs)
    dense = [(d, r) for d, r in zip(durs, recs) if r[2] == mmax]            # the cls-row launches of the last block are a different shape
    if not dense:
        return None
    avg_ms = sum(d for d, _ in dense) / len(dense)
    _, _, M, N, K, K2 = dense[0][1]
    fl, by = flops_of(M, N, K, K2), bytes_of(M, N, K, K2)
    tf = fl / (avg_ms * 1e-3) / 1e12
    gbs = by / (avg_ms * 1e-3) / 1e9
    return {"kernel": name, "what": what, "launches_timed": len(dense), "rows_per_launch": M, "avg_ms": round(avg_ms, 4),
            "algorithmic_flops": fl, "algorithmic_bytes": by, "mfma_tflops": round(tf, 2), "mfma_frac_of_peak": round(tf / PEAK_BF16_TFLOPS, 4),
            "hbm_gbs": round(gbs, 1), "hbm_frac_of_peak": round(gbs / PEAK_HBM_GBS, 4), "arithmetic_intensity_flop_per_byte": round(fl / by, 1)}


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(d, arrays):
    """--dump-outputs: every array as d/<name>.npy in float32. Copied to the host at once: later steps overwrite the step's outputs."""
    import numpy as np
    host = {k: v.detach().float().cpu().numpy() for k, v in arrays.items()}
    total = sum(a.nbytes for a in host.values())
    if total > DUMP_MAX_BYTES:
        raise SystemExit(f"--dump-outputs: {total} bytes of outputs, more than {DUMP_MAX_BYTES}")
    os.makedirs(d, exist_ok=True)
    for k, a in host.items():
        np.save(os.path.join(d, k + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", type=int, default=2, choices=sorted(CONFIGS), help="BASELINE.json configuration: 2 (default, the metric's), 4 ViT-B/16 r=16 b48, 5 few-shot b4")
    ap.add_argument("--batch", type=int, default=None, help="per-GPU images per forward (remain and forget each; default: the config's); with --scaling strong: the GLOBAL batch")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak")
    ap.add_argument("--dtype", default="fp16", help="fp16 (default since round 5: IEEE fp16 MFMA operands, loss-scaled backward) | bf16 | fp32 (parity mode)")
    ap.add_argument("--dropout", type=float, default=None)
    ap.add_argument("--full", action="store_true", help="after the timed region also run the CPU baseline, the secondary, eval and "
                    "memory-bound-kernel legs and, for graph-replayed configs, the eager steps of the roofline (off: only what the headline needs)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline (N = 1, config 2 only)")
    ap.add_argument("--graph", action="store_true", default=None, help="replay the step as captured HIP graph segments (the engines' default for launch-bound batches; default: the config's)")
    ap.add_argument("--no-graph", dest="graph", action="store_false")
    ap.add_argument("--no-eval", action="store_true", help="with --full: skip the eval_data leg (N = 1 only: test-set evaluation throughput, batches of 5 x batch)")
    ap.add_argument("--eval-batches", type=int, default=3)
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the secondary leg (N = 1, config 2, --dtype fp16 only: the same step on bf16 operands = BASELINE configs[1] as written, 3 warm-up + 10 timed steps after the timed region)")
    ap.add_argument("--no-mem-kernels", action="store_true", help="with --full: skip the two extra steps after the timed region that time the LayerNorm / attention launches (roofline.memory_bound_kernels)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last one computed (its 8 meters, "
                    "the updated LoRA parameters and their gradients) as DIR/<name>.npy in float32, on rank 0")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    C = CONFIGS[args.config]
    args.batch = C["batch"] if args.batch is None else args.batch
    args.dropout = C["dropout"] if args.dropout is None else args.dropout
    args.graph = C["graph"] if args.graph is None else args.graph
    if not args.full:
        args.no_cpu_baseline = args.no_eval = args.no_secondary = args.no_mem_kernels = True

    stub = os.environ.get("GSL_BENCH_STUB") == "1"
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(args))
    env_world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if not stub and not torch.cuda.is_available():
        raise SystemExit("bench.py needs a ROCm GPU (the GS-LoRA step has no CPU fallback)")
    # development knobs for exercising the world > 1 code path on a 1-GPU box: GSL_BENCH_ONE_DEVICE=1 puts every rank on cuda:0 and
    # GSL_BENCH_BACKEND=gloo replaces RCCL (which refuses two ranks on one device). Never set by the driver.
    if os.environ.get("GSL_BENCH_ONE_DEVICE") == "1":
        local = 0
    if stub:
        dev = torch.device("cpu")
    else:
        torch.cuda.set_device(local)
        dev = torch.device("cuda", local)
    if env_world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = "gloo" if stub else os.environ.get("GSL_BENCH_BACKEND", "nccl")      # "nccl" IS RCCL on ROCm
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    if env_world == 1 and os.environ.get("GSL_BENCH_DP1") == "1" and not stub:
        # development knob: a ONE-rank RCCL group with the data-parallel form of the step forced on (every collective is an identity):
        # measures what the packed all-reduce, the side-stream gradient reduction and RCCL's stream plumbing cost per step on one GPU
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(29500 + os.getpid() % 1000))
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        from gslora_hip import step as _step
        _step._dp_active = lambda: True
    world = dist.get_world_size() if dist.is_initialized() else 1
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the process group has {world} rank(s) (WORLD_SIZE={os.environ.get('WORLD_SIZE')}); "
                         "launch one rank per GPU with torch.distributed.run, or call bench.py without a launcher")
    if args.scaling == "strong":
        if args.batch % world:
            raise SystemExit(f"--scaling strong: the global batch {args.batch} is not divisible by {world} ranks")
        args.batch //= world

    if not stub:
        from gslora_hip import ops
    wl = (StubWorkload if stub else GsLoraWorkload)(args, rank, world, dev)
    B = args.batch

    def fence():
        if not stub:
            torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            if not stub:
                torch.cuda.synchronize()

    for _ in range(args.warmup):
        wl.step()
    static_in = wl.adopt_static_inputs() if (args.graph and not stub) else False
    fence()
    if not stub:
        ops.PROFILE = {"ffn1": [], "ffn2dx": []}
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]     # per-step HIP events (no sync inside the timed region)
        marks[0].record()
    t0 = time.perf_counter()
    for i in range(args.steps):
        pack = wl.step()
        if not stub:
            marks[i + 1].record()
    fence()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, wl.outputs(pack))
    prof = {}
    per_step = [0.0]
    prof_source = "HIP events around every launch inside the timed region"
    if not stub:
        per_step = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps))
        if args.graph:      # a replay makes no Python launch to bracket: time the same kernels in eager steps OUTSIDE the timed region
            ops.PROFILE = {"ffn1": [], "ffn2dx": []}
            if args.full:       # (a plain run carries no roofline for graph-replayed configs)
                for _ in range(3):
                    wl.step(eager=True)
                fence()
            prof_source = "HIP events around every launch of 3 eager steps run after the timed region (the timed steps are HIP-graph replays)"
        prof, ops.PROFILE = ops.PROFILE, None
        # north_star: "achieved HBM GB/s on the norm/softmax kernels": LayerNorm and attention launches bracketed by HIP events in TWO extra
        # steps AFTER the timed region (31 more event pairs per step inside it would serialise kernel hand-overs the step otherwise overlaps)
        mem_prof = None
        if world == 1 and not args.graph and not args.no_mem_kernels:
            ops.PROFILE = {"ln_fwd": [], "ln_bwd": [], "attn_fwd": [], "attn_bwd": []}
            for _ in range(2):
                wl.step()
            fence()
            mem_prof, ops.PROFILE = ops.PROFILE, None
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()
    meters = pack.tolist()
    secondary = None
    if world == 1 and not stub and args.config == 2 and args.dtype == "fp16" and not args.no_secondary:
        # BASELINE configs[1] names bf16: the same step, same batch, same kernels on bf16 operands, timed AFTER (outside) the primary region
        import copy
        a2 = copy.copy(args)
        a2.dtype = "bf16"
        wl2 = GsLoraWorkload(a2, rank, world, dev)
        for _ in range(3):
            wl2.step()
        fence()
        t2 = time.perf_counter()
        for _ in range(10):
            wl2.step()
        fence()
        e2 = time.perf_counter() - t2
        secondary = {"dtype": "bf16", "what": "the same step / batch / kernels on bf16 MFMA operands (BASELINE configs[1] as written; no loss scale), "
                                              "3 warm-up + 10 timed steps run after the primary timed region",
                     "steps": 10, "warmup": 3, "ms_per_step": round(1e3 * e2 / 10, 3), "value": round(2 * B * 10 / e2, 2), "unit": "images/s"}
        del wl2
        torch.cuda.empty_cache()
    eval_res = None
    if world == 1 and not stub and not args.no_eval:
        eval_res = wl.eval_leg(args.eval_batches)

    if rank == 0:
        C = CONFIGS[args.config]
        vitb = C["model"] == "vitb16"
        r = C["rank"]
        flop_alg, flop_exec = (FLOP_IMG_ALG_VITB, FLOP_IMG_EXEC_VITB) if vitb else (FLOP_IMG_ALG, FLOP_IMG_EXEC)
        kernels = []
        if prof.get("ffn1"):
            # fused FFN1: [x | s x A1^T] [W1 | B1]^T, bias + GELU + GELU' + dropout, TWO [M, mlp] outputs (h bf16, GELU' as the 8-bit code).
            # FLOPs = 2 M N (K + r); bytes = A + LoRA segment read, h (2 B) + GELU' (1 B) written
            kernels.append(kernel_roofline(
                "gsl_gemm_nt<BIAS_GELU_G8>", "fused FFN1 + LoRA-up K-segment + bias + GELU + 8-bit GELU' + dropout (forward)", prof["ffn1"],
                lambda M, N, K, K2: 2.0 * M * N * K + 2.0 * M * N * r, lambda M, N, K, K2: int(M * (K + K2) * 2 + M * N * 2 + M * N)))
        if prof.get("ffn2dx"):
            # FFN2-dX: dZ = (dY W2 + t A2) * GELU' with t = s dY B2 in the kernel, + the two LoRA-gradient reductions of its tiles.
            # FLOPs = 2 M N K + LoRA (down 2 M K r, up 2 M N r, two reductions 2 * 2 M N r); bytes = dY + 8-bit GELU' + h read, dZ written
            kernels.append(kernel_roofline(
                "gsl_gemm_nt_lora_mulgrad", "FFN2-dX x GELU' + in-kernel LoRA + dB1 / dA2 reductions (backward)", prof["ffn2dx"],
                lambda M, N, K, K2: 2.0 * M * N * K + 2.0 * M * K * r + 6.0 * M * N * r, lambda M, N, K, K2: int(M * K * 2 + 2 * M * N * 2 + M * N)))
        kernels = [k for k in kernels if k]
        mem_kernels = []
        if not stub and mem_prof:
            eb = 2      # bytes per element of the 16-bit modes' streams and operands (f32 parity mode: 4)
            if args.dtype == "fp32":
                eb = 4
            specs = [("ln_fwd", "gsl_layernorm_fwd", "LayerNorm forward: the stream read, the operand written (+ row statistics)", lambda M, D, T, H: int(M * D * 2 * eb + 8 * M)),
                     ("ln_bwd", "gsl_layernorm_bwd", "LayerNorm backward: dy, x and the residual gradient read; the stream gradient and its dropout-masked operand copy written",
                      lambda M, D, T, H: int(M * D * 5 * eb + 8 * M)),
                     ("attn_fwd", "gsl_attention_fwd", "attention forward (softmax in registers): qkv read, o + lse written", lambda M, D, T, H: int(M * D * 4 * eb + 4 * M * H)),
                     ("attn_bwd", "gsl_attention_bwd", "attention backward: qkv, o, dO, lse read; dqkv written", lambda M, D, T, H: int(M * D * 8 * eb + 4 * M * H))]
            for tag, name, what, by in specs:
                if mem_prof.get(tag):
                    k = kernel_roofline(name, what, mem_prof[tag], lambda M, D, T, H: 0.0, by)
                    if k:
                        k = {kk: k[kk] for kk in ("kernel", "what", "launches_timed", "rows_per_launch", "avg_ms", "algorithmic_bytes", "hbm_gbs", "hbm_frac_of_peak")}
                        k["timing_source"] = "HIP events around every launch of 2 steps run after the timed region"
                        mem_kernels.append(k)
        traffic, traffic_source = None, None
        try:   # HBM bytes per launch of the dominant kernel, from the committed PMC passes (rocprofv3 cannot wrap itself)
            pj = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
            if kernels and args.config == 2 and pj.get("rows_per_launch") == kernels[0]["rows_per_launch"]:
                traffic, traffic_source = pj["hbm_bytes_per_launch"], pj.get("source")
        except Exception:
            pass
        k0 = kernels[0] if kernels else None
        ips = world * 2 * B * args.steps / elapsed
        img = "224x224, ImageNet-normalised" if vitb else "112x112"
        metric = {2: "forgetting-step images/sec, ViT-P8S8 d6 112px r=8", 4: "forgetting-step images/sec, ViT-B/16 224px r=16",
                  5: "forgetting-step images/sec, ViT-P8S8 d6 112px r=8, few-shot batch"}[args.config]
        out = {
            "metric": metric, "value": round(ips, 2), "unit": "images/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 3),
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None, "dtype": args.dtype,
            "dtype_note": {"fp16": "IEEE fp16 MFMA operands (v_mfma_f32_16x16x32_f16: the rate and bytes of bf16, 11-bit significand), f32 accumulate, "
                                   "backward on loss-scaled gradients; --dtype bf16 runs the same kernels on bf16 operands (the secondary leg of --full). "
                                   "Two sub-16-bit approximations sit on the path in both 16-bit modes: GELU'*dropout-mask is saved as an 8-bit "
                                   "fixed-point code (q = round(GELU' * keep * 200 + 26), abs. error <= 0.0025/(1-p)), and GELU / GELU' of the fused "
                                   "FFN1 epilogue come from a 4096-entry table (|dPhi| <= 4.5e-4); both are inside the accuracy statistics of DESIGN.md section 7",
                           "bf16": "bf16 MFMA operands, f32 accumulate", "fp32": "exact-f32 parity kernels"}.get(args.dtype, args.dtype),
            "data": "synthetic",
            "config": {"workload": ("STUB (CPU plumbing test, not a measurement)" if stub else
                                    f"{C['name']}, per-GPU batch {B} remain + {B} forget ({img} synthetic), dropout {args.dropout}, prototype "
                                    f"term on (BND_pro {C['BND_pro']}, w_f {C['pro_f']}), FusedAdamW" + (", HIP-graph replay" if args.graph else "")),
                       "baseline_config": args.config, "global_batch": world * 2 * B, "tokens_per_image": T_TOK, "parallelism": f"dp{world}"},
        }
        if k0:
            # the step's roof is the bf16 MFMA peak; the dominant kernel is priced against it with 8(d)'s FLOPs
            # (2 M N (K + r)). Its HBM view (it writes two [M, mlp] outputs: 228 FLOP/B, below the 312 FLOP/B ridge) is carried beside it.
            out["roofline"] = {"bound": "mfma", "kernel": k0["kernel"] + " — " + k0["what"], "achieved": k0["mfma_tflops"],
                               "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": k0["mfma_frac_of_peak"], "traffic": traffic,
                               "traffic_source": traffic_source, "timing_source": prof_source, "launches_timed": k0["launches_timed"],
                               "rows_per_launch": k0["rows_per_launch"], "avg_ms": k0["avg_ms"],
                               "algorithmic_flops": k0["algorithmic_flops"], "algorithmic_bytes": k0["algorithmic_bytes"],
                               "hbm_view": {"achieved": k0["hbm_gbs"], "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": k0["hbm_frac_of_peak"]},
                               "kernels": sorted(kernels, key=lambda k: -k["avg_ms"] * k["launches_timed"]),
                               "dominant_by_time": max(kernels, key=lambda k: k["avg_ms"] * k["launches_timed"])["kernel"],
                               "memory_bound_kernels": mem_kernels}
        out.update({
            # primary: the FLOPs this path EXECUTES (the last block's tail runs on the cls rows); the 8(d) algorithmic count beside it credits
            # work that is provably never needed and is NOT the figure to quote
            "step_flops_frac_of_peak": round((flop_exec * world * 2 * B * args.steps / elapsed) / (world * PEAK_BF16_TFLOPS * 1e12), 4),
            "step_flops_frac_of_peak_on_8d_algorithmic_count": round((flop_alg * world * 2 * B * args.steps / elapsed) / (world * PEAK_BF16_TFLOPS * 1e12), 4),
            "flops_per_image": {"algorithmic_8d": flop_alg, "executed": round(flop_exec)},
            "last_step_meters": {"beta*loss_forget": meters[0], "loss_remain": meters[1], "total": meters[2]},
            "hip_graph": bool(args.graph),
            "hip_graph_static_inputs": bool(static_in),
            "hip_graph_counters": ({"eager_steps": wl.stepper.eager_steps, "captures": wl.stepper.captures, "replays": wl.stepper.replays,
                                    "failed_keys": len(wl.stepper.failed)} if args.graph and hasattr(wl.stepper, "replays") else None),
            "ms_per_step_events": {"median": round(per_step[len(per_step) // 2], 3), "p10": round(per_step[int(0.1 * (len(per_step) - 1))], 3),
                                   "p90": round(per_step[int(round(0.9 * (len(per_step) - 1)))], 3)},
        })
        if secondary:
            out["secondary"] = secondary
        if world > 1 or dist.is_initialized():
            comm = {"backend": dist.get_backend(), "world": dist.get_world_size()}
            try:
                comm["rccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
            except Exception as e:      # gloo stub runs / builds without the binding
                comm["rccl_version"] = None
            out["comm"] = comm
        if eval_res:
            out["eval"] = eval_res
        if world == 1 and not args.no_cpu_baseline and not stub and args.config == 2:
            out["cpu_baseline"] = cpu_baseline()
        elif args.full and not stub and args.config != 2:
            out["cpu_baseline_note"] = "timed on the configuration the metric is quoted on only (python bench.py --config 2 --full)"
    # the JSON line must be the LAST line of the job's stdout: RCCL writes its version banner through C stdio, which a piped stdout
    # only flushes at exit (i.e. after Python's own print) — push every rank's C buffer out first, then let rank 0 print
    sys.stdout.flush()
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except OSError:
        pass
    if dist.is_initialized() and world > 1:
        dist.barrier()
    if rank == 0:
        print(json.dumps(out), flush=True)
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
