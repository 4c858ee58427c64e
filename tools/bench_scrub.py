#!/usr/bin/env python
"""Cost of the SCRUB loss side (libgslora_kd.so) against the route that existed before it. Prints one JSON line per cell and a markdown
table; profiles/scrub.md holds the numbers of the last run. Not part of bench.py. Nothing here is a pass / fail threshold.

  kd     gsk_kd_ce_fwd + gsk_kd_ce_bwd (through gslora_hip.kd.kd_ce and one backward) at (B, C) = (512, 100), (512, 10572), (128, 93431)
         against losses.ce_sum_top1 (gsl_ce_fwd / gsl_ce_bwd) plus the torch formula for the KL with autograd. Achieved bytes / s against
         the bytes the fused pair must move: ys and yt read by the forward, read again by the backward, the gradient written (20 B C bytes).
  dist   gslora_hip.kd.ParamDist forward + backward over the parameter list of ViT-P8S8 without LoRA (FFN linears and the head train)
         against the per-tensor torch param_dist of the reference.
  step   one min step and one max step of gslora_hip.step.scrub_step at config-2 geometry on 512 images, fp16, against the same step
         assembled from ce_sum_top1, the torch KL and the torch param_dist, same process, same optimizer.

Both forms of a cell run in the same process in alternating blocks of `--block` repetitions (host clock around a block that ends in a device
synchronise), the order flipping from round to round; per form the median block time per repetition, min and max over `--iters` rounds.

    python tools/bench_scrub.py [--parts kd,dist,step] [--iters 7]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gs-lora_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

GEO = dict(image_size=112, patch_size=8, dim=512, depth=6, heads=8, mlp_dim=2048)
HYPER = dict(kd_T=2.0, sgda_gamma=0.99, sgda_alpha=0.001)


def ab(forms, args):
    """forms: {name: callable}. -> {name: (median, min, max) seconds per repetition}"""
    import torch
    names = list(forms)
    for f in forms.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {n: [] for n in names}
    for r in range(args.iters):
        for n in (names if r % 2 == 0 else names[::-1]):
            t0 = time.perf_counter()
            for _ in range(args.block):
                forms[n]()
            torch.cuda.synchronize()
            times[n].append((time.perf_counter() - t0) / args.block)
    return {n: (statistics.median(v), min(v), max(v)) for n, v in times.items()}


def torch_kd(ys, yt, T):
    import torch.nn.functional as F
    return F.kl_div(F.log_softmax(ys / T, dim=1), F.softmax(yt / T, dim=1), reduction="sum") * T ** 2 / ys.shape[0]


def part_kd(args):
    import torch
    from gslora_hip import _lib_kd as LK, kd, losses
    rows = []
    for B, C in ((512, 100), (512, 10572), (128, 93431)):
        ys = (torch.randn(B, C, device="cuda") * 3).requires_grad_()
        yt = torch.randn(B, C, device="cuda") * 3
        y = torch.randint(0, C, (B,), device="cuda")

        def fused():
            ys.grad = None
            kd.kd_ce(ys, yt, y, 2.0, 0.001, 0.99)[2].backward()

        def before():
            ys.grad = None
            (0.99 * losses.ce_sum_top1(ys, y)[0] / B + 0.001 * torch_kd(ys, yt, 2.0)).backward()

        res = ab(dict(fused=fused, before=before), args)
        t = res["fused"][0]
        rows.append(dict(part="kd", B=B, C=C, kernel="wave" if LK.kd_plan(B, C)[0] == LK.KD_WAVE else "block", fused_us=t * 1e6,
                         fused_min_us=res["fused"][1] * 1e6, fused_max_us=res["fused"][2] * 1e6, before_us=res["before"][0] * 1e6,
                         before_min_us=res["before"][1] * 1e6, before_max_us=res["before"][2] * 1e6, gb_per_s=20.0 * B * C / t / 1e9))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def build_model(dtype, dropout=0.0):
    from driver_reg import mark_only_ffn_as_trainable
    from vit_pytorch_face import ViT_face
    m = ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=100, dropout=dropout, emb_dropout=dropout, lora_rank=0, **GEO)
    mark_only_ffn_as_trainable(m, True)
    return m.to("cuda").set_compute_dtype(dtype).train()


def averaged(model):
    import torch
    swa = torch.optim.swa_utils.AveragedModel(model, avg_fn=lambda a, p, n: 0.9 * a + 0.1 * p)
    with torch.no_grad():
        for p in swa.parameters():
            p.add_(0.01 * torch.randn_like(p))
    return swa


def torch_dist(model, swa, p):
    import torch
    return p * sum(torch.norm(a - b) for a, b in zip(model.parameters(), swa.parameters()))


def part_dist(args):
    from gslora_hip import kd
    model = build_model("fp16")
    swa = averaged(model)
    pd = kd.ParamDist(model, swa, 0.1)

    def fused():
        model.zero_grad()
        pd.loss().backward()

    def before():
        model.zero_grad()
        torch_dist(model, swa, 0.1).backward()

    res = ab(dict(fused=fused, before=before), args)
    n_elems = sum(p.numel() for p in model.parameters())
    row = dict(part="dist", tensors=pd.n_entries, trainable=len(pd.trainable), elements=n_elems, fused_us=res["fused"][0] * 1e6,
               fused_min_us=res["fused"][1] * 1e6, fused_max_us=res["fused"][2] * 1e6, before_us=res["before"][0] * 1e6,
               before_min_us=res["before"][1] * 1e6, before_max_us=res["before"][2] * 1e6)
    print(json.dumps(row), flush=True)
    return [row]


def part_step(args):
    import torch
    from gslora_hip import kd, losses, step
    from gslora_hip.optim import create_optimizer
    rows = []
    model = build_model("fp16", dropout=0.1)
    teacher = copy.deepcopy(model).eval()
    for p in teacher.parameters():
        p.requires_grad_(False)
    swa = averaged(model)
    opt = create_optimizer(SimpleNamespace(opt="adamw", weight_decay=0.05, opt_eps=1e-8, opt_betas=None, lr=1e-6), model)
    crit = torch.nn.CrossEntropyLoss()
    x = torch.randn(512, 3, 112, 112, device="cuda")
    y = torch.randint(0, 100, (512,), device="cuda")
    for smoothing in (0.0, 0.1):
        pd = kd.ParamDist(model, swa, smoothing)
        for maximize in (False, True):
            def fused():
                step.scrub_step(model, teacher, opt, crit, x, y, maximize=maximize, dist=pd, **HYPER)

            def before():
                logits, _ = model(x, y)
                with torch.no_grad():
                    t_logits, _ = teacher(x, y)
                k = torch_kd(logits, t_logits, HYPER["kd_T"])
                total = -k if maximize else HYPER["sgda_gamma"] * losses.ce_sum_top1(logits, y)[0] / 512.0 + HYPER["sgda_alpha"] * k
                total = total + torch_dist(model, swa, smoothing)      # (the reference computes it with smoothing 0 too)
                opt.zero_grad()
                total.backward()
                step._arm_overflow_guard(model, opt)
                opt.step()

            res = ab(dict(fused=fused, before=before), args)
            rows.append(dict(part="step", step="max" if maximize else "min", smoothing=smoothing, fused_ms=res["fused"][0] * 1e3,
                             fused_min_ms=res["fused"][1] * 1e3, fused_max_ms=res["fused"][2] * 1e3, before_ms=res["before"][0] * 1e3,
                             before_min_ms=res["before"][1] * 1e3, before_max_ms=res["before"][2] * 1e3))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="kd,dist,step")
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--block", type=int, default=10)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("bench_scrub: no ROCm GPU is visible (the HIP path has no CPU fallback)")
    rows = []
    for part in args.parts.split(","):
        rows += dict(kd=part_kd, dist=part_dist, step=part_step)[part](args)
    print("\n| cell | fused (median, min - max) | before (median, min - max) |\n|---|---|---|")
    for r in rows:
        unit = "ms" if r["part"] == "step" else "us"
        cell = {k: v for k, v in r.items() if not k.startswith(("fused", "before", "gb"))}
        f = lambda w: f"{r[w + '_' + unit]:.1f} ({r[w + '_min_' + unit]:.1f} - {r[w + '_max_' + unit]:.1f}) {unit}"
        print(f"| {cell} | {f('fused')}{' %.0f GB/s' % r['gb_per_s'] if 'gb_per_s' in r else ''} | {f('before')} |")


if __name__ == "__main__":
    main()
