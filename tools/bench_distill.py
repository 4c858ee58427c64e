#!/usr/bin/env python
"""Cost of the loss side of the DER / DER++ / FDR baselines (libgslora_fd.so) against the same expression in torch ops on the same device
tensors, and of a whole step per method. Prints one JSON line per cell and a markdown table, and with --write stores the table in
profiles/distill_baselines.md. Not part of bench.py. Nothing here is a pass / fail threshold.

  dist   gslora_hip.fd.row_dist forward + backward over the remain rows of a fused [Btot, W] tensor (Btot = 3/2 B: a forget batch in front)
         against the torch expression with autograd on a slice of the same tensor: mode "sq" (DER, torch.norm(a - t, p=2) squared) at
         W = 512 (the embedding) and mode "rownorm" (FDR, torch.norm(a - t, 2, 1).mean()) at W = 100, 10 572 and 93 431 classes. Achieved
         bytes / s against the bytes the pair must move: a and t read by the forward, read again by the backward, the gradient of the whole
         fused tensor written (4 W (4 B + Btot) bytes).
  step   one gslora_hip.step.distill_step per method (lwf, der, derpp, fdr) at config-2 geometry, fp16, 256 forget + 256 remain (+ 256)
         images, against the same step assembled as the reference writes it: one student forward per batch, losses.ce_sum_top1, the torch
         distance, same process, same optimizer.

Both forms of a cell run in the same process in alternating blocks of `--block` repetitions (host clock around a block that ends in a device
synchronise), the order flipping from round to round; per form the median block time per repetition, min and max over `--iters` rounds.

    python tools/bench_distill.py [--parts dist,step] [--iters 7] [--write [--out FILE]]
"""
import argparse
import copy
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gs-lora_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_scrub import ab, build_model  # noqa: E402

LAMBDAS = {"lwf": ("lwf", 0.5, 1.0), "der": ("der", 0.1, 0.0), "derpp": ("der", 0.1, 0.1), "fdr": ("fdr", 0.1, 0.0)}


def torch_dist(a, t, mode):
    import torch
    if mode == "sq":
        n = torch.norm(a - t, p=2)
        return n * n
    return torch.norm(a - t, 2, 1).mean()


def part_dist(args):
    import torch
    from gslora_hip import _lib_fd as LF, fd
    rows = []
    for mode, B, W in (("sq", 512, 512), ("rownorm", 512, 100), ("rownorm", 512, 10572), ("rownorm", 128, 93431)):
        nf = B // 2
        full = (torch.randn(nf + B, W, device="cuda") * 3).requires_grad_()
        t = torch.randn(B, W, device="cuda") * 3

        def fused():
            full.grad = None
            fd.row_dist(full, nf, B, t, mode, 0.1)[1].backward()

        def before():
            full.grad = None
            (0.1 * torch_dist(full[nf:], t, mode)).backward()

        res = ab(dict(fused=fused, before=before), args)
        sec = res["fused"][0]
        rows.append(dict(part="dist", mode=mode, B=B, W=W, kernel="wave" if LF.rowdist_plan(B, W)[0] == LF.FD_WAVE else "block",
                         fused_us=sec * 1e6, fused_min_us=res["fused"][1] * 1e6, fused_max_us=res["fused"][2] * 1e6,
                         before_us=res["before"][0] * 1e6, before_min_us=res["before"][1] * 1e6, before_max_us=res["before"][2] * 1e6,
                         gb_per_s=4.0 * W * (4 * B + nf + B) / sec / 1e9))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def part_step(args):
    import torch
    from gslora_hip import losses, step
    from gslora_hip.optim import create_optimizer
    rows = []
    model = build_model("fp16", dropout=0.1)
    teacher = copy.deepcopy(model).eval()
    with torch.no_grad():
        for n, p in teacher.named_parameters():
            p.requires_grad_(False)
            if "fn.fn.net" in n and n.endswith("bias"):
                p.add_(0.05 * torch.randn_like(p))
    teacher.invalidate_operand_caches()
    opt = create_optimizer(SimpleNamespace(opt="adamw", weight_decay=0.05, opt_eps=1e-8, opt_betas=None, lr=1e-6), model)
    crit = torch.nn.CrossEntropyLoss()
    n = args.images
    mk = lambda: (torch.randn(n, 3, 112, 112, device="cuda"), torch.randint(0, 100, (n,), device="cuda"))
    (x_f, y_f), (x_r, y_r), (x_n, y_n) = mk(), mk(), mk()
    ce = lambda logits, y: losses.ce_sum_top1(logits, y)[0] / float(y.shape[0])
    for method, (m, lam, lam_aux) in LAMBDAS.items():
        extra = dict(x_n=x_n, y_n=y_n) if method == "derpp" else {}

        def fused():
            step.distill_step(model, teacher, opt, crit, x_f, y_f, x_r, y_r, method=m, lam=lam, lam_aux=lam_aux, **extra)

        def before():      # the reference's loop body: a forward per batch, the teacher's forward in every method (LwF's included)
            total = ce(model(x_f, y_f)[0], y_f)
            out_r, emb_r = model(x_r, y_r)
            with torch.no_grad():
                t_out, t_emb = teacher(x_r, y_r)
            if method == "lwf":
                total = total + lam_aux * ce(out_r, y_r)
            elif method == "fdr":
                total = total + lam * torch_dist(out_r, t_out, "rownorm")
            else:
                total = total + lam * torch_dist(emb_r, t_emb, "sq")
                if method == "derpp":
                    total = total + lam_aux * ce(model(x_n, y_n)[0], y_n)
            opt.zero_grad()
            total.backward()
            step._arm_overflow_guard(model, opt)
            opt.step()

        res = ab(dict(fused=fused, before=before), args)
        rows.append(dict(part="step", method=method, images=n * (3 if method == "derpp" else 2), fused_ms=res["fused"][0] * 1e3,
                         fused_min_ms=res["fused"][1] * 1e3, fused_max_ms=res["fused"][2] * 1e3, before_ms=res["before"][0] * 1e3,
                         before_min_ms=res["before"][1] * 1e3, before_max_ms=res["before"][2] * 1e3))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="dist,step")
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--images", type=int, default=256, help="images per batch of the step cells")
    ap.add_argument("--write", action="store_true", help="store the table in profiles/distill_baselines.md (or --out)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distill_baselines.md"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("bench_distill: no ROCm GPU is visible (the HIP path has no CPU fallback)")
    rows = []
    for part in args.parts.split(","):
        rows += dict(dist=part_dist, step=part_step)[part](args)
    lines = ["| cell | libgslora_fd / distill_step (median, min - max) | torch expression / assembled step (median, min - max) |", "|---|---|---|"]
    for r in rows:
        unit = "ms" if r["part"] == "step" else "us"
        cell = {k: v for k, v in r.items() if not k.startswith(("fused", "before", "gb"))}
        f = lambda w: f"{r[w + '_' + unit]:.1f} ({r[w + '_min_' + unit]:.1f} - {r[w + '_max_' + unit]:.1f}) {unit}"
        lines.append(f"| {cell} | {f('fused')}{' %.0f GB/s' % r['gb_per_s'] if 'gb_per_s' in r else ''} | {f('before')} |")
    table = "\n".join(lines)
    print("\n" + table)
    if args.write:
        dev = torch.cuda.get_device_name(0)
        text = ("# The distillation baselines: loss side and whole steps\n\n"
                f"Measured by `python tools/bench_distill.py --iters {args.iters} --block {args.block} --images {args.images} --write` on one "
                f"{dev} (torch {torch.__version__}). Every number below was measured in that run: host clock around blocks of "
                f"{args.block} repetitions that end in a device synchronise, both forms alternating in one process, median and min - max over "
                f"{args.iters} rounds. The cells and the byte count behind the GB/s column are described in the tool's docstring. No test "
                "asserts a time.\n\n" + table + "\n")
        out = args.out
        with open(out, "w") as fh:
            fh.write(text)
        print("wrote", out)


if __name__ == "__main__":
    main()
