#!/usr/bin/env python
"""Times the LIRF baseline on one MI355X: the attention-transfer kernels alone (device events around loops of calls, bytes from shapes)
against the torch expression of at_loss with autograd on the same tensors, and gslora_hip.step.lirf_step at config-2 geometry.

    python tools/bench_lirf.py [--out profiles/lirf_baseline.json] [--batch 128] [--iters 50]

Bytes counted: forward 2 * B * T * D * sizeof(element) (both streams once); backward B * T * D * (sizeof(stream) + 2 * sizeof(gradient))
(one read of the stream, one read and one write of the gradient). The tables and the workspace are B * D floats: not counted.
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gs-lora_amd")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def timed(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters      # ms per call


def torch_at_loss(x, y):
    def at(t):
        a = F.normalize(t.float().pow(2).mean(1).view(t.size(0), -1))
        return torch.where(a < 0.005, torch.zeros_like(a), a)
    return (at(x) - at(y)).pow(2).mean()


def kernels(B, T, D, dtype, iters):
    from gslora_hip import at as AT
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = torch.randn(B, T, D, device="cuda", generator=g).to(dtype)
    xt = torch.randn(B, T, D, device="cuda", generator=g).to(dtype)
    dmid = torch.zeros(B, T, D, device="cuda", dtype=dtype)
    coef, one = torch.full((1,), -300.0, device="cuda"), torch.ones(1, device="cuda")
    loss, G = AT.at_loss_value_and_table(xs, B, T, xt)
    es = xs.element_size()
    fwd = timed(lambda: AT.at_loss_value_and_table(xs, B, T, xt), iters)
    bwd = timed(lambda: AT.at_inject(dmid, xs, G, coef, one), iters)
    xr = xs.clone().requires_grad_(True)

    def torch_both():
        xr.grad = None
        torch_at_loss(xr, xt).backward()
    tfwd = timed(lambda: torch_at_loss(xs, xt), iters)
    tboth = timed(torch_both, iters)
    want = torch_at_loss(xs, xt)
    n = B * T * D
    return dict(B=B, T=T, D=D, dtype=str(dtype).replace("torch.", ""), fwd_ms=fwd, bwd_ms=bwd, fwd_GBps=2 * n * es / fwd / 1e6,
                bwd_GBps=3 * n * es / bwd / 1e6, torch_fwd_ms=tfwd, torch_fwd_bwd_ms=tboth, value=float(loss), torch_value=float(want))


def whole_step(batch, dtype, iters):
    from gslora_hip import step
    from gslora_hip.optim import create_optimizer
    from vit_pytorch_face import ViT_face, ViT_face_low, ViT_face_up
    kw = dict(loss_type="CosFace", GPU_ID=[0], num_class=100, image_size=112, patch_size=8, dim=512, depth=6, heads=8, mlp_dim=2048, dropout=0.1,
              emb_dropout=0.1, lora_rank=0)
    torch.manual_seed(0)
    state = ViT_face(**kw).state_dict()
    nets = [cls(**kw) for cls in (ViT_face_low, ViT_face_low, ViT_face_low, ViT_face_up)]
    for m in nets:
        m.load_state_dict(state, strict=False)
        m.to("cuda").set_compute_dtype(dtype)
        for p in m.parameters():
            p.requires_grad_(False)
    s, d, t, u = nets
    for n, p in s.named_parameters():
        p.requires_grad = "fn.fn.net" in n
    s.train(), d.train(), t.eval(), u.eval()
    opt = create_optimizer(SimpleNamespace(opt="adamw", weight_decay=0.05, opt_eps=1e-8, opt_betas=None, lr=1e-4), s)
    x_f, x_r = torch.rand(batch, 3, 112, 112, device="cuda"), torch.rand(batch, 3, 112, 112, device="cuda")
    y_f, y_r = torch.randint(0, 20, (batch,), device="cuda"), torch.randint(20, 100, (batch,), device="cuda")
    crit = torch.nn.CrossEntropyLoss()
    run = lambda: step.lirf_step(s, d, t, u, opt, crit, x_f, y_f, x_r, y_r, split=20, T=10.0, alpha=0.1)
    ms = timed(run, iters, warmup=5)
    pack = run()
    assert torch.isfinite(pack).all(), pack
    return dict(batch=batch, dtype=dtype, ms_per_step=ms, images_per_s=2 * batch / ms * 1e3, meters=pack.tolist())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("tools/bench_lirf.py measures on a ROCm GPU; there is nothing to time without one")
    res = dict(kernels=[kernels(B, 197, 512, dt, a.iters) for B in (16, 128, 512) for dt in (torch.float16, torch.float32)],
               steps=[whole_step(a.batch, dt, max(10, a.iters // 5)) for dt in ("fp16", "fp32")])
    for r in res["kernels"]:
        print("kernels", json.dumps(r))
    for r in res["steps"]:
        print("step", json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
