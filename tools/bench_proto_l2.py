#!/usr/bin/env python
"""Cost of a forgetting step with the l2 prototype distance against the same step with the KL distance, one process, one build:
ViT-P8S8 (112 px, depth 6, dim 512, LoRA r = 8, CosFace-100, fp16, dropout 0.1) at

  config 5: few-shot 4 + 4 images, HIP-graph replay (the one-launch loss tail: gsl_loss_tail against gsl_loss_tail_l2)
  config 2: 512 + 512 images, eager (the separate kernels: gsl_proto_kl_* against gsl_proto_l2_*)

Each distance has its own model, optimizer and stepper. A sample is a window of --steps steps between two device events; the two
distances alternate inside every round and the order flips from round to round. Reported per step: median / min / max over the rounds.
Prints one JSON line.

    python tools/bench_proto_l2.py [--rounds 12] [--steps 10] [--warmup 4] [--configs 5 2]
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

GEO = dict(image_size=112, patch_size=8, dim=512, depth=6, heads=8, mlp_dim=2048, lora_rank=8)
# BND_pro above both distances on this data, so that both hinges carry a gradient in both legs
HYPER = dict(beta=0.15, alpha=1e-4, BND=105.0, BND_pro=18.0, w_f=0.01, w_r=0.01, use_structure=True, group_type="block", use_prototype=True)
CONFIGS = {5: dict(batch=4, graph=True), 2: dict(batch=512, graph=False)}


def build(dev):
    import loralib as lora
    from vit_pytorch_face import ViT_face
    torch.manual_seed(1337)
    m = ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=100, dropout=0.1, emb_dropout=0.1, **GEO)
    lora.mark_only_lora_as_trainable(m)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "lora_B" in n:
                p.normal_(0.0, 0.02)
    return m.to(dev).set_compute_dtype("fp16").train()


def leg(cfg_id, args, dev):
    from gslora_hip.optim import FusedAdamW
    from gslora_hip.step import GraphedStep, gs_lora_step
    C = CONFIGS[cfg_id]
    B = C["batch"]
    g = torch.Generator().manual_seed(7)
    x_r, x_f = torch.rand(B, 3, 112, 112, generator=g).to(dev), torch.rand(B, 3, 112, 112, generator=g).to(dev)
    y_r, y_f = torch.randint(0, 80, (B,), generator=g).to(dev), torch.randint(80, 100, (B,), generator=g).to(dev)
    table = torch.randn(100, GEO["dim"], generator=g).to(dev)
    crit = torch.nn.CrossEntropyLoss()
    steppers, last = {}, {}
    for dist in ("kl", "l2"):
        m = build(dev)
        opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, weight_decay=0.05, eps=1e-8)
        kw = dict(HYPER, proto_table=table, proto_distance=dist)
        if C["graph"]:
            gs = GraphedStep(m, opt, crit)
            steppers[dist] = (lambda gs=gs, kw=kw: gs(x_r, y_r, x_f, y_f, **kw), gs)
        else:
            steppers[dist] = (lambda m=m, opt=opt, kw=kw: gs_lora_step(m, opt, crit, x_r, y_r, x_f, y_f, **kw), None)
    for dist, (fn, _) in steppers.items():
        for _ in range(args.warmup):
            last[dist] = fn()
    torch.cuda.synchronize()
    times = {d: [] for d in steppers}
    order = list(steppers)
    for r in range(args.rounds):
        for dist in (order if r % 2 == 0 else order[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                last[dist] = steppers[dist][0]()
            e1.record()
            e1.synchronize()
            times[dist].append(e0.elapsed_time(e1) / args.steps)
    res = {"batch": f"{B}+{B}", "graph": C["graph"]}
    for dist, v in times.items():
        gs = steppers[dist][1]
        res[dist] = dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v),
                         spread_pct=100.0 * (max(v) - min(v)) / statistics.median(v), meters=[round(t, 5) for t in last[dist].tolist()],
                         replays=None if gs is None else gs.replays)
        assert all(t == t for t in res[dist]["meters"]), (dist, res[dist]["meters"])
    res["l2_over_kl_median"] = res["l2"]["median_ms"] / res["kl"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--configs", type=int, nargs="*", default=[5, 2], choices=sorted(CONFIGS))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    out = {"tool": "bench_proto_l2", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "steps_per_sample": args.steps}
    for c in args.configs:
        out[f"config{c}"] = leg(c, args, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
