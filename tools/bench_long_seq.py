#!/usr/bin/env python
"""What a longer sequence costs: (1) the fp16 forgetting step of ViT_face at 128 px (T = 257) against 112 px (T = 197), config 2 geometry
(dim 512, depth 6, r 8, 512 + 512 images); (2) ViT-B/16 at 384 px (T = 577) against 224 px (T = 197), 48 + 48 images; (3) the attention
forward and backward alone at T in {197, 224, 257, 577, 785} with the same B * H (1024 images x 8 heads), fp16. Steps are alternated in one
process and timed with device events; the attention rows carry the FLOPs / bytes counted from the shapes. Prints one JSON line.

    python tools/bench_long_seq.py [--steps 6] [--warmup 2] [--reps 20] [--attn-only]
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

HYPER = dict(beta=0.15, alpha=1e-4, BND=105.0, BND_pro=18.0, w_f=0.01, w_r=0.01)
PEAK_16 = 2.5e15      # dense 16-bit MFMA (MI355X_MICROARCH.md)
HBM = 6.3e12          # achievable HBM bandwidth


def timed(fn, reps):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return dict(median_us=statistics.median(out), min_us=min(out), max_us=max(out))


def vit_face(image_size, dev):
    from vit_pytorch_face import ViT_face
    torch.manual_seed(1337)
    m = ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=100, image_size=image_size, patch_size=8, dim=512, depth=6, heads=8, mlp_dim=2048,
                 dropout=0.1, emb_dropout=0.1, lora_rank=8)
    return _finish(m, dev)


def vit_b16(image_size, dev):
    from util.utils import replace_ffn_with_lora
    from vit_pytorch_face import ModifiedViT
    from vit_pytorch_face.modified_VIT import vit_b_16
    torch.manual_seed(1337)
    m = replace_ffn_with_lora(ModifiedViT(vit_b_16(image_size=image_size, num_classes=100)), rank=16)
    with torch.no_grad():
        m.heads.head.weight.normal_(0, 0.02)
    return _finish(m, dev)


def _finish(m, dev):
    import loralib as lora
    lora.mark_only_lora_as_trainable(m)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "lora_B" in n:
                p.normal_(0.0, 0.02)
    return m.to(dev).set_compute_dtype("fp16").train()


def step_pair(builders, B, steps, warmup, dim):
    """builders: {tag: (fn, image_size)}; the steps of the two models alternated, the order flipped every step."""
    from gslora_hip.optim import FusedAdamW
    from gslora_hip.step import gs_lora_step
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(1337)
    runs = {}
    for tag, (fn, px) in builders.items():
        m = fn(px, dev)
        opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-2, weight_decay=0.05, eps=1e-8)
        mk = lambda: (torch.randint(0, 256, (B, 3, px, px), generator=g, dtype=torch.uint8).float() / 255.0).to(dev)
        x = (mk(), torch.randint(0, 80, (B,), generator=g).to(dev), mk(), torch.randint(80, 100, (B,), generator=g).to(dev))
        runs[tag] = (m, opt, x, [])
    proto = torch.randn(100, dim, generator=g).to(dev)
    kw = dict(beta=HYPER["beta"], alpha=HYPER["alpha"], BND=HYPER["BND"], use_structure=True, group_type="block", use_prototype=True,
              proto_table=proto, w_f=HYPER["w_f"], w_r=HYPER["w_r"], BND_pro=HYPER["BND_pro"])
    crit = torch.nn.CrossEntropyLoss()
    step = lambda t: gs_lora_step(runs[t][0], runs[t][1], crit, *runs[t][2], **kw)
    tags = list(runs)
    for _ in range(warmup):
        for t in tags:
            step(t)
    torch.cuda.synchronize()
    for i in range(steps):
        for t in (tags if i % 2 == 0 else tags[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            meters = step(t)
            e1.record()
            e1.synchronize()
            runs[t][3].append(e0.elapsed_time(e1))
            assert torch.isfinite(meters).all(), (t, meters.tolist())
    out = {t: dict(median_ms=statistics.median(r[3]), min_ms=min(r[3]), max_ms=max(r[3])) for t, r in runs.items()}
    del runs
    torch.cuda.empty_cache()
    return out


def attention(reps, items=1024 * 8, H=8):
    from gslora_hip import ops
    B = items // H
    scale = 64 ** -0.5
    res = {}
    for T in (197, 224, 257, 577, 785):
        g = torch.Generator(device="cuda").manual_seed(T)
        qkv = (torch.randn(B * T, 3 * H * 64, device="cuda", generator=g) * 1.5).half()
        d_o = torch.randn(B * T, H * 64, device="cuda", generator=g).half()
        o, lse = ops.attention_fwd(qkv, B, T, H, scale)
        for _ in range(3):
            ops.attention_fwd(qkv, B, T, H, scale)
            ops.attention_bwd(qkv, o, d_o, lse, B, T, H, scale)
        f = timed(lambda: ops.attention_fwd(qkv, B, T, H, scale), reps)
        b = timed(lambda: ops.attention_bwd(qkv, o, d_o, lse, B, T, H, scale), reps)
        # algorithmic work per (image, head): forward QK^T + PV = 4 T^2 64 FLOPs; backward dV, dP, dQ, dK = 8 T^2 64 (+ the S recompute:
        # the split form executes 14 T^2 64). Bytes: forward reads qkv, writes o + lse; backward reads qkv, o, dO, lse, writes dqkv (+ delta)
        ff, fb = 4.0 * T * T * 64 * items, 8.0 * T * T * 64 * items
        bf = items * T * (3 * 64 * 2 + 64 * 2 + 4)
        bb = items * T * (3 * 64 * 2 + 2 * 64 * 2 + 4 + 3 * 64 * 2 + 4)
        row = {}
        for name, t, fl, by in (("fwd", f, ff, bf), ("bwd", b, fb, bb)):
            us = t["median_us"]
            floor = max(fl / PEAK_16, by / HBM) * 1e6
            row[name] = dict(t, tflops=fl / us / 1e6, tbps=by / us / 1e6, flops=fl, bytes=by,
                             bound="mfma" if fl / PEAK_16 > by / HBM else "hbm", fraction_of_floor=floor / us,
                             mfma_peak_share=fl / PEAK_16 * 1e6 / us)
        row["pair_us"] = f["median_us"] + b["median_us"]
        res[f"T{T}"] = row
        del qkv, d_o, o, lse
    torch.cuda.empty_cache()
    res["pair_257_over_197"] = res["T257"]["pair_us"] / res["T197"]["pair_us"]
    res["pair_target_257_over_197"] = 2.0 * (257 / 197) ** 2
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--attn-only", action="store_true", help="only the attention rows (the profile run)")
    args = ap.parse_args()
    res = dict(what="long-sequence cost, fp16; steps alternated and timed with device events; attention alone at B*H = 8192")
    res["attention"] = attention(args.reps)
    if not args.attn_only:
        v = step_pair({"vit_112px_T197": (vit_face, 112), "vit_128px_T257": (vit_face, 128)}, 512, args.steps, args.warmup, 512)
        v["ratio"] = v["vit_128px_T257"]["median_ms"] / v["vit_112px_T197"]["median_ms"]
        res["vit_face_config2"] = v
        w = step_pair({"vitb16_224px_T197": (vit_b16, 224), "vitb16_384px_T577": (vit_b16, 384)}, 48, args.steps, args.warmup, 768)
        w["ratio"] = w["vitb16_384px_T577"]["median_ms"] / w["vitb16_224px_T197"]["median_ms"]
        res["vit_b16_48"] = w
    print(json.dumps(res))


if __name__ == "__main__":
    main()
