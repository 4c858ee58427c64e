#!/usr/bin/env python
"""uint8 image input against float32 input at bench config 2 geometry (112 px, 512 remain + 512 forget images, fp16, dropout 0.1).

 1. The patch gathers alone, one 512-image batch, fp16 operand: float source (gsl_patchify / gsl_unfold_patches) against uint8 NCHW and
    uint8 NHWC (gsl_patchify_u8 / gsl_unfold_patches_u8). Each sample is a window of --launches back-to-back launches between two device
    events; the versions are alternated inside every round and the order is rotated. Reported per launch: median / min / max over the
    rounds, and the fraction of the kernel's own HBM floor (bytes it must read + write / achievable bandwidth).
 2. The forgetting step (gslora_hip.step.gs_lora_step, eager) fed from HOST memory: pinned host batches cycled through two
    util.data_prefetcher rings (pinned staging + H2D on a copy stream), float32 x against uint8 bytes, wall-clock ms per step with one
    sync at the end of a run, next to the device-resident step of the same process. Runs are alternated.
Prints one JSON line.

    python tools/bench_u8_input.py [--rounds 30] [--launches 50] [--steps 12] [--warmup 3] [--runs 3]
"""
import argparse
import itertools
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gs-lora_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

GEO = dict(image_size=112, patch_size=8, dim=512, depth=6, heads=8, mlp_dim=2048, lora_rank=8)
HYPER = dict(beta=0.15, alpha=1e-4, BND=105.0, BND_pro=18.0, w_f=0.01, w_r=0.01)
HBM = 6.3e12      # achievable HBM bandwidth (MI355X guide), as tools/bench_vits.py


def stats(v):
    return dict(median_us=statistics.median(v), min_us=min(v), max_us=max(v), spread_pct=100.0 * (max(v) - min(v)) / statistics.median(v))


def gathers(args, dev):
    from gslora_hip import _lib as L
    from gslora_hip import ops
    lib = L.load()
    B, S, T = args.batch, 112, 197
    g = torch.Generator().manual_seed(1337)
    u = torch.randint(0, 256, (B, 3, S, S), generator=g, dtype=torch.uint8)
    x = ops.u8_reference(u, *ops.INPUT_NORM_IMAGENET).to(dev)
    u_nchw = u.to(dev)
    u_nhwc = u.permute(0, 2, 3, 1).contiguous().to(dev)
    tab = ops.u8_norm_table(*ops.INPUT_NORM_IMAGENET).to(dev)
    out_p = torch.empty(B * T, 192, device=dev, dtype=torch.float16)
    out_u = torch.empty(B * T, 448, device=dev, dtype=torch.float16)
    st = ops._stream()
    forms = {
        "patchify_f32": lambda: lib.gsl_patchify(x.data_ptr(), out_p.data_ptr(), B, 3, S, S, 8, L.F16, st),
        "patchify_u8_nchw": lambda: lib.gsl_patchify_u8(u_nchw.data_ptr(), L.U8_NCHW, tab.data_ptr(), out_p.data_ptr(), B, 3, S, S, 8, L.F16, st),
        "patchify_u8_nhwc": lambda: lib.gsl_patchify_u8(u_nhwc.data_ptr(), L.U8_NHWC, tab.data_ptr(), out_p.data_ptr(), B, 3, S, S, 8, L.F16, st),
        "unfold_f32": lambda: lib.gsl_unfold_patches(x.data_ptr(), out_u.data_ptr(), B, 3, S, S, 12, 8, 4, 448, L.F16, st),
        "unfold_u8_nchw": lambda: lib.gsl_unfold_patches_u8(u_nchw.data_ptr(), L.U8_NCHW, tab.data_ptr(), out_u.data_ptr(), B, 3, S, S, 12, 8, 4,
                                                            448, L.F16, st),
        "unfold_u8_nhwc": lambda: lib.gsl_unfold_patches_u8(u_nhwc.data_ptr(), L.U8_NHWC, tab.data_ptr(), out_u.data_ptr(), B, 3, S, S, 12, 8, 4,
                                                            448, L.F16, st),
    }
    # the uint8 forms write what the float form writes
    ref = {}
    for name, fn in forms.items():
        assert fn() == 0, name
        o = (out_p if name.startswith("patchify") else out_u).clone()
        k = name.split("_")[0]
        assert torch.equal(ref.setdefault(k, o).view(torch.int16), o.view(torch.int16)), name
    for fn in forms.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in forms}
    names = list(forms)
    for r in range(args.rounds):
        for n in names[r % len(names):] + names[:r % len(names)]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                forms[n]()
            e1.record()
            e1.synchronize()
            times[n].append(e0.elapsed_time(e1) * 1e3 / args.launches)
    img = B * 3 * S * S
    floor = {n: ((4 if n.endswith("f32") else 1) * img + B * T * (192 if n.startswith("patchify") else 448) * 2) for n in forms}
    res = {}
    for n in forms:
        res[n] = stats(times[n])
        res[n].update(floor_bytes=floor[n], floor_us=floor[n] / HBM * 1e6, fraction_of_floor=(floor[n] / HBM * 1e6) / res[n]["median_us"])
    return res


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
    return m.to(dev).set_compute_dtype("fp16").train().set_input_norm("totensor")      # (float batches are untouched by the opt-in)


def host_fed_step(args, dev):
    from gslora_hip import ops
    from gslora_hip.optim import FusedAdamW
    from gslora_hip.step import gs_lora_step
    from util.data_prefetcher import data_prefetcher
    B, NB = args.batch, 3
    g = torch.Generator().manual_seed(7)
    mk_u = lambda: torch.randint(0, 256, (B, 3, 112, 112), generator=g, dtype=torch.uint8)
    u_r, u_f = [mk_u() for _ in range(NB)], [mk_u() for _ in range(NB)]
    y_r = [torch.randint(0, 80, (B,), generator=g).pin_memory() for _ in range(NB)]
    y_f = [torch.randint(80, 100, (B,), generator=g).pin_memory() for _ in range(NB)]
    host = {
        "u8": ([t.pin_memory() for t in u_r], [t.pin_memory() for t in u_f]),
        "f32": ([ops.u8_reference(t, *ops.INPUT_NORM_TOTENSOR).pin_memory() for t in u_r],
                [ops.u8_reference(t, *ops.INPUT_NORM_TOTENSOR).pin_memory() for t in u_f]),
    }
    m = build(dev)
    opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-2, weight_decay=0.05, eps=1e-8)
    crit = torch.nn.CrossEntropyLoss()
    proto = torch.randn(100, GEO["dim"], generator=g).to(dev)
    kw = dict(beta=HYPER["beta"], alpha=HYPER["alpha"], BND=HYPER["BND"], use_structure=True, group_type="block", use_prototype=True,
              proto_table=proto, w_f=HYPER["w_f"], w_r=HYPER["w_r"], BND_pro=HYPER["BND_pro"])
    resident = {k: (v[0][0].to(dev), v[1][0].to(dev)) for k, v in host.items()}
    yr_d, yf_d = y_r[0].to(dev), y_f[0].to(dev)

    def run(mode, n):
        """n steps; returns wall-clock ms per step (one sync at the end)."""
        kind, fed = mode.split("_")
        if fed == "host":
            cyc = lambda xs, ys: itertools.cycle(list(zip(xs, ys)))
            it_r = data_prefetcher(cyc(host[kind][0], y_r), dev, prefetch=True)
            it_f = data_prefetcher(cyc(host[kind][1], y_f), dev, prefetch=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            if fed == "host":
                (xr, yr), (xf, yf) = it_r.next(), it_f.next()
            else:
                (xr, xf), yr, yf = resident[kind], yr_d, yf_d
            meters = gs_lora_step(m, opt, crit, xr, yr, xf, yf, **kw)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3 / n
        assert torch.isfinite(meters).all(), (mode, meters.tolist())
        return dt

    modes = ["f32_device", "u8_device", "f32_host", "u8_host"]
    for mode in modes:
        run(mode, args.warmup)
    times = {mode: [] for mode in modes}
    for r in range(args.runs):
        for mode in modes[r % len(modes):] + modes[:r % len(modes)]:
            times[mode].append(run(mode, args.steps))
    res = {mode: dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t), runs_ms=[round(v, 3) for v in t]) for mode, t in times.items()}
    px = 2 * B * 3 * 112 * 112
    res["h2d_bytes_per_step"] = {"f32": 4 * px + 2 * B * 8, "u8": px + 2 * B * 8}
    res["host_minus_device_ms"] = {k: res[k + "_host"]["median_ms"] - res[k + "_device"]["median_ms"] for k in ("f32", "u8")}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batch", type=int, default=512)
    args = ap.parse_args()
    dev = torch.device("cuda")
    res = dict(what="uint8 vs float32 image input, bench config 2 geometry (512-image batches, 112 px, fp16)",
               gathers=gathers(args, dev), step=host_fed_step(args, dev))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
