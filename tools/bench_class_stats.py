#!/usr/bin/env python
"""Cost of the per-class evaluation and of the ordered prototype sums, one process, one build: ViT-P8S8 (112 px, depth 6, dim 512, LoRA r = 8,
CosFace, model in fp16, evaluation in f32 as engine_cl.eval_data defaults to) on 5 batches of 512 images (config-2 evaluation geometry),
with C = 100 and C = 1000 classes.

  eval    engine_cl.eval_data (unchanged by the per-class work: the yardstick) against eval_data_per_class without and with the confusion
          matrix. A sample is one whole call between two host clock reads (every call ends in its host read); the three alternate inside
          every round and the order flips from round to round.
  proto   util.utils.calculate_prototypes against `index_add_prototypes` below, the accumulation it used before (sums.index_add_ /
          counts.index_add_: float atomics), restated here as the yardstick; same alternation. Also the accumulation alone on the 5 x 512
          stored embeddings between two device events, and the run-to-run scatter of the index_add_ prototypes (max |delta| against the
          first of --scatter-runs runs on the same embeddings; the ordered sums are compared the same way and must give 0).
Prints one JSON line.

    python tools/bench_class_stats.py [--rounds 8] [--warmup 2] [--classes 100 1000]
"""
import argparse
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
N_BATCH, BATCH = 5, 512


def build(dev, C):
    import loralib as lora
    from vit_pytorch_face import ViT_face
    torch.manual_seed(1337)
    m = ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=C, dropout=0.1, emb_dropout=0.1, **GEO)
    lora.mark_only_lora_as_trainable(m)
    return m.to(dev).set_compute_dtype("fp16")


def index_add_prototypes(backbone, dataset, batch_size, device, ncls):
    """calculate_prototypes as it accumulated before gsl_class_embed_sum (aug_num = 0 path)."""
    from torch.utils.data import DataLoader
    backbone.eval()
    sums = counts = None
    with torch.no_grad():
        for images, labels in DataLoader(dataset, batch_size=batch_size, shuffle=False):
            images, labels = images.to(device), labels.to(device).long()
            _, emb = backbone(images, labels)
            if sums is None:
                sums, counts = torch.zeros(ncls, emb.shape[1], device=emb.device), torch.zeros(ncls, device=emb.device)
            sums.index_add_(0, labels, emb)
            counts.index_add_(0, labels, torch.ones_like(labels, dtype=torch.float32))
    sums, counts = sums.cpu(), counts.cpu()
    return {int(c): (sums[c] / counts[c]) for c in torch.nonzero(counts).flatten().tolist()}


def alternate(fns, rounds, warmup):
    """{name: callable} -> {name: [seconds per call]}; every callable ends in a host read of its result."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    times, order = {k: [] for k in fns}, list(fns)
    for r in range(rounds):
        for k in (order if r % 2 == 0 else order[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fns[k]()
            times[k].append(time.perf_counter() - t0)
    return times


def stats(v, scale=1e3):
    med = statistics.median(v)
    return dict(median_ms=med * scale, min_ms=min(v) * scale, max_ms=max(v) * scale, spread_pct=100.0 * (max(v) - min(v)) / med)


def leg(C, args, dev):
    import contextlib
    import io
    import engine_cl
    from gslora_hip import ops
    from torch.utils.data import TensorDataset
    from util.utils import calculate_prototypes
    g = torch.Generator().manual_seed(7)
    x = torch.rand(N_BATCH * BATCH, 3, 112, 112, generator=g)
    y = torch.randint(0, C, (N_BATCH * BATCH,), generator=g)
    loader = [(x[i:i + BATCH].to(dev), y[i:i + BATCH].to(dev)) for i in range(0, x.shape[0], BATCH)]      # device-resident: no H2D in the window
    model = build(dev, C)
    quiet = contextlib.redirect_stdout(io.StringIO())
    res, last = {"classes": C, "images": x.shape[0]}, {}

    def run(name, fn):
        def call():
            with quiet:
                last[name] = fn()
        return call
    t = alternate({"eval_data": run("eval_data", lambda: engine_cl.eval_data(model, loader, dev, "bench")),
                   "per_class": run("per_class", lambda: engine_cl.eval_data_per_class(model, loader, dev, "bench")),
                   "per_class_confusion": run("per_class_confusion", lambda: engine_cl.eval_data_per_class(model, loader, dev, "bench", confusion=True))},
                  args.rounds, args.warmup)
    assert last["per_class"]["accuracy"] == last["eval_data"] == last["per_class_confusion"]["accuracy"]
    res["eval"] = {k: stats(v) for k, v in t.items()}
    res["eval"]["images_per_s_eval_data"] = x.shape[0] / statistics.median(t["eval_data"])
    for k in ("per_class", "per_class_confusion"):
        res["eval"][f"{k}_over_eval_data_median"] = statistics.median(t[k]) / statistics.median(t["eval_data"])
    # ---- prototypes, end to end (CPU data set, as the driver passes it)
    ds = TensorDataset(x, y)
    t = alternate({"index_add": run("index_add", lambda: index_add_prototypes(model, ds, BATCH, dev, C)),
                   "ordered": run("ordered", lambda: calculate_prototypes(model, ds, batch_size=BATCH, device=dev))}, max(3, args.rounds // 2), 1)
    res["proto"] = {k: stats(v) for k, v in t.items()}
    res["proto"]["ordered_over_index_add_median"] = statistics.median(t["ordered"]) / statistics.median(t["index_add"])
    res["proto"]["max_abs_diff_ordered_vs_index_add"] = max(float((last["ordered"][c] - last["index_add"][c]).abs().max()) for c in last["ordered"])
    # ---- the accumulation alone, on stored embeddings
    with torch.no_grad(), quiet:
        model.eval()
        embs = [model(xb, yb)[1].float().contiguous() for xb, yb in loader]
    labels = [yb for _, yb in loader]
    D = embs[0].shape[1]

    def acc_index_add():
        sums, counts = torch.zeros(C, D, device=dev), torch.zeros(C, device=dev)
        for e, yb in zip(embs, labels):
            sums.index_add_(0, yb, e)
            counts.index_add_(0, yb, torch.ones_like(yb, dtype=torch.float32))
        return sums / counts[:, None]

    def acc_ordered():
        sums, counts = torch.zeros(C, D, device=dev), torch.zeros(C + 1, dtype=torch.int64, device=dev)
        for e, yb in zip(embs, labels):
            ops.class_embed_sum(e, yb, sums, counts[:C], counts[C:])
        return ops.class_finish(counts[:C], sums=sums)[1]
    acc = {}
    for name, fn in (("index_add", acc_index_add), ("ordered", acc_ordered)):
        for _ in range(3):
            fn()
        v = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            e1.synchronize()
            v.append(e0.elapsed_time(e1) / 20 / 1e3)
        acc[name] = stats(v)
        runs = [fn().cpu() for _ in range(args.scatter_runs)]
        acc[name]["run_to_run_max_abs_diff"] = max(float(torch.nan_to_num(r - runs[0]).abs().max()) for r in runs[1:])
        acc[name]["runs_bit_identical"] = all(r.numpy().tobytes() == runs[0].numpy().tobytes() for r in runs[1:])
    assert acc["ordered"]["runs_bit_identical"]
    res["accumulate_5x512"] = acc
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scatter-runs", type=int, default=6)
    ap.add_argument("--classes", type=int, nargs="*", default=[100, 1000])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    out = {"tool": "bench_class_stats", "device": torch.cuda.get_device_name(0), "rounds": args.rounds}
    for C in args.classes:
        out[f"C{C}"] = leg(C, args, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
