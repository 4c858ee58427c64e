#!/usr/bin/env python
"""Cost of face verification at LFW size: 6 000 pairs at the config-2 geometry (ViT-P8S8 depth 6, 112 px, dim 512).

  * the embedding pass of perform_val (util.utils.pair_embeddings: 12 000 images + their flipped copies, device-resident float32, batches of
    --batch, original and flipped batch as two parts of one forward), images/s per evaluation dtype — the same forward as bench.py's `eval` leg;
  * the metric behind it: gsl_verif_pair_dist + gsl_verif_fold_counts + gsl_verif_select (HIP events around the three calls, median of --rounds),
    next to a numpy formulation of the same metric on the host (normalise, distances, 10 folds x 400 thresholds of np.less / logical_and / sum,
    as verification.calculate_roc loops) on the threads the process was given.

    python tools/bench_verification.py [--pairs 6000] [--batch 512] [--rounds 5]      -> one JSON line (profiles/verification.md)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gs-lora_amd"))


def numpy_metric(e0, e1, issame, folds, thresholds):
    s = e0.astype(np.float64) + e1.astype(np.float64)
    nrm = np.linalg.norm(s, axis=1, keepdims=True)
    nrm[nrm == 0] = 1.0
    n = s / nrm
    dist = np.sum(np.square(n[0::2] - n[1::2]), 1)
    P = len(dist)
    base, rem = divmod(P, folds)
    acc, start = np.zeros(folds), 0
    for f in range(folds):
        stop = start + base + (1 if f < rem else 0)
        test = np.zeros(P, bool)
        test[start:stop] = True
        tr_acc = np.zeros(len(thresholds))
        for i, t in enumerate(thresholds):
            pred = np.less(dist[~test], t)
            tr_acc[i] = (np.sum(np.logical_and(pred, issame[~test])) + np.sum(np.logical_and(~pred, ~issame[~test]))) / (P - (stop - start))
        for i, t in enumerate(thresholds):      # the per-threshold tpr / fpr of the test fold
            pred = np.less(dist[test], t)
            np.sum(np.logical_and(pred, issame[test])), np.sum(np.logical_and(pred, ~issame[test]))
        pred = np.less(dist[test], thresholds[int(np.argmax(tr_acc))])
        acc[f] = (np.sum(np.logical_and(pred, issame[test])) + np.sum(np.logical_and(~pred, ~issame[test]))) / (stop - start)
        start = stop
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=6000)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import loralib as lora
    from gslora_hip import ops
    from util import verification as V
    from util.utils import pair_embeddings
    from vit_pytorch_face import ViT_face
    torch.manual_seed(0)
    model = ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=100, image_size=112, patch_size=8, dim=512, depth=6, heads=8, mlp_dim=2048,
                     lora_rank=8)
    lora.mark_only_lora_as_trainable(model)
    model = model.to("cuda").eval()
    n = 2 * args.pairs
    x = torch.rand(n, 3, 112, 112, device="cuda")
    data_set = [x, x.flip(3)]
    issame = np.arange(args.pairs) % 2 == 0
    out = {"pairs": args.pairs, "batch": args.batch, "threads": torch.get_num_threads()}
    for dt in ("fp32", "fp16", "bf16"):
        model.set_compute_dtype(dt)
        pair_embeddings("cuda", 512, args.batch, model, [x[:args.batch], x[:args.batch]])      # warm-up
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0, e1 = pair_embeddings("cuda", 512, args.batch, model, data_set)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        out[f"embed_images_per_s_{dt}"] = round(2 * n / float(np.median(ts)), 1)
    th = torch.from_numpy(V.THRESHOLDS).cuda()
    same = torch.from_numpy(issame.astype(np.uint8)).cuda()
    ms = []
    for _ in range(args.rounds + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dist, xnorm, _ = ops.verif_pair_dist(e0, e1)
        counts, tot = ops.verif_fold_counts(dist, same, th, 10)
        res = ops.verif_select(counts, tot, th, xnorm)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    out["metric_three_calls_ms"] = round(float(np.median(ms[1:])), 4)
    t0 = time.perf_counter()
    tpr, fpr, acc, best, xn = V.roc_from_dist(V.THRESHOLDS, dist, issame, 10, xnorm)
    out["metric_with_host_read_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    h0, h1 = e0.cpu().numpy(), e1.cpu().numpy()
    t0 = time.perf_counter()
    ref_acc = numpy_metric(h0, h1, issame, 10, V.THRESHOLDS)
    out["numpy_metric_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    out["accuracy_hip_vs_numpy_max_abs"] = float(np.abs(acc - ref_acc).max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
