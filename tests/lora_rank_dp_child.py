"""Child process of tests/test_hip_lora_rank_models.py: ONE RANK of a two-rank data-parallel run of the HIP step at LoRA rank 32 (the
set-up of tests/dp_gloo_gpu_child.py: both ranks on the one GPU, gloo process group). Three eager steps on this rank's share of the batch;
writes the steps' meters, the first step's gradients and the LoRA parameters.
argv: rank world port dtype out.npz"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [HERE, ROOT, os.path.join(ROOT, "gs-lora_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from oracle import recipe  # noqa: E402
from dp_gloo_gpu_child import B, hyper, whole_batch  # noqa: E402
from test_hip_graph import build  # noqa: E402

STEPS, RANK = 3, 32


def config():
    return recipe.cfg_small2(lora_rank=RANK)


def main():
    rank, world, port, dtype, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
    from gslora_hip import step as S
    from gslora_hip.optim import FusedAdamW
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        cfg = config()
        m = build(cfg, dtype, 0.0)
        opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-2, weight_decay=0.05, eps=1e-8)
        crit = torch.nn.CrossEntropyLoss()
        kw = hyper(cfg)
        sl = slice(rank * B, (rank + 1) * B)
        packs, res = [], {}
        for s in range(STEPS):
            packs.append(S.gs_lora_step(m, opt, crit, *(t[sl].contiguous() for t in whole_batch(cfg, world, s)), **kw).cpu().numpy())
            if s == 0:      # the all-reduced gradients of the first step (the parameters are still the recipe's on every side)
                res.update({"grad1::" + n: a.grad.detach().float().cpu().numpy() for n, a in m.named_parameters() if a.requires_grad})
        torch.cuda.synchronize()
        res["packs"] = np.stack(packs)
        for n, a in m.named_parameters():
            if a.requires_grad:
                res[n] = a.detach().float().cpu().numpy()
        np.savez(out, **res)
    finally:
        dist.destroy_process_group()
    print("LORA-RANK-DP-OK", flush=True)


if __name__ == "__main__":
    main()
