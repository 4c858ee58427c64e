"""Child process of tests/test_hip_proto_l2.py: ONE RANK of a two-rank data-parallel run of the HIP step with proto_distance="l2", both
ranks on the one GPU under a gloo process group (tests/dp_gloo_gpu_child.py, whose batches and hyper-parameters it takes; BND_pro is
raised to 4 so that the l2 prototype hinge is active). Every step runs twice on twin models — eagerly, and as graph segments with eager
collectives in between — and the two must agree bit for bit.
argv: rank world port dtype out.npz"""
import copy
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [HERE, ROOT, os.path.join(ROOT, "gs-lora_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from oracle import recipe  # noqa: E402
import dp_gloo_gpu_child as K  # noqa: E402
from dp_gloo_gpu_child import STEPS, B, whole_batch  # noqa: E402,F401
from test_hip_graph import build  # noqa: E402


def hyper(cfg):
    return dict(K.hyper(cfg), BND_pro=4.0, proto_distance="l2")


def main():
    rank, world, port, dtype, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
    from gslora_hip import step as S
    from gslora_hip.optim import FusedAdamW
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        cfg = recipe.cfg_small2()
        m1 = build(cfg, dtype, 0.0)
        m2 = copy.deepcopy(m1)
        mk_opt = lambda m: FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-2, weight_decay=0.05, eps=1e-8)
        o1, o2 = mk_opt(m1), mk_opt(m2)
        crit = torch.nn.CrossEntropyLoss()
        kw = hyper(cfg)
        g = S.GraphedStep(m2, o2, crit)
        packs = []
        sl = slice(rank * B, (rank + 1) * B)
        for s in range(STEPS):
            xr, yr, xf, yf = (t[sl].contiguous() for t in whole_batch(cfg, world, s))
            p1 = S.gs_lora_step(m1, o1, crit, xr, yr, xf, yf, **kw)       # eager data-parallel step
            p2 = g(xr, yr, xf, yf, **kw)                                    # graph segments + eager collectives
            torch.cuda.synchronize()
            assert torch.equal(p1, p2), (s, p1.tolist(), p2.tolist())
            packs.append(p1.cpu().numpy())
        assert (g.eager_steps, g.captures, g.replays) == (1, 1, STEPS - 1), (g.eager_steps, g.captures, g.replays)
        res = {"packs": np.stack(packs)}
        for (n, a), (_, c) in zip(m1.named_parameters(), m2.named_parameters()):
            if a.requires_grad:
                assert torch.equal(a, c), n
                res[n] = a.detach().float().cpu().numpy()
        np.savez(out, **res)
    finally:
        dist.destroy_process_group()
    print("DP-L2-OK", flush=True)


if __name__ == "__main__":
    main()
