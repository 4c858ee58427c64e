"""Golden fixtures above LoRA rank 16, from the REAL reference (imported unmodified through oracle.make_golden.install_shims) on the
deterministic recipe of oracle/recipe.py. Runs only where the reference sources are checked out (the build machine); the GPU tests
(tests/test_hip_lora_rank_models.py) read the arrays alone.

    python tools/make_golden_lora_rank.py                      # all five fixtures
    python tools/make_golden_lora_rank.py rank32_small2_b3     # one of them

Writes tests/golden/:
  rank32_small2_b3.npz          cfg_small2(lora_rank=32), CosFace, FFN site
  rank64_small2_b3.npz          cfg_small2(lora_rank=64)
  rank20_attn_small_b3.npz      cfg_small_attn(lora_rank=20): 3 r = 60 of the 64 columns of the QKV LoRA K segment
      keys as small2_b3.npz: fwd_* / eval_* logits and embeddings, losses1, grad1::*, total_inactive, grad_inactive::*
  rank48_vitb_small2_b3.npz     cfg_vitb_small2(lora_rank=48), the ViT-B/16 adapter (keys as vitb_small2_b3.npz, oracle/make_golden_vitb.py)
  rank32_small6_engine.npz      cfg_small6(lora_rank=32): three steps of engine_cl.train_one_epoch + torch AdamW
                                (keys as arcface_small6_engine.npz)

The LoRA tensors grow with the rank and a committed fixture stays below 1 MB, so a fixture that would not fit drops whole families of
keys, in this order, until it does: grad_inactive::* (the second backward, with both hinges inactive; total_inactive stays), then
param1::* and param3::* of the engine fixture (the trajectory is then held by the meters of all three steps and the first-step
gradients; the test follows the optimizer with the oracle's AdamW on the same gradients). At these shapes: rank64_small2_b3 drops
grad_inactive::*, rank32_small6_engine drops param1::* and param3::*.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import recipe  # noqa: E402
from oracle import make_golden_vitb as VB  # noqa: E402
from oracle.make_golden import install_shims  # noqa: E402
import make_golden_heads as H  # noqa: E402

LIMIT = 1_000_000
DROP_ORDER = ("grad_inactive::", "param1::", "param3::")


def save_fitting(out, tag, res):
    """H.save, dropping key families in DROP_ORDER until the compressed file is below LIMIT bytes."""
    path = os.path.join(out, f"{tag}.npz")
    dropped = []
    for prefix in (None,) + DROP_ORDER:
        if prefix is not None:
            if not any(k.startswith(prefix) for k in res):
                continue
            res = {k: v for k, v in res.items() if not k.startswith(prefix)}
            dropped.append(prefix + "*")
        np.savez_compressed(path, **res)
        if os.path.getsize(path) < LIMIT:
            break
    else:
        raise SystemExit(f"{tag}: {os.path.getsize(path)} bytes with {dropped} dropped")
    print(f"[golden] {tag}: {len(res)} arrays, {os.path.getsize(path) / 1e6:.2f} MB, dropped {dropped or 'nothing'}")


def vitb_case(tag, cfg, batch, out):
    VB.run_case(tag, cfg, batch, out)
    size = os.path.getsize(os.path.join(out, f"{tag}.npz"))
    if size >= LIMIT:
        raise SystemExit(f"{tag}: {size} bytes")


CASES = {
    "rank32_small2_b3": lambda out: H.model_case("rank32_small2_b3", recipe.cfg_small2(lora_rank=32), "CosFace", 3, out),
    "rank64_small2_b3": lambda out: H.model_case("rank64_small2_b3", recipe.cfg_small2(lora_rank=64), "CosFace", 3, out),
    "rank20_attn_small_b3": lambda out: H.model_case("rank20_attn_small_b3", recipe.cfg_small_attn(lora_rank=20), "CosFace", 3, out),
    "rank48_vitb_small2_b3": lambda out: vitb_case("rank48_vitb_small2_b3", recipe.cfg_vitb_small2(lora_rank=48), 3, out),
    "rank32_small6_engine": lambda out: H.engine_case("rank32_small6_engine", recipe.cfg_small6(lora_rank=32), "CosFace", 2, out),
}


def main():
    install_shims()
    H.save = save_fitting
    torch.manual_seed(0)
    torch.set_num_threads(8)
    out = os.path.join(ROOT, "tests", "golden")
    only = sys.argv[1:]
    for tag, run in CASES.items():
        if not only or tag in only:
            run(out)


if __name__ == "__main__":
    main()
