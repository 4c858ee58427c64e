"""Golden fixtures above the single-panel attention limit (T = 257 tokens: 128 px images, patch / stride 8), from the REAL reference
(imported unmodified through oracle.make_golden.install_shims) on the deterministic recipe of oracle/recipe.py. Runs only where the
reference sources are checked out (the build machine); the GPU tests (tests/test_hip_attention_long.py) read the arrays alone.

    python tools/make_golden_longseq.py                              # all five fixtures
    python tools/make_golden_longseq.py longseq_small2_cosface_b3    # one of them

Writes tests/golden/:
  longseq_small2_cosface_b3.npz    cfg_small2 at 128 px, CosFace, pool cls (the last block's cls forward runs above 256 keys)
  longseq_small2_arcface_b3.npz    cfg_small2 at 128 px, ArcFace, pool mean
  longseq_vits_small2_b3.npz       ViTs_face, cfg_small2 at 128 px, 12 x 12 windows at stride 8, pad 4, CosFace
  longseq_attn_small_b3.npz        cfg_small_attn (--lora_pos Attention) at 128 px, CosFace
      keys as small2_b3.npz: fwd_* / eval_* logits and embeddings, losses1, grad1::*, total_inactive, grad_inactive::*
  longseq_small6_engine.npz        cfg_small6 at 128 px, CosFace: three steps of engine_cl.train_one_epoch + torch AdamW
                                   (keys as arcface_small6_engine.npz)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import recipe  # noqa: E402
from oracle.make_golden import HYPER, install_shims  # noqa: E402
import make_golden_heads as H  # noqa: E402
import make_golden_vits as V  # noqa: E402

PX = 128      # (128 / 8)^2 + 1 = 257 tokens


def long_cfg(cfg, **kw):
    return dict(cfg, image_size=PX, **kw)


def build_vit_face(cfg, head, pool, state):
    import loralib as lora
    from vit_pytorch_face import ViT_face
    m = ViT_face(loss_type=head, GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
                 dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], pool=pool, dropout=0.0, emb_dropout=0.0,
                 lora_rank=cfg["lora_rank"], lora_pos=cfg.get("lora_pos", "FFN"))
    m.load_state_dict({k: torch.tensor(v) for k, v in state.items()}, strict=True)
    lora.mark_only_lora_as_trainable(m)
    return m


def model_case(tag, cfg, head, pool, batch, out):
    """The keys of make_golden_heads.model_case, with the pooling mode passed to the reference."""
    state = recipe.make_state(cfg)
    model = build_vit_face(cfg, head, pool, state)
    res = {}
    xr, yr, xf, yf = H.batches(cfg, batch)
    proto = {c: torch.tensor(v) for c, v in enumerate(recipe.make_prototypes(cfg))}
    model.train()
    with torch.no_grad():
        lo, em = model(xr, yr)
        res["fwd_logits"], res["fwd_emb"] = lo.numpy(), em.numpy()
    model.eval()
    with torch.no_grad():
        lo, em = model(xr, yr)
        res["eval_logits"], res["eval_emb"] = lo.numpy(), em.numpy()
    model.train()
    model.load_state_dict({k: torch.tensor(v) for k, v in state.items()})      # undo the merge / un-merge drift
    total, parts = H.total_loss(model, cfg, xr, yr, xf, yf, HYPER, proto)
    model.zero_grad()
    total.backward()
    res["losses1"] = np.array(parts, dtype=np.float64)
    res.update({f"grad1::{n}": g for n, g in H.grads(model).items()})
    total, _ = H.total_loss(model, cfg, xr, yr, xf, yf, dict(HYPER, BND=5.0, BND_pro=0.1), proto)      # both hinges inactive
    model.zero_grad()
    total.backward()
    res["total_inactive"] = np.float64(total.item())
    res.update({f"grad_inactive::{n}": g for n, g in H.grads(model).items()})
    H.save(out, tag, res)


CASES = {
    "longseq_small2_cosface_b3": lambda out: model_case("longseq_small2_cosface_b3", long_cfg(recipe.cfg_small2()), "CosFace", "cls", 3, out),
    "longseq_small2_arcface_b3": lambda out: model_case("longseq_small2_arcface_b3", long_cfg(recipe.cfg_small2()), "ArcFace", "mean", 3, out),
    "longseq_vits_small2_b3": lambda out: V.model_case("longseq_vits_small2_b3", long_cfg(recipe.cfg_small2()), "CosFace", 12, 4, "cls", 3, out),
    "longseq_attn_small_b3": lambda out: model_case("longseq_attn_small_b3", long_cfg(recipe.cfg_small_attn()), "CosFace", "cls", 3, out),
    "longseq_small6_engine": lambda out: H.engine_case("longseq_small6_engine", long_cfg(recipe.cfg_small6()), "CosFace", 2, out),
}


def main():
    install_shims()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    out = os.path.join(ROOT, "tests", "golden")
    only = sys.argv[1:]
    for tag, run in CASES.items():
        if not only or tag in only:
            run(out)


if __name__ == "__main__":
    main()
