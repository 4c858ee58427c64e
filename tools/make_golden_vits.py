"""Golden fixtures of ViTs_face (overlapping nn.Unfold patch stage), from the REAL reference vit_pytorch_face/vits_face.py (imported
unmodified) on the deterministic recipe of oracle/recipe.py. Runs only where the reference sources are checked out (the build machine);
the GPU tests read the arrays alone.

    python tools/make_golden_vits.py                    # all four fixtures
    python tools/make_golden_vits.py vits_small2_b3     # one of them

The state is recipe.make_state(cfg) (ViTs_face has ViT_face's parameter names) with patch_to_embedding.weight replaced by a recipe draw of
shape [dim, C*k*k], U(+-1/sqrt(C*k*k)) like the other dense weights (vits_state() below; the tests rebuild it the same way).
Writes tests/golden/:
  vits_small2_b3.npz          cfg_small2, k 12, stride 8, pad 4, CosFace
  vits_k10p1_small2_b3.npz    cfg_small2, k 10, stride 8, pad 1 (the right / bottom taps of the last windows fall in the padding),
                              ArcFace, pool mean
      keys as small2_b3.npz: fwd_* / eval_* logits and embeddings, losses1, grad1::*, total_inactive, grad_inactive::*, param_names
  vits_small6_engine.npz      cfg_small6, k 12 / pad 4, CosFace: three steps of the reference's engine_cl.train_one_epoch + torch AdamW
                              (keys as arcface_small6_engine.npz)
  vits_full_b2.npz            the reference driver's ViTs geometry (112 px, k 12, stride 8, pad 4, dim 512, depth 6, r 8, 100 classes), B 2:
                              fwd_* / eval_* logits and embeddings and grad1::* of the 24 LoRA tensors (no weights)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from oracle import recipe  # noqa: E402
from oracle.make_golden import HYPER, ListLoader, install_shims  # noqa: E402
import make_golden_heads as H  # noqa: E402


def vits_state(cfg, k, seed=1337):
    """recipe.make_state(cfg) with the [dim, C*k*k] patch weight of the unfold stage."""
    st = recipe.make_state(cfg, seed=seed)
    fan_in = cfg["channels"] * k * k
    bound = 1.0 / float(np.sqrt(fan_in))
    st["patch_to_embedding.weight"] = np.ascontiguousarray(
        recipe.uniform("patch_to_embedding.weight", (cfg["dim"], fan_in), seed, -bound, bound), dtype=np.float32)
    return st


def build_reference(cfg, head, k, pad, pool, state):
    import loralib as lora
    from vit_pytorch_face.vits_face import ViTs_face
    m = ViTs_face(loss_type=head, GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
                  ac_patch_size=k, pad=pad, dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], pool=pool,
                  dropout=0.0, emb_dropout=0.0, lora_rank=cfg["lora_rank"])
    keys = set(m.state_dict())
    m.load_state_dict({n: torch.tensor(v) for n, v in state.items() if n in keys}, strict=True)
    lora.mark_only_lora_as_trainable(m)
    return m


def model_case(tag, cfg, head, k, pad, pool, batch, out, full=False):
    state = vits_state(cfg, k)
    model = build_reference(cfg, head, k, pad, pool, state)
    res = {} if full else {"param_names": np.array([n for n, _ in model.named_parameters()])}
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
    model.load_state_dict({n: torch.tensor(v) for n, v in state.items() if n in model.state_dict()})      # undo the merge drift
    total, parts = H.total_loss(model, cfg, xr, yr, xf, yf, HYPER, proto)
    model.zero_grad()
    total.backward()
    res["losses1"] = np.array(parts, dtype=np.float64)
    res.update({f"grad1::{n}": g for n, g in H.grads(model).items()})
    if not full:
        total, _ = H.total_loss(model, cfg, xr, yr, xf, yf, dict(HYPER, BND=5.0, BND_pro=0.1), proto)      # both hinges inactive
        model.zero_grad()
        total.backward()
        res["total_inactive"] = np.float64(total.item())
        res.update({f"grad_inactive::{n}": g for n, g in H.grads(model).items()})
        res["param_shapes"] = np.array([list(p.shape) + [0] * (3 - p.dim()) for _, p in model.named_parameters()], dtype=np.int64)
    H.save(out, tag, res)


def engine_case(tag, cfg, head, k, pad, batch, out, n_steps=3):
    import engine_cl
    from util import utils as rutil
    model = build_reference(cfg, head, k, pad, "cls", vits_state(cfg, k))
    res = {"param_names": np.array([n for n, _ in model.named_parameters()])}
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=HYPER["lr"], weight_decay=HYPER["wd"], eps=1e-8, betas=(0.9, 0.999))
    meters = {n: rutil.AverageMeter() for n in H.METER_NAMES}
    proto = {c: torch.tensor(v) for c, v in enumerate(recipe.make_prototypes(cfg))}
    cfgd = {"DATA_ROOT": "./data/casia100/", "BND_pro": HYPER["BND_pro"], "MULTI_GPU": False, "WORK_PATH": "/tmp", "BACKBONE_NAME": "VITs"}
    batch_ctr = 0
    for s in range(n_steps):
        xr, yr, xf, yf = H.batches(cfg, batch, s)
        ret = engine_cl.train_one_epoch(
            model=model, dataloader_forget=ListLoader([(xf, yf)]), dataloader_remain=ListLoader([(xr, yr)]), device=torch.device("cpu"),
            criterion=torch.nn.CrossEntropyLoss(), optimizer=opt, epoch=0, beta=HYPER["beta"], alpha=HYPER["alpha"], BND=HYPER["BND"],
            batch=batch_ctr, testloader_forget=None, testloader_remain=None, forget_acc_before=0.0, highest_H_mean=0.0, cfg=cfgd,
            task_i="0", use_prototype=True, prototype_dict=proto, prototype_weight_forget=HYPER["pro_f_weight"],
            prototype_weight_remain=HYPER["pro_r_weight"], **meters)
        batch_ctr = ret[0]
        res[f"meters{s + 1}"] = np.array([meters[n].val for n in H.METER_NAMES], dtype=np.float64)
        if s == 0:
            res.update({f"grad1::{n}": g for n, g in H.grads(model).items()})
        if s in (0, n_steps - 1):
            res.update({f"param{s + 1}::{n}": p.detach().numpy().copy() for n, p in model.named_parameters() if p.requires_grad})
    res[f"meters{n_steps}_avg"] = np.array([meters[n].avg for n in H.METER_NAMES], dtype=np.float64)
    res["batch_ctr"] = np.int64(batch_ctr)
    H.save(out, tag, res)


CASES = {
    "vits_small2_b3": lambda out: model_case("vits_small2_b3", recipe.cfg_small2(), "CosFace", 12, 4, "cls", 3, out),
    "vits_k10p1_small2_b3": lambda out: model_case("vits_k10p1_small2_b3", recipe.cfg_small2(), "ArcFace", 10, 1, "mean", 3, out),
    "vits_small6_engine": lambda out: engine_case("vits_small6_engine", recipe.cfg_small6(), "CosFace", 12, 4, 2, out),
    "vits_full_b2": lambda out: model_case("vits_full_b2", recipe.cfg_full(), "CosFace", 12, 4, "cls", 2, out, full=True),
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
