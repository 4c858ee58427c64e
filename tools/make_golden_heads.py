"""Golden fixtures of the ArcFace and Softmax heads, from the REAL reference (imported unmodified) on the deterministic recipe of
oracle/recipe.py. Runs only where the reference sources are checked out (the build machine); the GPU tests read the arrays alone.

    python tools/make_golden_heads.py                      # all four fixtures
    python tools/make_golden_heads.py arcface_small2_b3    # one of them

writes tests/golden/{arcface_small2_b3, arcface_attn_small_b3, softmax_small2_b3, arcface_small6_engine}.npz. The keys follow
small2_b3.npz (oracle/make_golden.py): fwd_* / eval_* logits and embeddings (train mode, then eval = merged LoRA), losses1 and
grad1::* of the GS-LoRA total loss, grad_inactive::* / total_inactive with both hinges inactive, and param_names (the reference's
named_parameters order). The Softmax fixture runs with a non-zero head bias, recipe.uniform("loss.bias", ...). The engine fixture holds
three steps of the reference's engine_cl.train_one_epoch + torch AdamW on cfg_small6: meters{1,2,3} (per-step values), meters3_avg,
grad1::*, param1::* / param3::* and batch_ctr, as full_b2.npz does.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import recipe  # noqa: E402
from oracle.make_golden import HYPER, ListLoader, install_shims  # noqa: E402


def head_state(cfg, head):
    """The recipe's state dict with the head's parameters (ArcFace: the same loss.weight as CosFace; Softmax: plus a non-zero bias)."""
    st = recipe.make_state(cfg)
    if head == "Softmax":
        st["loss.bias"] = recipe.uniform("loss.bias", (cfg["num_class"],), 1337, -0.5, 0.5)
    return st


def build_reference(cfg, head, state):
    import loralib as lora
    from vit_pytorch_face import ViT_face
    m = ViT_face(loss_type=head, GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
                 dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], dropout=0.0, emb_dropout=0.0,
                 lora_rank=cfg["lora_rank"], lora_pos=cfg.get("lora_pos", "FFN"))
    m.load_state_dict({k: torch.tensor(v) for k, v in state.items()}, strict=True)
    lora.mark_only_lora_as_trainable(m)
    return m


def batches(cfg, batch, s=0):
    nf = max(2, cfg["num_class"] // 5)
    return (torch.tensor(recipe.make_images(cfg, batch, seed=100 + s, tag="xr")),
            torch.tensor(recipe.make_labels(cfg, batch, seed=100 + s, tag="yr", lo=0, hi=cfg["num_class"] - nf)),
            torch.tensor(recipe.make_images(cfg, batch, seed=200 + s, tag="xf")),
            torch.tensor(recipe.make_labels(cfg, batch, seed=200 + s, tag="yf", lo=cfg["num_class"] - nf, hi=cfg["num_class"])))


def total_loss(model, cfg, xr, yr, xf, yf, hy, proto):
    """The GS-LoRA total loss of engine_cl.py:59-125, by hand (engine_cl hard-codes six structure groups)."""
    import engine as engine_single
    import engine_cl
    crit = torch.nn.CrossEntropyLoss()
    lo_r, em_r = model(xr, yr)
    lo_f, em_f = model(xf, yf)
    ce_r, ce_f = crit(lo_r, yr), crit(lo_f, yf)
    sl = engine_single.get_structure_loss(model, num_layers=cfg["depth"], group_type="block", group_pos=cfg.get("lora_pos", "FFN"))
    kl_f = engine_cl.get_prototype_loss(em_f, yf, proto)
    kl_r = engine_cl.get_prototype_loss(em_r, yr, proto)
    total = (hy["beta"] * torch.relu(hy["BND"] - ce_f) + ce_r + hy["alpha"] * sl
             + hy["pro_f_weight"] * torch.relu(hy["BND_pro"] - kl_f) + hy["pro_r_weight"] * kl_r)
    return total, [ce_f.item(), ce_r.item(), total.item(), sl.item(), kl_f.item(), kl_r.item()]


def grads(model):
    return {n: p.grad.numpy().copy() for n, p in model.named_parameters() if p.requires_grad}


def model_case(tag, cfg, head, batch, out):
    state = head_state(cfg, head)
    model = build_reference(cfg, head, state)
    res = {"param_names": np.array([n for n, _ in model.named_parameters()])}
    xr, yr, xf, yf = batches(cfg, batch)
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
    total, parts = total_loss(model, cfg, xr, yr, xf, yf, HYPER, proto)
    model.zero_grad()
    total.backward()
    res["losses1"] = np.array(parts, dtype=np.float64)
    res.update({f"grad1::{n}": g for n, g in grads(model).items()})
    total, _ = total_loss(model, cfg, xr, yr, xf, yf, dict(HYPER, BND=5.0, BND_pro=0.1), proto)      # both hinges inactive
    model.zero_grad()
    total.backward()
    res["total_inactive"] = np.float64(total.item())
    res.update({f"grad_inactive::{n}": g for n, g in grads(model).items()})
    save(out, tag, res)


METER_NAMES = ("losses_forget", "losses_remain", "losses_total", "losses_structure", "top1_forget", "top1_remain",
               "losses_prototype_forget", "losses_prototype_remain")


def engine_case(tag, cfg, head, batch, out, n_steps=3):
    import engine_cl
    from util import utils as rutil
    model = build_reference(cfg, head, head_state(cfg, head))
    res = {"param_names": np.array([n for n, _ in model.named_parameters()])}
    params = [p for p in model.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=HYPER["lr"], weight_decay=HYPER["wd"], eps=1e-8, betas=(0.9, 0.999))
    meters = {k: rutil.AverageMeter() for k in METER_NAMES}
    proto = {c: torch.tensor(v) for c, v in enumerate(recipe.make_prototypes(cfg))}
    cfgd = {"DATA_ROOT": "./data/casia100/", "BND_pro": HYPER["BND_pro"], "MULTI_GPU": False, "WORK_PATH": "/tmp", "BACKBONE_NAME": "VIT"}
    batch_ctr = 0
    for s in range(n_steps):
        xr, yr, xf, yf = batches(cfg, batch, s)
        ret = engine_cl.train_one_epoch(
            model=model, dataloader_forget=ListLoader([(xf, yf)]), dataloader_remain=ListLoader([(xr, yr)]), device=torch.device("cpu"),
            criterion=torch.nn.CrossEntropyLoss(), optimizer=opt, epoch=0, beta=HYPER["beta"], alpha=HYPER["alpha"], BND=HYPER["BND"],
            batch=batch_ctr, testloader_forget=None, testloader_remain=None, forget_acc_before=0.0, highest_H_mean=0.0, cfg=cfgd,
            task_i="0", use_prototype=True, prototype_dict=proto, prototype_weight_forget=HYPER["pro_f_weight"],
            prototype_weight_remain=HYPER["pro_r_weight"], **meters)
        batch_ctr = ret[0]
        res[f"meters{s + 1}"] = np.array([meters[k].val for k in METER_NAMES], dtype=np.float64)
        if s == 0:
            res.update({f"grad1::{n}": g for n, g in grads(model).items()})
        if s in (0, n_steps - 1):
            res.update({f"param{s + 1}::{n}": p.detach().numpy().copy() for n, p in model.named_parameters() if p.requires_grad})
    res[f"meters{n_steps}_avg"] = np.array([meters[k].avg for k in METER_NAMES], dtype=np.float64)
    res["batch_ctr"] = np.int64(batch_ctr)
    save(out, tag, res)


def save(out, tag, res):
    path = os.path.join(out, f"{tag}.npz")
    np.savez_compressed(path, **res)
    print(f"[golden] {tag}: {len(res)} arrays, {os.path.getsize(path) / 1e6:.2f} MB")


CASES = {
    "arcface_small2_b3": lambda out: model_case("arcface_small2_b3", recipe.cfg_small2(), "ArcFace", 3, out),
    "arcface_attn_small_b3": lambda out: model_case("arcface_attn_small_b3", recipe.cfg_small_attn(), "ArcFace", 3, out),
    "softmax_small2_b3": lambda out: model_case("softmax_small2_b3", recipe.cfg_small2(), "Softmax", 3, out),
    "arcface_small6_engine": lambda out: engine_case("arcface_small6_engine", recipe.cfg_small6(), "ArcFace", 2, out),
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
