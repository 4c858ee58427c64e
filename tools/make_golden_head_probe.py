"""Golden fixtures of the linear probe (a trainable classifier head), from the REAL reference (imported unmodified through
oracle.make_golden.install_shims) on the deterministic recipe of oracle/recipe.py. Runs only where the reference sources are checked out
(the build machine); the tests read the arrays alone.

    python tools/make_golden_head_probe.py                         # all five fixtures
    python tools/make_golden_head_probe.py head_open_small2_b3     # one of them
    python tools/make_golden_head_probe.py --out DIR [tags ...]    # into another directory (tests/test_head_probe_host.py regenerates there)

Writes tests/golden/:
  head_probe_small2_{cosface,arcface,softmax}_b3.npz
        cfg_small2, trainability by the rule of train/backbone_forget_main.py:596-600 (requires_grad = "loss" in name), one step of
        :657-659 on the recipe's remain batch of 3: `logits`, `loss`, `prec1` (train_accuracy, topk=(1,)), `grad::loss.weight` (Softmax:
        also `grad::loss.bias`, with the recipe's non-zero bias of tools/make_golden_heads.head_state), `y` and `param_names`.
        The ArcFace fixture runs on a head weight whose label rows of samples 0 and 1 are turned towards -emb_0 / +emb_1, so that the label
        cosines (`cos_y`) lie on BOTH sides of the threshold th = cos(pi - m) and none within 1e-3 of it; `state::loss.weight` holds that
        weight. Its `easy_*` keys are the same step with easy_margin = True (label cosines of both signs).
  head_probe_small6_engine.npz
        cfg_small6, CosFace: three steps of :657-670 (forward, CE, train_accuracy, zero_grad, backward, step) on the recipe's remain + forget
        batches (2 + 2 images per step) with torch.optim.AdamW in timm's grouping (decay on loss.weight): `weight{1,2,3}` after every step,
        `losses`, `prec1`, `y{1,2,3}`, `hyper_lr`, `hyper_wd`.
  head_open_small2_b3.npz
        cfg_small2, CosFace, LoRA AND the head trainable (the baselines' --ffn_open) under tools/make_golden_heads.total_loss: `losses1`,
        `grad1::*` of every LoRA tensor and of loss.weight.
No reference text is copied or edited.
"""
import math
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

HEADS = {"cosface": "CosFace", "arcface": "ArcFace", "softmax": "Softmax"}


def only_head_trainable(model):
    """The rule of train/backbone_forget_main.py:596-600."""
    for name, param in model.named_parameters():
        param.requires_grad = "loss" in name
    return [n for n, p in model.named_parameters() if p.requires_grad]


def probe_forward_backward(model, x, y):
    """:657-662 and :668-669: outputs, CE, train_accuracy, backward. -> (logits, loss, prec1)"""
    from util import utils as rutil
    outputs, _ = model(x.float(), y)
    loss = torch.nn.CrossEntropyLoss()(outputs, y)
    prec1 = rutil.train_accuracy(outputs.data, y, topk=(1,))
    model.zero_grad()
    loss.backward()
    return outputs.detach().numpy().copy(), np.float64(loss.item()), np.float64(float(prec1))


def arcface_weight(model, x, y, state):
    """The recipe's head weight with the label rows of samples 0 and 1 turned towards -emb_0 and +emb_1 (norms kept): label cosines
    near -0.95, +0.6 and the natural one of sample 2."""
    assert len(set(y.tolist())) == len(y), "the ArcFace case needs distinct labels"
    with torch.no_grad():
        _, emb = model(x.float(), y)
    W = torch.tensor(state["loss.weight"]).clone()
    for i, (target, keep) in enumerate(((-0.95, 0.05), (0.6, 0.4))):
        e = emb[i] / emb[i].norm()
        w = W[y[i]] / W[y[i]].norm()
        w_perp = w - (w @ e) * e
        row = target * e + math.sqrt(1.0 - target * target) * w_perp / w_perp.norm()
        W[y[i]] = row * torch.tensor(state["loss.weight"])[y[i]].norm()
    return W.numpy()


def probe_case(tag, out):
    kind = tag.split("_")[3]
    head, cfg = HEADS[kind], recipe.cfg_small2()
    state = H.head_state(cfg, head)
    x, y, _, _ = H.batches(cfg, 3)
    model = H.build_reference(cfg, head, state)
    res = {"param_names": np.array([n for n, _ in model.named_parameters()]), "y": y.numpy().copy()}
    if kind == "arcface":
        model.train()
        state["loss.weight"] = arcface_weight(model, x, y, state)
        model.load_state_dict({k: torch.tensor(v) for k, v in state.items()}, strict=True)
        res["state::loss.weight"] = state["loss.weight"].copy()
    trainable = only_head_trainable(model)
    assert trainable == (["loss.weight", "loss.bias"] if kind == "softmax" else ["loss.weight"]), trainable
    model.train()      # :631
    variants = [("", False)] + ([("easy_", True)] if kind == "arcface" else [])
    for prefix, easy in variants:
        if kind == "arcface":
            model.loss.easy_margin = easy
            with torch.no_grad():
                _, emb = model(x.float(), y)
                W = model.loss.weight
                cos_y = ((emb / emb.norm(dim=1, keepdim=True)) @ (W / W.norm(dim=1, keepdim=True)).t())[torch.arange(len(y)), y]
            res["cos_y"] = cos_y.numpy().copy()
            th = model.loss.th
            if easy:
                assert (cos_y > 1e-3).any() and (cos_y < -1e-3).any(), cos_y      # label cosines of both signs
            else:
                assert (cos_y > th).any() and (cos_y < th).any() and ((cos_y - th).abs() > 1e-3).all(), (cos_y, th)
        logits, loss, prec1 = probe_forward_backward(model, x, y)
        res[prefix + "logits"], res[prefix + "loss"], res[prefix + "prec1"] = logits, loss, prec1
        for n, p in model.named_parameters():
            assert (p.grad is not None) == (n in trainable), n
            if n in trainable:
                res[f"{prefix}grad::{n}"] = p.grad.numpy().copy()
    H.save(out, tag, res)


def engine_case(tag, out, n_steps=3):
    cfg = recipe.cfg_small6()
    model = H.build_reference(cfg, "CosFace", H.head_state(cfg, "CosFace"))
    trainable = only_head_trainable(model)
    assert trainable == ["loss.weight"]
    # timm's create_optimizer grouping: no decay for biases / 1-D tensors, decay for the rest (loss.weight is 2-D)
    opt = torch.optim.AdamW([dict(params=[model.loss.weight], weight_decay=HYPER["wd"])], lr=HYPER["lr"], eps=1e-8, betas=(0.9, 0.999))
    from util import utils as rutil
    criterion = torch.nn.CrossEntropyLoss()
    model.train()
    res = {"param_names": np.array([n for n, _ in model.named_parameters()]), "hyper_lr": np.float64(HYPER["lr"]), "hyper_wd": np.float64(HYPER["wd"])}
    losses, precs = [], []
    for s in range(n_steps):
        xr, yr, xf, yf = H.batches(cfg, 2, s)
        inputs, labels = torch.cat((xr, xf)), torch.cat((yr, yf))      # the combined loader's mix of remain and forget images
        outputs, _ = model(inputs.float(), labels)                     # :657
        loss = criterion(outputs, labels)                              # :658
        prec1 = rutil.train_accuracy(outputs.data, labels, topk=(1,))  # :662
        opt.zero_grad()                                                # :668-670
        loss.backward()
        opt.step()
        losses.append(loss.item())
        precs.append(float(prec1))
        res[f"y{s + 1}"] = labels.numpy().copy()
        res[f"weight{s + 1}"] = model.loss.weight.detach().numpy().copy()
    res["losses"], res["prec1"] = np.array(losses, dtype=np.float64), np.array(precs, dtype=np.float64)
    H.save(out, tag, res)


def open_case(tag, out):
    cfg = recipe.cfg_small2()
    model = H.build_reference(cfg, "CosFace", H.head_state(cfg, "CosFace"))
    model.loss.weight.requires_grad = True      # LoRA (build_reference) and the head
    res = {"param_names": np.array([n for n, _ in model.named_parameters()])}
    xr, yr, xf, yf = H.batches(cfg, 3)
    proto = {c: torch.tensor(v) for c, v in enumerate(recipe.make_prototypes(cfg))}
    model.train()
    total, parts = H.total_loss(model, cfg, xr, yr, xf, yf, HYPER, proto)
    model.zero_grad()
    total.backward()
    res["losses1"] = np.array(parts, dtype=np.float64)
    g = H.grads(model)
    assert "loss.weight" in g and sum("lora_" in n for n in g) == 4 * cfg["depth"]
    res.update({f"grad1::{n}": v for n, v in g.items()})
    H.save(out, tag, res)


CASES = {
    "head_probe_small2_cosface_b3": probe_case,
    "head_probe_small2_arcface_b3": probe_case,
    "head_probe_small2_softmax_b3": probe_case,
    "head_probe_small6_engine": engine_case,
    "head_open_small2_b3": open_case,
}


def main():
    install_shims()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    args = sys.argv[1:]
    out = os.path.join(ROOT, "tests", "golden")
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    for tag, run in CASES.items():
        if not args or tag in args:
            run(tag, out)


if __name__ == "__main__":
    main()
