"""Golden fixtures of FFN-weight training (the reference's --only_ffn mode), from the REAL reference (imported unmodified through
oracle.make_golden.install_shims) on the deterministic recipe of oracle/recipe.py. Runs only where the reference sources are checked out
(the build machine); the tests read the arrays alone.

    python tools/make_golden_ffn_train.py                       # both fixtures
    python tools/make_golden_ffn_train.py ffn_l2_small_engine   # one of them
    python tools/make_golden_ffn_train.py --out DIR [tags ...]  # into another directory (tests/test_ffn_train_host.py regenerates there)

Writes tests/golden/:
  ffn_train_small2_b3.npz
        cfg_small2(lora_rank=0), CosFace, dropout 0; trainability by the rule of train/train_own_forget_cl.py:432-439 (requires_grad =
        "fn.fn.net" in name or "loss" in name); one forward and backward of the mean cross-entropy on the recipe's remain batch of 3:
        `logits`, `loss`, `grad::*` of the twelve FFN tensors and of loss.weight, `y`, `param_names`.
  ffn_l2_small_engine.npz
        cfg_small(lora_rank=0), CosFace: three steps of engine_cl.py:490-512 (forward, CE, get_reg_loss, zero_grad, backward, step) on the
        recipe's remain + forget batches (2 + 2 images per step) with torch.optim.AdamW in timm's grouping (no decay on biases) and one L2
        term as train_own_forget_cl.py:1416-1440 builds it (importance 1, task_param the initial weights). After the first step the
        optimizer has moved every weight by about lr, so `reg_lambda` is chosen to make the term about as large as the cross-entropy from
        step 2 on (the term is exactly zero in step 1, where the weights are the task's): `losses` [3, 3] = (CE, regularisation, total) per
        step, `prec1`, `y{1,2,3}`, `final::*` every trainable tensor after step 3, `hyper_lr`, `hyper_wd`, `reg_lambda`.
No reference text is copied or edited.
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

REG_LAMBDA = 4.0      # sum (p - p0)^2 over the 33 k trainable values is ~ 33e3 * lr^2 = 3.3 after one AdamW step at lr 1e-2; CE is 35 .. 47


def state_without_lora(cfg):
    """The recipe's state of a model built with lora_rank = 0: the reference's loralib.Linear has no lora_A / lora_B then."""
    return {k: v for k, v in recipe.make_state(cfg).items() if "lora_" not in k}      # (the recipe lists them with zero rows)


def build_reference(cfg, state):
    from vit_pytorch_face import ViT_face
    m = ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
                 dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], dropout=0.0, emb_dropout=0.0, lora_rank=0)
    m.load_state_dict({k: torch.tensor(v) for k, v in state.items()}, strict=True)
    return m


def only_ffn_trainable(model):
    """The rule of train/train_own_forget_cl.py:432-439."""
    for name, param in model.named_parameters():
        param.requires_grad = "fn.fn.net" in name or "loss" in name
    return [n for n, p in model.named_parameters() if p.requires_grad]


def train_case(tag, out):
    cfg = recipe.cfg_small2(lora_rank=0)
    model = build_reference(cfg, state_without_lora(cfg))
    trainable = only_ffn_trainable(model)
    assert len(trainable) == 4 * cfg["depth"] + 1 and trainable[-1] == "loss.weight", trainable
    x, y, _, _ = H.batches(cfg, 3)
    model.train()
    outputs, _ = model(x.float(), y)
    loss = torch.nn.CrossEntropyLoss()(outputs, y)
    model.zero_grad()
    loss.backward()
    res = {"param_names": np.array([n for n, _ in model.named_parameters()]), "y": y.numpy().copy(),
           "logits": outputs.detach().numpy().copy(), "loss": np.float64(loss.item())}
    res.update({f"grad::{n}": v for n, v in H.grads(model).items()})
    H.save(out, tag, res)


def engine_case(tag, out, n_steps=3):
    import engine_cl
    from util import utils as rutil
    cfg = recipe.cfg_small(lora_rank=0)
    model = build_reference(cfg, state_without_lora(cfg))
    trainable = only_ffn_trainable(model)
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    # timm's create_optimizer grouping: no decay for biases / 1-D tensors, decay for the rest
    no_decay = [p for n, p in named if p.ndim <= 1 or n.endswith(".bias")]
    decay = [p for n, p in named if not (p.ndim <= 1 or n.endswith(".bias"))]
    opt = torch.optim.AdamW([dict(params=no_decay, weight_decay=0.0), dict(params=decay, weight_decay=HYPER["wd"])], lr=HYPER["lr"], eps=1e-8,
                            betas=(0.9, 0.999))
    # train_own_forget_cl.py:1416-1440: the task's weights and the identity importance of the L2 baseline
    task_param = {n: p.clone().detach() for n, p in named}
    importance = {n: p.clone().detach().fill_(1) for n, p in named}
    terms = {0: {"importance": importance, "task_param": task_param}}
    criterion = torch.nn.CrossEntropyLoss()
    model.train()
    res = {"param_names": np.array([n for n, _ in model.named_parameters()]), "trainable": np.array(trainable),
           "hyper_lr": np.float64(HYPER["lr"]), "hyper_wd": np.float64(HYPER["wd"]), "reg_lambda": np.float64(REG_LAMBDA)}
    losses, precs = [], []
    for s in range(n_steps):
        xr, yr, xf, yf = H.batches(cfg, 2, s)
        inputs, labels = torch.cat((xr, xf)), torch.cat((yr, yf))
        outputs, _ = model(inputs.float(), labels)                                             # :493
        loss_ce = criterion(outputs, labels)                                                   # :496
        loss_reg = engine_cl.get_reg_loss(model, terms, REG_LAMBDA, torch.device("cpu"))       # :500-502
        total = loss_reg + loss_ce                                                             # :507
        opt.zero_grad()                                                                        # :510-512
        total.backward()
        opt.step()
        losses.append([loss_ce.item(), loss_reg.item(), total.item()])
        precs.append(float(rutil.train_accuracy(outputs.data, labels, topk=(1,))))
        res[f"y{s + 1}"] = labels.numpy().copy()
    res["losses"], res["prec1"] = np.array(losses, dtype=np.float64), np.array(precs, dtype=np.float64)
    res.update({f"final::{n}": p.detach().numpy().copy() for n, p in named})
    H.save(out, tag, res)


CASES = {"ffn_train_small2_b3": train_case, "ffn_l2_small_engine": engine_case}


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
