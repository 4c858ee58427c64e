"""GPU tests of the regularisation baselines end to end on cfg_small (lora_rank = 0, CosFace, the --only_ffn rule): the importance matrices of
gslora_hip.reg.calculate_importance against the REAL reference's model (tests/golden/importance_small.npz), the epoch loop
engine_reg.train_one_epoch_regularzation against the REAL reference engine (tests/golden/reg_epoch_small_engine.npz — both from
tools/make_golden_reg_baselines.py), and driver_reg.

f32: per-batch gradients within 1e-4 * max(1, |g|_max), the project's parity bar; the importance within what that bar allows (derived in
importance_bound). fp16 / bf16: per-batch gradients within 1 % / 6 % relative Frobenius error, and the importance bit-equal to the kernel's
expression applied to the path's own gradients."""
import json
import os
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import recipe

import test_hip_ffn_train as T

pytestmark = pytest.mark.gpu

SIZES = (3, 2)
ARGS = dict(opt="adamw", weight_decay=0.05, opt_eps=1e-8, opt_betas=None)


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "importance_small.npz"))


def importance_loader(cfg, g=None):
    loader = []
    for b, size in enumerate(SIZES):
        x, y, _, _ = T.batches(cfg, size, b)
        if g is not None:
            assert y.cpu().tolist() == g[f"y::{b}"].tolist()
        loader.append((x, y))
    return loader


def batch_gradients(m, loader, kind):
    """The eval-mode gradients of every batch, by the steps calculate_importance takes (the model is left in train())."""
    from gslora_hip import losses, reg
    out = []
    m.eval()
    for x, y in loader:
        logits, _ = m(x, y)
        loss = reg.sq_mean(logits) if kind == "mas" else losses.ce_sum_top1(logits, y)[0] / float(x.shape[0])
        m.zero_grad()
        loss.backward()
        out.append({n: p.grad.detach().cpu().clone() for n, p in m.named_parameters() if p.requires_grad})
    m.zero_grad()
    m.train()
    return out


def torch_accumulate(omega, grads, kind):
    """The reference's accumulation (train_own_forget_cl.py:1505-1509, :1556-1558) on CPU tensors, in place."""
    for size, g in zip(SIZES, grads):
        for n, om in omega.items():
            if kind == "ewc":
                om += g[n] ** 2 * size / len(grads)
            else:
                om += g[n].abs() / len(grads)
    return omega


def importance_bound(g, kind, name, passes=1):
    """What a per-batch gradient error of delta_b = 1e-4 * max(1, |g_b|_max) — the parity bar — allows per element of the importance:
    EWC  sum_b w_b * delta_b * (2 |g_b| + delta_b), w_b = len(batch_b) / len(loader) ((g + d)^2 - g^2 = d (2 g + d));
    MAS  sum_b delta_b / len(loader) (| |g + d| - |g| | <= |d|). From the fixture's stored gradients."""
    L, total = len(SIZES), 0.0
    for b, size in enumerate(SIZES):
        gb = np.abs(g[f"grad_{kind}::{b}::{name}"].astype(np.float64))
        delta = 1e-4 * max(1.0, gb.max())
        total = total + (size / L * delta * (2.0 * gb + delta) if kind == "ewc" else delta / L + 0.0 * gb)
    return passes * total


def within(got, want, bound, what):
    got, want = got.detach().cpu().numpy().astype(np.float64), want.astype(np.float64)
    ulp4 = 4.0 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    ratio = (np.abs(got - want) / (bound + ulp4)).max()
    print(f"{what}: max |err| / bound = {ratio:.4f}")
    return ratio <= 1.0


# ---------------------------------------------------------------------------------------------------------------- importance, f32
def test_importance_f32_matches_the_reference_fixture(fixture):
    from gslora_hip import _lib_reg, reg
    g, cfg = fixture, recipe.cfg_small(lora_rank=0)
    m = T.build(cfg, "fp32")
    names = [n for n, p in m.named_parameters() if p.requires_grad]
    assert names == g["trainable"].tolist()
    loader = importance_loader(cfg, g)
    for kind in ("ewc", "mas"):
        for b, grads in enumerate(batch_gradients(m, loader, kind)):
            for n in names:
                assert T.bar_ok(grads[n], g[f"grad_{kind}::{b}::{n}"], f"{kind} batch {b} {n}"), (kind, b, n)
    crit = torch.nn.CrossEntropyLoss()
    ewc = reg.calculate_importance(m, loader, "ewc", criterion=crit)
    assert m.training and _lib_reg.loaded() and ewc.skipped == 0 and list(ewc) == names
    mas = reg.calculate_importance(m, loader, "mas")
    assert m.training and mas.skipped == 0
    for n in names:
        assert ewc[n].dtype == torch.float32 and ewc[n].shape == m.get_parameter(n).shape
        assert within(ewc[n], g[f"ewc::{n}"], importance_bound(g, "ewc", n), f"ewc {n}"), n
        assert within(mas[n], g[f"mas::{n}"], importance_bound(g, "mas", n), f"mas {n}"), n
    first = {n: v.clone() for n, v in ewc.items()}
    online = reg.calculate_importance(m, loader, "ewc", criterion=crit, prior=ewc)      # --online: continues IN PLACE
    for n in names:
        assert online[n] is ewc[n] and not torch.equal(ewc[n], first[n])
        assert within(online[n], g[f"ewc_online::{n}"], importance_bound(g, "ewc", n, passes=2), f"ewc online {n}"), n
    ones = reg.calculate_importance(m, None, "l2")
    assert list(ones) == names and all(bool((v == 1).all()) and v.shape == m.get_parameter(n).shape and v.is_cuda for n, v in ones.items())


class WithIdleParameter(torch.nn.Module):
    """The model plus a parameter that requires a gradient and never receives one."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner
        self.idle = torch.nn.Parameter(torch.zeros(5, device="cuda"))

    def forward(self, x, y):
        return self.inner(x, y)


def test_a_tensor_without_a_gradient_keeps_its_importance():
    from gslora_hip import reg
    cfg = recipe.cfg_small(lora_rank=0)
    w = WithIdleParameter(T.build(cfg, "fp32"))
    prior = {n: torch.full(p.shape, 0.25, device="cuda") for n, p in w.named_parameters() if p.requires_grad}
    prior["idle"] = torch.tensor([1.0, -2.0, 3e-40, 0.0, 7.0], device="cuda")
    keep = prior["idle"].clone()
    imp = reg.calculate_importance(w, importance_loader(cfg), "mas", prior=prior)
    assert torch.equal(imp["idle"].view(torch.int32), keep.view(torch.int32)) and w.idle.grad is None
    assert all(bool((v > 0.25).any()) for n, v in imp.items() if n != "idle") and w.training and w.inner.training


# ---------------------------------------------------------------------------------------------------------------- importance, 16-bit modes
@pytest.mark.parametrize("mode,band", [("fp16", 0.01), ("bf16", 0.06)])
def test_importance_16bit_modes(fixture, mode, band):
    from gslora_hip import reg
    g, cfg = fixture, recipe.cfg_small(lora_rank=0)
    m = T.build(cfg, mode)
    names = [n for n, p in m.named_parameters() if p.requires_grad]
    loader = importance_loader(cfg, g)
    for kind in ("ewc", "mas"):
        grads = batch_gradients(m, loader, kind)
        worst = 0.0
        for b in range(len(SIZES)):
            for n in names:
                want = g[f"grad_{kind}::{b}::{n}"].astype(np.float64)
                rel = np.linalg.norm(grads[b][n].numpy() - want) / np.linalg.norm(want)
                worst = max(worst, rel)
                assert rel <= band, (kind, b, n, rel)
        print(f"{mode} {kind}: worst relative Frobenius error of a per-batch gradient {worst:.5f} (band {band})")
        imp = reg.calculate_importance(m, loader, kind, criterion=torch.nn.CrossEntropyLoss())
        assert imp.skipped == 0 and m.training
        want = torch_accumulate({n: torch.zeros_like(grads[0][n]) for n in names}, grads, kind)
        for n in names:      # the kernel's expression on the path's own gradients, bit for bit
            assert torch.equal(imp[n].cpu().view(torch.int32), want[n].view(torch.int32)), (kind, n)


def test_fp16_saturated_batch_is_skipped_without_a_host_sync():
    from gslora_hip import reg
    cfg = recipe.cfg_small(lora_rank=0)
    m = T.build(cfg, "fp16")
    with torch.no_grad():
        # the last block's FFN: nothing but the head's LayerNorm follows, and the scaled gradients behind it leave the fp16 range (a weight
        # of an earlier block does not do it: the next block's LayerNorm divides the gradient by what the forward was multiplied with)
        m.transformer.layers[-1][1].fn.fn.net[3].weight.mul_(2000.0)
    loader = importance_loader(cfg)[:1]
    prior = {n: torch.full(p.shape, 0.5, device="cuda") for n, p in m.named_parameters() if p.requires_grad}
    torch.cuda.synchronize()
    calls = {"item": 0}
    item = torch.Tensor.item

    def counting_item(self):
        calls["item"] += 1
        return item(self)
    mp = pytest.MonkeyPatch()
    mp.setattr(torch.Tensor, "item", counting_item)
    try:
        try:
            torch.cuda.set_sync_debug_mode("warn")
            debug = True
        except Exception:
            debug = False
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            imp = reg.calculate_importance(m, loader, "ewc", criterion=torch.nn.CrossEntropyLoss(), prior=prior)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        mp.undo()
    syncs = [str(w.message) for w in seen if "synchroniz" in str(w.message)]
    print(f"sync debug mode available: {debug}; synchronising calls seen: {len(syncs)}; .item() calls: {calls['item']}")
    assert calls["item"] == 1      # the read of the counter at the end
    assert not debug or len(syncs) <= 1, syncs
    assert imp.skipped == 1 and m.training
    assert all(bool((v == 0.5).all()) for v in imp.values())
    assert m.runner().loss_scale_report()["saturated"]


# ---------------------------------------------------------------------------------------------------------------- the epoch loop
def epoch_setup(g, golden_dir):
    from gslora_hip.optim import create_optimizer
    cfg = recipe.cfg_small(lora_rank=0)
    m = T.build(cfg, "fp32")
    imp = np.load(os.path.join(golden_dir, "importance_small.npz"))      # term 0: the EWC importance the reference engine ran with
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    assert [n for n, _ in named] == g["trainable"].tolist()
    shift = float(g["shift"])
    terms = {0: {"importance": {n: torch.tensor(imp[f"ewc::{n}"]).cuda() for n, _ in named}, "task_param": {n: p.clone().detach() for n, p in named}},
             1: {"importance": {n: p.clone().detach().fill_(1) for n, p in named}, "task_param": {n: p.clone().detach() + shift for n, p in named}}}
    opt = create_optimizer(SimpleNamespace(lr=float(g["hyper_lr"]), **{**ARGS, "weight_decay": float(g["hyper_wd"])}), m)
    loader = []
    for s in range(6):
        x, y, _, _ = T.batches(cfg, 2, 10 + s)
        assert y.cpu().tolist() == g[f"y{s + 1}"].tolist()
        loader.append((x, y))
    return m, terms, opt, loader


def test_epoch_loop_matches_the_reference_engine(golden_dir):
    import engine_reg
    from gslora_hip.step import ffn_reg_step
    from util.utils import AverageMeter

    class Recording(AverageMeter):
        def __init__(self):
            super().__init__()
            self.seen = []

        def update(self, val, n=1):
            self.seen.append(float(val))
            super().update(val, n)

    g = np.load(os.path.join(golden_dir, "reg_epoch_small_engine.npz"))
    lam, crit = float(g["reg_lambda"]), torch.nn.CrossEntropyLoss()
    m, terms, opt, loader = epoch_setup(g, golden_dir)
    meters = [Recording(), Recording(), Recording()]
    batch, best, m_ce, m_reg, m_total = engine_reg.train_one_epoch_regularzation(
        model=m, criterion=crit, data_loader_cl_forget=loader, optimizer=opt, device=torch.device("cuda"), epoch=0, batch=0, reg_lambda=lam,
        regularization_terms=terms, losses_CE=meters[0], losses_regularization=meters[1], losses_total=meters[2], task_i=0,
        testloader_forget=None, testloader_remain=None, forget_acc_before=0.0, highest_H_mean=0.0, cfg={})
    assert batch == int(g["batch"]) == 6 and best == 0.0 and m.training
    steps = np.array([r.seen for r in meters]).T
    assert steps.shape == (5, 3)      # the engine re-binds fresh meters at its display in step 5, as the reference does
    for s in range(5):
        print(f"step {s + 1}: (CE, reg, total) {steps[s].tolist()} vs {g['steps'][s].tolist()}")
        for got, want in zip(steps[s], g["steps"][s]):
            assert abs(got - want) <= 1e-4 * max(1.0, abs(want)), s
    for meter, want in zip((m_ce, m_reg, m_total), g["returned"]):
        assert meter is not meters[0] and meter.count == want[3] == 2
        for got, w in zip((meter.val, meter.avg, meter.sum), want[:3]):
            assert abs(got - w) <= 1e-4 * max(1.0, abs(w))
    for n, p in m.named_parameters():
        if p.requires_grad:
            err = np.abs(p.detach().cpu().numpy() - g[f"final::{n}"]).max()
            print(f"after step 6 {n}: err {err:.3e}")
            assert err <= 1e-4, n
    # the same six steps with the dict form of ffn_reg_step (get_reg_loss's own launches): the same bits
    m2, terms2, opt2, loader2 = epoch_setup(g, golden_dir)
    for x, y in loader2:
        ffn_reg_step(m2, opt2, crit, x, y, regularization_terms=terms2, reg_lambda=lam)
    for (n, p), (_, q) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.equal(p.detach(), q.detach()), n


# ---------------------------------------------------------------------------------------------------------------- the driver
def test_driver_reg_runs_two_tasks(tmp_path):
    import driver_reg
    common = ["--small", "--num_class", "20", "--num_tasks", "2", "--per_forget_cls", "4", "--epochs", "1", "--batch_size", "16", "--dropout", "0.0"]
    rep, out, (model, terms) = driver_reg.main(common + ["--ewc", "--ewc_lambda", "10", "--dtype", "fp32", "--outdir", str(tmp_path / "ewc")])
    lines = [json.loads(ln) for ln in open(os.path.join(out, "reg_report.jsonl"))]
    assert len(rep) == len(lines) == 2 and [r["task"] for r in lines] == [0, 1] and sorted(terms) == [0, 1]
    for r in rep:
        assert r["kind"] == "ewc" and r["n_terms"] == 2 and r["steps"] == 2 and r["importance_sum"] > 0 and r["skipped_importance_batches"] == 0
        assert all(np.isfinite(v) for e in r["epochs"] for v in e.values()) and len(r["forget_cls"]) == 4
    assert rep[1]["epochs"][0]["losses_regularization"] > 0      # the second task starts away from the first term's weights
    assert not any(p.requires_grad for n, p in model.named_parameters() if "fn.fn.net" not in n)
    rep, out, (model, terms) = driver_reg.main(common + ["--MAS", "--online", "--ffn_open", "--dtype", "bf16", "--outdir", str(tmp_path / "mas")])
    assert [r["n_terms"] for r in rep] == [1, 1] and sorted(terms) == [0] and all(r["importance_sum"] > 0 and r["online"] for r in rep)
    assert rep[1]["importance_sum"] > 0 and model.loss.weight.requires_grad
