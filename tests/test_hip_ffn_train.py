"""GPU tests of FFN-weight training on the HIP path (the reference's --only_ffn mode, train/train_own_forget_cl.py:432-439): the models with
trainable `fn.fn.net` tensors against the REAL reference (tests/golden/ffn_train_small2_b3.npz, ffn_l2_small_engine.npz —
tools/make_golden_ffn_train.py) and, for the cases the fixtures do not hold (pool='mean', dropout, ViTs_face), against torch autograd on the
CPU oracle with the same weights and masks.

f32: logits within 1e-4, every gradient within 1e-4 * max(1, |g|_max), the project's parity bar. bf16 / fp16: per tensor a relative Frobenius
error <= 6 % and a cosine > 0.995, the tolerance DESIGN.md section 1 declares for the gradients of the speed modes."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import gslora_oracle as O
from oracle import recipe

pytestmark = pytest.mark.gpu


def state_of(cfg, k=None):
    st = {n: v for n, v in recipe.make_state(cfg).items() if "lora_" not in n}
    if k is not None:      # ViTs_face: the embedding reads C * k * k window values (= tests/test_hip_vits.vits_state)
        fan_in = cfg["channels"] * k * k
        bound = 1.0 / float(np.sqrt(fan_in))
        st["patch_to_embedding.weight"] = np.ascontiguousarray(recipe.uniform("patch_to_embedding.weight", (cfg["dim"], fan_in), 1337, -bound, bound),
                                                               dtype=np.float32)
    return {n: torch.tensor(v) for n, v in st.items()}


def only_ffn(model, head=True):
    """The rule of train/train_own_forget_cl.py:432-439 (head=False: the FFN alone, loss.weight frozen)."""
    for n, p in model.named_parameters():
        p.requires_grad = "fn.fn.net" in n or (head and "loss" in n)
    return [n for n, p in model.named_parameters() if p.requires_grad]


def build(cfg, dtype="fp32", dropout=0.0, pool="cls", head=True, vits=None, state=None):
    from vit_pytorch_face import ViT_face, ViTs_face
    kw = dict(loss_type="CosFace", GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
              dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], pool=pool, dropout=dropout, emb_dropout=dropout,
              lora_rank=0)
    m = ViTs_face(ac_patch_size=vits[0], pad=vits[1], **kw) if vits else ViT_face(**kw)
    m.load_state_dict(state or state_of(cfg, vits[0] if vits else None), strict=True)
    only_ffn(m, head)
    return m.to("cuda").set_compute_dtype(dtype).train()


def batches(cfg, batch, s=0):
    nf = max(2, cfg["num_class"] // 5)
    mk = lambda a: torch.tensor(a).cuda()
    return (mk(recipe.make_images(cfg, batch, seed=100 + s, tag="xr")),
            mk(recipe.make_labels(cfg, batch, seed=100 + s, tag="yr", lo=0, hi=cfg["num_class"] - nf)),
            mk(recipe.make_images(cfg, batch, seed=200 + s, tag="xf")),
            mk(recipe.make_labels(cfg, batch, seed=200 + s, tag="yf", lo=cfg["num_class"] - nf, hi=cfg["num_class"])))


def ce_backward(m, x, y):
    from gslora_hip import losses
    logits, _ = m(x, y)
    loss = losses.ce_sum_top1(logits, y)[0] / x.shape[0]
    loss.backward()
    return logits.detach(), loss.detach()


def grads_of(m):
    return {n: p.grad.detach().cpu().numpy().copy() for n, p in m.named_parameters() if p.requires_grad}


def bar_ok(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bar = 1e-4 * max(1.0, np.abs(want).max())
    err = np.abs(got - want).max()
    print(f"{what}: max err / bar = {err / bar:.4f}")
    return err <= bar


def oracle_grads(st, x, y, cfg, names, *, pool="cls", vits=None, keep=None):
    """Mean cross-entropy of the reference forward on the CPU (oracle/gslora_oracle.py's arithmetic, restated here so that dropout masks, the
    mean pool and ViTs_face's overlapping windows can be injected) and its autograd gradients. keep(i, width, site) -> mask * 1 / (1 - p)."""
    st = {n: v.clone().requires_grad_(n in names) for n, v in st.items()}
    B, D, H = x.shape[0], cfg["dim"], cfg["heads"]
    x = x.cpu().float()
    tok = F.unfold(x, vits[0], stride=cfg["patch_size"], padding=vits[1]).transpose(1, 2) if vits else O.patchify(x, cfg["patch_size"])
    t = F.linear(tok, st["patch_to_embedding.weight"], st["patch_to_embedding.bias"])
    T = t.shape[1] + 1
    t = torch.cat((st["cls_token"].expand(B, -1, -1), t), 1) + st["pos_embedding"][:, :T]
    one = lambda i, w, site: 1.0
    keep = keep or one
    t = t * keep(-1, D, 1_000_000)
    for i in range(cfg["depth"]):
        a, f = f"transformer.layers.{i}.0.fn", f"transformer.layers.{i}.1.fn"
        xn = F.layer_norm(t, (D,), st[f"{a}.norm.weight"], st[f"{a}.norm.bias"], 1e-5)
        q, k, v = [u.reshape(B, T, H, 64).permute(0, 2, 1, 3) for u in F.linear(xn, st[f"{a}.fn.to_qkv.weight"]).chunk(3, -1)]
        att = (torch.einsum("bhid,bhjd->bhij", q, k) * D ** -0.5).softmax(-1)
        o = torch.einsum("bhij,bhjd->bhid", att, v).permute(0, 2, 1, 3).reshape(B, T, -1)
        t = F.linear(o, st[f"{a}.fn.to_out.0.weight"], st[f"{a}.fn.to_out.0.bias"]) * keep(i, D, 4 * i) + t
        xn = F.layer_norm(t, (D,), st[f"{f}.norm.weight"], st[f"{f}.norm.bias"], 1e-5)
        h = F.gelu(F.linear(xn, st[f"{f}.fn.net.0.weight"], st[f"{f}.fn.net.0.bias"])) * keep(i, cfg["mlp_dim"], 4 * i + 1)
        t = F.linear(h, st[f"{f}.fn.net.3.weight"], st[f"{f}.fn.net.3.bias"]) * keep(i, D, 4 * i + 2) + t
    emb = F.layer_norm(t.mean(1) if pool == "mean" else t[:, 0], (D,), st["mlp_head.0.weight"], st["mlp_head.0.bias"], 1e-5)
    logits = O.cosface(emb, st["loss.weight"], y.cpu())
    loss = F.cross_entropy(logits, y.cpu())
    gr = torch.autograd.grad(loss, [st[n] for n in names])
    return logits.detach(), {n: g.numpy() for n, g in zip(names, gr)}


# ---------------------------------------------------------------------------------------------------------------- against the reference
def test_f32_matches_the_reference_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "ffn_train_small2_b3.npz"))
    cfg = recipe.cfg_small2(lora_rank=0)
    m = build(cfg, "fp32")
    trainable = [n for n, p in m.named_parameters() if p.requires_grad]
    assert trainable == [k[6:] for k in g.files if k.startswith("grad::")] and len(trainable) == 13
    x, y, _, _ = batches(cfg, 3)
    assert y.cpu().tolist() == g["y"].tolist()
    logits, loss = ce_backward(m, x, y)
    assert bar_ok(logits.cpu(), g["logits"], "logits") and np.abs(logits.cpu().numpy() - g["logits"]).max() <= 1e-4
    assert abs(loss.item() - float(g["loss"])) <= 1e-4 * max(1.0, float(g["loss"]))
    got = grads_of(m)
    for n in trainable:
        assert got[n].shape == g[f"grad::{n}"].shape and bar_ok(got[n], g[f"grad::{n}"], n), n
    for n, p in m.named_parameters():
        assert (p.grad is not None) == (n in trainable), n
    from gslora_hip import _lib_train
    assert _lib_train.loaded()


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_16bit_modes_stay_within_the_declared_gradient_tolerance(golden_dir, mode):
    g = np.load(os.path.join(golden_dir, "ffn_train_small2_b3.npz"))
    cfg = recipe.cfg_small2(lora_rank=0)
    m = build(cfg, mode)
    x, y, _, _ = batches(cfg, 3)
    ce_backward(m, x, y)
    got = grads_of(m)
    worst_rel, worst_cos = 0.0, 1.0
    for n, v in got.items():
        want = g[f"grad::{n}"].astype(np.float64)
        rel = np.linalg.norm(v - want) / np.linalg.norm(want)
        cos = float((v.astype(np.float64) * want).sum() / (np.linalg.norm(v.astype(np.float64)) * np.linalg.norm(want)))
        print(f"{mode} {n}: rel Frobenius {rel:.4f}, cosine {cos:.5f}")
        worst_rel, worst_cos = max(worst_rel, rel), min(worst_cos, cos)
        assert rel <= 0.06 and cos > 0.995, n
    print(f"{mode}: worst rel Frobenius {worst_rel:.4f}, worst cosine {worst_cos:.5f}")
    if mode == "fp16":
        rep = m.runner().loss_scale_report()
        print("fp16 loss scale:", rep)
        assert rep["exponent"] == 11 and rep["S"] > 0 and not rep["saturated"]
        assert m.runner().overflow_guard() is not None      # what _arm_overflow_guard hands the optimizer for such a step


# ---------------------------------------------------------------------------------------------------------------- further model cases
def test_mean_pool_runs_a_dense_last_block():
    cfg = recipe.cfg_small2(lora_rank=0)
    m = build(cfg, "fp32", pool="mean")
    x, y, _, _ = batches(cfg, 3)
    logits, _ = ce_backward(m, x, y)
    names = [n for n, p in m.named_parameters() if p.requires_grad]
    want_logits, want = oracle_grads(state_of(cfg), x, y, cfg, names, pool="mean")
    assert (logits.cpu() - want_logits).abs().max() <= 1e-4
    got = grads_of(m)
    for n in names:
        assert bar_ok(got[n], want[n], f"mean pool {n}"), n


def test_dropout_gradients_use_the_masks_of_the_forward():
    from gslora_hip import ops
    cfg, p, B = recipe.cfg_small2(lora_rank=0), 0.1, 3
    m = build(cfg, "fp32", dropout=p)
    x, y, _, _ = batches(cfg, B)
    r = m.runner()
    r.drop_calls = 41
    logits, _ = ce_backward(m, x, y)
    seed, T = (r.drop_seed << 20) + 42, m.num_tokens
    mask = lambda n, site: ops.dropout_mask(n, p, seed, site, "cuda").cpu().float() / (1 - p)

    def keep(i, width, site):      # the last block runs on the cls rows only: its counters index a compact [B, width] tensor
        if i < cfg["depth"] - 1:
            return mask(B * T * width, site).reshape(B, T, width)
        full = torch.ones(B, T, width)
        full[:, 0] = mask(B * width, site).reshape(B, width)
        return full
    names = [n for n, q in m.named_parameters() if q.requires_grad]
    want_logits, want = oracle_grads(state_of(cfg), x, y, cfg, names, keep=keep)
    assert (logits.cpu() - want_logits).abs().max() <= 1e-4
    got = grads_of(m)
    for n in names:
        assert bar_ok(got[n], want[n], f"dropout {n}"), n


def test_vits_face_trains_its_ffn_weights():
    cfg, vits = recipe.cfg_small2(lora_rank=0), (12, 4)
    m = build(cfg, "fp32", vits=vits)
    x, y, _, _ = batches(cfg, 3)
    logits, _ = ce_backward(m, x, y)
    names = [n for n, p in m.named_parameters() if p.requires_grad]
    assert len(names) == 13
    want_logits, want = oracle_grads(state_of(cfg, vits[0]), x, y, cfg, names, vits=vits)
    assert (logits.cpu() - want_logits).abs().max() <= 1e-4
    got = grads_of(m)
    for n in names:
        assert bar_ok(got[n], want[n], f"ViTs_face {n}"), n


def test_a_second_backward_without_zero_grad_doubles_the_gradients():
    cfg = recipe.cfg_small2(lora_rank=0)
    m = build(cfg, "fp32")
    x, y, _, _ = batches(cfg, 3)
    ce_backward(m, x, y)
    first = {n: p.grad.clone() for n, p in m.named_parameters() if p.requires_grad}
    ce_backward(m, x, y)
    for n, p in m.named_parameters():
        if p.requires_grad:
            assert torch.equal(p.grad, first[n] + first[n]), n
    m.zero_grad()
    ce_backward(m, x, y)
    for n, p in m.named_parameters():
        if p.requires_grad:
            assert torch.equal(p.grad, first[n]), n      # the same bits on every call


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_the_forward_after_a_step_uses_the_new_weights(mode):
    """The optimizer writes through raw pointers and bumps _version: the 16-bit [N, K] / [K, N] operand copies of W1 and W2 are re-made by the
    runner's existing cache keys. The logits move, and they are those of a freshly built model loaded with the updated state."""
    from gslora_hip.optim import create_optimizer
    cfg = recipe.cfg_small2(lora_rank=0)
    m = build(cfg, mode)
    opt = create_optimizer(SimpleNamespace(opt="adamw", lr=1e-2, weight_decay=0.05, opt_eps=1e-8, opt_betas=None), m)
    x, y, _, _ = batches(cfg, 3)
    w = m.transformer.layers[0][1].fn.fn.net[0].weight
    v0 = w._version
    before, _ = ce_backward(m, x, y)
    opt.step()
    assert w._version > v0
    with torch.no_grad():
        after, _ = m(x, y)
    assert (after - before).abs().max() > 1e-3
    fresh = build(cfg, mode, state={n: v.detach().cpu().clone() for n, v in m.state_dict().items()})
    with torch.no_grad():
        again, _ = fresh(x, y)
    assert torch.equal(after, again)
    # ... and the backward's transposed copies too: the gradients of the next step are the fresh model's
    m.zero_grad()
    ce_backward(m, x, y)
    ce_backward(fresh, x, y)
    for (n, a), (_, b) in zip(m.named_parameters(), fresh.named_parameters()):
        if a.requires_grad:
            assert torch.equal(a.grad, b.grad), n


# ---------------------------------------------------------------------------------------------------------------- the step
def l2_terms(m):
    """train_own_forget_cl.py:1416-1440: the task's weights and the identity importance."""
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    return {0: {"importance": {n: p.clone().detach().fill_(1) for n, p in named}, "task_param": {n: p.clone().detach() for n, p in named}}}


def test_ffn_reg_step_three_steps_match_the_reference_engine(golden_dir):
    from gslora_hip.optim import create_optimizer
    from gslora_hip.step import ffn_reg_step
    g = np.load(os.path.join(golden_dir, "ffn_l2_small_engine.npz"))
    cfg = recipe.cfg_small(lora_rank=0)
    m = build(cfg, "fp32")
    assert [n for n, p in m.named_parameters() if p.requires_grad] == g["trainable"].tolist()
    frozen = {n: p.detach().clone() for n, p in m.named_parameters() if not p.requires_grad}
    opt = create_optimizer(SimpleNamespace(opt="adamw", lr=float(g["hyper_lr"]), weight_decay=float(g["hyper_wd"]), opt_eps=1e-8, opt_betas=None), m)
    terms, lam, crit = l2_terms(m), float(g["reg_lambda"]), torch.nn.CrossEntropyLoss()
    for s in range(3):
        xr, yr, xf, yf = batches(cfg, 2, s)
        x, y = torch.cat((xr, xf)), torch.cat((yr, yf))
        assert y.cpu().tolist() == g[f"y{s + 1}"].tolist()
        meters = ffn_reg_step(m, opt, crit, x, y, regularization_terms=terms, reg_lambda=lam)
        assert meters.shape == (4,) and meters.is_cuda
        ce, reg, total, prec1 = meters.tolist()
        print(f"step {s + 1}: CE {ce:.6f} vs {g['losses'][s][0]:.6f}, reg {reg:.6f} vs {g['losses'][s][1]:.6f}, total {total:.6f} vs {g['losses'][s][2]:.6f}")
        for got, want in zip((ce, reg, total), g["losses"][s]):
            assert abs(got - want) <= 1e-4 * max(1.0, abs(want))
        assert prec1 == g["prec1"][s]
    for n, p in m.named_parameters():
        if p.requires_grad:
            err = np.abs(p.detach().cpu().numpy() - g[f"final::{n}"]).max()
            print(f"after step 3 {n}: err {err:.3e}")
            assert err <= 1e-4, n
        else:
            assert torch.equal(p.detach(), frozen[n]) and p.grad is None, n


def test_get_reg_loss_keeps_the_reference_signature_and_meaning():
    import engine_cl
    cfg = recipe.cfg_small(lora_rank=0)
    m = build(cfg, "fp32")
    dev = torch.device("cuda")
    zero = engine_cl.get_reg_loss(m, None, 3.0, dev)
    assert zero.dim() == 0 and zero.item() == 0.0
    terms = l2_terms(m)
    g = torch.Generator().manual_seed(3)
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    for n, p in named:      # move the task's weights away, give every element its own importance
        terms[0]["task_param"][n] = p.detach() + 0.1 * torch.randn(p.shape, generator=g).cuda()
        terms[0]["importance"][n] = torch.rand(p.shape, generator=g).cuda()
    terms[1] = l2_terms(m)[0]
    for n, p in named:
        terms[1]["task_param"][n] = p.detach() - 0.05
    loss = engine_cl.get_reg_loss(m, terms, 0.5, dev)
    ref = sum((t["importance"][n].double() * (p.detach().double() - t["task_param"][n].double()) ** 2).sum() for t in terms.values() for n, p in named)
    assert loss.dim() == 0 and abs(loss.item() - 0.5 * ref.item()) <= 1e-5 * ref.item()
    (loss * 2.0).backward()
    for n, p in named:
        want = sum(2.0 * 0.5 * 2.0 * t["importance"][n] * (p.detach() - t["task_param"][n]) for t in terms.values())
        assert (p.grad - want).abs().max() <= 1e-5 * want.abs().max(), n


def test_head_and_ffn_train_together_and_ffn_alone():
    from gslora_hip.optim import create_optimizer
    from gslora_hip.step import ffn_reg_step
    cfg = recipe.cfg_small2(lora_rank=0)
    x, y, _, _ = batches(cfg, 3)
    args = SimpleNamespace(opt="adamw", lr=1e-2, weight_decay=0.05, opt_eps=1e-8, opt_betas=None)
    both, alone = build(cfg, "fp32", head=True), build(cfg, "fp32", head=False)
    ce_backward(both, x, y)
    ce_backward(alone, x, y)
    assert both.loss.weight.grad is not None and alone.loss.weight.grad is None
    for (n, a), (_, b) in zip(both.named_parameters(), alone.named_parameters()):
        if b.requires_grad:
            assert torch.equal(a.grad, b.grad), n      # the FFN gradients do not depend on whether the head trains
    for m, head in ((both, True), (alone, False)):
        w0, f0 = m.loss.weight.detach().clone(), m.transformer.layers[1][1].fn.fn.net[3].bias.detach().clone()
        ffn_reg_step(m, create_optimizer(args, m), torch.nn.CrossEntropyLoss(), x, y)
        assert torch.equal(m.loss.weight.detach(), w0) != head
        assert not torch.equal(m.transformer.layers[1][1].fn.fn.net[3].bias.detach(), f0)
