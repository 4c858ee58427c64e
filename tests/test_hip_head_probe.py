"""GPU tests of the linear probe: gsl_head_wgrad against torch autograd (float64, CPU), the models with a trainable head against the REAL
reference (tests/golden/head_probe_*.npz, head_open_small2_b3.npz — tools/make_golden_head_probe.py), the head-only step that keeps nothing
of the blocks, the 16-bit modes, HIP-graph replay of head_probe_step, ViTs_face and the driver.

Gradient bar of the project: |err| <= 1e-4 * max(1, |g|) elementwise (f32 mode). The random op-test shapes are the issue's: at B <= 130
torch's own f32 autograd stays below 0.17 of that bar, so it has a 6x margin over f32 rounding there."""
import copy
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import recipe

pytestmark = pytest.mark.gpu

SHAPES = [(1, 5, 64), (3, 23, 192), (65, 100, 512), (130, 257, 1024), (7, 1100, 64)]
# (name, ops kind, ArcFace margin, easy_margin, bias). The ArcFace margin of the plain variant is 1.5: th = cos(pi - 1.5) = -0.07 puts random
# label cosines on both sides of the threshold (with the default 0.5, th = -0.88, a random cosine never falls below it).
KINDS = [("cosface", "cosface", 0.35, False, False), ("arcface", "arcface", 1.5, False, False), ("arcface_easy", "arcface", 0.5, True, False),
         ("linear_bias", "linear", 0.0, False, True), ("linear", "linear", 0.0, False, False)]
S = 64.0


def bar_ok(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"{what}: max err / bar = {err.max() / 1e-4:.4f}")
    return err.max() <= 1e-4


def op_inputs(B, C, D, seed):
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn(B, D, generator=g)
    bound = math.sqrt(6.0 / (C + D))      # xavier_uniform_, as the heads initialise their weight
    W = (torch.rand(C, D, generator=g) * 2 - 1) * bound
    dl = torch.randn(B, C, generator=g)
    label = torch.randint(0, C, (B,), generator=g)
    return emb, W, dl, label


def arc_constants(m):
    return math.cos(m), math.sin(m), math.cos(math.pi - m), math.sin(math.pi - m) * m


def reference_wgrad(kind, emb, W, dl, label, cos_y32, m, easy, bias):
    """torch autograd in float64 on the CPU. The ArcFace branch of each sample is the one the f32 label cosine selects (the kernel's rule:
    the comparison the forward made), so a cosine that rounds across the threshold cannot split the two."""
    W = W.double().requires_grad_(True)
    emb, dl = emb.double(), dl.double()
    b = torch.zeros(W.shape[0], dtype=torch.float64, requires_grad=True) if bias else None
    if kind == "linear":
        logits = F.linear(emb, W, b)
    else:
        cos = F.linear(F.normalize(emb), F.normalize(W))
        onehot = F.one_hot(label, W.shape[0]).double()
        if kind == "cosface":
            logits = S * (cos - m * onehot)
        else:
            cos_m, sin_m, th, mm = arc_constants(m)
            sine = torch.sqrt((1.0 - cos * cos).clamp(min=0.0))
            phi = cos * cos_m - sine * sin_m
            above = (cos_y32 > (torch.tensor(0.0) if easy else torch.tensor(th, dtype=torch.float64).float()))[:, None]
            phi = torch.where(above, phi, cos if easy else cos - mm)
            logits = S * (onehot * phi + (1.0 - onehot) * cos)
    (logits * dl).sum().backward()
    return W.grad, (b.grad if bias else None)


def label_cosines(emb, W, label):
    cos = F.linear(F.normalize(emb.double()), F.normalize(W.double()))
    return cos[torch.arange(emb.shape[0]), label].float()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("case", KINDS, ids=lambda k: k[0])
def test_head_wgrad_matches_float64_autograd(shape, case):
    from gslora_hip import ops
    name, kind, m, easy, bias = case
    B, C, D = shape
    emb, W, dl, label = op_inputs(B, C, D, seed=B * 1000 + C)
    cos_y = label_cosines(emb, W, label)
    want_w, want_b = reference_wgrad(kind, emb, W, dl, label, cos_y, m, easy, bias)
    dev = lambda t: t.cuda().contiguous()
    kw = dict(cos_s=S, m=m, easy_margin=easy, label=dev(label), cos_y=dev(cos_y), bias=bias)
    # every element is written: the output buffers start as NaN
    dW = torch.full((C, D), float("nan"), device="cuda")
    db = torch.full((C,), float("nan"), device="cuda") if bias else None
    got_w, got_b = ops.head_wgrad(dev(dl), dev(emb), dev(W), kind, dW=dW, dbias=db, **kw)
    assert got_w is dW and not torch.isnan(dW).any()
    assert bar_ok(got_w.cpu(), want_w, f"{name} {shape} dW")
    assert (got_b is not None) == bias      # dbias exists for the biased linear head only
    if bias:
        assert got_b is db and not torch.isnan(db).any() and bar_ok(got_b.cpu(), want_b, f"{name} {shape} dbias")
    # a second call, into fresh buffers: the same bits (the order of the sum over b is fixed by the shape)
    again_w, again_b = ops.head_wgrad(dev(dl), dev(emb), dev(W), kind, **kw)
    assert torch.equal(again_w, got_w) and (not bias or torch.equal(again_b, got_b))
    if kind == "arcface":
        th = 0.0 if easy else arc_constants(m)[2]
        if B >= 65:
            assert (cos_y > th).any() and (cos_y < th).any(), "the case exercises both branches of phi"


@pytest.mark.parametrize("kind", ["cosface", "arcface"])
def test_head_wgrad_zero_weight_row_follows_the_clamp_derivative(kind):
    from gslora_hip import ops
    B, C, D = 9, 7, 128
    emb, W, dl, label = op_inputs(B, C, D, seed=5)
    W[3] = 0.0
    label[0] = 3      # the zero row is also a label row (its cosine is 0)
    cos_y = label_cosines(emb, W, label)
    want, _ = reference_wgrad(kind, emb, W, dl, label, cos_y, 0.5, False, False)
    got, _ = ops.head_wgrad(dl.cuda(), emb.cuda(), W.cuda(), kind, cos_s=S, m=0.5, label=label.cuda(), cos_y=cos_y.cuda())
    got = got.cpu().double()
    assert torch.isfinite(got).all() and got[3].abs().max() > 1e9      # d What / 1e-12, no projection term
    # within 1e-4 relative of torch's, element by element. The floor: an element is a sum of B = 9 f32 products of size up to the row's
    # largest, so it carries an absolute rounding error of up to ~(B + 3) * 2^-24 = 7e-7 of that size whatever its own value; below a
    # hundredth of the row's largest the bound is therefore the absolute 1e-4 * 1e-2 = 1e-6 of it
    floor = 1e-2 * want[3].abs().max()
    err = (got[3] - want[3]).abs() / want[3].abs().clamp(min=floor)
    print(f"zero row {kind}: worst relative error {err.max().item():.3e} (bound 1e-4)")
    assert (err <= 1e-4).all()
    rest = [c for c in range(C) if c != 3]
    assert bar_ok(got[rest], want[rest], f"{kind} rows beside the zero row")


# ---------------------------------------------------------------------------------------------------------------- models
def head_state(cfg, head):      # = tools/make_golden_heads.py
    st = recipe.make_state(cfg)
    if head == "Softmax":
        st["loss.bias"] = recipe.uniform("loss.bias", (cfg["num_class"],), 1337, -0.5, 0.5)
    return st


def build(cfg, head="CosFace", dtype="fp32", dropout=0.0, train="head", weight=None):
    """train: "head" (train/backbone_forget_main.py:596-600), "lora" (mark_only_lora_as_trainable) or "both" (--ffn_open)."""
    from vit_pytorch_face import ViT_face
    m = ViT_face(loss_type=head, GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
                 dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], dropout=dropout, emb_dropout=dropout,
                 lora_rank=cfg["lora_rank"])
    st = {k: torch.tensor(v) for k, v in head_state(cfg, head).items()}
    if weight is not None:
        st["loss.weight"] = torch.tensor(weight)
    m.load_state_dict({k: v for k, v in st.items() if cfg["lora_rank"] > 0 or "lora_" not in k}, strict=True)
    set_trainable(m, train)
    return m.to("cuda").set_compute_dtype(dtype).train()


def set_trainable(m, train):
    for n, p in m.named_parameters():
        p.requires_grad = ("loss" in n and train in ("head", "both")) or ("lora_" in n and train in ("lora", "both"))


def batches(cfg, batch, s=0):      # = tools/make_golden_heads.batches
    nf = max(2, cfg["num_class"] // 5)
    mk = lambda a: torch.tensor(a).cuda()
    return (mk(recipe.make_images(cfg, batch, seed=100 + s, tag="xr")),
            mk(recipe.make_labels(cfg, batch, seed=100 + s, tag="yr", lo=0, hi=cfg["num_class"] - nf)),
            mk(recipe.make_images(cfg, batch, seed=200 + s, tag="xf")),
            mk(recipe.make_labels(cfg, batch, seed=200 + s, tag="yf", lo=cfg["num_class"] - nf, hi=cfg["num_class"])))


def probe_forward_backward(m, x, y):
    """backbone_forget_main.py:657-669 on the HIP kernels. -> (logits, loss, prec1)"""
    from gslora_hip import losses
    logits, _ = m(x, y)
    ce, hits = losses.ce_sum_top1(logits, y)
    loss = ce / x.shape[0]
    m.zero_grad()
    loss.backward()
    # train_accuracy (util/utils.py:354-368): the hit count times 100 / batch, in f32
    return logits.detach().cpu().numpy(), loss.item(), float(np.float32(hits.item()) * np.float32(100.0 / x.shape[0]))


@pytest.mark.parametrize("head", ["CosFace", "ArcFace", "Softmax"])
def test_model_head_gradients_match_the_reference(golden_dir, head):
    g = np.load(os.path.join(golden_dir, f"head_probe_small2_{head.lower()}_b3.npz"))
    cfg = recipe.cfg_small2()
    m = build(cfg, head, weight=g["state::loss.weight"] if head == "ArcFace" else None)
    x, y, _, _ = batches(cfg, 3)
    assert y.cpu().tolist() == g["y"].tolist()
    for prefix, easy in [("", False)] + ([("easy_", True)] if head == "ArcFace" else []):
        if head == "ArcFace":
            m.loss.easy_margin = easy
        logits, loss, prec1 = probe_forward_backward(m, x, y)
        print(f"{head} {prefix}: logits err {np.abs(logits - g[prefix + 'logits']).max():.3e}, loss err {abs(loss - float(g[prefix + 'loss'])):.3e}")
        assert np.abs(logits - g[prefix + "logits"]).max() <= 1e-4
        assert abs(loss - float(g[prefix + "loss"])) <= 1e-4
        assert prec1 == float(g[prefix + "prec1"])
        names = [n for n, p in m.named_parameters() if p.grad is not None]
        assert names == (["loss.weight", "loss.bias"] if head == "Softmax" else ["loss.weight"])
        for n in names:
            assert bar_ok(dict(m.named_parameters())[n].grad.cpu(), g[f"{prefix}grad::{n}"], f"{head} {prefix}{n}")


def test_probe_trajectory_matches_the_reference(golden_dir):
    from gslora_hip.optim import create_optimizer
    from gslora_hip.step import head_probe_step
    g = np.load(os.path.join(golden_dir, "head_probe_small6_engine.npz"))
    cfg = recipe.cfg_small6()
    m = build(cfg, "CosFace")
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    opt = create_optimizer(SimpleNamespace(opt="adamw", lr=float(g["hyper_lr"]), weight_decay=float(g["hyper_wd"]), opt_eps=1e-8, opt_betas=None), m)
    crit = torch.nn.CrossEntropyLoss()
    for s in range(3):
        xr, yr, xf, yf = batches(cfg, 2, s)
        x, y = torch.cat((xr, xf)), torch.cat((yr, yf))
        assert y.cpu().tolist() == g[f"y{s + 1}"].tolist()
        meters = head_probe_step(m, opt, crit, x, y)
        assert meters.shape == (2,) and meters.is_cuda
        err = (m.loss.weight.detach().cpu().numpy() - g[f"weight{s + 1}"])
        loss, prec1 = meters.tolist()
        print(f"step {s + 1}: weight err {np.abs(err).max():.3e}, loss {loss:.6f} vs {g['losses'][s]:.6f}, prec1 {prec1} vs {g['prec1'][s]}")
        assert np.abs(err).max() <= 1e-4
        assert abs(loss - g["losses"][s]) <= 1e-4 * max(1.0, abs(g["losses"][s])) and prec1 == g["prec1"][s]
    for n, p in m.named_parameters():
        if n != "loss.weight":
            assert torch.equal(p.detach(), before[n]), f"{n} changed"
            assert p.grad is None, f"{n} has a gradient"
    assert not torch.equal(m.loss.weight.detach(), before["loss.weight"])


def total_loss(model, cfg, xr, yr, xf, yf, hy, proto):      # = tools/make_golden_heads.total_loss on the HIP losses
    import engine
    import engine_cl
    from gslora_hip import losses
    lo_r, em_r = model(xr, yr)
    lo_f, em_f = model(xf, yf)
    ce_r = losses.ce_sum_top1(lo_r, yr)[0] / xr.shape[0]
    ce_f = losses.ce_sum_top1(lo_f, yf)[0] / xf.shape[0]
    sl = engine.get_structure_loss(model, num_layers=cfg["depth"], group_type="block", group_pos="FFN")
    kl_f = engine_cl.get_prototype_loss(em_f, yf, proto)
    kl_r = engine_cl.get_prototype_loss(em_r, yr, proto)
    return (hy["beta"] * torch.relu(hy["BND"] - ce_f) + ce_r + hy["alpha"] * sl
            + hy["pro_f_weight"] * torch.relu(hy["BND_pro"] - kl_f) + hy["pro_r_weight"] * kl_r)


HYPER = dict(lr=1e-2, wd=0.05, beta=0.15, alpha=1e-2, BND=105.0, BND_pro=2.0, pro_f_weight=0.05, pro_r_weight=0.1)      # = oracle/make_golden.HYPER


def test_head_and_lora_together(golden_dir):
    g = np.load(os.path.join(golden_dir, "head_open_small2_b3.npz"))
    cfg = recipe.cfg_small2()
    xr, yr, xf, yf = batches(cfg, 3)
    proto = {c: torch.tensor(v).cuda() for c, v in enumerate(recipe.make_prototypes(cfg))}
    grads = {}
    for train in ("both", "lora", "head"):
        m = build(cfg, "CosFace", train=train)
        total = total_loss(m, cfg, xr, yr, xf, yf, HYPER, proto)
        m.zero_grad()
        total.backward()
        grads[train] = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    lora_names = [n for n in grads["both"] if "lora_" in n]
    assert len(lora_names) == 4 * cfg["depth"] and set(grads["both"]) == set(lora_names) | {"loss.weight"}
    assert set(grads["lora"]) == set(lora_names) and set(grads["head"]) == {"loss.weight"}
    for n in grads["both"]:
        assert bar_ok(grads["both"][n].cpu(), g[f"grad1::{n}"], n)
    for n in lora_names:      # the head's one extra launch leaves the LoRA chain alone
        assert torch.equal(grads["both"][n], grads["lora"][n]), n
    # ... and the head's gradient is the head-only one: the same dlogits (f32, no dropout), the same kernel, the same accumulation
    assert torch.equal(grads["both"]["loss.weight"], grads["head"]["loss.weight"])


def test_head_only_step_skips_the_backbone():
    cfg = recipe.cfg_small2()
    x, y, _, _ = batches(cfg, 32)
    # (a) no LoRA at all: no bucket, and backward() succeeds
    m0 = build(dict(cfg, lora_rank=0), "CosFace")
    probe_forward_backward(m0, x, y)
    assert m0.runner().bucket is None and torch.isfinite(m0.loss.weight.grad).all() and m0.loss.weight.grad.abs().max() > 0
    # (b) fp16 with frozen LoRA: a LoRA step first creates the loss-scale state, the head-only step leaves it alone
    m = build(cfg, "CosFace", dtype="fp16", dropout=0.1, train="lora")

    def peak_of_step():
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        probe_forward_backward(m, x, y)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    peak_of_step()      # warm-up: operand caches, bucket, packs
    peak_lora = peak_of_step()
    gscale = m.runner().gscale.clone()
    assert gscale[0] > 0 and 4 <= gscale[3] <= 15
    lora_grad = m.lora_bucket().grad.clone()
    set_trainable(m, "head")
    m.zero_grad()
    peak_of_step()      # warm-up of the head-only form
    peak_head = peak_of_step()
    assert torch.equal(m.runner().gscale, gscale), "the head-only step touched the loss-scale / overflow-guard state"
    assert torch.equal(m.lora_bucket().grad, lora_grad) and torch.isfinite(m.loss.weight.grad).all()
    # a condition on the saved activations: any block tensor kept by the head-only forward would put its peak at the LoRA step's
    print(f"peak bytes of a step beyond the resident state: LoRA {peak_lora}, head only {peak_head}")
    assert peak_head < peak_lora


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_16_bit_modes_within_the_declared_tolerance(dtype):
    cfg = recipe.cfg_small2()
    x, y, _, _ = batches(cfg, 64)
    out = {}
    for dt in ("fp32", dtype):
        m = build(cfg, "CosFace", dtype=dt)
        logits, _, _ = probe_forward_backward(m, x, y)
        out[dt] = (logits, m.loss.weight.grad.double().flatten())
    ref, got = out["fp32"][1], out[dtype][1]
    rel = ((got - ref).norm() / ref.norm()).item()
    cos = (torch.dot(got, ref) / (got.norm() * ref.norm())).item()
    dlog = np.abs(out[dtype][0] - out["fp32"][0]).max()
    print(f"{dtype} vs fp32 at batch 64: head gradient rel Frobenius {rel:.5f}, cosine {cos:.6f}, logits max abs {dlog:.4f}")
    assert rel <= 0.06 and cos > 0.995 and dlog <= 0.25      # the declared tolerance of the speed modes


def test_graph_replay_equals_eager_steps():
    from gslora_hip.optim import create_optimizer
    from gslora_hip.step import head_probe_step
    cfg = recipe.cfg_small2()
    args = SimpleNamespace(opt="adamw", lr=1e-2, weight_decay=0.05, opt_eps=1e-8, opt_betas=None)
    crit = torch.nn.CrossEntropyLoss()
    data = [(torch.cat(b[0::2]), torch.cat(b[1::2])) for b in (batches(cfg, 4, s) for s in range(4))]
    runs = {}
    for mode in ("eager", "graph"):
        torch.manual_seed(4321)      # the runner derives its dropout stream from torch's seed
        m = build(cfg, "CosFace", dtype="fp16", dropout=0.1)
        opt = create_optimizer(args, m)
        meters = [head_probe_step(m, opt, crit, *data[0])]      # both: one eager step (operand caches, optimizer state)
        if mode == "eager":
            meters += [head_probe_step(m, opt, crit, x, y) for x, y in data[1:]]
        else:
            r = m.runner()
            xs, ys = data[1][0].clone(), data[1][1].clone()
            seed_dev = torch.zeros(1, device="cuda", dtype=torch.int64)
            opt.graph_sync()
            calls0 = r.drop_calls
            torch.cuda.synchronize()
            opt.graph_mode, r.seed_dev = True, seed_dev
            graph = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(graph, capture_error_mode="thread_local"):
                    static_out = head_probe_step(m, opt, crit, xs, ys)
            finally:
                opt.graph_mode, r.seed_dev = False, None
            nfwd, r.drop_calls = r.drop_calls - calls0, calls0      # nothing ran during the capture
            assert nfwd == 1
            for x, y in data[1:]:
                xs.copy_(x)
                ys.copy_(y)
                opt.graph_sync()
                seed_dev.fill_((r.drop_seed << 20) + r.drop_calls)
                graph.replay()
                r.drop_calls += nfwd
                opt.graph_replayed()
                meters.append(static_out.clone())
        runs[mode] = (torch.stack(meters).cpu(), m.loss.weight.detach().clone().cpu())
    assert torch.isfinite(runs["eager"][0]).all()
    assert torch.equal(runs["eager"][0], runs["graph"][0]), "meters differ"
    assert torch.equal(runs["eager"][1], runs["graph"][1]), "loss.weight differs"


def test_vits_face_head_gradient_is_the_op():
    from gslora_hip import ops
    from vit_pytorch_face import ViTs_face
    cfg = recipe.cfg_small2()
    torch.manual_seed(7)
    m = ViTs_face(loss_type="ArcFace", GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
                  ac_patch_size=12, pad=4, dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"],
                  lora_rank=cfg["lora_rank"])
    set_trainable(m, "head")
    m = m.to("cuda").set_compute_dtype("fp32").train()
    x, y, _, _ = batches(cfg, 5)
    logits, emb = m(x, y)
    dl = torch.randn(logits.shape, generator=torch.Generator().manual_seed(3)).cuda()
    logits.backward(dl)
    cos_y = (F.linear(F.normalize(emb.detach()), F.normalize(m.loss.weight.detach())))[torch.arange(5), y]
    # the runner's own cos_y is what the node used; recompute the op from the forward's saved quantities through a second forward
    with torch.no_grad():
        _, emb2, saved = m.runner().forward(x, y, save="head")
    assert torch.equal(emb2, emb.detach()) and torch.allclose(saved["cos_y"], cos_y, atol=1e-5)
    want, _ = ops.head_wgrad(dl, emb.detach().contiguous(), m.loss.weight.detach(), "arcface", cos_s=m.loss.s, m=m.loss.m,
                             easy_margin=m.loss.easy_margin, label=y, cos_y=saved["cos_y"])
    assert torch.equal(m.loss.weight.grad, want)


def test_driver_probe_record(tmp_path):
    import driver_cl
    argv = ["--small", "--num_class", "10", "--num_tasks", "1", "--per_forget_cls", "3", "--epochs", "1", "--batch_size", "16",
            "--samples_per_class", "4", "--dtype", "fp32", "--dropout", "0.0"]
    parent_keys = {"task", "steps", "lrs", "hypers", "norms", "total_loss", "forget_before", "forget_after", "remain_before", "remain_after",
                   "ema_acc", "ema_accs", "forget_cls"}
    off, _, _ = driver_cl.main(argv + ["--outdir", str(tmp_path / "off")])
    assert set(off[0]) == parent_keys      # without the flag the record is the parent commit's
    on, _, model = driver_cl.main(argv + ["--probe_epochs", "1", "--outdir", str(tmp_path / "on")])
    rec = on[0]
    assert set(rec) == parent_keys | {"probe"} and {k: rec[k] for k in parent_keys} == off[0]      # the probe runs on a copy, behind the tasks
    probe = rec["probe"]
    assert probe["trainable"] == ["loss.weight"] and probe["steps"] == 3 and len(probe["forget_acc"]) == len(probe["remain_acc"]) == 1
    for v in [probe["forget_before"], probe["remain_before"], *probe["forget_acc"], *probe["remain_acc"], *probe["losses"], *probe["top1"]]:
        assert math.isfinite(v)
    for v in [probe["forget_before"], probe["remain_before"], *probe["forget_acc"], *probe["remain_acc"]]:
        assert 0.0 <= v <= 100.0
    assert not model.loss.weight.requires_grad      # the driver's own model keeps its trainability
