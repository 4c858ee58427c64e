"""The l2 prototype distance (reference engine_cl.py:593-594: torch.mean((output - prototype_tensor) ** 2)) and precision@k
(util/utils.py:354-368) on the HIP path:
 (a) gsl_proto_l2_fwd / gsl_proto_l2_bwd against float64 torch, `accumulate`, a NaN table row;
 (b) gsl_loss_tail_l2 against the separate kernels: coefficients and gradients bit-identical, meters within one ulp;
 (c) the whole model in f32 against the real reference (tests/golden/proto_l2_small2_b3.npz, proto_l2_small6_engine.npz,
     tools/make_golden_proto_l2.py) at the bars of test_hip_model.py / test_hip_heads.py;
 (d) fp16 / bf16 against the path's own f32 mode within the bands of test_hip_bf16_pinned.py;
 (e) HIP-graph replay, the graph key, two data-parallel ranks;
 (f) train_accuracy(topk=...) against tests/golden/topk_small.npz."""
import copy
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import gslora_oracle as O
from oracle import recipe

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("losses_forget", "losses_remain", "losses_total", "losses_structure", "top1_forget", "top1_remain", "losses_prototype_forget",
         "losses_prototype_remain")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    from gslora_hip import _lib
    from gslora_hip import ops as _ops
    _lib.load()
    return _ops


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def ulps(a, b):
    """Largest distance between two finite f32 tensors of equal signs, in units in the last place."""
    ia, ib = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()
    return int((ia - ib).abs().max())


# ------------------------------------------------------------------------------------------------------------ (a) the kernel pair
@pytest.mark.parametrize("D", [128, 512, 768])
@pytest.mark.parametrize("B", [1, 3, 512])
def test_proto_l2_fwd_bwd_match_float64(ops, B, D):
    C = 37
    emb, table = rnd(B, D, seed=1).cuda(), rnd(C, D, seed=2, scale=1.5).cuda()
    y = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(3)).cuda()
    out = ops.proto_l2_fwd(emb, y, table)
    e64 = emb.double().requires_grad_(True)
    ref = ((e64 - table.double()[y]) ** 2).mean(1).sum()
    rel = abs(out.item() - ref.item()) / abs(ref.item())
    print(f"[proto_l2 B={B} D={D}] sum {out.item():.6f} ref {ref.item():.6f} rel {rel:.2e}")
    assert rel <= 1e-6
    coef = torch.tensor([0.37], device="cuda")
    g = ops.proto_l2_bwd(emb, y, table, coef, 1.5)
    (gref,) = torch.autograd.grad(ref * (0.37 * 1.5), e64)
    err = (g.double() - gref).abs().max().item() / gref.abs().max().item()
    print(f"[proto_l2 B={B} D={D}] gradient error / max|g| {err:.2e}")
    assert err <= 1e-6


def test_proto_l2_bwd_accumulates_and_a_missing_prototype_is_not_finite(ops):
    B, D, C = 5, 192, 7
    emb, table = rnd(B, D, seed=1).cuda(), rnd(C, D, seed=2).cuda()
    y = torch.tensor([0, 3, 6, 3, 1]).cuda()
    coef = torch.tensor([1.0], device="cuda")
    g = ops.proto_l2_bwd(emb, y, table, coef, 1.0)
    base = rnd(B, D, seed=5).cuda()
    acc = base.clone()
    ops.proto_l2_bwd(emb, y, table, coef, 1.0, demb=acc)      # a passed buffer is accumulated into by default, as in proto_kl_bwd
    assert torch.equal(acc, base + g)
    over = base.clone()
    ops.proto_l2_bwd(emb, y, table, coef, 1.0, demb=over, accumulate=False)
    assert torch.equal(over, g)
    # a class without a prototype is a NaN table row (losses.prototype_table): the sum, and so every meter, is not finite
    from gslora_hip import losses
    table_d = losses.prototype_table({c: table[c].cpu() for c in (0, 1, 6)}, torch.device("cuda"))
    assert table_d.shape == (7, D) and torch.isnan(table_d[3]).all()
    assert not torch.isfinite(ops.proto_l2_fwd(emb, y, table_d)).any()
    assert torch.isfinite(ops.proto_l2_fwd(emb[:1], y[:1], table_d)).all()
    gd = ops.proto_l2_bwd(emb, y, table_d, coef, 1.0)
    assert torch.isnan(gd[1]).all() and torch.isnan(gd[3]).all() and torch.equal(gd[[0, 2, 4]], g[[0, 2, 4]])
    # a label outside the table: NaN, and no out-of-bounds read
    y_out = torch.tensor([0, 7, -1, 3, 1]).cuda()
    assert torch.isnan(ops.proto_l2_fwd(emb, y_out, table)).all()
    go = ops.proto_l2_bwd(emb, y_out, table, coef, 1.0)
    assert torch.isnan(go[1]).all() and torch.isnan(go[2]).all() and torch.equal(go[[0, 3, 4]], g[[0, 3, 4]])


def test_proto_l2_nodes_are_differentiable_and_match_torch():
    import engine_cl
    from gslora_hip import losses
    B, D, C = 6, 128, 9
    table = rnd(C, D, seed=2).cuda()
    proto = {c: table[c].cpu() for c in range(C)}
    y = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(3)).cuda()
    emb = rnd(B, D, seed=1).cuda().requires_grad_(True)
    loss = engine_cl.get_prototype_loss(emb, y, proto, distance="l2")
    (g,) = torch.autograd.grad(loss * 3.0, emb)
    e2 = emb.detach().clone().requires_grad_(True)
    ref = torch.mean((e2 - table[y]) ** 2)      # the reference's expression
    (g2,) = torch.autograd.grad(ref * 3.0, e2)
    assert abs(loss.item() - ref.item()) <= 1e-6 * abs(ref.item()) and (g - g2).abs().max() <= 1e-6 * g2.abs().max()
    e3 = emb.detach().clone().requires_grad_(True)
    f, r = losses.proto_l2_sum_split(e3, y, table, 2)
    assert torch.equal(f, losses.proto_l2_sum(emb[2:], y[2:], table)) and torch.equal(r, losses.proto_l2_sum(emb[:2], y[:2], table))
    (g3,) = torch.autograd.grad(f / 4 * 3.0, e3)
    assert (g3[:2] == 0).all() and (g3[2:] - torch.autograd.grad(torch.mean((e2[2:] - table[y[2:]]) ** 2) * 3.0, e2)[0][2:]).abs().max() <= 1e-6 * g2.abs().max()
    assert engine_cl.get_prototype_loss(emb, y, proto, distance="euclidean") == 0.0


# ------------------------------------------------------------------------------------------------------------ (b) the one-launch tail
@pytest.mark.parametrize("N,nr,C,D,struct", [(8, 4, 100, 512, True), (96, 48, 100, 768, False), (37, 5, 12, 128, True), (256, 255, 100, 512, True),
                                             (19, 7, 1024, 1024, True), (17, 1, 65, 65, True), (5, 4, 1024, 1024, True)])
def test_loss_tail_l2_equals_the_separate_kernels(ops, N, nr, C, D, struct):
    """gsl_loss_tail_l2 against gsl_ce_fwd / gsl_proto_l2_fwd / gsl_loss_combine / gsl_ce_bwd / gsl_proto_l2_bwd on the two row ranges:
    every output bit-identical (one set of row functions and one scalar tail, csrc/loss.hip), for active and inactive hinges."""
    logits = (rnd(N, C, seed=1, scale=3.0)).cuda()
    labels = torch.randint(0, C, (N,), generator=torch.Generator().manual_seed(2)).cuda()
    emb, table = rnd(N, D, seed=3).cuda(), rnd(C, D, seed=4).cuda()
    st = torch.tensor(13.5, device="cuda") if struct else None
    for BND, BND_pro in ((105.0, 50.0), (0.5, 1e-4)):      # hinges active / inactive (the l2 mean of two unit normals is about 2)
        hyper = dict(beta=0.15, BND=BND, alpha=1e-2, w_f=0.05, w_r=0.1, BND_pro=BND_pro)
        total, meters, coefs, dl, de = ops.loss_tail_l2(logits, labels, nr, emb, table, st, **hyper)
        cr, cf = ops.ce_fwd(logits[:nr], labels[:nr]), ops.ce_fwd(logits[nr:], labels[nr:])
        kf, kr = ops.proto_l2_fwd(emb[nr:], labels[nr:], table)[0], ops.proto_l2_fwd(emb[:nr], labels[:nr], table)[0]
        t0, m0, c0 = ops.loss_combine(cr[0], cf[0], kf, kr, st, cr[1], cf[1], float(nr), float(N - nr), **hyper)
        assert (c0[2] != 0) == (BND_pro == 50.0)
        print(f"[loss_tail_l2 N={N} D={D} BND_pro={BND_pro}] total {ulps(total.reshape(1), t0.reshape(1))} ulp, meters {ulps(meters, m0)} ulp")
        assert torch.equal(coefs, c0) and torch.equal(total, t0) and torch.equal(meters, m0)
        dl0 = torch.empty_like(logits)
        ops.ce_bwd(logits[:nr], labels[:nr], c0[0:1].contiguous(), 1.0, dlogits=dl0[:nr], accumulate=False)
        ops.ce_bwd(logits[nr:], labels[nr:], c0[1:2].contiguous(), 1.0, dlogits=dl0[nr:], accumulate=False)
        assert torch.equal(dl, dl0)
        de0 = torch.empty_like(emb)
        ops.proto_l2_bwd(emb[:nr], labels[:nr], table, c0[3:4].contiguous(), 1.0, demb=de0[:nr], accumulate=False)
        ops.proto_l2_bwd(emb[nr:], labels[nr:], table, c0[2:3].contiguous(), 1.0, demb=de0[nr:], accumulate=False)
        assert torch.equal(de, de0)
    with pytest.raises(RuntimeError, match="prototype table"):
        ops.loss_tail_l2(logits, labels, nr, None, None, st, **hyper)
    # a NaN table row poisons total and meters here too
    bad = table.clone()
    bad[int(labels[0])] = float("nan")
    total, meters, _, _, _ = ops.loss_tail_l2(logits, labels, nr, emb, bad, st, **hyper)
    assert not torch.isfinite(total) and not torch.isfinite(meters).all()


def test_step_with_the_tail_equals_the_step_with_separate_kernels(monkeypatch):
    """gs_lora_step(proto_distance="l2") at a few-shot batch: LOSS_TAIL on (one launch) and off (the autograd nodes): same parameters, bit for bit."""
    from gslora_hip import step as S
    from gslora_hip.optim import FusedAdamW
    from test_hip_graph import batch, build
    cfg = recipe.cfg_small2()
    proto = torch.tensor(recipe.make_prototypes(cfg)).cuda()
    kw = dict(beta=0.15, alpha=1e-2, BND=105.0, use_structure=True, group_type="block", use_prototype=True, proto_table=proto,
              w_f=0.05, w_r=0.1, BND_pro=4.0, proto_distance="l2")
    res = []
    for tail in (True, False):
        monkeypatch.setattr(S, "LOSS_TAIL", tail)
        m = build(cfg, "fp32", 0.0)
        opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-2, weight_decay=0.05, eps=1e-8)
        packs = [S.gs_lora_step(m, opt, torch.nn.CrossEntropyLoss(), *batch(cfg, 4, s), **kw) for s in range(2)]
        res.append((packs, [p.detach().clone() for p in m.parameters() if p.requires_grad]))
    for a, b in zip(res[0][0], res[1][0]):
        assert ulps(a, b) <= 1 and a[6] > 0
    for a, b in zip(res[0][1], res[1][1]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ (c) against the reference
def hyper_of(g):
    return {k[len("hyper_"):]: float(g[k]) for k in g.files if k.startswith("hyper_")}


def total_loss_l2(model, cfg, xr, yr, xf, yf, hy, proto):
    """test_hip_heads.total_loss with distance="l2"."""
    import engine
    import engine_cl
    from gslora_hip import losses
    lo_r, em_r = model(xr, yr)
    lo_f, em_f = model(xf, yf)
    ce_r = losses.ce_sum_top1(lo_r, yr)[0] / xr.shape[0]
    ce_f = losses.ce_sum_top1(lo_f, yf)[0] / xf.shape[0]
    sl = engine.get_structure_loss(model, num_layers=cfg["depth"], group_type="block", group_pos=cfg.get("lora_pos", "FFN"))
    l2_f = engine_cl.get_prototype_loss(em_f, yf, proto, distance="l2")
    l2_r = engine_cl.get_prototype_loss(em_r, yr, proto, distance="l2")
    total = (hy["beta"] * torch.relu(hy["BND"] - ce_f) + ce_r + hy["alpha"] * sl
             + hy["pro_f_weight"] * torch.relu(hy["BND_pro"] - l2_f) + hy["pro_r_weight"] * l2_r)
    return total, [ce_f.item(), ce_r.item(), total.item(), sl.item(), l2_f.item(), l2_r.item()]


def test_model_f32_matches_reference(golden_dir):
    """Losses, LoRA gradients (prototype hinge active, then both hinges inactive) and group norms at the 1e-4 bar of test_hip_model.py."""
    from gslora_hip.losses import group_report
    from test_hip_heads import batches, build, head_state, lora_grads
    cfg = recipe.cfg_small2()
    g = np.load(os.path.join(golden_dir, "proto_l2_small2_b3.npz"))
    hy = hyper_of(g)
    m = build(cfg, "CosFace").train()
    xr, yr, xf, yf = batches(cfg, 3)
    with torch.no_grad():
        lo, em = m(xr, yr)
        assert np.abs(lo.cpu().numpy() - g["fwd_logits"]).max() < 1e-4
        assert np.abs(em.cpu().numpy() - g["fwd_emb"]).max() < 1e-4
    m.load_state_dict({k: torch.tensor(v) for k, v in head_state(cfg, "CosFace").items()})
    proto = {c: torch.tensor(v) for c, v in enumerate(recipe.make_prototypes(cfg))}
    total, got = total_loss_l2(m, cfg, xr, yr, xf, yf, hy, proto)
    print("[proto_l2 model] losses", got, "reference", g["losses1"].tolist())
    for a, r in zip(got, g["losses1"]):
        assert abs(a - r) < 1e-4 * max(1.0, abs(r)), (got, g["losses1"])
    assert got[4] < hy["BND_pro"]      # the prototype hinge is active: grad1 carries its gradient
    total.backward()
    for k, v in lora_grads(m).items():
        r = g[f"grad1::{k}"]
        assert np.abs(v - r).max() < 1e-4 * max(1.0, np.abs(r).max()), k
    rep = group_report(m, "block", tau=0.0)
    ref_norms = O.group_lasso_norms(O.to_torch(recipe.make_state(cfg)), cfg, "block")
    assert np.abs(rep["group_norm"].cpu().numpy() - ref_norms.numpy()).max() < 1e-4
    assert abs(float(rep["loss"][0]) - g["losses1"][3]) < 1e-4 * max(1.0, g["losses1"][3])
    for p in m.parameters():
        p.grad = None
    total, _ = total_loss_l2(m, cfg, xr, yr, xf, yf, dict(hy, BND=5.0, BND_pro=0.1), proto)      # both hinges inactive
    assert abs(total.item() - float(g["total_inactive"])) < 1e-4 * max(1.0, abs(float(g["total_inactive"])))
    total.backward()
    for k, v in lora_grads(m).items():
        r = g[f"grad_inactive::{k}"]
        assert np.abs(v - r).max() < 1e-4 * max(1.0, np.abs(r).max()), k


@pytest.mark.parametrize("graph", [False, "auto"])
def test_engine_three_steps_f32_match_reference(golden_dir, graph):
    """engine_cl.train_one_epoch with cfg PROTO_DISTANCE = "l2" + FusedAdamW on cfg_small6 against the reference's engine with its
    prototype loss bound to distance="l2": the bars of test_hip_heads.test_arcface_engine_three_steps_f32_match_reference."""
    import engine_cl
    from gslora_hip.optim import FusedAdamW
    from test_hip_heads import batches, build, head_state, lora_grads
    from util.utils import AverageMeter
    cfg, b = recipe.cfg_small6(), 2
    g = np.load(os.path.join(golden_dir, "proto_l2_small6_engine.npz"))
    hy = hyper_of(g)
    m = build(cfg, "CosFace")
    opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=hy["lr"], weight_decay=hy["wd"], eps=1e-8)
    meters = {k: AverageMeter() for k in NAMES}
    proto = {c: torch.tensor(v) for c, v in enumerate(recipe.make_prototypes(cfg))}
    cfgd = {"DATA_ROOT": "./data/casia100/", "BND_pro": hy["BND_pro"], "MULTI_GPU": False, "WORK_PATH": "/tmp", "BACKBONE_NAME": "VIT",
            "PROTO_DISTANCE": "l2", "HIP_GRAPH": graph}
    batch_ctr, track = 0, None
    for s in range(3):
        xr, yr, xf, yf = batches(cfg, b, s)
        ret = engine_cl.train_one_epoch(
            model=m, dataloader_forget=[(xf.cpu(), yf.cpu())], dataloader_remain=[(xr.cpu(), yr.cpu())], device=torch.device("cuda"),
            criterion=torch.nn.CrossEntropyLoss(), optimizer=opt, epoch=0, beta=hy["beta"], alpha=hy["alpha"], BND=hy["BND"],
            batch=batch_ctr, testloader_forget=None, testloader_remain=None, forget_acc_before=0.0, highest_H_mean=0.0, cfg=cfgd,
            task_i="0", use_prototype=True, prototype_dict=proto, prototype_weight_forget=hy["pro_f_weight"],
            prototype_weight_remain=hy["pro_r_weight"], **meters)
        batch_ctr = ret[0]
        got = np.array([meters[k].val for k in NAMES])
        print(f"[proto_l2 engine step {s}] meters", got.tolist())
        assert np.abs(got - g[f"meters{s + 1}"]).max() < 1e-3, (s, got, g[f"meters{s + 1}"])
        assert got[6] > 0      # the prototype hinge is active in every step
        g_hip = {n: torch.tensor(v) for n, v in lora_grads(m).items()}
        if s == 0:
            for k, v in g_hip.items():
                r = g[f"grad1::{k}"]
                assert np.abs(v.numpy() - r).max() < 1e-4 * max(1.0, np.abs(r).max()), k
            track = {n: (torch.tensor(head_state(cfg, "CosFace")[n]), torch.zeros_like(v), torch.zeros_like(v)) for n, v in g_hip.items()}
        params = {n: p.detach().cpu() for n, p in m.named_parameters() if p.requires_grad}
        for n in g_hip:      # the HIP AdamW on the HIP gradients = the oracle's AdamW on the same gradients
            track[n] = O.adamw_update(*track[n][:1], g_hip[n], *track[n][1:], s + 1, hy["lr"], hy["wd"])
            assert (params[n] - track[n][0]).abs().max() < 2e-6, (s, n)
        if s in (0, 2):      # against the reference's parameters (AdamW is ill-conditioned where |g| ~ eps: bounded, not pinned)
            for n, p in params.items():
                diff = np.abs(p.numpy() - g[f"param{s + 1}::{n}"])
                well = np.abs(g[f"grad1::{n}"]) > 1e-6
                if s == 0:
                    assert diff[well].max(initial=0.0) < 2e-4, n
                else:
                    assert np.mean(diff < 1e-3) > 0.99, n
                assert diff.max() <= 2.05 * hy["lr"] * (s + 1), n
    assert np.abs(np.array([meters[k].avg for k in NAMES]) - g["meters3_avg"]).max() < 2e-3
    assert batch_ctr == int(g["batch_ctr"])


# ------------------------------------------------------------------------------------------------------------ (d) the speed modes
@pytest.mark.parametrize("mode16", ["bf16", "fp16"])
def test_full_model_speed_mode_vs_f32_batch64_l2(mode16):
    """test_hip_bf16_pinned.test_full_model_speed_mode_vs_f32_batch64 with the l2 distance in the place of the KL: the same model, batch,
    weights and the same declared bands (VS_F32_BAND)."""
    import loralib as lora
    from gslora_hip import losses
    from test_hip_bf16_pinned import VS_F32_BAND
    from vit_pytorch_face import ViT_face
    torch.manual_seed(0)
    B = 64
    m = ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=100, image_size=112, patch_size=8, dim=512, depth=6, heads=8, mlp_dim=2048,
                 dropout=0.0, emb_dropout=0.0, lora_rank=8)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "lora_B" in n:
                p.normal_(0, 0.02)
    lora.mark_only_lora_as_trainable(m)
    m = m.cuda().train()
    gen = torch.Generator().manual_seed(5)
    x = torch.rand(2 * B, 3, 112, 112, generator=gen).cuda()
    y = torch.randint(0, 100, (2 * B,), generator=gen).cuda()
    proto = torch.randn(100, 512, generator=gen).cuda()
    res = {}
    for mode in ("fp32", mode16):
        mm = copy.deepcopy(m).set_compute_dtype(mode)
        lo, em = mm(x, y)
        ce_r = losses.ce_sum_top1(lo[:B], y[:B])[0] / B
        ce_f = losses.ce_sum_top1(lo[B:], y[B:])[0] / B
        l2 = losses.proto_l2_sum(em[:B], y[:B], proto) / B
        total = 0.15 * torch.relu(105.0 - ce_f) + ce_r + 1e-4 * losses.structure_loss(mm, "block") + 0.05 * l2
        total.backward()
        res[mode] = (lo.detach().float(), em.detach().float(), torch.cat([p.grad.reshape(-1) for p in mm.parameters() if p.requires_grad]),
                     total.item())
    a, b = res["fp32"], res[mode16]
    d_logit = float((a[0] - b[0]).abs().max())
    d_emb = float((a[1] - b[1]).abs().max())
    rel = float((a[2] - b[2]).norm() / a[2].norm())
    cos = float(torch.dot(a[2], b[2]) / (a[2].norm() * b[2].norm()))
    print(f"[l2, {mode16} vs f32, B=64+64] logits {d_logit:.4f} emb {d_emb:.4f} loss {a[3]:.5f}/{b[3]:.5f} grad rel {rel:.4f} cos {cos:.6f}")
    bl, be, br, bc = VS_F32_BAND[mode16]
    assert d_logit < bl and d_emb < be
    assert abs(a[3] - b[3]) < 5e-3 * max(1.0, abs(a[3]))
    assert rel < br and cos > bc


# ------------------------------------------------------------------------------------------------------------ (e) graph, key, ranks
def l2_kw(cfg):
    return dict(beta=0.15, alpha=1e-2, BND=105.0, use_structure=True, group_type="block", use_prototype=True,
                proto_table=torch.tensor(recipe.make_prototypes(cfg)).cuda(), w_f=0.05, w_r=0.1, BND_pro=4.0, proto_distance="l2")


@pytest.mark.parametrize("dtype,b", [("fp16", 6), ("fp32", 6), ("fp16", 24)])
def test_graph_replay_of_an_l2_step_bit_identical_to_eager(dtype, b):
    """b = 6: the one-launch loss tail is captured; b = 24 (48 rows): the separate l2 kernels are."""
    from gslora_hip.optim import FusedAdamW
    from gslora_hip.step import GraphedStep, gs_lora_step
    from test_hip_graph import batch, build
    cfg = recipe.cfg_small2()
    m1 = build(cfg, dtype, 0.1)
    m2 = copy.deepcopy(m1)
    mk_opt = lambda m: FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-2, weight_decay=0.05, eps=1e-8)
    o1, o2 = mk_opt(m1), mk_opt(m2)
    crit = torch.nn.CrossEntropyLoss()
    kw = l2_kw(cfg)
    g = GraphedStep(m2, o2, crit)
    for s in range(4):
        xr, yr, xf, yf = batch(cfg, b, s)
        p1 = gs_lora_step(m1, o1, crit, xr, yr, xf, yf, **kw)
        p2 = g(xr, yr, xf, yf, **kw)
        assert torch.equal(p1, p2), (s, p1.tolist(), p2.tolist())
        assert torch.isfinite(p1).all() and p1[6] > 0 and p1[7] > 0
        for (n, a), (_, c) in zip(m1.named_parameters(), m2.named_parameters()):
            if a.requires_grad:
                assert torch.equal(a, c), (s, n)
    assert (g.eager_steps, g.captures, g.replays) == (1, 1, 3)


def test_a_kl_step_after_l2_steps_equals_a_kl_step_on_a_fresh_model():
    """The distance is part of the graph key and leaves no state behind. One model, one optimizer, one GraphedStep: three l2 steps (eager,
    capture + replay, replay); the LoRA weights and AdamW's moments / step count are then put back IN PLACE (what a step is meant to
    change); the KL steps that follow must be a new key (eager, capture + replay, replay) and equal the KL steps of a fresh model bit for
    bit. f32 without dropout: no loss-scale history and no dropout counter to put back."""
    from gslora_hip.optim import FusedAdamW
    from gslora_hip.step import GraphedStep
    from test_hip_graph import batch, build
    cfg, b = recipe.cfg_small2(), 6
    crit = torch.nn.CrossEntropyLoss()
    kw_l2 = l2_kw(cfg)
    kw_kl = dict(kw_l2, BND_pro=2.0, proto_distance="kl")
    mk_opt = lambda m: FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-2, weight_decay=0.05, eps=1e-8)

    def steps(g, m, kw):
        packs = [g(*batch(cfg, b, s), **kw) for s in range(3)]
        return packs, [p.detach().clone() for p in m.parameters() if p.requires_grad]

    fresh = build(cfg, "fp32", 0.0)
    g_fresh = GraphedStep(fresh, mk_opt(fresh), crit)
    want_packs, want_params = steps(g_fresh, fresh, kw_kl)
    assert (g_fresh.eager_steps, g_fresh.captures, g_fresh.replays) == (1, 1, 2)

    m = build(cfg, "fp32", 0.0)
    start = [p.detach().clone() for p in m.parameters() if p.requires_grad]
    opt = mk_opt(m)
    g = GraphedStep(m, opt, crit)
    l2_packs, l2_params = steps(g, m, kw_l2)
    assert (g.eager_steps, g.captures, g.replays) == (1, 1, 2)
    assert not torch.equal(l2_packs[0][6:], want_packs[0][6:])      # another distance: other prototype meters ...
    assert any(not torch.equal(a, w) for a, w in zip(l2_params, want_params))      # ... and another trajectory
    with torch.no_grad():
        for p, p0 in zip([p for p in m.parameters() if p.requires_grad], start):
            p.copy_(p0)
        for ent in opt._flat.values():
            ent["m"].zero_()
            ent["v"].zero_()
            ent["step"] = 0
    got_packs, got_params = steps(g, m, kw_kl)
    assert (g.eager_steps, g.captures, g.replays) == (2, 2, 4) and len(g.graphs) == 2      # the KL steps did not replay the l2 graph
    for a, w in zip(got_packs, want_packs):
        assert torch.equal(a, w), (a.tolist(), w.tolist())
    for a, w in zip(got_params, want_params):
        assert torch.equal(a, w)


def _run_ranks(tmp_path, dtype):
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    outs = [str(tmp_path / f"rank{r}.npz") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dp_proto_l2_child.py"), str(r), "2", str(port), dtype, outs[r]],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    logs = [p.communicate(timeout=900) for p in procs]
    assert all(p.returncode == 0 and "DP-L2-OK" in lg[0] for p, lg in zip(procs, logs)), [(p.returncode, lg[0][-500:], lg[1][-3000:]) for p, lg in zip(procs, logs)]
    return [dict(np.load(o)) for o in outs]


@pytest.mark.parametrize("dtype,tol", [("fp32", 2e-5), ("fp16", 4e-3)])
def test_two_ranks_on_one_gpu_equal_the_single_process_l2_step(tmp_path, dtype, tol):
    """tests/test_hip_dp_two_ranks.py with proto_distance="l2" (its tolerances): the l2 sums ride in the pack8 slots of the KL sums, so the
    prototype hinge sees the GLOBAL batch mean; eager and graph-segment steps agree bit for bit on each rank (asserted in the child)."""
    sys.path.insert(0, HERE)
    import dp_proto_l2_child as C
    from gslora_hip.optim import FusedAdamW
    from gslora_hip.step import gs_lora_step
    from test_hip_graph import build
    r0, r1 = _run_ranks(tmp_path, dtype)
    for k in r0:      # identical replicas and identical global meters on both ranks, bit for bit
        assert np.array_equal(r0[k], r1[k]), k
    cfg = recipe.cfg_small2()
    m = build(cfg, dtype, 0.0)
    opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-2, weight_decay=0.05, eps=1e-8)
    crit = torch.nn.CrossEntropyLoss()
    kw = C.hyper(cfg)
    packs = np.stack([gs_lora_step(m, opt, crit, *C.whole_batch(cfg, 2, s), **kw).cpu().numpy() for s in range(C.STEPS)])
    assert (packs[:, 6] > 0).all() and (packs[:, 7] > 0).all()
    assert np.allclose(r0["packs"], packs, rtol=tol, atol=tol), (r0["packs"], packs)
    worst = 0.0
    for n, p in m.named_parameters():
        if p.requires_grad:
            a, b = p.detach().float().cpu().numpy(), r0[n]
            worst = max(worst, float(np.abs(a - b).max() / (np.abs(a).max() + 1e-12)))
    assert worst < tol * 5, worst


# ------------------------------------------------------------------------------------------------------------ (f) precision@k
def test_train_accuracy_topk_equals_the_reference(golden_dir):
    from util.utils import train_accuracy
    g = np.load(os.path.join(golden_dir, "topk_small.npz"))
    lo, y = torch.tensor(g["logits"]).cuda(), torch.tensor(g["labels"]).cuda()
    for name in ("1_5", "5_1_3"):
        ks = tuple(int(k) for k in g[f"topk_{name}"])
        res = train_accuracy(lo, y, topk=ks)
        assert isinstance(res, list) and len(res) == len(ks) and all(r.dim() == 0 and r.dtype == torch.float32 and r.is_cuda for r in res)
        got = np.array([r.item() for r in res], dtype=np.float32)
        assert got.tobytes() == g[f"perk_{name}"].tobytes(), (ks, got, g[f"perk_{name}"])      # one percentage per k, in the order given
        assert np.float32(res[0].item()) == g[f"ret_{name}"]      # what the reference returns for the tuple: its first entry
    # the same through a list, and on a labels tensor that lives on the host / is int32
    assert [r.item() for r in train_accuracy(lo, y.cpu().int(), topk=[5, 1, 3])] == g["perk_5_1_3"].tolist()


def test_train_accuracy_top1_keeps_its_fused_path_and_agrees_with_topk(ops):
    from util.utils import train_accuracy
    lo = rnd(301, 1000, seed=7).cuda()
    y = torch.randint(0, 1000, (301,), generator=torch.Generator().manual_seed(8)).cuda()
    y[::3] = lo[::3].argmax(1)
    got = train_accuracy(lo, y, topk=(1,))
    want = ops.ce_fwd(lo, y)[1] * (100.0 / 301)      # the value of the parent commit: the hit count of the fused CE / top-1 launch
    assert got.dim() == 0 and torch.equal(got, want) and torch.equal(got, train_accuracy(lo, y))
    multi = train_accuracy(lo, y, topk=(1, 1000, 7))
    assert torch.equal(multi[0], got) and multi[1].item() == 100.0
    rank = (lo > lo.gather(1, y[:, None])).sum(1)
    hits = ops.topk_hits(lo, y, (1, 7, 1000, 16))
    assert hits.dtype == torch.int32 and hits.tolist() == [int((rank < k).sum()) for k in (1, 7, 1000, 16)]
    y_bad = y.clone()
    y_bad[0], y_bad[1] = -1, 1000      # never a hit, and no out-of-bounds read
    assert ops.topk_hits(lo, y_bad, (1000,)).item() == 299
