"""The ArcFace and Softmax heads of ViT_face on the GPU (reference vit_pytorch_face/vit_face.py:14-143).

 (a) gsl_head_fwd_margin / gsl_head_bwd_margin with the ArcFace kind against a float64 torch-autograd restatement of the reference
     formula, on rows constructed to take every branch (cos_y > th, cos_y <= th, easy_margin on both sides of 0), for every x dtype,
     pool cls / mean, compact / dense gradients, the dropout copy dxb and the two-pass fp16 loss scale;
 (b) the CosFace kind of the margin pair is bit-identical to gsl_head_fwd / gsl_head_bwd;
 (c) the whole model against the real reference (tests/golden/*_b3.npz and arcface_small6_engine.npz, tools/make_golden_heads.py);
 (d) HIP-graph replay of an ArcFace step, and driver_cl --head ArcFace."""
import copy
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import gslora_oracle as O
from oracle import recipe

pytestmark = pytest.mark.gpu

HYPER = dict(lr=1e-2, wd=0.05, beta=0.15, alpha=1e-2, BND=105.0, BND_pro=2.0, pro_f_weight=0.05, pro_r_weight=0.1)
GRAD_BAND = {"bf16": (0.06, 0.995), "fp16": (0.01, 0.9999)}      # test_hip_bf16_pinned.py


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    from gslora_hip import ops as _ops
    from gslora_hip import _lib
    _lib.load()
    return _ops


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


# ------------------------------------------------------------------------------------------------------------ (a) op level
B, T, D, C = 8, 6, 256, 40
S_ARC, M_ARC = 64.0, 0.5
TARGETS = [0.7, 0.2, -0.5, -0.95, -0.99, 0.9, -0.2, 0.4]      # th = cos(pi - 0.5) = -0.878: rows 3 and 4 take the cos - mm branch


def pooled_emb(x64, g, b, pool_mean):
    xb = x64.view(B, T, D)
    return F.layer_norm(xb.mean(1) if pool_mean else xb[:, 0], (D,), g, b, 1e-5)


def make_case(xdt, pool_mean, seed=0):
    """x in the format under test; W with the label rows set so that cos(emb, W[y_b]) = TARGETS[b]."""
    x = rnd(B * T, D, seed=seed + 1, scale=2.0).to(xdt)
    g, b = 1 + 0.1 * rnd(D, seed=seed + 2), 0.1 * rnd(D, seed=seed + 3)
    y = torch.randperm(C, generator=torch.Generator().manual_seed(seed + 4))[:B]
    W = rnd(C, D, seed=seed + 5)
    e = F.normalize(pooled_emb(x.double(), g, b, pool_mean))
    u = rnd(B, D, seed=seed + 6)
    u = F.normalize(u - (u * e).sum(1, keepdim=True) * e)
    t = torch.tensor(TARGETS, dtype=torch.float64)[:, None]
    W[y] = 0.7 * (t * e + torch.sqrt(1 - t * t) * u)
    return x, g, b, W, y


def ref_arcface(x, g, b, W, y, easy, pool_mean, dl, de):
    """The reference ArcFace (vit_face.py:110-143) in float64 with autograd: logits, emb, cos_y, d loss / d x."""
    x64 = x.double().requires_grad_(True)
    emb = pooled_emb(x64, g, b, pool_mean)
    cos = F.normalize(emb) @ F.normalize(W.float().double()).T
    cy = cos.gather(1, y[:, None])
    sine = torch.sqrt(1.0 - cy * cy)
    phi = cy * math.cos(M_ARC) - sine * math.sin(M_ARC)
    phi = torch.where(cy > 0, phi, cy) if easy else torch.where(cy > math.cos(math.pi - M_ARC), phi, cy - math.sin(math.pi - M_ARC) * M_ARC)
    logits = S_ARC * cos.scatter(1, y[:, None], phi)
    (dx,) = torch.autograd.grad((logits * dl.double()).sum() + (emb * de.double()).sum(), x64)
    return logits.detach(), emb.detach(), cy.detach()[:, 0], dx


XDTS = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
OPDT = {torch.float32: torch.float32, torch.bfloat16: torch.bfloat16, torch.float16: torch.float16}      # dxb format allowed with x


@pytest.mark.parametrize("xname", list(XDTS))
@pytest.mark.parametrize("pool", ["cls_compact", "cls_dense", "mean"])
def test_arcface_op_matches_float64_autograd(ops, xname, pool):
    xdt = XDTS[xname]
    pool_mean, compact = pool == "mean", pool == "cls_compact"
    x, g, b, W, y = make_case(xdt, pool_mean)
    xc, gc, bc, yc = x.cuda(), g.float().cuda(), b.float().cuda(), y.cuda()
    Wn = ops.cosface_prep(W.float().cuda())
    dl, de = rnd(B, C, seed=11).float(), rnd(B, D, seed=12, scale=0.5).float()
    for easy in (False, True):
        logits, emb, mean, rstd, cos_y = ops.head_fwd_margin(xc, B, T, D, gc, bc, 1e-5, Wn, yc, S_ARC, 0.0, "arcface", m=M_ARC,
                                                             easy_margin=easy, pool_mean=pool_mean)
        lo_r, emb_r, cy_r, dx_r = ref_arcface(x, gc.cpu().double(), bc.cpu().double(), W, y, easy, pool_mean, dl, de)
        # the rows take the branches they were built for
        th = math.cos(math.pi - M_ARC)
        assert (cy_r[3:5] <= th).all() and (cy_r[[0, 1, 2, 5, 6, 7]] > th).all()
        assert (cy_r > 0).sum() == 4 and (cy_r < 0).sum() == 4
        assert (emb.cpu().double() - emb_r).abs().max() < 1e-5
        assert (cos_y.cpu().double() - cy_r).abs().max() < 1e-6
        assert (logits.cpu().double() - lo_r).abs().max() < 5e-5, (easy, (logits.cpu().double() - lo_r).abs().max())
        dt = OPDT[xdt]
        dx, dxb = ops.head_bwd_margin(dl.cuda(), de.cuda(), xc, B, T, D, gc, mean, rstd, emb, Wn, S_ARC, dt, "arcface", m=M_ARC,
                                      easy_margin=easy, cos_y=cos_y, label=yc, p_drop=0.25, seed=5, site=3, pool_mean=pool_mean,
                                      compact=compact)
        ref = dx_r.view(B, T, D)[:, 0] if compact else dx_r
        got = dx.cpu().double().view(ref.shape)
        assert (got - ref).abs().max() < 2e-5 * max(1.0, ref.abs().max().item()), (easy, (got - ref).abs().max())
        keep = ops.dropout_mask(B * T * D, 0.25, 5, 3, "cuda").cpu().view(B, T, D).float()
        keep = keep[:, 0] if compact else keep.view(B * T, D)
        want = dx.cpu() * keep * (1.0 / 0.75)
        tol = 1e-6 if dt == torch.float32 else 1e-2
        assert ((dxb.cpu().float() - want).abs() - tol * want.abs()).max() <= 1e-6
        if pool == "cls_dense":
            assert (got.view(B, T, D)[:, 1:] == 0).all()


def test_arcface_fp16_loss_scaled_backward(ops):
    """The two-pass loss scale: the stored gradient is S x the unscaled one and gscale[0..1] = {S, 1/S}, S * max|g| in [2^10, 2^11)."""
    x, g, b, W, y = make_case(torch.float16, False, seed=20)
    xc, gc, bc, yc = x.cuda(), g.float().cuda(), b.float().cuda(), y.cuda()
    Wn = ops.cosface_prep(W.float().cuda())
    dl, de = rnd(B, C, seed=21, scale=1e-2).float().cuda(), rnd(B, D, seed=22, scale=1e-3).float().cuda()
    logits, emb, mean, rstd, cos_y = ops.head_fwd_margin(xc, B, T, D, gc, bc, 1e-5, Wn, yc, S_ARC, 0.0, "arcface", m=M_ARC)
    args = (dl, de, xc, B, T, D, gc, mean, rstd, emb, Wn, S_ARC, torch.float16, "arcface")
    kw = dict(m=M_ARC, cos_y=cos_y, label=yc, compact=True)
    dx_u, _ = ops.head_bwd_margin(*args, **kw)
    gscale = torch.zeros(4, device="cuda")
    dx_s, _ = ops.head_bwd_margin(*args, gscale=gscale, **kw)
    S = gscale[0].item()
    assert S == 2.0 ** round(math.log2(S)) and gscale[1].item() == 1.0 / S
    assert 1024.0 <= S * dx_u.abs().max().item() < 2048.0
    assert torch.equal(dx_s, dx_u * S)
    lo_r, _, _, dx_r = ref_arcface(x, gc.cpu().double(), bc.cpu().double(), W, y, False, False, dl.cpu(), de.cpu())
    ref = dx_r.view(B, T, D)[:, 0]
    assert (dx_u.cpu().double() - ref).abs().max() < 2e-5 * max(1.0, ref.abs().max().item())


# ------------------------------------------------------------------------------------------------------------ (b) CosFace kind
@pytest.mark.parametrize("xname", list(XDTS))
def test_cosface_through_the_margin_pair_is_bit_identical(ops, xname):
    xdt = XDTS[xname]
    x, g, b, W, y = make_case(xdt, False, seed=30)
    xc, gc, bc, yc = x.cuda(), g.float().cuda(), b.float().cuda(), y.cuda()
    Wn = ops.cosface_prep(W.float().cuda())
    a = ops.head_fwd(xc, B, T, D, gc, bc, 1e-5, Wn, yc, 64.0, 0.35)
    m = ops.head_fwd_margin(xc, B, T, D, gc, bc, 1e-5, Wn, yc, 64.0, 0.35, "cosface", m=0.5, easy_margin=True)
    assert m[4] is None and all(torch.equal(p, q) for p, q in zip(a, m[:4]))
    logits, emb, mean, rstd = a
    dl, de = rnd(B, C, seed=31).float().cuda(), rnd(B, D, seed=32).float().cuda()
    dt = OPDT[xdt]
    for compact in (True, False):
        gs1 = torch.zeros(4, device="cuda") if dt == torch.float16 else None
        gs2 = torch.zeros(4, device="cuda") if dt == torch.float16 else None
        common = (dl, de, xc, B, T, D, gc, mean, rstd, emb, Wn, 64.0, dt)
        kw = dict(p_drop=0.1, seed=9, site=2, compact=compact)
        r1 = ops.head_bwd(*common, gscale=gs1, **kw)
        r2 = ops.head_bwd_margin(*common, "cosface", m=0.5, gscale=gs2, **kw)
        assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])
        if gs1 is not None:
            assert torch.equal(gs1, gs2)


# ------------------------------------------------------------------------------------------------------------ (c) model level
FIXTURES = {"arcface_small2_b3": (recipe.cfg_small2(), "ArcFace"), "arcface_attn_small_b3": (recipe.cfg_small_attn(), "ArcFace"),
            "softmax_small2_b3": (recipe.cfg_small2(), "Softmax")}


def head_state(cfg, head):      # = tools/make_golden_heads.py
    st = recipe.make_state(cfg)
    if head == "Softmax":
        st["loss.bias"] = recipe.uniform("loss.bias", (cfg["num_class"],), 1337, -0.5, 0.5)
    return st


def build(cfg, head, dtype="fp32", dropout=0.0, **kw):
    import loralib as lora
    from vit_pytorch_face import ViT_face
    m = ViT_face(loss_type=head, GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
                 dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], dropout=dropout, emb_dropout=dropout,
                 lora_rank=cfg["lora_rank"], lora_pos=cfg.get("lora_pos", "FFN"), **kw)
    m.load_state_dict({k: torch.tensor(v) for k, v in head_state(cfg, head).items()}, strict=True)
    lora.mark_only_lora_as_trainable(m)
    return m.to("cuda").set_compute_dtype(dtype)


def batches(cfg, batch, s=0):
    nf = max(2, cfg["num_class"] // 5)
    mk = lambda a: torch.tensor(a).cuda()
    return (mk(recipe.make_images(cfg, batch, seed=100 + s, tag="xr")),
            mk(recipe.make_labels(cfg, batch, seed=100 + s, tag="yr", lo=0, hi=cfg["num_class"] - nf)),
            mk(recipe.make_images(cfg, batch, seed=200 + s, tag="xf")),
            mk(recipe.make_labels(cfg, batch, seed=200 + s, tag="yf", lo=cfg["num_class"] - nf, hi=cfg["num_class"])))


def total_loss(model, cfg, xr, yr, xf, yf, hy, proto):
    import engine
    import engine_cl
    from gslora_hip import losses
    lo_r, em_r = model(xr, yr)
    lo_f, em_f = model(xf, yf)
    ce_r = losses.ce_sum_top1(lo_r, yr)[0] / xr.shape[0]
    ce_f = losses.ce_sum_top1(lo_f, yf)[0] / xf.shape[0]
    sl = engine.get_structure_loss(model, num_layers=cfg["depth"], group_type="block", group_pos=cfg.get("lora_pos", "FFN"))
    kl_f = engine_cl.get_prototype_loss(em_f, yf, proto)
    kl_r = engine_cl.get_prototype_loss(em_r, yr, proto)
    total = (hy["beta"] * torch.relu(hy["BND"] - ce_f) + ce_r + hy["alpha"] * sl
             + hy["pro_f_weight"] * torch.relu(hy["BND_pro"] - kl_f) + hy["pro_r_weight"] * kl_r)
    return total, [ce_f.item(), ce_r.item(), total.item(), sl.item(), kl_f.item(), kl_r.item()]


def lora_grads(model):
    return {n: p.grad.detach().cpu().numpy().copy() for n, p in model.named_parameters() if p.requires_grad}


@pytest.mark.parametrize("tag", list(FIXTURES))
def test_model_f32_matches_reference(golden_dir, tag):
    cfg, head = FIXTURES[tag]
    g = np.load(os.path.join(golden_dir, f"{tag}.npz"))
    m = build(cfg, head).train()
    xr, yr, xf, yf = batches(cfg, 3)
    with torch.no_grad():
        lo, em = m(xr, yr)
        assert np.abs(lo.cpu().numpy() - g["fwd_logits"]).max() < 1e-4
        assert np.abs(em.cpu().numpy() - g["fwd_emb"]).max() < 1e-4
        m.eval()
        lo, em = m(xr, yr)
        assert np.abs(lo.cpu().numpy() - g["eval_logits"]).max() < 1e-4
        assert np.abs(em.cpu().numpy() - g["eval_emb"]).max() < 1e-4
        m.train()
    m.load_state_dict({k: torch.tensor(v) for k, v in head_state(cfg, head).items()})
    proto = {c: torch.tensor(v) for c, v in enumerate(recipe.make_prototypes(cfg))}
    total, got = total_loss(m, cfg, xr, yr, xf, yf, HYPER, proto)
    for a, r in zip(got, g["losses1"]):
        assert abs(a - r) < 1e-4 * max(1.0, abs(r)), (got, g["losses1"])
    total.backward()
    for k, v in lora_grads(m).items():
        r = g[f"grad1::{k}"]
        assert np.abs(v - r).max() < 1e-4 * max(1.0, np.abs(r).max()), k
    for p in m.parameters():
        p.grad = None
    total, _ = total_loss(m, cfg, xr, yr, xf, yf, dict(HYPER, BND=5.0, BND_pro=0.1), proto)
    assert abs(total.item() - float(g["total_inactive"])) < 1e-4 * max(1.0, abs(float(g["total_inactive"])))
    total.backward()
    for k, v in lora_grads(m).items():
        r = g[f"grad_inactive::{k}"]
        assert np.abs(v - r).max() < 1e-4 * max(1.0, np.abs(r).max()), k


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("tag", list(FIXTURES))
def test_model_16bit_close_to_reference(golden_dir, tag, mode):
    cfg, head = FIXTURES[tag]
    g = np.load(os.path.join(golden_dir, f"{tag}.npz"))
    m = build(cfg, head, mode).train()
    xr, yr, xf, yf = batches(cfg, 3)
    with torch.no_grad():
        lo, em = m(xr, yr)
    # the bands of test_forward_bf16_close_to_reference
    assert np.abs(lo.cpu().numpy() - g["fwd_logits"]).max() < 0.25
    assert np.abs(em.cpu().numpy() - g["fwd_emb"]).max() < 0.05
    proto = {c: torch.tensor(v) for c, v in enumerate(recipe.make_prototypes(cfg))}
    total, _ = total_loss(m, cfg, xr, yr, xf, yf, HYPER, proto)
    total.backward()
    for k, v in lora_grads(m).items():
        r, a = g[f"grad1::{k}"].ravel().astype(np.float64), v.ravel().astype(np.float64)
        if np.linalg.norm(r) == 0:
            continue
        rel = np.linalg.norm(a - r) / np.linalg.norm(r)
        cos = float(a @ r) / (np.linalg.norm(a) * np.linalg.norm(r))
        assert rel < GRAD_BAND[mode][0] and cos > GRAD_BAND[mode][1], (mode, k, rel, cos)


def test_softmax_head_pools_mean_and_needs_a_label_for_logits():
    """The linear path passes pool = 'mean' through; without a label the Softmax model returns emb alone (reference :541-548)."""
    cfg = recipe.cfg_small2()
    sm = build(cfg, "Softmax", pool="mean").eval()
    cf = build(cfg, "CosFace", pool="mean").eval()
    xr, yr, _, _ = batches(cfg, 3)
    with torch.no_grad():
        lo, em = sm(xr, yr)
        _, em_c = cf(xr, yr)
        em_only = sm(xr)
    assert torch.equal(em, em_c) and torch.equal(em_only, em)
    ref = em @ sm.loss.weight.T + sm.loss.bias
    assert (lo - ref).abs().max() < 1e-4


NAMES = ("losses_forget", "losses_remain", "losses_total", "losses_structure", "top1_forget", "top1_remain", "losses_prototype_forget",
         "losses_prototype_remain")


def test_arcface_engine_three_steps_f32_match_reference(golden_dir):
    """engine_cl.train_one_epoch + FusedAdamW on cfg_small6 with ArcFace: meters of every step, first-step gradients, parameters."""
    import engine_cl
    from gslora_hip.optim import FusedAdamW
    from util.utils import AverageMeter
    cfg, b = recipe.cfg_small6(), 2
    g = np.load(os.path.join(golden_dir, "arcface_small6_engine.npz"))
    m = build(cfg, "ArcFace")
    opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=HYPER["lr"], weight_decay=HYPER["wd"], eps=1e-8)
    meters = {k: AverageMeter() for k in NAMES}
    proto = {c: torch.tensor(v) for c, v in enumerate(recipe.make_prototypes(cfg))}
    cfgd = {"DATA_ROOT": "./data/casia100/", "BND_pro": HYPER["BND_pro"], "MULTI_GPU": False, "WORK_PATH": "/tmp", "BACKBONE_NAME": "VIT"}
    batch_ctr, track = 0, None
    for s in range(3):
        xr, yr, xf, yf = batches(cfg, b, s)
        ret = engine_cl.train_one_epoch(
            model=m, dataloader_forget=[(xf.cpu(), yf.cpu())], dataloader_remain=[(xr.cpu(), yr.cpu())], device=torch.device("cuda"),
            criterion=torch.nn.CrossEntropyLoss(), optimizer=opt, epoch=0, beta=HYPER["beta"], alpha=HYPER["alpha"], BND=HYPER["BND"],
            batch=batch_ctr, testloader_forget=None, testloader_remain=None, forget_acc_before=0.0, highest_H_mean=0.0, cfg=cfgd,
            task_i="0", use_prototype=True, prototype_dict=proto, prototype_weight_forget=HYPER["pro_f_weight"],
            prototype_weight_remain=HYPER["pro_r_weight"], **meters)
        batch_ctr = ret[0]
        got = np.array([meters[k].val for k in NAMES])
        assert np.abs(got - g[f"meters{s + 1}"]).max() < 1e-3, (s, got, g[f"meters{s + 1}"])
        g_hip = {n: torch.tensor(v) for n, v in lora_grads(m).items()}
        if s == 0:
            for k, v in g_hip.items():
                r = g[f"grad1::{k}"]
                assert np.abs(v.numpy() - r).max() < 1e-4 * max(1.0, np.abs(r).max()), k
            track = {n: (torch.tensor(head_state(cfg, "ArcFace")[n]), torch.zeros_like(v), torch.zeros_like(v)) for n, v in g_hip.items()}
        params = {n: p.detach().cpu() for n, p in m.named_parameters() if p.requires_grad}
        for n in g_hip:      # the HIP AdamW on the HIP gradients = the oracle's AdamW on the same gradients
            track[n] = O.adamw_update(*track[n][:1], g_hip[n], *track[n][1:], s + 1, HYPER["lr"], HYPER["wd"])
            assert (params[n] - track[n][0]).abs().max() < 2e-6, (s, n)
        if s in (0, 2):      # against the reference's parameters (AdamW is ill-conditioned where |g| ~ eps: bounded, not pinned)
            for n, p in params.items():
                diff = np.abs(p.numpy() - g[f"param{s + 1}::{n}"])
                well = np.abs(g[f"grad1::{n}"]) > 1e-6
                if s == 0:
                    assert diff[well].max(initial=0.0) < 2e-4, n
                else:
                    assert np.mean(diff < 1e-3) > 0.99, n
                assert diff.max() <= 2.05 * HYPER["lr"] * (s + 1), n
    assert np.abs(np.array([meters[k].avg for k in NAMES]) - g["meters3_avg"]).max() < 2e-3
    assert batch_ctr == int(g["batch_ctr"])


# ------------------------------------------------------------------------------------------------------------ (d) graph and driver
def test_arcface_graph_replay_bit_identical_to_eager():
    from gslora_hip.optim import FusedAdamW
    from gslora_hip.step import GraphedStep, gs_lora_step
    cfg, b = recipe.cfg_small2(), 6
    m1 = build(cfg, "ArcFace", "fp16", dropout=0.1).train()
    m2 = copy.deepcopy(m1)
    mk_opt = lambda m: FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-2, weight_decay=0.05, eps=1e-8)
    o1, o2 = mk_opt(m1), mk_opt(m2)
    crit = torch.nn.CrossEntropyLoss()
    proto = torch.tensor(recipe.make_prototypes(cfg)).cuda()
    kw = dict(beta=0.15, alpha=1e-2, BND=105.0, use_structure=True, group_type="block", use_prototype=True, proto_table=proto,
              w_f=0.05, w_r=0.1, BND_pro=2.0)
    g = GraphedStep(m2, o2, crit)
    for s in range(4):
        xr, yr, xf, yf = batches(cfg, b, s)
        p1 = gs_lora_step(m1, o1, crit, xr, yr, xf, yf, **kw)
        p2 = g(xr, yr, xf, yf, **kw)
        assert torch.equal(p1, p2), (s, p1.tolist(), p2.tolist())
        assert torch.isfinite(p1).all()
        for (n, a), (_, c) in zip(m1.named_parameters(), m2.named_parameters()):
            if a.requires_grad:
                assert torch.equal(a, c), (s, n)
    assert (g.eager_steps, g.captures, g.replays) == (1, 1, 3)


def test_driver_two_tasks_with_arcface(tmp_path):
    import driver_cl
    from vit_pytorch_face import ArcFace
    rep, out, model = driver_cl.main(["--small", "--num_class", "20", "--num_tasks", "2", "--per_forget_cls", "4", "--epochs", "1",
                                      "--batch_size", "16", "--samples_per_class", "4", "--dtype", "fp16", "--head", "ArcFace",
                                      "--outdir", str(tmp_path)])
    assert isinstance(model.loss, ArcFace)
    assert [r["task"] for r in rep] == [0, 1]
    for r in rep:
        assert len(r["norms"]) == 3 and all(np.isfinite(r["norms"])) and np.isfinite(r["total_loss"])
    assert os.path.exists(os.path.join(out, "task-level", "Backbone_task_1.pth"))
