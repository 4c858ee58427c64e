"""Attention above the single-panel limit (224 < T <= 1025; the cls forward above 256): the multi-panel online-softmax kernels against a
float64 torch reference, the rescale corner cases, the cls-query kernels, determinism; the models at T = 257 against the real reference
(tests/golden/longseq_*.npz, tools/make_golden_longseq.py), HIP-graph replay, and ViT-B/16 at T = 577 against the CPU oracle. Tolerances are those of test_attention in test_hip_ops.py."""
import copy
import os

import numpy as np
import pytest
import torch

from oracle import recipe

pytestmark = pytest.mark.gpu

DTS = [torch.float32, torch.bfloat16, torch.float16]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    from gslora_hip import ops as _ops
    from gslora_hip import _lib
    _lib.load()
    return _ops


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + 1000 * len(shape) + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def tol(dt, f32, h16):
    return f32 if dt == torch.float32 else h16


def to_head_major(qkv, B, T, H):
    return qkv.view(B, T, 3, H, 64).permute(0, 3, 2, 1, 4).contiguous().view(B * T, 3 * H * 64)


def ref64(qkv, d_o, B, T, H, scale):
    """float64 forward (o, lse) and backward (dqkv) of the values the kernel sees."""
    x = qkv.double().cpu().requires_grad_(True)
    q, k, v = x.reshape(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = torch.einsum("bhid,bhjd->bhij", q, k) * scale
    o = torch.einsum("bhij,bhjd->bhid", s.softmax(-1), v).permute(0, 2, 1, 3).reshape(B * T, H * 64)
    lse = s.logsumexp(-1)
    o.backward(d_o.double().cpu())
    return o.detach(), lse.detach(), x.grad


def check(ops, qkv, d_o, B, T, H, scale, dt, layout=0):
    """qkv / d_o: f32 CPU tensors; run the kernels in dt and compare with the float64 reference of the dt-rounded values."""
    qd, gd = qkv.to(dt), d_o.to(dt)
    o_r, l_r, g_r = ref64(qd.float(), gd.float(), B, T, H, scale)
    qin = qd.cuda()
    if layout == 1:
        qin = to_head_major(qin, B, T, H)
    o, lse = ops.attention_fwd(qin, B, T, H, scale, layout=layout)
    e_o = (o.double().cpu() - o_r).abs().max().item()
    e_l = (lse.double().cpu() - l_r).abs().max().item()
    assert e_o < tol(dt, 2e-5, 2e-2), e_o
    assert e_l < tol(dt, 2e-5, 2e-3), e_l
    dqkv = ops.attention_bwd(qin, o, gd.cuda(), lse, B, T, H, scale, layout=layout)
    e_g = (dqkv.double().cpu() - g_r).abs().max().item()
    assert e_g < tol(dt, 5e-5, 3e-2) * max(1.0, g_r.abs().max().item()), e_g
    return o, lse, dqkv


# (T, B, H): B * H stays small — the few-items regime splits an item's query / key tiles over several workgroups
CASES = [(225, 2, 1), (240, 1, 2), (241, 2, 12), (256, 3, 1), (257, 2, 2), (320, 1, 12), (577, 2, 1), (785, 1, 2), (1025, 1, 12)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("T,B,H", CASES)
def test_long_attention_matches_float64(ops, dt, T, B, H):
    scale = (H * 64) ** -0.5 * 3.0
    qkv = rnd(B * T, 3 * H * 64, seed=T + H, scale=1.5)
    d_o = rnd(B * T, H * 64, seed=T + 5)
    check(ops, qkv, d_o, B, T, H, scale, dt)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("T,B,H", [(225, 2, 1), (257, 2, 2), (577, 1, 12), (1025, 1, 2)])
def test_long_attention_head_major_input(ops, dt, T, B, H):
    """qkv_layout 1 (head-major): against float64, and bit-identical to the token-major input."""
    scale = 64 ** -0.5
    qkv = rnd(B * T, 3 * H * 64, seed=T, scale=1.5)
    d_o = rnd(B * T, H * 64, seed=T + 7)
    a = check(ops, qkv, d_o, B, T, H, scale, dt, layout=1)
    b = check(ops, qkv, d_o, B, T, H, scale, dt, layout=0)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("dt", DTS)
def test_long_attention_at_training_batch(ops, dt):
    """More (image, head) items than CUs: one workgroup per block of <= 16 tiles, no further split."""
    B, T, H = 40, 257, 8
    scale = 64 ** -0.5
    check(ops, rnd(B * T, 3 * H * 64, seed=3, scale=1.5), rnd(B * T, H * 64, seed=4), B, T, H, scale, dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", ["jump_in_last_panel", "max_in_first_panel", "uniform"])
def test_online_softmax_rescale(ops, dt, case):
    """Forced rescales: (a) one key of the LAST 64-key panel scores far above everything before it for chosen queries, so their running
    max jumps there; (b) the max sits in the first panel and every later panel underflows to zero; (c) all scores equal."""
    B, T, H = 2, 300, 2
    scale = 64 ** -0.5
    qkv = rnd(B * T, 3 * H * 64, seed=21, scale=0.5).view(B, T, 3, H, 64)
    if case == "uniform":
        qkv[:, :, 0] = 0.0      # q = 0: every score 0, o = mean of V, lse = log T
    else:
        key = 290 if case == "jump_in_last_panel" else 3
        # score gaps > 7 / > 45: (b)'s later panels weigh e^-45 against the first one's 1 — zero in the 16-bit P operand, below f32 rounding
        boost = 4.0 if case == "jump_in_last_panel" else 25.0
        for qi in (0, 7, 299):
            qkv[:, qi, 0] = qkv[:, qi, 0] / qkv[:, qi, 0].norm(dim=-1, keepdim=True) * 4.0
        qkv[:, key, 1] = (qkv[:, 0, 0] + qkv[:, 7, 0] + qkv[:, 299, 0]) * boost
    qkv = qkv.reshape(B * T, -1).contiguous()
    if case != "uniform":      # the spike dominates the chosen queries' rows by a wide margin
        q, k, _ = qkv.view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
        s = torch.einsum("bhid,bhjd->bhij", q, k)[:, :, [0, 7, 299]] * scale
        top2 = s.topk(2, -1).values
        assert (s.argmax(-1) == key).all() and ((top2[..., 0] - top2[..., 1]) > (5.0 if key == 290 else 45.0)).all()
    d_o = rnd(B * T, H * 64, seed=22)
    o, lse, _ = check(ops, qkv, d_o, B, T, H, scale, dt)
    if case == "uniform":
        v = qkv.to(dt).float().view(B, T, 3, H, 64)[:, :, 2]
        assert (o.float().cpu().view(B, T, H, 64) - v.mean(1, keepdim=True)).abs().max() < tol(dt, 2e-5, 1e-2)
        assert (lse.cpu() - np.log(T)).abs().max() < tol(dt, 2e-5, 2e-3)


CLS_CASES = [(3, 257, 2, 0), (2, 577, 12, 0), (2, 257, 2, 1), (3, 577, 2, 1), (2, 257, 2, 2), (2, 577, 12, 2)]


@pytest.mark.parametrize("dt,B,T,H,hm", [(dt, *c) for dt in DTS for c in CLS_CASES if not (c[3] == 1 and dt == torch.float32)])
def test_long_cls_kernels(ops, dt, B, T, H, hm):
    """The cls-query forward above 256 keys equals row 0 of the dense forward (and float64); the cls backward, fed the compact and the full
    forward tensors, equals the dense backward fed zeros elsewhere (head-major qkv, layout 1, is a 16-bit layout)."""
    scale = 64 ** -0.5
    qkv = rnd(B * T, 3 * H * 64, seed=61 + T, scale=1.2).cuda().to(dt)
    inner = H * 64
    o_d, lse_d = ops.attention_fwd(qkv, B, T, H, scale)
    if hm == 2:
        qin, q_cls = qkv[:, inner:].contiguous(), qkv.view(B, T, 3 * inner)[:, 0, :inner].contiguous()
    else:
        qin, q_cls = (to_head_major(qkv, B, T, H) if hm else qkv), None
    o_c, lse_c = ops.attention_fwd_cls(qin, B, T, H, scale, layout=hm, q_cls=q_cls)
    q, k, v = [t.reshape(B, T, H, 64).permute(0, 2, 1, 3) for t in qkv.double().cpu().chunk(3, -1)]
    s0 = torch.einsum("bhd,bhjd->bhj", q[:, :, 0], k) * scale
    ref_o = torch.einsum("bhj,bhjd->bhd", s0.softmax(-1), v).reshape(B, inner)
    assert (o_c.double().cpu() - ref_o).abs().max() < tol(dt, 2e-5, 2e-2)
    assert (lse_c.double().cpu() - s0.logsumexp(-1)).abs().max() < tol(dt, 2e-5, 2e-3)
    assert (o_c.float() - o_d.view(B, T, -1)[:, 0].float()).abs().max() < tol(dt, 2e-5, 3e-2)
    assert (lse_c - lse_d[:, :, 0]).abs().max() < tol(dt, 2e-5, 2e-3)
    d_cls = rnd(B, inner, seed=62).cuda().to(dt)
    d_full = torch.zeros(B * T, inner, device="cuda", dtype=dt)
    d_full.view(B, T, -1)[:, 0] = d_cls
    ref = ops.attention_bwd(qkv, o_d, d_full, lse_d, B, T, H, scale).float().cpu()
    bound = tol(dt, 2e-5, 2e-2) * max(1.0, ref.abs().max().item())
    for o_, l_ in ((o_c, lse_c), (o_d, lse_d)):      # compact and full forward tensors
        got = ops.attention_bwd_cls(qin, o_, d_cls, l_, B, T, H, scale, layout=hm, q_cls=q_cls)
        if hm == 2:
            dkv, dq = got
            got = torch.cat([torch.zeros(B * T, inner, device="cuda", dtype=dt), dkv], 1)
            got.view(B, T, -1)[:, 0, :inner] = dq
        assert (got.float().cpu() - ref).abs().max() < bound


@pytest.mark.parametrize("dt", DTS)
def test_long_attention_is_deterministic(ops, dt):
    B, T, H = 3, 577, 4
    scale = 64 ** -0.5
    qkv = rnd(B * T, 3 * H * 64, seed=9, scale=1.5).cuda().to(dt)
    d_o = rnd(B * T, H * 64, seed=10).cuda().to(dt)
    runs = []
    for _ in range(2):
        o, lse = ops.attention_fwd(qkv, B, T, H, scale)
        runs.append((o, lse, ops.attention_bwd(qkv, o, d_o, lse, B, T, H, scale)))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- models at T = 257 / 577
def vit_face(cfg, dtype, pool="cls"):
    import loralib as lora
    from vit_pytorch_face import ViT_face
    m = ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
                 dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], pool=pool, lora_rank=cfg["lora_rank"])
    m.load_state_dict({k: torch.tensor(v) for k, v in recipe.make_state(cfg).items()})
    lora.mark_only_lora_as_trainable(m)
    return m.to("cuda").set_compute_dtype(dtype).train()


# ---- against the real reference (tests/golden/longseq_*.npz, tools/make_golden_longseq.py): 128 px images, patch / stride 8, T = 257
HYPER = dict(lr=1e-2, wd=0.05, beta=0.15, alpha=1e-2, BND=105.0, BND_pro=2.0, pro_f_weight=0.05, pro_r_weight=0.1)      # oracle/make_golden.py
GRAD_BAND = {"bf16": (0.06, 0.995), "fp16": (0.01, 0.9999)}      # test_hip_bf16_pinned.py
LONG = lambda c: dict(c, image_size=128)
FIXTURES = {      # tag: (cfg, head, pool, backbone)
    "longseq_small2_cosface_b3": (LONG(recipe.cfg_small2()), "CosFace", "cls", "VIT"),
    "longseq_small2_arcface_b3": (LONG(recipe.cfg_small2()), "ArcFace", "mean", "VIT"),
    "longseq_vits_small2_b3": (LONG(recipe.cfg_small2()), "CosFace", "cls", "VITs"),
    "longseq_attn_small_b3": (LONG(recipe.cfg_small_attn()), "CosFace", "cls", "VIT"),
}


def ref_state(cfg, net):      # = tools/make_golden_longseq.py (ViTs: tools/make_golden_vits.py's 12 x 12 patch weight)
    st = recipe.make_state(cfg)
    if net == "VITs":
        fan_in = cfg["channels"] * 12 * 12
        bound = 1.0 / float(np.sqrt(fan_in))
        st["patch_to_embedding.weight"] = np.ascontiguousarray(
            recipe.uniform("patch_to_embedding.weight", (cfg["dim"], fan_in), 1337, -bound, bound), dtype=np.float32)
    return {k: torch.tensor(v) for k, v in st.items()}


def build(cfg, head, pool, net, dtype="fp32"):
    import loralib as lora
    from vit_pytorch_face import ViT_face, ViTs_face
    kw = dict(loss_type=head, GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
              dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], pool=pool, lora_rank=cfg["lora_rank"])
    if net == "VITs":
        m = ViTs_face(ac_patch_size=12, pad=4, **kw)
    else:
        m = ViT_face(lora_pos=cfg.get("lora_pos", "FFN"), **kw)
    m.load_state_dict(ref_state(cfg, net), strict=True)
    lora.mark_only_lora_as_trainable(m)
    m = m.to("cuda").set_compute_dtype(dtype)
    assert m.num_tokens == 257
    return m


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


def close(a, r, tol=1e-4):
    return np.abs(a - r).max() < tol * max(1.0, np.abs(r).max())


@pytest.mark.parametrize("tag", list(FIXTURES))
def test_model_at_257_tokens_f32_matches_reference(golden_dir, tag):
    """f32: logits / embeddings (train and eval = merged LoRA) <= 1e-4, the loss terms and the LoRA gradients <= 1e-4 * max(1, |g|), with
    both hinges active and inactive. CosFace / pool cls runs the last block's cls forward above 256 keys; --lora_pos Attention runs the
    attention-site forward and backward (no Q split, no LayerNorm fold) on the panel kernels."""
    cfg, head, pool, net = FIXTURES[tag]
    g = np.load(os.path.join(golden_dir, f"{tag}.npz"))
    m = build(cfg, head, pool, net).train()
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
    m.load_state_dict(ref_state(cfg, net))
    proto = {c: torch.tensor(v) for c, v in enumerate(recipe.make_prototypes(cfg))}
    total, got = total_loss(m, cfg, xr, yr, xf, yf, HYPER, proto)
    for a, r in zip(got, g["losses1"]):
        assert abs(a - r) < 1e-4 * max(1.0, abs(r)), (got, g["losses1"])
    total.backward()
    grads = lora_grads(m)
    assert grads
    for n, v in grads.items():
        assert close(v, g[f"grad1::{n}"]), n
    for p in m.parameters():
        p.grad = None
    total, _ = total_loss(m, cfg, xr, yr, xf, yf, dict(HYPER, BND=5.0, BND_pro=0.1), proto)
    assert abs(total.item() - float(g["total_inactive"])) < 1e-4 * max(1.0, abs(float(g["total_inactive"])))
    total.backward()
    for n, v in lora_grads(m).items():
        assert close(v, g[f"grad_inactive::{n}"]), n


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("tag", list(FIXTURES))
def test_model_at_257_tokens_16bit_within_grad_band(golden_dir, tag, mode):
    """The two speed modes against the same fixtures: logits / embeddings within the bands of the ViTs / heads tests, every LoRA gradient
    tensor within GRAD_BAND (relative Frobenius error AND cosine similarity)."""
    cfg, head, pool, net = FIXTURES[tag]
    g = np.load(os.path.join(golden_dir, f"{tag}.npz"))
    m = build(cfg, head, pool, net, mode).train()
    xr, yr, xf, yf = batches(cfg, 3)
    with torch.no_grad():
        lo, em = m(xr, yr)
    assert np.abs(lo.cpu().numpy() - g["fwd_logits"]).max() < 0.25
    assert np.abs(em.cpu().numpy() - g["fwd_emb"]).max() < 0.05
    proto = {c: torch.tensor(v) for c, v in enumerate(recipe.make_prototypes(cfg))}
    total, _ = total_loss(m, cfg, xr, yr, xf, yf, HYPER, proto)
    total.backward()
    checked = 0
    for n, v in lora_grads(m).items():
        r, a = g[f"grad1::{n}"].ravel().astype(np.float64), v.ravel().astype(np.float64)
        if np.linalg.norm(r) == 0:
            continue
        rel = np.linalg.norm(a - r) / np.linalg.norm(r)
        cos = float(a @ r) / (np.linalg.norm(a) * np.linalg.norm(r))
        assert rel < GRAD_BAND[mode][0] and cos > GRAD_BAND[mode][1], (mode, n, rel, cos)
        checked += 1
    assert checked > 0


NAMES = ("losses_forget", "losses_remain", "losses_total", "losses_structure", "top1_forget", "top1_remain", "losses_prototype_forget",
         "losses_prototype_remain")


def test_engine_three_steps_at_257_tokens_f32_match_reference(golden_dir):
    """engine_cl.train_one_epoch + FusedAdamW on cfg_small6 at 128 px: meters of every step, first-step gradients, parameters (as the
    engine tests of test_hip_vits.py / test_hip_heads.py)."""
    import engine_cl
    from gslora_hip.optim import FusedAdamW
    from oracle import gslora_oracle as O
    from util.utils import AverageMeter
    cfg, b = LONG(recipe.cfg_small6()), 2
    g = np.load(os.path.join(golden_dir, "longseq_small6_engine.npz"))
    m = build(cfg, "CosFace", "cls", "VIT")
    opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=HYPER["lr"], weight_decay=HYPER["wd"], eps=1e-8)
    meters = {n: AverageMeter() for n in NAMES}
    proto = {c: torch.tensor(v) for c, v in enumerate(recipe.make_prototypes(cfg))}
    cfgd = {"DATA_ROOT": "./data/casia100/", "BND_pro": HYPER["BND_pro"], "MULTI_GPU": False, "WORK_PATH": "/tmp", "BACKBONE_NAME": "VIT"}
    st0 = ref_state(cfg, "VIT")
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
        got = np.array([meters[n].val for n in NAMES])
        assert np.abs(got - g[f"meters{s + 1}"]).max() < 1e-3, (s, got, g[f"meters{s + 1}"])
        g_hip = {n: torch.tensor(v) for n, v in lora_grads(m).items()}
        if s == 0:
            for n, v in g_hip.items():
                assert close(v.numpy(), g[f"grad1::{n}"]), n
            track = {n: (st0[n].clone(), torch.zeros_like(v), torch.zeros_like(v)) for n, v in g_hip.items()}
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
    assert np.abs(np.array([meters[n].avg for n in NAMES]) - g["meters3_avg"]).max() < 2e-3
    assert batch_ctr == int(g["batch_ctr"])


def test_fp16_step_at_257_tokens_graph_replay_bit_identical_to_eager():
    from gslora_hip.optim import FusedAdamW
    from gslora_hip.step import GraphedStep, gs_lora_step
    cfg = dict(recipe.cfg_small6(), image_size=128)
    b = 6
    m1 = vit_face(cfg, "fp16")
    m2 = copy.deepcopy(m1)
    mk_opt = lambda m: FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-2, weight_decay=0.05, eps=1e-8)
    o1, o2 = mk_opt(m1), mk_opt(m2)
    crit = torch.nn.CrossEntropyLoss()
    proto = torch.tensor(recipe.make_prototypes(cfg)).cuda()
    kw = dict(beta=0.15, alpha=1e-2, BND=105.0, use_structure=True, group_type="block", use_prototype=True, proto_table=proto,
              w_f=0.05, w_r=0.1, BND_pro=2.0)
    g = GraphedStep(m2, o2, crit)
    nf = max(2, cfg["num_class"] // 5)
    mk = lambda a: torch.tensor(a).cuda()
    for s in range(4):
        xr = mk(recipe.make_images(cfg, b, seed=100 + s, tag="xr"))
        yr = mk(recipe.make_labels(cfg, b, seed=100 + s, tag="yr", lo=0, hi=cfg["num_class"] - nf))
        xf = mk(recipe.make_images(cfg, b, seed=200 + s, tag="xf"))
        yf = mk(recipe.make_labels(cfg, b, seed=200 + s, tag="yf", lo=cfg["num_class"] - nf, hi=cfg["num_class"]))
        p1 = gs_lora_step(m1, o1, crit, xr, yr, xf, yf, **kw)
        p2 = g(xr, yr, xf, yf, **kw)
        assert torch.equal(p1, p2) and torch.isfinite(p1).all(), s
        for (n, a), (_, c) in zip(m1.named_parameters(), m2.named_parameters()):
            if a.requires_grad:
                assert torch.equal(a, c), (s, n)
    assert (g.eager_steps, g.captures, g.replays) == (1, 1, 3)


def test_vit_b16_384px_f32_matches_the_oracle():
    """ModifiedViT(vit_b_16(image_size=384)): T = 577, the full ViT-B/16 geometry, f32, 2 + 2 images, against oracle/tv_vit.py on the CPU
    (as test_hip_vitb.py's full-geometry test): logits / embeddings <= 1e-4, LoRA gradients <= 1e-4 * max(1, |g|)."""
    import engine_cl
    import loralib as lora
    from gslora_hip import losses
    from oracle import tv_vit as TV
    from util.utils import replace_ffn_with_lora
    from vit_pytorch_face import ModifiedViT
    from vit_pytorch_face.modified_VIT import vit_b_16
    hyper = dict(lr=1e-2, wd=0.05, beta=0.15, alpha=1e-2, BND=8.0, BND_pro=2.0, pro_f_weight=0.05, pro_r_weight=0.1)
    cfg = dict(recipe.cfg_vitb(lora_rank=16, num_class=100), image_size=384)
    st = recipe.make_tv_state(cfg)
    b = 2
    mk = lambda a: torch.tensor(a)
    xr, xf = mk(recipe.make_images(cfg, b, seed=300, tag="xr")), mk(recipe.make_images(cfg, b, seed=400, tag="xf"))
    yr, yf = mk(recipe.make_labels(cfg, b, seed=300, tag="yr", lo=0, hi=80)), mk(recipe.make_labels(cfg, b, seed=400, tag="yf", lo=80, hi=100))
    proto_np = recipe.make_prototypes(cfg)
    om = TV.build(cfg, st).train()
    out = TV.step_losses(om, xr, yr, xf, yf, hyper, torch.tensor(np.stack([proto_np[c] for c in range(cfg["num_class"])])))
    named = [(n, p) for n, p in om.named_parameters() if p.requires_grad]
    ref_g = dict(zip([n for n, _ in named], torch.autograd.grad(out["total"], [p for _, p in named])))
    vit = vit_b_16(image_size=384, num_classes=100)
    m = replace_ffn_with_lora(ModifiedViT(vit), rank=16)
    m.load_state_dict({k: torch.tensor(v) for k, v in st.items()}, strict=True)
    m = m.to("cuda").set_compute_dtype("fp32")
    lora.mark_only_lora_as_trainable(m)
    m.train()
    assert m.hip_spec().num_tokens == 577
    proto = {k: torch.tensor(proto_np[k]) for k in range(cfg["num_class"])}
    lo_r, em_r = m(xr.cuda(), yr.cuda())
    lo_f, em_f = m(xf.cuda(), yf.cuda())
    ce_r = losses.ce_sum_top1(lo_r, yr.cuda())[0] / b
    ce_f = losses.ce_sum_top1(lo_f, yf.cuda())[0] / b
    sl = engine_cl.get_structure_loss(m, imagenet=True)
    kl_f, kl_r = engine_cl.get_prototype_loss(em_f, yf.cuda(), proto), engine_cl.get_prototype_loss(em_r, yr.cuda(), proto)
    H = hyper
    total = (H["beta"] * torch.relu(H["BND"] - ce_f) + ce_r + H["alpha"] * sl + H["pro_f_weight"] * torch.relu(H["BND_pro"] - kl_f)
             + H["pro_r_weight"] * kl_r)
    total.backward()
    for got, ref in ((lo_r, out["logits_r"]), (lo_f, out["logits_f"]), (em_r, out["emb_r"]), (em_f, out["emb_f"])):
        assert (got.detach().cpu() - ref.detach()).abs().max() < 1e-4
    grads = {n: p.grad.detach().cpu() for n, p in m.named_parameters() if p.requires_grad}
    assert len(grads) == 48
    for n, r in ref_g.items():
        e = float((grads[n] - r).abs().max()) / max(1.0, float(r.abs().max()))
        assert e < 1e-4, (n, e)
