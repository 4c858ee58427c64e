"""ViTs_face on the GPU (reference vit_pytorch_face/vits_face.py:414-509, overlapping nn.Unfold patch stage).

 (a) gsl_unfold_patches is bit-identical to F.unfold(img, k, padding=pad, stride=s).transpose(1, 2) cast to the output format, with the
     zero cls row and the zero K padding, written into a NaN-filled buffer (every element is written);
 (b) the patch GEMM at the padded K of the unfold path (320, 448) with the three PATCH epilogues;
 (c) the whole model against the real reference (tests/golden/vits_*.npz, tools/make_golden_vits.py): f32, bf16 / fp16, three engine
     steps, the driver's full geometry;
 (d) HIP-graph replay of a ViTs fp16 step, and driver_cl --net VITs."""
import copy
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


def images(B, C, H, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, C, H, H, generator=g) * 4.0 - 2.0      # (well inside fp16 range)


def unfold_ref(img, k, s, pad, dtype, kpad):
    """F.unfold on the CPU, with the zero cls row per image and the zero K padding, cast to the output format."""
    B = img.shape[0]
    u = F.unfold(img, k, padding=pad, stride=s).transpose(1, 2)
    out = torch.zeros(B, 1 + u.shape[1], kpad)
    out[:, 1:, :u.shape[2]] = u
    return out.reshape(-1, kpad).to(dtype)


# ------------------------------------------------------------------------------------------------------------ (a) the gather
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
GEOMS = [(112, 12, 8, 4), (48, 12, 8, 4), (48, 10, 8, 1), (40, 16, 8, 4), (48, 8, 8, 0)]


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("geom", GEOMS)
def test_unfold_bit_identical_to_torch_unfold(ops, dname, C, geom):
    from gslora_hip import _lib as L
    dt = DTYPES[dname]
    H, k, s, pad = geom
    B = 3
    img = images(B, C, H, seed=H + k + C)
    kpad = -(-C * k * k // 64) * 64
    ref = unfold_ref(img, k, s, pad, dt, kpad)
    out = torch.full(ref.shape, float("nan"), device="cuda", dtype=dt)
    xc = img.cuda()
    L.check(L.load().gsl_unfold_patches(xc.data_ptr(), out.data_ptr(), B, C, H, H, k, s, pad, kpad, ops.code(dt), ops._stream()), "unfold")
    got = out.cpu()
    assert not torch.isnan(got.float()).any()
    assert torch.equal(got, ref)
    assert torch.equal(ops.unfold_patches(xc, k, s, pad, dt).cpu(), ref)


@pytest.mark.parametrize("dname", list(DTYPES))
def test_unfold_two_batches_land_in_consecutive_rows(ops, dname):
    dt = DTYPES[dname]
    a, b = images(3, 3, 48, seed=1), images(2, 3, 48, seed=2)
    got = ops.unfold_patches((a.cuda(), b.cuda()), 12, 8, 4, dt).cpu()
    assert got.shape == (5 * 37, 448)
    assert torch.equal(got, unfold_ref(torch.cat([a, b]), 12, 8, 4, dt, 448))


def test_unfold_wider_ldo_and_refusals(ops):
    """A leading dimension above the padded K is zero-filled too; the argument checks name what they refuse."""
    from gslora_hip import _lib as L
    img = images(2, 3, 48, seed=3).cuda()
    out = torch.full((2 * 37, 512), float("nan"), device="cuda", dtype=torch.float16)
    L.check(L.load().gsl_unfold_patches(img.data_ptr(), out.data_ptr(), 2, 3, 48, 48, 12, 8, 4, 512, L.F16, ops._stream()), "unfold")
    assert torch.equal(out.cpu(), unfold_ref(img.cpu(), 12, 8, 4, torch.float16, 512))
    lib = L.load()
    for args in ((12, 8, 12, 448), (12, 0, 4, 448), (12, 8, 4, 424), (12, 8, 4, 444)):      # pad >= k, stride 0, ldo < C*k*k, ldo % 8
        k, s, pad, ldo = args
        assert lib.gsl_unfold_patches(img.data_ptr(), out.data_ptr(), 2, 3, 48, 48, k, s, pad, ldo, L.F16, ops._stream()) == -1, args
    assert lib.gsl_unfold_patches(img.data_ptr(), out.data_ptr(), 2, 3, 8, 8, 24, 8, 4, 1728, L.F16, ops._stream()) == -1      # no window


# ------------------------------------------------------------------------------------------------------------ (b) the padded-K patch GEMM
def relerr(a, b):
    return (a - b).abs().max().item() / max(1e-12, b.abs().max().item())


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("k,pad", [(10, 1), (12, 4)])      # K = 320, 448
def test_patch_gemm_at_padded_k(ops, dname, k, pad):
    from gslora_hip import _lib as L
    dt = DTYPES[dname]
    B, H, N = 4, 48, 128
    T = 37
    img = images(B, 3, H, seed=k)
    Kc, kpad = 3 * k * k, -(-3 * k * k // 64) * 64
    A = ops.unfold_patches(img.cuda(), k, 8, pad, dt)
    g = torch.Generator().manual_seed(5)
    w = torch.zeros(N, kpad)
    w[:, :Kc] = torch.randn(N, Kc, generator=g) * Kc ** -0.5
    bias, pos, cls = torch.randn(N, generator=g), torch.randn(T, N, generator=g), torch.randn(N, generator=g)
    Wc = w.cuda().to(dt)
    acc = A.cpu().float() @ Wc.cpu().float().t() + bias
    tok = torch.arange(B * T) % T
    ref = torch.where((tok == 0)[:, None], cls[None, :].expand(B * T, N), acc) + pos[tok]
    o32 = torch.empty(B * T, N, device="cuda", dtype=torch.float32)
    ops.gemm_nt(A, Wc, o32, epilogue=L.EPI_PATCH, bias=bias.cuda(), pos=pos.cuda(), cls=cls.cuda(), T=T)
    assert relerr(o32.cpu(), ref) < (2e-5 if dt == torch.float32 else 2e-3)
    if dt != torch.float32:      # the 16-bit stream outputs: the f32 result, rounded once (test_hip_ops.py)
        for sdt, epi in ((torch.bfloat16, L.EPI_PATCH_BF16), (torch.float16, L.EPI_PATCH_F16)):
            o16 = torch.full((B * T, N), 7.0, device="cuda", dtype=sdt)
            ops.gemm_nt(A, Wc, o16, epilogue=epi, bias=bias.cuda(), pos=pos.cuda(), cls=cls.cuda(), T=T)
            assert torch.equal(o16, o32.to(sdt)), sdt


# ------------------------------------------------------------------------------------------------------------ (c) model level
FIXTURES = {"vits_small2_b3": (recipe.cfg_small2(), "CosFace", 12, 4, "cls"),
            "vits_k10p1_small2_b3": (recipe.cfg_small2(), "ArcFace", 10, 1, "mean")}


def vits_state(cfg, k, seed=1337):      # = tools/make_golden_vits.py
    st = recipe.make_state(cfg, seed=seed)
    fan_in = cfg["channels"] * k * k
    bound = 1.0 / float(np.sqrt(fan_in))
    st["patch_to_embedding.weight"] = np.ascontiguousarray(
        recipe.uniform("patch_to_embedding.weight", (cfg["dim"], fan_in), seed, -bound, bound), dtype=np.float32)
    return {n: torch.tensor(v) for n, v in st.items()}


def build(cfg, head="CosFace", k=12, pad=4, pool="cls", dtype="fp32", dropout=0.0):
    import loralib as lora
    from vit_pytorch_face import ViTs_face
    m = ViTs_face(loss_type=head, GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
                  ac_patch_size=k, pad=pad, dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], pool=pool,
                  dropout=dropout, emb_dropout=dropout, lora_rank=cfg["lora_rank"])
    m.load_state_dict(vits_state(cfg, k), strict=True)
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
    sl = engine.get_structure_loss(model, num_layers=cfg["depth"], group_type="block", group_pos="FFN")
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
def test_model_f32_matches_reference(golden_dir, tag):
    cfg, head, k, pad, pool = FIXTURES[tag]
    g = np.load(os.path.join(golden_dir, f"{tag}.npz"))
    m = build(cfg, head, k, pad, pool).train()
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
    m.load_state_dict(vits_state(cfg, k))
    proto = {c: torch.tensor(v) for c, v in enumerate(recipe.make_prototypes(cfg))}
    total, got = total_loss(m, cfg, xr, yr, xf, yf, HYPER, proto)
    for a, r in zip(got, g["losses1"]):
        assert abs(a - r) < 1e-4 * max(1.0, abs(r)), (got, g["losses1"])
    total.backward()
    for n, v in lora_grads(m).items():
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
def test_model_16bit_close_to_reference(golden_dir, tag, mode):
    cfg, head, k, pad, pool = FIXTURES[tag]
    g = np.load(os.path.join(golden_dir, f"{tag}.npz"))
    m = build(cfg, head, k, pad, pool, mode).train()
    xr, yr, xf, yf = batches(cfg, 3)
    with torch.no_grad():
        lo, em = m(xr, yr)
    assert np.abs(lo.cpu().numpy() - g["fwd_logits"]).max() < 0.25
    assert np.abs(em.cpu().numpy() - g["fwd_emb"]).max() < 0.05
    proto = {c: torch.tensor(v) for c, v in enumerate(recipe.make_prototypes(cfg))}
    total, _ = total_loss(m, cfg, xr, yr, xf, yf, HYPER, proto)
    total.backward()
    for n, v in lora_grads(m).items():
        r, a = g[f"grad1::{n}"].ravel().astype(np.float64), v.ravel().astype(np.float64)
        if np.linalg.norm(r) == 0:
            continue
        rel = np.linalg.norm(a - r) / np.linalg.norm(r)
        cos = float(a @ r) / (np.linalg.norm(a) * np.linalg.norm(r))
        assert rel < GRAD_BAND[mode][0] and cos > GRAD_BAND[mode][1], (mode, n, rel, cos)


def test_model_refuses_images_of_another_size():
    cfg = recipe.cfg_small2()
    m = build(cfg).eval()
    with torch.no_grad(), pytest.raises(ValueError, match="built for 48 x 48"):
        m(torch.zeros(2, 3, 56, 56, device="cuda"))


NAMES = ("losses_forget", "losses_remain", "losses_total", "losses_structure", "top1_forget", "top1_remain", "losses_prototype_forget",
         "losses_prototype_remain")


def test_engine_three_steps_f32_match_reference(golden_dir):
    """engine_cl.train_one_epoch + FusedAdamW on cfg_small6 (k 12, pad 4): meters of every step, first-step gradients, parameters."""
    import engine_cl
    from gslora_hip.optim import FusedAdamW
    from util.utils import AverageMeter
    cfg, b = recipe.cfg_small6(), 2
    g = np.load(os.path.join(golden_dir, "vits_small6_engine.npz"))
    m = build(cfg)
    opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=HYPER["lr"], weight_decay=HYPER["wd"], eps=1e-8)
    meters = {n: AverageMeter() for n in NAMES}
    proto = {c: torch.tensor(v) for c, v in enumerate(recipe.make_prototypes(cfg))}
    cfgd = {"DATA_ROOT": "./data/casia100/", "BND_pro": HYPER["BND_pro"], "MULTI_GPU": False, "WORK_PATH": "/tmp", "BACKBONE_NAME": "VITs"}
    st0 = vits_state(cfg, 12)
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


def test_full_geometry_f32_matches_reference(golden_dir):
    """The reference driver's ViTs (112 px, 12 x 12 windows at stride 8, pad 4: K = 432 -> 448, 197 tokens), B 2."""
    cfg = recipe.cfg_full()
    g = np.load(os.path.join(golden_dir, "vits_full_b2.npz"))
    m = build(cfg).train()
    xr, yr, xf, yf = batches(cfg, 2)
    with torch.no_grad():
        lo, em = m(xr, yr)
        assert np.abs(lo.cpu().numpy() - g["fwd_logits"]).max() < 1e-4
        assert np.abs(em.cpu().numpy() - g["fwd_emb"]).max() < 1e-4
        m.eval()
        lo, em = m(xr, yr)
        assert np.abs(lo.cpu().numpy() - g["eval_logits"]).max() < 1e-4
        assert np.abs(em.cpu().numpy() - g["eval_emb"]).max() < 1e-4
        m.train()
    m.load_state_dict(vits_state(cfg, 12))
    proto = {c: torch.tensor(v) for c, v in enumerate(recipe.make_prototypes(cfg))}
    total, _ = total_loss(m, cfg, xr, yr, xf, yf, HYPER, proto)
    total.backward()
    grads = lora_grads(m)
    assert len(grads) == 24
    for n, v in grads.items():
        r = g[f"grad1::{n}"]
        assert (np.abs(v - r) <= 1e-4 * np.maximum(1.0, np.abs(r))).all(), n


# ------------------------------------------------------------------------------------------------------------ (d) graph and driver
def test_graph_replay_bit_identical_to_eager():
    from gslora_hip.optim import FusedAdamW
    from gslora_hip.step import GraphedStep, gs_lora_step
    cfg, b = recipe.cfg_small2(), 6
    m1 = build(cfg, dtype="fp16", dropout=0.1).train()
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


def test_driver_two_tasks_with_vits(tmp_path):
    import driver_cl
    from vit_pytorch_face import ViTs_face
    rep, out, model = driver_cl.main(["--small", "--net", "VITs", "--num_class", "20", "--num_tasks", "2", "--per_forget_cls", "4",
                                      "--epochs", "2", "--batch_size", "16", "--samples_per_class", "4", "--dtype", "fp16",
                                      "--outdir", str(tmp_path)])
    assert isinstance(model, ViTs_face) and (model.ac_patch_size, model.pad, model.num_tokens) == (12, 4, 37)
    assert [r["task"] for r in rep] == [0, 1]
    for r in rep:
        assert len(r["norms"]) == 3 and all(np.isfinite(r["norms"])) and np.isfinite(r["total_loss"])
        assert r["forget_after"] <= r["forget_before"], r
    ck = os.path.join(out, "task-level", "Backbone_task_1.pth")
    assert os.path.exists(ck)
    fresh = ViTs_face(loss_type="CosFace", GPU_ID=[0], num_class=20, image_size=48, patch_size=8, ac_patch_size=12, pad=4, dim=128, depth=3,
                      heads=2, mlp_dim=256, lora_rank=8)
    fresh.load_state_dict(torch.load(ck, map_location="cpu"), strict=True)      # the merged checkpoint reloads strict
