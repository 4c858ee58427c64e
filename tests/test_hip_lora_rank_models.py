"""LoRA ranks above 16 through the models and the step (the two-launch K-segment GEMMs and the rank-32 / rank-64 gradient reductions of
csrc/lora.hip), against the real reference: tests/golden/rank*.npz from tools/make_golden_lora_rank.py.

f32 mode at the project's bars (logits / embeddings / group norms 1e-4, LoRA gradients 1e-4 * max(1, |g|), selection mask exact, the engine
trajectory as tests/test_hip_heads.py holds arcface_small6_engine); fp16 / bf16 against the f32 mode of the same model within the declared
tolerance of DESIGN section 1 (logits 0.25, embeddings 0.1, gradients GRAD_BAND of test_hip_heads.py); the real widths once; graph replay;
ViTs_face; merged weights in eval mode; two data-parallel ranks."""
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

import test_hip_heads as TH
import test_hip_vitb as TB
import test_hip_vits as TV

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HYPER, GRAD_BAND = TH.HYPER, TH.GRAD_BAND
FIXTURES = {"rank32_small2_b3": recipe.cfg_small2(lora_rank=32), "rank64_small2_b3": recipe.cfg_small2(lora_rank=64),
            "rank20_attn_small_b3": recipe.cfg_small_attn(lora_rank=20)}


def protos(cfg):
    return {c: torch.tensor(v) for c, v in enumerate(recipe.make_prototypes(cfg))}


def close(a, r, tol=1e-4):
    return np.abs(a - r).max() < tol * max(1.0, np.abs(r).max())


def block_of(name):
    return int(name.split("layers.")[1].split(".")[0])


# ------------------------------------------------------------------------------------------------------------ f32 against the reference
@pytest.mark.parametrize("tag", list(FIXTURES))
def test_model_f32_matches_reference(golden_dir, tag):
    from gslora_hip import losses
    cfg = FIXTURES[tag]
    g = np.load(os.path.join(golden_dir, f"{tag}.npz"))
    m = TH.build(cfg, "CosFace").train()
    xr, yr, xf, yf = TH.batches(cfg, 3)
    with torch.no_grad():
        lo, em = m(xr, yr)
        assert np.abs(lo.cpu().numpy() - g["fwd_logits"]).max() < 1e-4
        assert np.abs(em.cpu().numpy() - g["fwd_emb"]).max() < 1e-4
        m.eval()      # merged weights
        lo, em = m(xr, yr)
        assert np.abs(lo.cpu().numpy() - g["eval_logits"]).max() < 1e-4
        assert np.abs(em.cpu().numpy() - g["eval_emb"]).max() < 1e-4
        m.train()
    state = TH.head_state(cfg, "CosFace")
    m.load_state_dict({k: torch.tensor(v) for k, v in state.items()})
    # group-lasso norms of the blocks and the selection mask, against float64 on the recipe's tensors
    sq = np.zeros(cfg["depth"])
    for k, v in state.items():
        if "lora_" in k:
            sq[block_of(k)] += (v.astype(np.float64) ** 2).sum()
    norms = np.sqrt(sq)
    srt = np.sort(norms)
    tau = float(0.5 * (srt[0] + srt[1]))      # between the two smallest norms: the mask holds both values, no norm is near tau
    rep = losses.group_report(m, "block", tau=tau)
    assert np.abs(rep["group_norm"].cpu().numpy() - norms).max() < 1e-4
    assert rep["mask"].cpu().numpy().astype(bool).tolist() == (norms > tau).tolist()
    total, got = TH.total_loss(m, cfg, xr, yr, xf, yf, HYPER, protos(cfg))
    for a, r in zip(got, g["losses1"]):
        assert abs(a - r) < 1e-4 * max(1.0, abs(r)), (got, g["losses1"])
    total.backward()
    for k, v in TH.lora_grads(m).items():
        assert close(v, g[f"grad1::{k}"]), k
    for p in m.parameters():
        p.grad = None
    total, _ = TH.total_loss(m, cfg, xr, yr, xf, yf, dict(HYPER, BND=5.0, BND_pro=0.1), protos(cfg))
    assert abs(total.item() - float(g["total_inactive"])) < 1e-4 * max(1.0, abs(float(g["total_inactive"])))
    total.backward()
    for k, v in TH.lora_grads(m).items():
        if f"grad_inactive::{k}" in g.files:      # (dropped from the rank-64 fixture to keep the file below 1 MB)
            assert close(v, g[f"grad_inactive::{k}"]), k


def test_eval_mode_merged_weights_at_rank_64(golden_dir):
    """model.eval() merges W + s B A with r = 64 = half the width of the model: logits of the merged forward, and the round trip back."""
    cfg = FIXTURES["rank64_small2_b3"]
    g = np.load(os.path.join(golden_dir, "rank64_small2_b3.npz"))
    m = TH.build(cfg, "CosFace").eval()
    xr, yr, _, _ = TH.batches(cfg, 3)
    with torch.no_grad():
        lo, em = m(xr, yr)
        assert np.abs(lo.cpu().numpy() - g["eval_logits"]).max() < 1e-4
        assert np.abs(em.cpu().numpy() - g["eval_emb"]).max() < 1e-4
        m.train()
        lo, _ = m(xr, yr)
        assert np.abs(lo.cpu().numpy() - g["fwd_logits"]).max() < 1e-4


def test_vit_b16_rank_48_f32_matches_reference(golden_dir, tmp_path):
    """ModifiedViT at rank 48 (tests/test_hip_vitb.py: test_forward_f32..., test_grads_small2_vs_reference)."""
    import engine_cl
    from gslora_hip import losses
    cfg, b = recipe.cfg_vitb_small2(lora_rank=48), 3
    g = np.load(os.path.join(golden_dir, "rank48_vitb_small2_b3.npz"))
    m, _, sub = TB.build_sub(cfg, "fp32", tmp=tmp_path)
    xr, yr, xf, yf = TB.batches(sub, cfg, b)
    m.train()
    with torch.no_grad():
        assert np.abs(m(xr, yr)[0].cpu().numpy() - g["fwd_logits"]).max() < 1e-4
    m.eval()
    assert np.abs(m.state_dict()["encoder.layers.encoder_layer_0.mlp.0.weight"].cpu().numpy() - g["merged_w_l0_mlp0"]).max() < 1e-6
    with torch.no_grad():
        assert np.abs(m(xr, yr)[0].cpu().numpy() - g["eval_logits"]).max() < 1e-4
    m.train()
    proto_np = recipe.make_prototypes(sub)
    proto = {c: torch.tensor(proto_np[c]) for c in range(sub["num_class"])}
    lo_r, em_r = m(xr, yr)
    lo_f, em_f = m(xf, yf)
    ce_r, ce_f = losses.ce_sum_top1(lo_r, yr)[0] / b, losses.ce_sum_top1(lo_f, yf)[0] / b
    sl = losses.structure_loss(m, "block")
    kl_f, kl_r = engine_cl.get_prototype_loss(em_f, yf, proto), engine_cl.get_prototype_loss(em_r, yr, proto)
    H = TB.HYPER
    total = (H["beta"] * torch.relu(H["BND"] - ce_f) + ce_r + H["alpha"] * sl
             + H["pro_f_weight"] * torch.relu(H["BND_pro"] - kl_f) + H["pro_r_weight"] * kl_r)
    total.backward()
    got = [ce_f.item(), ce_r.item(), total.item(), sl.item(), kl_f.item(), kl_r.item()]
    for a, r in zip(got, g["losses1"]):
        assert abs(a - r) < 1e-4 * max(1.0, abs(r)), (got, g["losses1"])
    for n, p in m.named_parameters():
        if p.requires_grad:
            assert close(p.grad.cpu().numpy(), g[f"grad1::{n}"]), n


def test_engine_three_steps_f32_at_rank_32(golden_dir):
    """engine_cl.train_one_epoch + FusedAdamW on cfg_small6(lora_rank=32), as test_hip_heads.py holds arcface_small6_engine: meters of every
    step, first-step gradients, the HIP AdamW against the oracle's on the same gradients. (param1 / param3 are not in this fixture: the
    rank-32 LoRA tensors would put it above 1 MB, tools/make_golden_lora_rank.py.)"""
    import engine_cl
    from gslora_hip.optim import FusedAdamW
    from util.utils import AverageMeter
    cfg, b = recipe.cfg_small6(lora_rank=32), 2
    g = np.load(os.path.join(golden_dir, "rank32_small6_engine.npz"))
    m = TH.build(cfg, "CosFace")
    opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=HYPER["lr"], weight_decay=HYPER["wd"], eps=1e-8)
    meters = {k: AverageMeter() for k in TH.NAMES}
    cfgd = {"DATA_ROOT": "./data/casia100/", "BND_pro": HYPER["BND_pro"], "MULTI_GPU": False, "WORK_PATH": "/tmp", "BACKBONE_NAME": "VIT"}
    batch_ctr, track = 0, None
    for s in range(3):
        xr, yr, xf, yf = TH.batches(cfg, b, s)
        ret = engine_cl.train_one_epoch(
            model=m, dataloader_forget=[(xf.cpu(), yf.cpu())], dataloader_remain=[(xr.cpu(), yr.cpu())], device=torch.device("cuda"),
            criterion=torch.nn.CrossEntropyLoss(), optimizer=opt, epoch=0, beta=HYPER["beta"], alpha=HYPER["alpha"], BND=HYPER["BND"],
            batch=batch_ctr, testloader_forget=None, testloader_remain=None, forget_acc_before=0.0, highest_H_mean=0.0, cfg=cfgd,
            task_i="0", use_prototype=True, prototype_dict=protos(cfg), prototype_weight_forget=HYPER["pro_f_weight"],
            prototype_weight_remain=HYPER["pro_r_weight"], **meters)
        batch_ctr = ret[0]
        got = np.array([meters[k].val for k in TH.NAMES])
        assert np.abs(got - g[f"meters{s + 1}"]).max() < 1e-3, (s, got, g[f"meters{s + 1}"])
        g_hip = {n: torch.tensor(v) for n, v in TH.lora_grads(m).items()}
        if s == 0:
            for k, v in g_hip.items():
                assert close(v.numpy(), g[f"grad1::{k}"]), k
            track = {n: (torch.tensor(TH.head_state(cfg, "CosFace")[n]), torch.zeros_like(v), torch.zeros_like(v)) for n, v in g_hip.items()}
        params = {n: p.detach().cpu() for n, p in m.named_parameters() if p.requires_grad}
        for n in g_hip:      # the HIP AdamW on the HIP gradients = the oracle's AdamW on the same gradients
            track[n] = O.adamw_update(*track[n][:1], g_hip[n], *track[n][1:], s + 1, HYPER["lr"], HYPER["wd"])
            assert (params[n] - track[n][0]).abs().max() < 2e-6, (s, n)
    assert np.abs(np.array([meters[k].avg for k in TH.NAMES]) - g["meters3_avg"]).max() < 2e-3
    assert batch_ctr == int(g["batch_ctr"])


# ------------------------------------------------------------------------------------------------------------ 16-bit modes against f32
def forward_backward(m, cfg, b=3):
    xr, yr, xf, yf = TH.batches(cfg, b)
    with torch.no_grad():
        lo, em = m(xr, yr)
    total, _ = TH.total_loss(m, cfg, xr, yr, xf, yf, HYPER, protos(cfg))
    total.backward()
    return lo.float().cpu().numpy(), em.float().cpu().numpy(), TH.lora_grads(m)


def within_band(got, ref, mode, what):
    """The declared tolerance of DESIGN section 1: logits 0.25, embeddings 0.1, LoRA gradients relative Frobenius / cosine."""
    assert np.abs(got[0] - ref[0]).max() < 0.25, (what, "logits")
    assert np.abs(got[1] - ref[1]).max() < 0.1, (what, "emb")
    for k, v in got[2].items():
        r, a = ref[2][k].ravel().astype(np.float64), v.ravel().astype(np.float64)
        if np.linalg.norm(r) == 0:
            continue
        rel = np.linalg.norm(a - r) / np.linalg.norm(r)
        cos = float(a @ r) / (np.linalg.norm(a) * np.linalg.norm(r))
        assert rel < GRAD_BAND[mode][0] and cos > GRAD_BAND[mode][1], (what, k, rel, cos)


_F32 = {}


def f32_of(tag):
    """The f32 mode's forward and gradients of a fixture's model: computed once, shared by the 16-bit cases, never changed."""
    if tag not in _F32:
        _F32[tag] = forward_backward(TH.build(FIXTURES[tag], "CosFace").train(), FIXTURES[tag])
    return _F32[tag]


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("tag", list(FIXTURES))
def test_model_16bit_close_to_the_f32_mode(tag, mode):
    cfg = FIXTURES[tag]
    m = TH.build(cfg, "CosFace", mode).train()
    got = forward_backward(m, cfg)
    within_band(got, f32_of(tag), mode, f"{tag} {mode}")
    if mode == "fp16":
        rep = m._runner.loss_scale_report()
        assert rep is not None and not rep["saturated"], rep


def build_real_widths(dtype, r=32):
    """The real widths (dim 512, mlp 2048, 112 px / patch 8 -> 197 tokens), two blocks: the reductions run at N = 2048 and N = 512."""
    cfg = dict(recipe.cfg_full(lora_rank=r, num_class=20), depth=2)
    return cfg, TH.build(cfg, "CosFace", dtype).train()


def test_real_widths_rank_32_fp16_and_fp32x3_against_f32():
    """2 + 2 images at the real widths, r = 32: 788 rows, the batched MFMA form at N = 2048 and N = 512 in fp16, the chunked VALU form in
    the two f32 modes. fp16 within the declared tolerance of the f32 mode; fp32x3 at the f32 bars."""
    cfg, m32 = build_real_widths("fp32")
    ref = forward_backward(m32, cfg, b=2)
    del m32
    _, m16 = build_real_widths("fp16")
    got = forward_backward(m16, cfg, b=2)
    within_band(got, ref, "fp16", "real widths fp16")
    assert not m16._runner.loss_scale_report()["saturated"]
    del m16
    _, m3 = build_real_widths("fp32x3")
    lo, em, gr = forward_backward(m3, cfg, b=2)
    assert np.abs(lo - ref[0]).max() < 1e-4 and np.abs(em - ref[1]).max() < 1e-4
    for k, v in gr.items():
        assert close(v, ref[2][k]), k


def test_graph_replay_of_the_rank_32_step_is_bit_identical_to_eager():
    from gslora_hip.optim import FusedAdamW
    from gslora_hip.step import GraphedStep, gs_lora_step
    from test_hip_graph import batch, build
    cfg, b = recipe.cfg_small2(lora_rank=32), 6
    m1 = build(cfg, "fp16", 0.1)
    m2 = copy.deepcopy(m1)
    mk_opt = lambda m: FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-2, weight_decay=0.05, eps=1e-8)
    o1, o2 = mk_opt(m1), mk_opt(m2)
    crit = torch.nn.CrossEntropyLoss()
    kw = dict(beta=0.15, alpha=1e-2, BND=105.0, use_structure=True, group_type="block", use_prototype=True,
              proto_table=torch.tensor(recipe.make_prototypes(cfg)).cuda(), w_f=0.05, w_r=0.1, BND_pro=2.0)
    g = GraphedStep(m2, o2, crit)
    for s in range(4):
        xr, yr, xf, yf = batch(cfg, b, s)
        p1 = gs_lora_step(m1, o1, crit, xr, yr, xf, yf, **kw)
        p2 = g(xr, yr, xf, yf, **kw)
        assert torch.equal(p1, p2), (s, p1.tolist(), p2.tolist())
        for (n, a), (_, c) in zip(m1.named_parameters(), m2.named_parameters()):
            if a.requires_grad:
                assert torch.equal(a, c), (s, n)
    assert (g.eager_steps, g.captures, g.replays) == (1, 1, 3)


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_vits_face_at_rank_32(mode):
    """ViTs_face (overlapping patches) at r = 32: the 16-bit modes within the declared tolerance of its f32 mode."""
    cfg = recipe.cfg_small2(lora_rank=32)

    def run(dtype):
        m = TV.build(cfg, dtype=dtype).train()
        xr, yr, xf, yf = TV.batches(cfg, 3)
        with torch.no_grad():
            lo, em = m(xr, yr)
        total, _ = TV.total_loss(m, cfg, xr, yr, xf, yf, HYPER, protos(cfg))
        total.backward()
        return lo.float().cpu().numpy(), em.float().cpu().numpy(), TV.lora_grads(m)
    if "vits" not in _F32:
        _F32["vits"] = run("fp32")
    ref = _F32["vits"]
    assert all(np.isfinite(v).all() and np.abs(v).max() > 0 for v in ref[2].values())
    within_band(run(mode), ref, mode, f"ViTs_face {mode}")


# ------------------------------------------------------------------------------------------------------------ two data-parallel ranks
def test_two_ranks_at_rank_32_equal_the_single_process_step(tmp_path):
    """tests/test_hip_dp_two_ranks.py at r = 32 (f32 mode): identical replicas on both ranks, equal to the single-process step on the whole
    batch: meters and first-step gradients within that test's f32 tolerance, parameters as far as AdamW conditions them."""
    sys.path.insert(0, HERE)
    import lora_rank_dp_child as C
    from test_hip_graph import build
    from gslora_hip.optim import FusedAdamW
    from gslora_hip.step import gs_lora_step
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    outs = [str(tmp_path / f"rank{r}.npz") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "lora_rank_dp_child.py"), str(r), "2", str(port), "fp32", outs[r]],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    try:
        logs = [p.communicate(timeout=300) for p in procs]      # each rank under its own time limit
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 and "LORA-RANK-DP-OK" in lg[0] for p, lg in zip(procs, logs)), \
        [(p.returncode, lg[0][-500:], lg[1][-3000:]) for p, lg in zip(procs, logs)]
    r0, r1 = (dict(np.load(o)) for o in outs)
    for k in r0:
        assert np.array_equal(r0[k], r1[k]), k
    cfg, tol = C.config(), 2e-5
    m = build(cfg, "fp32", 0.0)
    opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-2, weight_decay=0.05, eps=1e-8)
    crit = torch.nn.CrossEntropyLoss()
    kw = C.hyper(cfg)
    packs, grad1 = [], {}
    for s in range(C.STEPS):
        packs.append(gs_lora_step(m, opt, crit, *C.whole_batch(cfg, 2, s), **kw).cpu().numpy())
        if s == 0:
            grad1 = {n: p.grad.detach().float().cpu().numpy() for n, p in m.named_parameters() if p.requires_grad}
    assert np.allclose(r0["packs"], np.stack(packs), rtol=tol, atol=tol), (r0["packs"], packs)
    # The gradients are linear in the batch: two half-batch sums against one whole-batch sum differ by the f32 summation order alone.
    for n, gw in grad1.items():
        assert np.abs(r0["grad1::" + n] - gw).max() < tol * max(1.0, np.abs(gw).max()), n
    # The parameters went through three AdamW updates, lr * m / (sqrt(v) + eps): where |g| is of the order of eps = 1e-8 the quotient
    # turns a summation-order difference of the gradient into a difference of up to the whole step (the remark in
    # tests/test_hip_heads.py: bounded there, not pinned). So: no element further apart than AdamW can move it (2.05 * lr per step, as
    # that test bounds it), and the well-conditioned bulk, 99 % of every tensor, within the 5 * tol of tests/test_hip_dp_two_ranks.py.
    for n, p in m.named_parameters():
        if p.requires_grad:
            a, b = p.detach().float().cpu().numpy(), r0[n]
            diff = np.abs(a - b)
            assert diff.max() <= 2.05 * 1e-2 * C.STEPS, n
            assert np.mean(diff < 5 * tol * np.abs(a).max()) > 0.99, (n, float(np.mean(diff < 5 * tol * np.abs(a).max())))
