"""Model- and step-level parity of the HIP path against (a) the golden vectors produced by the real
reference and (b) the CPU oracle on the same seeded inputs.

Tolerances (north_star): f32 mode — logits / per-group LoRA norms within 1e-4 absolute, group
selection mask bit-exact. bf16 mode (speed mode: bf16 GEMM operands, f32 accumulate, f32 residual
stream) — stated per assertion; logits carry the CosFace scale 64, so 0.25 absolute is ~4e-3 on
the cosine."""
import copy
import os

import numpy as np
import pytest
import torch

from oracle import gslora_oracle as O
from oracle import recipe

pytestmark = pytest.mark.gpu

CASES = {"small_b5": (recipe.cfg_small(), 5), "small2_b3": (recipe.cfg_small2(), 3), "full_b2": (recipe.cfg_full(), 2)}
HYPER = dict(lr=1e-2, wd=0.05, beta=0.15, alpha=1e-2, BND=105.0, BND_pro=2.0, pro_f_weight=0.05, pro_r_weight=0.1)


def build(cfg, dtype="fp32", dropout=0.0, state=None):
    import loralib as lora
    from vit_pytorch_face import ViT_face
    m = ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"],
                 patch_size=cfg["patch_size"], dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"],
                 dropout=dropout, emb_dropout=dropout, lora_rank=cfg["lora_rank"])
    state = state or recipe.make_state(cfg)
    m.load_state_dict({k: torch.tensor(v) for k, v in state.items()}, strict=True)
    lora.mark_only_lora_as_trainable(m)
    return m.to("cuda").set_compute_dtype(dtype)


def batches(cfg, batch, s=0):
    nf = max(2, cfg["num_class"] // 5)
    mk = lambda a: torch.tensor(a).cuda()
    return (mk(recipe.make_images(cfg, batch, seed=100 + s, tag="xr")),
            mk(recipe.make_labels(cfg, batch, seed=100 + s, tag="yr", lo=0, hi=cfg["num_class"] - nf)),
            mk(recipe.make_images(cfg, batch, seed=200 + s, tag="xf")),
            mk(recipe.make_labels(cfg, batch, seed=200 + s, tag="yf", lo=cfg["num_class"] - nf, hi=cfg["num_class"])))


def lora_grads(model):
    return {n: p.grad.detach().cpu().numpy().copy() for n, p in model.named_parameters() if p.requires_grad}


def total_loss(model, xr, yr, xf, yf, hy, proto):
    import engine
    import engine_cl
    crit_sum = lambda lo, y: torch.nn.functional.cross_entropy(lo, y)
    lo_r, em_r = model(xr, yr)
    lo_f, em_f = model(xf, yf)
    from gslora_hip import losses
    ce_r = losses.ce_sum_top1(lo_r, yr)[0] / xr.shape[0]
    ce_f = losses.ce_sum_top1(lo_f, yf)[0] / xf.shape[0]
    sl = engine.get_structure_loss(model, num_layers=model.depth, group_type="block")
    kl_f = engine_cl.get_prototype_loss(em_f, yf, proto)
    kl_r = engine_cl.get_prototype_loss(em_r, yr, proto)
    pro = hy["pro_f_weight"] * torch.relu(hy["BND_pro"] - kl_f) + hy["pro_r_weight"] * kl_r
    total = hy["beta"] * torch.relu(hy["BND"] - ce_f) + ce_r + hy["alpha"] * sl + pro
    return total, dict(ce_f=ce_f, ce_r=ce_r, sl=sl, kl_f=kl_f, kl_r=kl_r, logits_r=lo_r, emb_r=em_r)


@pytest.mark.parametrize("tag", list(CASES))
def test_forward_f32_matches_reference(tag, golden_dir):
    cfg, b = CASES[tag]
    g = np.load(os.path.join(golden_dir, f"{tag}.npz"))
    m = build(cfg, "fp32").train()
    xr, yr, _, _ = batches(cfg, b)
    with torch.no_grad():
        logits, emb = m(xr, yr)
        emb2 = m(xr)
    assert np.abs(logits.cpu().numpy() - g["fwd_logits"]).max() < 1e-4
    assert np.abs(emb.cpu().numpy() - g["fwd_emb"]).max() < 1e-4
    assert np.abs(emb2.cpu().numpy() - g["fwd_emb_nolabel"]).max() < 1e-4
    # eval(): loralib merge semantics, merged weights and logits match the reference's eval pass
    m.eval()
    w = m.state_dict()["transformer.layers.0.1.fn.fn.net.0.weight"].cpu().numpy()
    assert np.abs(w - g["merged_w_l0_net0"]).max() < 1e-6
    with torch.no_grad():
        le, ee = m(xr, yr)
    assert np.abs(le.cpu().numpy() - g["eval_logits"]).max() < 1e-4
    m.train()
    with torch.no_grad():
        lt, _ = m(xr, yr)
    assert np.abs(lt.cpu().numpy() - g["roundtrip_logits"]).max() < 1e-4


@pytest.mark.parametrize("tag", list(CASES))
def test_forward_bf16_close_to_reference(tag, golden_dir):
    cfg, b = CASES[tag]
    g = np.load(os.path.join(golden_dir, f"{tag}.npz"))
    m = build(cfg, "bf16").train()
    xr, yr, _, _ = batches(cfg, b)
    with torch.no_grad():
        logits, emb = m(xr, yr)
    # bf16 operands through depth x (attention + FFN): cosine error ~4e-3 -> logits (x64) within 0.25
    assert np.abs(logits.cpu().numpy() - g["fwd_logits"]).max() < 0.25
    assert np.abs(emb.cpu().numpy() - g["fwd_emb"]).max() < 0.05


@pytest.mark.parametrize("tag", list(CASES))
def test_group_norms_and_mask_match_reference(tag, golden_dir):
    import engine
    from gslora_hip.losses import group_report
    from util.cal_norm import get_norm_of_lora
    cfg, b = CASES[tag]
    g = np.load(os.path.join(golden_dir, f"{tag}.npz"))
    m = build(cfg, "fp32")
    st = O.to_torch(recipe.make_state(cfg))
    for gt in ("block", "lora", "matrix"):
        sl = engine.get_structure_loss(m, num_layers=cfg["depth"], group_type=gt).item()
        assert abs(sl - float(g[f"structure_loss_engine_{gt}"])) < 1e-4
        cn = np.array([float(v) for v in get_norm_of_lora(m, type="L2", group_num=cfg["depth"], group_type=gt)])
        assert np.abs(cn - g[f"cal_norm_{gt}"]).max() < 1e-4
        rep = group_report(m, gt, tau=0.0)
        ref_norms = O.group_lasso_norms(st, cfg, gt)
        assert np.abs(rep["group_norm"].cpu().numpy() - ref_norms.numpy()).max() < 1e-4
        assert rep["mask"].cpu().bool().tolist() == O.group_mask(ref_norms, 0.0).tolist()       # bit-exact mask
    if cfg["depth"] == 6:
        import engine_cl
        assert abs(engine_cl.get_structure_loss(m).item() - float(g["structure_loss"])) < 1e-4
    # an exactly-zero group is deselected, and its gradient is 0 rather than NaN
    with torch.no_grad():
        for p in m.lora_bucket().params[:4]:
            p.zero_()
    rep = group_report(m, "block", tau=0.0)
    assert rep["mask"].cpu().tolist()[0] == 0 and all(rep["mask"].cpu().tolist()[1:])
    sl = engine.get_structure_loss(m, num_layers=cfg["depth"], group_type="block")
    sl.backward()
    assert all(torch.isfinite(p.grad).all() for p in m.lora_bucket().params)
    assert all((p.grad == 0).all() for p in m.lora_bucket().params[:4])


@pytest.mark.parametrize("tag", ["small_b5", "small2_b3"])
def test_grads_f32_match_reference(tag, golden_dir):
    cfg, b = CASES[tag]
    g = np.load(os.path.join(golden_dir, f"{tag}.npz"))
    m = build(cfg, "fp32").train()
    xr, yr, xf, yf = batches(cfg, b)
    proto = {c: torch.tensor(v) for c, v in enumerate(recipe.make_prototypes(cfg))}
    total, parts = total_loss(m, xr, yr, xf, yf, HYPER, proto)
    ref = g["losses1"]
    got = [parts["ce_f"].item(), parts["ce_r"].item(), total.item(), parts["sl"].item(), parts["kl_f"].item(), parts["kl_r"].item()]
    for a, r in zip(got, ref):
        assert abs(a - r) < 1e-4 * max(1.0, abs(r))
    m.zero_grad()
    total.backward()
    for k, v in lora_grads(m).items():
        r = g[f"grad1::{k}"]
        assert np.abs(v - r).max() < 1e-4 * max(1.0, np.abs(r).max()), k
    # both hinges inactive
    hy2 = dict(HYPER, BND=5.0, BND_pro=0.1)
    for p in m.parameters():
        p.grad = None
    total2, _ = total_loss(m, xr, yr, xf, yf, hy2, proto)
    assert abs(total2.item() - float(g["total_inactive"])) < 1e-3
    total2.backward()
    for k, v in lora_grads(m).items():
        r = g[f"grad_inactive::{k}"]
        assert np.abs(v - r).max() < 1e-4 * max(1.0, np.abs(r).max()), k


def test_full_engine_three_steps_f32_match_reference(golden_dir):
    """The build's engine_cl.train_one_epoch + FusedAdamW reproduce the reference engine + torch AdamW:
    meters, first-step LoRA gradients, parameters after 1 and 3 steps."""
    import engine_cl
    from gslora_hip.optim import FusedAdamW
    from util.utils import AverageMeter
    cfg, b = CASES["full_b2"]
    g = np.load(os.path.join(golden_dir, "full_b2.npz"))
    m = build(cfg, "fp32")
    opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=HYPER["lr"], weight_decay=HYPER["wd"], eps=1e-8)
    crit = torch.nn.CrossEntropyLoss()
    names = ["losses_forget", "losses_remain", "losses_total", "losses_structure", "top1_forget", "top1_remain",
             "losses_prototype_forget", "losses_prototype_remain"]
    meters = {k: AverageMeter() for k in names}
    proto = {c: torch.tensor(v) for c, v in enumerate(recipe.make_prototypes(cfg))}
    cfgd = {"DATA_ROOT": "./data/casia100/", "BND_pro": HYPER["BND_pro"], "MULTI_GPU": False, "WORK_PATH": "/tmp", "BACKBONE_NAME": "VIT"}
    batch_ctr = 0
    for s in range(3):
        xr, yr, xf, yf = batches(cfg, b, s)
        ret = engine_cl.train_one_epoch(
            model=m, dataloader_forget=[(xf.cpu(), yf.cpu())], dataloader_remain=[(xr.cpu(), yr.cpu())],
            device=torch.device("cuda"), criterion=crit, optimizer=opt, epoch=0, beta=HYPER["beta"], alpha=HYPER["alpha"],
            BND=HYPER["BND"], batch=batch_ctr, testloader_forget=None, testloader_remain=None, forget_acc_before=0.0,
            highest_H_mean=0.0, cfg=cfgd, task_i="0", use_prototype=True, prototype_dict=proto,
            prototype_weight_forget=HYPER["pro_f_weight"], prototype_weight_remain=HYPER["pro_r_weight"], **meters)
        batch_ctr = ret[0]
        assert len(ret) == 10
        if s == 0:
            got = np.array([meters[k].val for k in names])
            assert np.abs(got - g["meters1"]).max() < 1e-3, (got, g["meters1"])
            for k, v in lora_grads(m).items():
                r = g[f"grad1::{k}"]
                assert np.abs(v - r).max() < 1e-4 * max(1.0, np.abs(r).max()), k
        # optimizer parity, decomposed so that it is well-conditioned: (1) the first-step gradients match the
        # reference (above); (2) the HIP AdamW applied to the HIP gradients equals the oracle's AdamW applied
        # to the SAME gradients (AdamW's lr*m/(sqrt(v)+eps) has d(update)/dg up to lr/eps = 1e6 where |g|~eps,
        # so comparing parameters across two different gradient roundings is meaningless there).
        g_hip = {n: torch.tensor(v) for n, v in lora_grads(m).items()}
        if s == 0:
            track = {n: (torch.tensor(recipe.make_state(cfg)[n]), torch.zeros_like(g_hip[n]), torch.zeros_like(g_hip[n])) for n in g_hip}
        for n in g_hip:
            p0, m0, v0 = track[n]
            track[n] = O.adamw_update(p0, g_hip[n], m0, v0, s + 1, HYPER["lr"], HYPER["wd"])
            got_p = dict(m.named_parameters())[n].detach().cpu()
            assert (got_p - track[n][0]).abs().max() < 2e-6, (s, n)
        if s == 0:   # against the reference's parameters where the update is well-conditioned
            for n in g_hip:
                well = np.abs(g[f"grad1::{n}"]) > 1e-6
                diff = np.abs(dict(m.named_parameters())[n].detach().cpu().numpy() - g[f"param1::{n}"])
                assert diff[well].max(initial=0.0) < 2e-4, n
                assert diff.max() <= 2.05 * HYPER["lr"], n
    got = np.array([meters[k].avg for k in names])
    assert np.abs(got - g["meters3_avg"]).max() < 2e-3
    assert batch_ctr == int(g["batch_ctr"])


def test_bf16_grads_close_to_f32():
    """speed mode vs parity mode on the same inputs: LoRA gradients agree to bf16 accuracy
    (relative Frobenius error per tensor < 6 %, cosine > 0.995)."""
    cfg, b = recipe.cfg_small2(), 6
    proto = {c: torch.tensor(v) for c, v in enumerate(recipe.make_prototypes(cfg))}
    xr, yr, xf, yf = batches(cfg, b)
    grads = {}
    for dt in ("fp32", "bf16"):
        m = build(cfg, dt).train()
        total, _ = total_loss(m, xr, yr, xf, yf, HYPER, proto)
        total.backward()
        grads[dt] = lora_grads(m)
    for k in grads["fp32"]:
        a, r = grads["bf16"][k].ravel(), grads["fp32"][k].ravel()
        if np.linalg.norm(r) == 0:
            continue
        assert np.linalg.norm(a - r) / np.linalg.norm(r) < 0.06, k
        assert float(a @ r) / (np.linalg.norm(a) * np.linalg.norm(r)) > 0.995, k


def test_oracle_step_parity_larger_batch():
    """f32 HIP step vs the CPU oracle on a batch the golden files do not cover (ragged: 7 + 5)."""
    cfg = recipe.cfg_small2()
    st_np = recipe.make_state(cfg)
    m = build(cfg, "fp32", state=st_np).train()
    xr, yr, _, _ = batches(cfg, 7, s=3)
    _, _, xf, yf = batches(cfg, 5, s=4)
    proto_np = recipe.make_prototypes(cfg)
    proto = {c: torch.tensor(v) for c, v in enumerate(proto_np)}
    total, parts = total_loss(m, xr, yr, xf, yf, HYPER, proto)
    total.backward()
    losses, grads, _, _ = O.train_step(st_np, cfg, xr.cpu(), yr.cpu(), xf.cpu(), yf.cpu(), HYPER, proto=torch.tensor(proto_np))
    assert abs(total.item() - float(losses["total"])) < 1e-4 * max(1, abs(float(losses["total"])))
    assert (parts["logits_r"].detach().cpu() - losses["logits_r"]).abs().max() < 1e-4
    for k, v in lora_grads(m).items():
        r = grads[k].numpy()
        assert np.abs(v - r).max() < 1e-4 * max(1.0, np.abs(r).max()), k


def test_dropout_path_is_deterministic_and_unbiased():
    """p=0.1 (the reference's training setting) cannot be bit-matched to torch's Bernoulli stream; check
    determinism for a fixed (seed, call), that different calls differ, and that the mean output over
    masks approaches the p=0 output (inverted-dropout scaling is unbiased)."""
    cfg = recipe.cfg_small2()
    m = build(cfg, "fp32", dropout=0.1).train()
    xr, yr, _, _ = batches(cfg, 4)
    with torch.no_grad():
        r = m.runner()
        r.drop_calls = 10
        a, _ = m(xr, yr)
        r.drop_calls = 10
        b, _ = m(xr, yr)
        c, _ = m(xr, yr)
    assert torch.equal(a, b) and not torch.equal(a, c)
    m.eval()
    with torch.no_grad():
        e, _ = m(xr, yr)
        e2, _ = m(xr, yr)
    assert torch.equal(e, e2)          # eval: no dropout
    # backward regenerates the same masks: gradient of a fixed-seed stochastic forward is reproducible
    m.train()
    gs = []
    for _ in range(2):
        for p in m.parameters():
            p.grad = None
        m.runner().drop_calls = 77
        lo, em = m(xr, yr)
        (lo.square().mean() + em.sum()).backward()
        gs.append(lora_grads(m))
    assert all(np.array_equal(gs[0][k], gs[1][k]) for k in gs[0])


def test_dropout_grads_match_autograd_with_same_masks():
    """With p>0 the backward must use exactly the masks of the forward. Rebuild the masks on the host
    with gsl_dropout_mask and differentiate the oracle forward (masks injected) with autograd."""
    from gslora_hip import ops
    cfg = recipe.cfg_small()
    st_np = recipe.make_state(cfg)
    p = 0.2
    m = build(cfg, "fp32", dropout=p, state=st_np).train()
    xr, yr, _, _ = batches(cfg, 3)
    r = m.runner()
    r.drop_calls = 41
    lo, em = m(xr, yr)
    seed = (r.drop_seed << 20) + 42
    (lo.square().mean() + em.sum()).backward()
    got = lora_grads(m)
    # oracle with identical masks: the mask-injected forward of tests/large_row_reference.py (which knows the sites, and that the last
    # block's counters index a compact [B, width] tensor: it runs on the cls rows only under pool='cls')
    import large_row_reference as LR
    keep = lambda n, site: ops.dropout_mask(n, p, seed, site, "cuda").cpu().float() / (1 - p)
    st = O.to_torch(st_np, requires_grad_lora=True)
    logits, emb, _ = LR.forward(st, xr.cpu(), yr.cpu(), cfg, keep=keep, dtype=torch.float32)
    assert (lo.detach().cpu() - logits.detach()).abs().max() < 1e-4
    names = [k for k in st if "lora_" in k]
    gr = torch.autograd.grad(logits.square().mean() + emb.sum(), [st[k] for k in names])
    for k, gref in zip(names, gr):
        assert np.abs(got[k] - gref.numpy()).max() < 1e-4 * max(1.0, gref.abs().max().item()), k


def test_task_chain_merge_save_reload_reinit():
    """Continual-learning plumbing (train_own_forget_cl.py:524-536, 1696-1705): save in eval (merged)
    mode, reload, re-initialise LoRA (B=0) -> logits unchanged; deepcopy keeps working."""
    from util.utils import reinitialize_lora_parameters
    cfg = recipe.cfg_small2()
    m = build(cfg, "fp32").train()
    xr, yr, _, _ = batches(cfg, 3)
    with torch.no_grad():
        before, _ = m(xr, yr)
    m.eval()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m.train()
    m2 = build(cfg, "fp32")
    missing = m2.load_state_dict(sd, strict=False)
    reinitialize_lora_parameters(m2)
    m2.train()
    with torch.no_grad():
        after, _ = m2(xr, yr)
    assert (before - after).abs().max() < 1e-4
    assert all((p == 0).all() for n, p in m2.named_parameters() if "lora_B" in n)
    bound = O.reinit_bound(cfg["dim"])
    a0 = dict(m2.named_parameters())["transformer.layers.0.1.fn.fn.net.0.lora_A"]
    assert a0.abs().max() <= bound + 1e-7 and a0.abs().max() > 0.8 * bound
    m3 = copy.deepcopy(m).train()
    with torch.no_grad():
        again, _ = m3(xr, yr)
    assert (before - again).abs().max() < 1e-5
    assert m3.lora_bucket() is not m.lora_bucket()


def test_prototypes_match_reference(golden_dir):
    from util.utils import calculate_prototypes
    for tag, (cfg, b) in CASES.items():
        g = np.load(os.path.join(golden_dir, f"{tag}.npz"))
        m = build(cfg, "fp32")
        xr, yr, xf, yf = batches(cfg, b)
        ds = torch.utils.data.TensorDataset(torch.cat([xr, xf]).cpu(), torch.cat([yr, yf]).cpu())
        protos = calculate_prototypes(m, ds, batch_size=3, device="cuda")
        assert sorted(protos) == list(g["proto_keys"])
        got = np.stack([protos[k].numpy() for k in sorted(protos)])
        assert np.abs(got - g["proto_vals"]).max() < 1e-4
        assert not m.training      # the reference leaves the model in eval() too


def test_cpu_inputs_fail_loudly():
    cfg = recipe.cfg_small()
    m = build(cfg, "fp32")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 3, 40, 40), torch.zeros(1, dtype=torch.long))


def test_own_cl_driver_two_tasks(tmp_path):
    """The build's counterpart of train_own_forget_cl.py: task loop with prototypes, per-task optimizer and
    cosine schedule, engine_cl.train_one_epoch, LoRA-norm report, merged checkpoint, reload + re-init."""
    import driver_cl
    rep, out, model = driver_cl.main(["--small", "--num_class", "20", "--num_tasks", "2", "--per_forget_cls", "4", "--epochs", "2",
                                      "--batch_size", "16", "--samples_per_class", "4", "--dtype", "fp32", "--dropout", "0.0",
                                      "--outdir", str(tmp_path)])
    assert [r["task"] for r in rep] == [0, 1]
    order = O.class_order(20, 1337)
    assert rep[0]["forget_cls"] == order[16:20] and rep[1]["forget_cls"] == order[12:16]       # en1 = num_first - i*per_forget
    for r in rep:
        assert abs(r["lrs"][0] - 1e-2) < 1e-12 and abs(r["lrs"][1] - O.cosine_lr(1, epochs=2)) < 1e-12
        assert len(r["norms"]) == 3 and all(np.isfinite(r["norms"])) and np.isfinite(r["total_loss"])
        n_remain = (16 - 4 * r["task"]) * 4              # remain classes shrink by per_forget_cls every task
        assert r["steps"] == 2 * -(-n_remain // 16)      # two epochs over the remain loader (drop_last=False)
    assert os.path.exists(os.path.join(out, "task-level", "Backbone_task_1.pth"))
    # the saved checkpoint is in merged form: loading it and zeroing B reproduces the trained model's eval logits
    sd = torch.load(os.path.join(out, "task-level", "Backbone_task_1.pth"), map_location="cpu")
    x = torch.rand(3, 3, 48, 48).cuda(); y = torch.tensor([1, 2, 3]).cuda()
    model.eval()
    with torch.no_grad():
        ref, _ = model(x, y)
    m2 = copy.deepcopy(model)
    m2.load_state_dict(sd)
    from util.utils import reinitialize_lora_parameters
    reinitialize_lora_parameters(m2)
    m2.train()
    with torch.no_grad():
        got, _ = m2(x, y)
    assert (ref - got).abs().max() < 1e-4


def test_own_cl_driver_ema_model_reproduces_reference_quirk(tmp_path):
    """--average_weight (reference train_own_forget_cl.py:502-507, 1058-1098): the EMA model is a deep copy taken in eval() — its
    adapters stay flagged merged — into which the TRAIN-mode (un-merged) parameters are copied / averaged. Reproduced, not fixed: at
    epoch == ema_epoch the EMA model therefore evaluates the frozen backbone without the current adapters."""
    import driver_cl
    rep, out, (model, ema) = driver_cl.main(["--small", "--num_class", "20", "--num_tasks", "1", "--per_forget_cls", "4", "--epochs", "2",
                                             "--batch_size", "16", "--samples_per_class", "4", "--dtype", "fp32", "--dropout", "0.0",
                                             "--average_weight", "--ema_epoch", "1", "--ema_decay", "0.9", "--outdir", str(tmp_path)])
    assert rep[0]["ema_acc"] is not None and all(0.0 <= a <= 100.0 for a in rep[0]["ema_acc"])
    assert all(blk.l1.merged and blk.l2.merged for blk in ema.hip_spec().blocks)
    x = torch.rand(3, 3, 48, 48).cuda(); y = torch.tensor([1, 2, 3]).cuda()
    base = copy.deepcopy(model).train()           # the trained model with its adapters zeroed = frozen backbone only
    with torch.no_grad():
        for n, p in base.named_parameters():
            if n.endswith("lora_B"):
                p.zero_()
        want, _ = base(x, y)
        ema.eval()
        got, _ = ema(x, y)
    assert (want - got).abs().max() < 1e-4


def _fresh(cfg, dtype="fp32"):
    from gslora_hip.optim import FusedAdamW
    m = build(cfg, dtype).train()
    opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-2, weight_decay=0.05, eps=1e-8)
    return m, opt


def test_fused_batch_step_equals_two_forward_step():
    """gs_lora_step concatenates the remain and forget batches into one forward; with p=0 that must be exactly the
    reference's two-forward arithmetic (per-sample network)."""
    from gslora_hip import losses
    from gslora_hip.step import gs_lora_step
    cfg = recipe.cfg_small2()
    xr, yr, xf, yf = batches(cfg, 5)
    proto = losses.prototype_table({c: torch.tensor(v) for c, v in enumerate(recipe.make_prototypes(cfg))}, "cuda")
    outs = []
    for fuse in (True, False):
        m, opt = _fresh(cfg)
        pack = gs_lora_step(m, opt, torch.nn.CrossEntropyLoss(), xr, yr, xf, yf, beta=0.15, alpha=1e-2, BND=105.0, use_prototype=True,
                            proto_table=proto, w_f=0.05, w_r=0.1, BND_pro=2.0, fuse_batches=fuse)
        outs.append((pack.cpu(), {n: p.detach().cpu().clone() for n, p in m.named_parameters() if p.requires_grad}))
    assert (outs[0][0] - outs[1][0]).abs().max() < 1e-4
    for n in outs[0][1]:
        assert (outs[0][1][n] - outs[1][1][n]).abs().max() < 1e-5, n


def test_single_task_engine_alpha_gate_grouping_and_fewshot_swap():
    """engine.train_one_epoch (reference engine.py): structure term gated by ALPHA_EPOCH, GROUP_TYPE grouping, literal
    prototype bound 18, and the few-shot loader inversion (iterate the longer forget loader, cycle the remain loader)."""
    import engine
    from util.utils import AverageMeter
    cfg = recipe.cfg_small2()
    names = ["losses_forget", "losses_remain", "losses_total", "losses_structure", "top1_forget", "top1_remain"]
    proto = {c: torch.tensor(v) for c, v in enumerate(recipe.make_prototypes(cfg))}
    def run(epoch, cfgd, n_forget_batches, n_remain_batches):
        m, opt = _fresh(cfg)
        fb = [tuple(t.cpu() for t in batches(cfg, 4, s)[2:]) for s in range(n_forget_batches)]
        rb = [tuple(t.cpu() for t in batches(cfg, 4, s)[:2]) for s in range(n_remain_batches)]
        meters = {k: AverageMeter() for k in names}
        ret = engine.train_one_epoch(model=m, dataloader_forget=fb, dataloader_remain=rb, device=torch.device("cuda"),
                                     criterion=torch.nn.CrossEntropyLoss(), optimizer=opt, epoch=epoch, beta=0.15, alpha=1e-2, BND=105.0,
                                     batch=0, testloader_forget=None, testloader_remain=None, forget_acc_before=0.0, highest_H_mean=0.0,
                                     cfg=cfgd, use_prototype=True, prototype_dict=proto, prototype_weight_forget=0.05,
                                     prototype_weight_remain=0.1, **meters)
        return ret, meters
    base = {"ALPHA_EPOCH": 1, "GROUP_TYPE": "lora", "GROUP_POS": "FFN", "NUM_LAYERS": cfg["depth"], "few_shot": False,
            "MULTI_GPU": False, "WORK_PATH": "/tmp", "BACKBONE_NAME": "VIT"}
    ret, met = run(0, base, 1, 2)                       # epoch < ALPHA_EPOCH: no structure term
    assert ret[0] == 2 and met["losses_structure"].val == 0.0 and len(ret) == 10
    ret, met = run(1, base, 1, 2)                       # gated on; 'lora' grouping = 2*depth groups
    st = O.to_torch(recipe.make_state(cfg))
    # the meter holds alpha * structure of the parameters at the LAST step; at step 1 it equals the oracle on the initial state
    ret1, met1 = run(1, base, 1, 1)
    assert abs(met1["losses_structure"].val - 1e-2 * O.structure_loss(st, cfg, "lora").item()) < 1e-5
    ret, met = run(1, dict(base, few_shot=True), 3, 1)  # few-shot inversion: 3 forget batches drive the loop
    assert ret[0] == 3
    ret, met = run(1, dict(base, few_shot=False), 3, 1)
    assert ret[0] == 1


def test_fused_adamw_state_dict_round_trip():
    """FusedAdamW.state_dict() speaks torch.optim.AdamW's layout (step / exp_avg / exp_avg_sq per parameter): a checkpoint taken after two
    steps continues identically in a fresh FusedAdamW and in torch.optim.AdamW (the flat moments used to be dropped)."""
    from gslora_hip.optim import FusedAdamW
    cfg = recipe.cfg_small2()
    proto = {c: torch.tensor(v) for c, v in enumerate(recipe.make_prototypes(cfg))}
    m = build(cfg, "fp32").train()
    params = [p for p in m.parameters() if p.requires_grad]
    opt = FusedAdamW(params, lr=1e-2, weight_decay=0.05, eps=1e-8)
    for s in range(2):
        xr, yr, xf, yf = batches(cfg, 3, s)
        total, _ = total_loss(m, xr, yr, xf, yf, HYPER, proto)
        opt.zero_grad()
        total.backward()
        opt.step()
    sd = copy.deepcopy(opt.state_dict())
    assert len(sd["state"]) == len(params) and all(float(v["step"]) == 2.0 for v in sd["state"].values())
    p0 = [p.detach().clone() for p in params]
    xr, yr, xf, yf = batches(cfg, 3, 2)
    total, _ = total_loss(m, xr, yr, xf, yf, HYPER, proto)
    opt.zero_grad()
    total.backward()
    grads = [p.grad.detach().clone() for p in params]
    opt.step()
    want = [p.detach().clone() for p in params]
    # (1) torch.optim.AdamW restored from the same checkpoint, same gradients
    tp = [torch.nn.Parameter(q.clone()) for q in p0]
    topt = torch.optim.AdamW(tp, lr=1e-2, weight_decay=0.05, eps=1e-8)
    topt.load_state_dict(copy.deepcopy(sd))      # (torch keeps references to the tensors it is handed and steps them in place)
    for q, g in zip(tp, grads):
        q.grad = g.clone()
    topt.step()
    for q, w in zip(tp, want):
        assert (q.detach() - w).abs().max() < 2e-6
    # (2) a fresh FusedAdamW restored from the checkpoint
    with torch.no_grad():
        for p, q in zip(params, p0):
            p.copy_(q)
    opt2 = FusedAdamW(params, lr=1e-2, weight_decay=0.05, eps=1e-8)
    opt2.load_state_dict(sd)
    for p, g in zip(params, grads):
        p.grad.copy_(g)
    opt2.step()
    for p, w in zip(params, want):
        assert torch.equal(p.detach(), w)


def test_prototype_label_outside_table_is_loud():
    """A batch label without a prototype: the reference raises KeyError (engine_cl.py:587-589); the device-side look-up cannot raise
    without a host sync, so the loss turns NaN — never an out-of-bounds read, never a silent all-zero prototype."""
    import engine_cl
    emb = torch.randn(4, 64, device="cuda")
    proto = {0: torch.randn(64), 2: torch.randn(64)}
    ok = engine_cl.get_prototype_loss(emb, torch.tensor([0, 2, 2, 0], device="cuda"), proto)
    assert torch.isfinite(ok)
    assert torch.isnan(engine_cl.get_prototype_loss(emb, torch.tensor([0, 1, 2, 0], device="cuda"), proto))      # class 1: hole in the table
    assert torch.isnan(engine_cl.get_prototype_loss(emb, torch.tensor([0, 2, 7, 0], device="cuda"), proto))      # class 7: beyond the table


@pytest.mark.parametrize("cfgname", ["small2", "full"])
def test_bf16_step_identical_in_both_qkv_layouts(monkeypatch, cfgname):
    """The head-major qkv stash (default in bf16 mode) and the token-major one (vit_runner.QKV_HEAD_MAJOR = False) run the same arithmetic in the same
    order — the QKV GEMM's store only permutes, the attention kernels only address differently: logits, embeddings, loss and every
    LoRA gradient of a training step with dropout are BIT-IDENTICAL."""
    from gslora_hip import vit_runner
    cfg, b = (recipe.cfg_small2(), 6) if cfgname == "small2" else (recipe.cfg_full(), 2)
    proto = {c: torch.tensor(v) for c, v in enumerate(recipe.make_prototypes(cfg))}
    xr, yr, xf, yf = batches(cfg, b)
    res = {}
    for hm in (True, False):
        monkeypatch.setattr(vit_runner, "QKV_HEAD_MAJOR", hm)
        torch.manual_seed(7)                       # the dropout stream is seeded from torch's seed when the runner is built
        m = build(cfg, "bf16", dropout=0.1).train()
        total, aux = total_loss(m, xr, yr, xf, yf, HYPER, proto)
        total.backward()
        res[hm] = (aux["logits_r"].detach().clone(), aux["emb_r"].detach().clone(), total.detach().clone(), lora_grads(m))
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1]) and torch.equal(res[True][2], res[False][2])
    for k, v in res[True][3].items():
        assert np.array_equal(v, res[False][3][k]), k


@pytest.mark.parametrize("knob,value,exact", [("TAIL_CLS", False, False), ("QSPLIT", False, False), ("GP8", False, False),
                                              ("FWD_STREAM", "bf16", False), ("FWD_STREAM", "f32", False), ("GRAD_STREAM_BF16", False, False)])
def test_bf16_step_under_every_remaining_runner_knob(monkeypatch, knob, value, exact):
    """every switch left in gslora_hip/vit_runner.py is exercised. The decided schedule forms (the last block's tail on
    the cls rows, Q projected for the cls rows only) are EXACT re-arrangements: against the forms they replaced the same bf16 step agrees to
    accumulation-order noise. The three precision knobs of the speed mode (8-bit GELU', bf16 forward / gradient residual streams) against
    their other forms (fp16 / bf16 / f32 forward stream): inside the declared bf16 band (logits 0.25 abs at scale 64, LoRA gradients 6 % relative Frobenius / cosine 0.995)."""
    from gslora_hip import vit_runner
    cfg, b = recipe.cfg_small2(), 6
    proto = {c: torch.tensor(v) for c, v in enumerate(recipe.make_prototypes(cfg))}
    xr, yr, xf, yf = batches(cfg, b)
    res = {}
    for alt in (False, True):
        if alt:
            monkeypatch.setattr(vit_runner, knob, value)
        torch.manual_seed(7)
        m = build(cfg, "bf16", dropout=0.0).train()
        total, aux = total_loss(m, xr, yr, xf, yf, HYPER, proto)
        total.backward()
        res[alt] = (aux["logits_r"].detach().float().clone(), total.detach().clone(), lora_grads(m))
    schedule = knob in ("TAIL_CLS", "QSPLIT")
    assert (res[False][0] - res[True][0]).abs().max().item() <= (0.05 if schedule else 0.25)      # (scale-64 logits: 0.05 = 8e-4 on the cosine)
    g0 = np.concatenate([v.ravel() for v in res[False][2].values()]).astype(np.float64)
    g1 = np.concatenate([v.ravel() for v in res[True][2].values()]).astype(np.float64)
    rel = np.linalg.norm(g0 - g1) / np.linalg.norm(g0)
    cos = float(g0 @ g1) / (np.linalg.norm(g0) * np.linalg.norm(g1))
    print(f"[knob {knob}={value}] logits max|d| {(res[False][0] - res[True][0]).abs().max().item():.4f}, LoRA-gradient rel. Frobenius {rel:.5f}, cosine {cos:.6f}")
    assert rel < (0.01 if schedule else 0.06) and cos > (0.9999 if schedule else 0.995)


@pytest.mark.parametrize("dtype,stream,dropout,tol_l,tol_g", [("fp16", "f16", 0.0, 0.05, 0.01), ("fp16", "f16", 0.1, 0.05, 0.01), ("bf16", "bf16", 0.1, 0.25, 0.06)])
def test_fp16_step_with_layernorm1_folded_into_the_qkv_projection_equals_the_unfolded_form(monkeypatch, dtype, stream, dropout, tol_l, tol_g):
    """Round 5: where the forward stream and the operands share one 16-bit format (fp16 mode; bf16 operands with GSLORA_FWD_STREAM=bf16)
    LayerNorm 1 is folded into the QKV GEMM (EPI_STORE_LN: the GEMM reads the stream with gamma folded into the weight and finishes the
    normalisation in its epilogue; LayerNorm 1 shrinks to its row statistics). Both forms compute the reference's ln1 -> to_qkv
    (vit_face.py:316-323, 358-360); they differ by rounding only (the folded form skips the 16-bit rounding of LN(x)): fp16 logits within 0.05
    at scale 64, LoRA gradients within 1 % relative Frobenius — far inside the fp16 band — (bf16: the declared bf16 band), including the last
    block's Q-split form, and with dropout ON (p = 0.1, the same counter-hash masks in both forms)."""
    from gslora_hip import vit_runner
    cfg, b = recipe.cfg_small2(), 6
    proto = {c: torch.tensor(v) for c, v in enumerate(recipe.make_prototypes(cfg))}
    xr, yr, xf, yf = batches(cfg, b)
    res = {}
    monkeypatch.setattr(vit_runner, "FWD_STREAM", stream)
    for fold in (True, False):
        monkeypatch.setattr(vit_runner, "LN1_FOLD", fold)
        torch.manual_seed(7)
        m = build(cfg, dtype, dropout=dropout).train()
        total, aux = total_loss(m, xr, yr, xf, yf, HYPER, proto)
        total.backward()
        res[fold] = (aux["logits_r"].detach().float().clone(), total.detach().clone(), lora_grads(m))
    dl = (res[False][0] - res[True][0]).abs().max().item()
    g0 = np.concatenate([v.ravel() for v in res[False][2].values()]).astype(np.float64)
    g1 = np.concatenate([v.ravel() for v in res[True][2].values()]).astype(np.float64)
    rel = np.linalg.norm(g0 - g1) / np.linalg.norm(g0)
    print(f"[LN1 fold on / off, {dtype} operands, {stream} stream, dropout {dropout}] logits max|d| {dl:.4f}, LoRA-gradient rel. Frobenius {rel:.5f}")
    assert dl <= tol_l and rel < tol_g
    assert not torch.equal(res[False][0], res[True][0])      # (the fold is live in this mode)
