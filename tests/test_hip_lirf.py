"""GPU tests of the LIRF baseline: ViT_face_low / ViT_face_up, the one pass over both halves with the attention-transfer gradient entering
at the boundary (vit_pytorch_face.vit_face.low_up_forward, ViTRunner._inject_at), gslora_hip.step.lirf_step and the loop over it. Models:
recipe.cfg_small (depth 2: one block each side, so the boundary block IS the cls-row-only last block) and recipe.cfg_small2 (depth 3: the odd
split, one lower and two upper blocks), lora_rank = 0, CosFace, dropout 0, the --only_ffn rule on the student's half.

The step's reference is a float64 restatement of the two half networks and of baselines/LIRFtrain.py:104-164 written here in plain torch,
fed the same weights: it holds the path of the attention-transfer term to the weights, which no route through existing pieces does (the
mid stream enters those only by value). Bars: values within 1e-4 * max(1, |want|), gradients within 1e-4 of the tensor's largest element,
weights within the parity bar (test_hip_ffn_train.bar_ok); 16-bit gradients within the 6 % relative Frobenius error and cosine > 0.995
that tests/test_hip_ffn_train.py declares. The REAL reference's loop (tests/golden/lirf_small*.npz, lirf_small2*.npz,
tools/make_golden_lirf.py) is compared under the widening rule of tests/test_hip_scrub.py (allowance). The loop, the driver and a fresh
process that runs the other steps close the file."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import recipe

import test_hip_ffn_train as T

pytestmark = pytest.mark.gpu

ARGS = dict(opt="adamw", weight_decay=0.05, opt_eps=1e-8, opt_betas=None, lr=1e-4)
FAR_SEED, FAR_LO, FAR_HI = 77, 0.7, 1.3
LIRF_T, ALPHA = 2.0, 0.5
CFGS = {"small": lambda: recipe.cfg_small(lora_rank=0), "small2": lambda: recipe.cfg_small2(lora_rank=0)}


def kwargs_of(cfg, pool="cls", dropout=0.0):
    return dict(loss_type="CosFace", GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
                dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], pool=pool, dropout=dropout, emb_dropout=dropout,
                lora_rank=0)


def build_half(cls, cfg, mode="fp32", state=None, train=False, **kw):
    m = cls(**kwargs_of(cfg, **kw))
    res = m.load_state_dict(state or T.state_of(cfg), strict=False)
    assert not res.missing_keys
    for p in m.parameters():
        p.requires_grad_(False)
    m = m.to("cuda").set_compute_dtype(mode)
    return m.train() if train else m.eval()


def far_state(cfg):
    """The `far` teacher: every FFN weight matrix scaled element-wise by recipe.uniform("far::" + name, shape, 77, 0.7, 1.3), lower blocks
    included."""
    st = T.state_of(cfg)
    for n in st:
        if "fn.fn.net" in n and n.endswith("weight"):
            st[n] = st[n] * torch.tensor(recipe.uniform("far::" + n, tuple(st[n].shape), FAR_SEED, FAR_LO, FAR_HI))
    return st


def setup(cfg, mode="fp32", far=True):
    """student_low (the --only_ffn rule), deposit_low, teacher_low, teacher_up, the optimizer over student_low, and the fixture's loaders:
    three forget batches of 3 and three remain batches of 2."""
    from gslora_hip.optim import create_optimizer
    from vit_pytorch_face import ViT_face_low, ViT_face_up
    tstate = far_state(cfg) if far else None
    student = build_half(ViT_face_low, cfg, mode, train=True)
    names = T.only_ffn(student, head=False)
    deposit = build_half(ViT_face_low, cfg, mode, train=True)
    teacher_low = build_half(ViT_face_low, cfg, mode, state=tstate)
    teacher_up = build_half(ViT_face_up, cfg, mode, state=tstate)
    opt = create_optimizer(SimpleNamespace(**ARGS), student)
    forget, remain = [], []
    for s in (40, 41, 42):
        x_r, y_r, x_f, y_f = T.batches(cfg, 3, s)
        forget.append((x_f, y_f))
        remain.append((x_r[:2], y_r[:2]))
    return SimpleNamespace(student=student, deposit=deposit, teacher_low=teacher_low, teacher_up=teacher_up, opt=opt, forget=forget,
                           remain=remain, names=names, split=cfg["num_class"] // 2)


def run_step(s, **kw):
    from gslora_hip import step
    return step.lirf_step(s.student, s.deposit, s.teacher_low, s.teacher_up, s.opt, torch.nn.CrossEntropyLoss(), *s.forget[0], *s.remain[0],
                          split=s.split, T=LIRF_T, alpha=ALPHA, **kw)


# ---------------------------------------------------------------------------------------------------------------- the float64 restatement
def low64(st, x, cfg):
    """ViT_face_low.forward of the reference (vit_face.py:638-665) in the dtype of `st`."""
    p, D, H = cfg["patch_size"], cfg["dim"], cfg["heads"]
    b, c, hh, ww = x.shape
    tok = x.reshape(b, c, hh // p, p, ww // p, p).permute(0, 2, 4, 3, 5, 1).reshape(b, (hh // p) * (ww // p), p * p * c)
    t = F.linear(tok, st["patch_to_embedding.weight"], st["patch_to_embedding.bias"])
    t = torch.cat((st["cls_token"].expand(b, -1, -1), t), 1) + st["pos_embedding"][:, :t.shape[1] + 1]
    return blocks64(st, t, cfg, range(cfg["depth"] // 2))


def blocks64(st, t, cfg, which):
    D, H = cfg["dim"], cfg["heads"]
    B, Tn = t.shape[:2]
    for i in which:
        a, f = f"transformer.layers.{i}.0.fn", f"transformer.layers.{i}.1.fn"
        xn = F.layer_norm(t, (D,), st[f"{a}.norm.weight"], st[f"{a}.norm.bias"], 1e-5)
        q, k, v = [u.reshape(B, Tn, H, 64).permute(0, 2, 1, 3) for u in F.linear(xn, st[f"{a}.fn.to_qkv.weight"]).chunk(3, -1)]
        attn = (torch.einsum("bhid,bhjd->bhij", q, k) * D ** -0.5).softmax(-1)
        o = torch.einsum("bhij,bhjd->bhid", attn, v).permute(0, 2, 1, 3).reshape(B, Tn, H * 64)
        t = F.linear(o, st[f"{a}.fn.to_out.0.weight"], st[f"{a}.fn.to_out.0.bias"]) + t
        xn = F.layer_norm(t, (D,), st[f"{f}.norm.weight"], st[f"{f}.norm.bias"], 1e-5)
        h = F.gelu(F.linear(xn, st[f"{f}.fn.net.0.weight"], st[f"{f}.fn.net.0.bias"]))
        t = F.linear(h, st[f"{f}.fn.net.3.weight"], st[f"{f}.fn.net.3.bias"]) + t
    return t


def up64(st, mid, y, cfg):
    """ViT_face_up.forward of the reference (:755-781) with CosFace (s 64, m 0.35)."""
    t = blocks64(st, mid, cfg, range(cfg["depth"] // 2, cfg["depth"]))
    emb = F.layer_norm(t[:, 0], (cfg["dim"],), st["mlp_head.0.weight"], st["mlp_head.0.bias"], 1e-5)
    cosine = F.linear(F.normalize(emb), F.normalize(st["loss.weight"]))
    one_hot = torch.zeros_like(cosine).scatter_(1, y.view(-1, 1), 1.0)
    return (one_hot * (cosine - 0.35) + (1.0 - one_hot) * cosine) * 64.0


def at64(x):
    a = F.normalize(x.pow(2).mean(1).view(x.size(0), -1))
    return torch.where(a < 0.005, torch.zeros_like(a), a)


def step64(cfg, s, far, at_weight=-300.0):
    """One step of baselines/LIRFtrain.py:104-164 in float64 on the CPU. -> (meters [CE, AT, KP, PT_RE, total, REPLAY], gradients by name)"""
    d64 = lambda st: {n: v.double() for n, v in st.items()}
    st_s, st_t = d64(T.state_of(cfg)), d64(far_state(cfg) if far else T.state_of(cfg))
    for n in s.names:
        st_s[n].requires_grad_(True)
    (x_f, y_f), (x_r, y_r) = s.forget[0], s.remain[0]
    x_f, y_f, x_r, y_r = x_f.cpu().double(), y_f.cpu(), x_r.cpu().double(), y_r.cpu()
    split, Tt, a = s.split, LIRF_T, ALPHA
    mid_s = low64(st_s, x_f, cfg)
    S = up64(st_t, mid_s, y_f, cfg)
    with torch.no_grad():
        mid_t = low64(st_t, x_f, cfg)
        Tf = up64(st_t, mid_t, y_f, cfg)
        Dp = up64(st_t, low64(d64(T.state_of(cfg)), x_f, cfg), y_f, cfg)
    kl = lambda u, v: F.kl_div(F.log_softmax(u / Tt, 1), F.softmax(v / Tt, 1), reduction="batchmean") * (a * Tt * Tt)
    ce = F.cross_entropy(S, y_f) * (1 - a)
    at = (at64(mid_s) - at64(mid_t)).pow(2).mean()
    kp = kl(S[:, split:], Tf[:, split:])
    pt_re = kl(Dp[:, :split], Tf[:, :split]) + F.cross_entropy(Dp, y_f) * (1 - a)
    replay = F.cross_entropy(up64(st_t, low64(st_s, x_r, cfg), y_r, cfg), y_r)
    total = ce + at_weight * at + 10 * kp + 0.05 * pt_re + 5 * replay
    grads = torch.autograd.grad(total, [st_s[n] for n in s.names])
    frac = float((at64(mid_t) == 0).double().mean())
    print(f"float64 step: at() entries under the threshold {frac:.3f}")
    return np.array([v.item() for v in (ce, at, kp, pt_re, total, replay)]), {n: g.numpy() for n, g in zip(s.names, grads)}


@pytest.fixture(scope="module")
def ref_steps():
    cache = {}

    def get(name, far=True, at_weight=-300.0):
        key = (name, far, at_weight)
        if key not in cache:
            cfg = CFGS[name]()
            cache[key] = step64(cfg, setup(cfg, far=far), far, at_weight)
        return cache[key]
    return get


# ---------------------------------------------------------------------------------------------------------------- split equals the whole
@pytest.mark.parametrize("pool", ["cls", "mean"])
@pytest.mark.parametrize("name", list(CFGS))
def test_up_of_low_equals_the_whole_network(name, pool):
    """Same weights, fp32, no_grad: the halves run the kernels the whole network runs, in the same order on the same bits (the lower
    half's last block is dense like every block but the whole network's last) — the logits and the embedding are bit-equal."""
    from vit_pytorch_face import ViT_face, ViT_face_low, ViT_face_up
    cfg = CFGS[name]()
    whole = ViT_face(**kwargs_of(cfg, pool=pool))
    whole.load_state_dict(T.state_of(cfg))
    whole = whole.to("cuda").set_compute_dtype("fp32").eval()
    low, up = build_half(ViT_face_low, cfg, pool=pool), build_half(ViT_face_up, cfg, pool=pool)
    x, y, x2, _ = T.batches(cfg, 3)
    with torch.no_grad():
        want, want_emb = whole(x, y)
        mid = low(x)
        got, got_emb = up(mid, y)
        assert mid.shape == (3, whole.num_tokens, cfg["dim"]) and mid.dtype == torch.float32
        assert torch.equal(got, want) and torch.equal(got_emb, want_emb)
        assert torch.equal(up(mid), want_emb), "without a label: the embedding alone"
        both = low((x, x2))      # a tuple of batches is one batch
        assert torch.equal(both[:3], mid) and torch.equal(both[3:], low(x2))
        # uint8 images under set_input_norm, like ViT_face
        u8 = (x * 255).round().to(torch.uint8)
        for m in (whole, low):
            m.set_input_norm("totensor")
        assert torch.equal(up(low(u8), y)[0], whole(u8, y)[0])
    for dt in ("fp16", "bf16"):      # the stream dtype of a 16-bit mode crosses the boundary as it is
        for m in (whole, low, up):
            m.set_input_norm(None).set_compute_dtype(dt)
        with torch.no_grad():
            mid = low(x)
            assert mid.dtype == torch.float16
            assert torch.equal(up(mid, y)[0], whole(x, y)[0]) and torch.equal(up(mid.float(), y)[0], whole(x, y)[0])


def test_a_standalone_call_with_gradients_is_refused_on_the_gpu():
    from vit_pytorch_face import ViT_face_low
    cfg = CFGS["small"]()
    low = build_half(ViT_face_low, cfg, train=True)
    T.only_ffn(low, head=False)
    x = T.batches(cfg, 2)[0]
    with pytest.raises(RuntimeError, match="gslora_hip.step.lirf_step"):
        low(x)
    with torch.no_grad():
        assert low(x).shape[0] == 2


# ---------------------------------------------------------------------------------------------------------------- the step
@pytest.mark.parametrize("far", [True, False], ids=["far", "copy"])
@pytest.mark.parametrize("name", list(CFGS))
def test_lirf_step_against_the_float64_restatement(name, far, ref_steps):
    cfg = CFGS[name]()
    s = setup(cfg, far=far)
    before = {n: p.detach().clone() for n, p in s.student.named_parameters()}
    frozen = {id(p): p.detach().clone() for m in (s.deposit, s.teacher_low, s.teacher_up) for p in m.parameters()}
    got = run_step(s)
    assert got.is_cuda and got.shape == (6,) and got.dtype == torch.float32
    got = got.cpu().numpy().astype(np.float64)
    want, want_grads = ref_steps(name, far)
    print(name, "far" if far else "copy", "\ngot ", got, "\nwant", want)
    for k, what in enumerate(("CE", "AT", "KP", "PT_RE", "total", "REPLAY")):
        assert abs(got[k] - want[k]) <= 1e-4 * max(1.0, abs(want[k])), (what, got[k], want[k])
    if far:
        assert got[1] > 0 and abs(got[1] - want[1]) <= 1e-4 * want[1] + 1e-9, "AT is far below 1: held relative to its own size too"
    else:
        assert got[1] == 0.0, "a copied teacher: the student's forget rows of the fused pass and the teacher's are the same bits"
        assert abs(got[2]) <= 1e-6
    params = dict(s.student.named_parameters())
    assert [n for n, p in params.items() if p.requires_grad] == s.names and all("fn.fn.net" in n for n in s.names)
    for n in s.names:
        w = want_grads[n]
        err = np.abs(params[n].grad.detach().double().cpu().numpy() - w).max()
        print(f"grad {n}: |want|_max {np.abs(w).max():.3e}, max err / (1e-4 |want|_max) = {err / (1e-4 * np.abs(w).max()):.4f}")
        assert err <= 1e-4 * np.abs(w).max(), n
    # weights: AdamW in float64 on the float64 gradients
    for n in s.names:
        p64 = before[n].double().cpu().requires_grad_(True)
        o = torch.optim.AdamW([p64], lr=ARGS["lr"], weight_decay=0.0 if p64.ndim <= 1 else ARGS["weight_decay"], eps=ARGS["opt_eps"])      # (no decay for biases)
        p64.grad = torch.tensor(want_grads[n])
        o.step()
        assert T.bar_ok(params[n].detach().cpu(), p64.detach(), f"weight {n}"), n
        assert not torch.equal(params[n].detach(), before[n]), n
    for n, p in params.items():
        if n not in s.names:
            assert torch.equal(p.detach(), before[n]) and p.grad is None, n
    for m in (s.deposit, s.teacher_low, s.teacher_up):
        for p in m.parameters():
            assert p.grad is None and torch.equal(p.detach(), frozen[id(p)]), "deposit and teachers receive nothing and do not move"


@pytest.mark.parametrize("name", list(CFGS))
def test_the_comparison_rests_on_the_injected_gradient(name, ref_steps):
    """The same step with the attention-transfer weight forced to 0 moves the lower blocks' gradients by more than the comparison bar
    (and matches the float64 step without the term): the comparison above rests on the injection."""
    cfg = CFGS[name]()
    s_on, s_off = setup(cfg), setup(cfg)
    run_step(s_on)
    got_off = run_step(s_off, _at_weight=0.0).cpu().numpy().astype(np.float64)
    want_off, grads_off = ref_steps(name, True, 0.0)
    assert abs(got_off[4] - want_off[4]) <= 1e-4 * max(1.0, abs(want_off[4]))
    on, off = dict(s_on.student.named_parameters()), dict(s_off.student.named_parameters())
    ratios = []
    for n in s_on.names:
        g_on, g_off = on[n].grad.double().cpu().numpy(), off[n].grad.double().cpu().numpy()
        assert np.abs(g_off - grads_off[n]).max() <= 1e-4 * np.abs(grads_off[n]).max(), n
        ratios.append(np.abs(g_on - g_off).max() / (1e-4 * np.abs(g_on).max()))
        print(f"{name} {n}: the term moves the gradient by {ratios[-1]:.1f} x the comparison bar")
    assert min(ratios) > 1.0, ratios


def grads_of_one_step(name, mode):
    cfg = CFGS[name]()
    s = setup(cfg, mode)
    pack = run_step(s)
    from vit_pytorch_face.vit_face import low_up_pair
    report = low_up_pair(s.student, s.teacher_up).runner().loss_scale_report() if mode == "fp16" else None
    return {n: p.grad.detach().double().cpu().numpy().copy() for n, p in s.student.named_parameters() if p.requires_grad}, pack, report


def close_16bit(got, want, what):
    for n, w in want.items():
        v = got[n]
        rel = np.linalg.norm(v - w) / np.linalg.norm(w)
        cos = float((v * w).sum() / (np.linalg.norm(v) * np.linalg.norm(w)))
        print(f"{what} {n}: rel Frobenius {rel:.4f}, cosine {cos:.5f}")
        assert rel <= 0.06 and cos > 0.995, (what, n)


@pytest.mark.parametrize("name", list(CFGS))
def test_one_16bit_step_against_the_f32_step(name, monkeypatch):
    from gslora_hip import vit_runner
    f32, _, _ = grads_of_one_step(name, "fp32")
    bf, _, _ = grads_of_one_step(name, "bf16")
    close_16bit(bf, f32, "bf16")
    h, pack, rep = grads_of_one_step(name, "fp16")
    print("fp16 loss scale:", rep)
    assert rep is not None and not rep["saturated"] and torch.isfinite(pack).all()
    close_16bit(h, f32, "fp16")
    # a loss scale sixteen times smaller gives the same gradients: a missed or doubled scale at the injection would not
    monkeypatch.setattr(vit_runner, "GRAD_TARGET_EXP", (rep["exponent"] or 11) - 4)
    h2, _, rep2 = grads_of_one_step(name, "fp16")
    print("fp16 loss scale, target exponent moved by 4:", rep2)
    assert rep2["S"] != rep["S"]
    close_16bit(h2, f32, "fp16, exponent - 4")


def test_an_exotic_criterion_keeps_its_semantics():
    cfg = CFGS["small"]()
    s1, s2 = setup(cfg), setup(cfg)
    from gslora_hip import step

    class Smoothed(torch.nn.Module):
        def forward(self, logits, y):
            return F.cross_entropy(logits, y, label_smoothing=0.0)
    a = run_step(s1).cpu().numpy()
    b = step.lirf_step(s2.student, s2.deposit, s2.teacher_low, s2.teacher_up, s2.opt, Smoothed(), *s2.forget[0], *s2.remain[0],
                       split=s2.split, T=LIRF_T, alpha=ALPHA).cpu().numpy()
    assert np.abs(a - b).max() <= 1e-4 * max(1.0, np.abs(a).max())
    for (n, p), q in zip(s1.student.named_parameters(), s2.student.parameters()):
        if p.requires_grad:
            assert (p.grad - q.grad).abs().max() <= 1e-4 * p.grad.abs().max(), n


def test_invalidate_reaches_the_pair_and_dropout_follows_each_half():
    from vit_pytorch_face.vit_face import ViT_face_low, ViT_face_up, low_up_forward, low_up_pair
    cfg = CFGS["small2"]()
    low = build_half(ViT_face_low, cfg, "bf16", train=True)
    T.only_ffn(low, head=False)
    up = build_half(ViT_face_up, cfg, "bf16", dropout=0.5)      # eval(): its dropout rate is not in force
    x, y = T.batches(cfg, 3)[:2]
    logits = low_up_forward(low, up, x, y)[0]
    with torch.no_grad():
        want = up(low(x), y)[0]
    assert torch.equal(logits.detach(), want), "student.train() with rate 0 under an upper half in eval(): no dropout anywhere"
    up.train()
    assert not torch.equal(low_up_forward(low, up, x, y)[0].detach(), want), "the upper half's own mode switches its dropout on"
    up.eval()
    pair = low_up_pair(low, up)
    assert pair is low_up_pair(low, up) and any(k and k[0] != "zeros" for k in pair.runner()._wcache)
    up.invalidate_operand_caches()
    assert not any(k and k[0] != "zeros" for k in pair.runner()._wcache)
    low_up_forward(low, up, x, y)
    low.invalidate_operand_caches()
    assert not any(k and k[0] != "zeros" for k in pair.runner()._wcache)
    with torch.no_grad():      # a weight written through .data, then invalidated: the pair sees the new value
        up.loss.weight.data.neg_()      # (CosFace normalises its rows: a sign is what survives)
    up.invalidate_operand_caches()
    with torch.no_grad():
        want2 = up(low(x), y)[0]
    assert torch.equal(low_up_forward(low, up, x, y)[0].detach(), want2) and not torch.equal(want2, want)


# ---------------------------------------------------------------------------------------------------------------- the reference's loop
def allowance(want32, want64):
    """tests/test_hip_scrub.py: the parity bar 1e-4 * max(1, |want|); where the reference's own f32 run leaves its f64 run by more than a
    quarter of that bar, four times that recorded deviation."""
    bar = 1e-4 * np.maximum(1.0, np.abs(want32))
    dev = np.abs(want32 - want64)
    return np.where(dev > bar / 4, 4 * dev, bar)


def recording():
    from util.utils import AverageMeter

    class Recording(AverageMeter):
        def __init__(self):
            super().__init__()
            self.seen = []

        def update(self, val, n=1):
            self.seen.append(float(val))
            super().update(val, n)
    return Recording()


METERS = ("losses_CE", "losses_AT", "kd_lossesKP", "losses_pt_re", "losses_total", "losses_remain")


@pytest.mark.parametrize("teacher_kind", ["copy", "far"])
@pytest.mark.parametrize("name", list(CFGS))
def test_the_loop_against_the_reference_fixture(golden_dir, name, teacher_kind):
    """tests/golden/lirf_<cfg>*.npz (tools/make_golden_lirf.py): the REAL train_one_epoch_LIRF on the real half networks, 3 steps per
    teacher. Meters, the gradients the last step left and (far teacher) the final weights, against the reference's f32 run and against its
    f64 run: per element the plain bar where the reference's f32 run stays within a quarter of it, else four times the recorded deviation.
    AT is far below 1, so its column is also held relative to its own size (1e-4 |want|, widened the same way)."""
    from baselines.LIRFtrain import train_one_epoch_LIRF
    from gslora_hip import at as AT
    g = np.load(os.path.join(golden_dir, f"lirf_{name}.npz"))
    cfg = CFGS[name]()
    lr, wd, T_, alpha, split = g["hyper"].tolist()
    assert (lr, wd, T_, alpha, int(split)) == (ARGS["lr"], ARGS["weight_decay"], LIRF_T, ALPHA, cfg["num_class"] // 2)
    s = setup(cfg, far=teacher_kind == "far")
    assert s.names == g["trainable"].tolist()
    with torch.no_grad():      # the at() tables of step 1
        for net, key in ((s.student, "at_s"), (s.teacher_low, "at_t")):
            net.eval()
            got = AT.at(net(s.forget[0][0])).cpu().numpy()
            want = g[f"{key}::{teacher_kind}"]
            assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max(), key
    meters = {k: recording() for k in METERS}
    out = train_one_epoch_LIRF(s.student, s.deposit, s.teacher_low, s.teacher_up, s.forget, s.remain, torch.nn.CrossEntropyLoss(), s.opt,
                               torch.device("cuda"), 0, 0, *meters.values(), "0", None, None, 0.0, 0.0,
                               dict(PER_FORGET_CLS=s.split, LIRF_T=LIRF_T, LIRF_alpha=ALPHA))
    assert out[0] == 3 and len(out) == 8
    got = np.array([meters[k].seen for k in METERS]).T
    want, want64 = g[f"meters::{teacher_kind}"], g[f"meters64::{teacher_kind}"]
    assert got.shape == want.shape
    ratio = np.abs(got - want) / allowance(want, want64)
    ratio64 = np.abs(got - want64) / allowance(want64, want)
    print(f"{name} {teacher_kind} meters: max |err| / allowance per column {ratio.max(0)}; vs the f64 run {ratio64.max(0)}")
    print(f"got\n{got}\nwant\n{want}")
    assert (ratio <= 1.0).all() and (ratio64 <= 1.0).all(), (ratio, ratio64)
    at_bar = 1e-4 * np.abs(want[:, 1])
    at_allow = np.where(np.abs(want[:, 1] - want64[:, 1]) > at_bar / 4, 4 * np.abs(want[:, 1] - want64[:, 1]), at_bar)
    print(f"AT column: |err| / (relative allowance) {np.abs(got[:, 1] - want[:, 1]) / np.maximum(at_allow, 1e-300)}")
    assert (np.abs(got[:, 1] - want[:, 1]) <= at_allow).all()
    if teacher_kind == "copy":
        assert got[0, 1] == 0.0
    else:
        assert (got[:, 1] > 0).all()
    params = dict(s.student.named_parameters())
    kinds = [("grad", lambda p: p.grad)] + ([("final", lambda p: p)] if teacher_kind == "far" else [])
    for kind, pick in kinds:
        t32 = np.load(os.path.join(golden_dir, f"lirf_{name}_{teacher_kind}_{kind}.npz"))
        tdf = np.load(os.path.join(golden_dir, f"lirf_{name}_{teacher_kind}_{kind}_diff.npz"))
        for n in s.names:
            w32 = t32[f"{kind}::{teacher_kind}::{n}"].astype(np.float64)
            diff = tdf[f"{kind}_diff::{teacher_kind}::{n}"].astype(np.float64)
            scale = np.abs(w32).max() if kind == "grad" else max(1.0, np.abs(w32).max())
            bar = 1e-4 * scale
            allow = np.where(np.abs(diff) > bar / 4, 4 * np.abs(diff), bar)
            v = pick(params[n]).detach().cpu().numpy().astype(np.float64)
            err, err64 = np.abs(v - w32), np.abs(v - (w32 + diff))
            print(f"{name} {teacher_kind} {kind} {n}: |want|_max {np.abs(w32).max():.3e}, max err / allowance = {(err / allow).max():.3f}, "
                  f"vs the f64 run {(err64 / allow).max():.3f}; widened elements {(allow > bar).mean():.4f}")
            assert (err <= allow).all(), (kind, n)
            assert (err64 <= allow).all(), (kind, n, "the f64 run")


# ---------------------------------------------------------------------------------------------------------------- the loop
def test_the_loop_trains_the_students_ffn_and_nothing_else(capsys):
    from baselines.LIRFtrain import eval_data_LIRF, train_one_epoch_LIRF
    from util.utils import AverageMeter
    cfg = CFGS["small"]()
    s = setup(cfg)
    snap = lambda m: {n: p.detach().clone() for n, p in m.named_parameters()}
    before = {k: snap(m) for k, m in (("student", s.student), ("deposit", s.deposit), ("teacher_low", s.teacher_low), ("teacher_up", s.teacher_up))}
    meters = {k: AverageMeter() for k in ("losses_CE", "losses_AT", "kd_lossesKP", "losses_pt_re", "losses_total", "losses_remain")}
    test_f, test_r = [s.forget[0]], [s.remain[0]]
    out = train_one_epoch_LIRF(s.student, s.deposit, s.teacher_low, s.teacher_up, s.forget * 2, s.remain, torch.nn.CrossEntropyLoss(), s.opt,
                               torch.device("cuda"), 0, 0, *meters.values(), "0", test_f, test_r, 50.0, 0.0,
                               dict(PER_FORGET_CLS=s.split, LIRF_T=LIRF_T, LIRF_alpha=ALPHA))
    assert len(out) == 8 and out[0] == 6 and out[2:] == tuple(meters.values())
    text = capsys.readouterr().out
    assert "Task 0 Epoch 1 Batch 5" in text and "Accuracy in LIRF" in text
    assert meters["losses_total"].count == 3, "reset after the fifth batch: the sixth alone is left"
    assert s.student.training and 0.0 <= out[1] <= 100.0
    for k, m in (("deposit", s.deposit), ("teacher_low", s.teacher_low), ("teacher_up", s.teacher_up)):
        for n, p in m.named_parameters():
            assert torch.equal(p.detach(), before[k][n]), (k, n)
    assert not any(n.startswith(f"transformer.layers.{i}.") for n in before["student"] for i in range(cfg["depth"] // 2, cfg["depth"]))
    for n, p in s.student.named_parameters():
        assert torch.equal(p.detach(), before["student"][n]) == ("fn.fn.net" not in n), n
    acc = eval_data_LIRF(s.student, s.teacher_up, test_f, torch.device("cuda"), "forget")
    assert 0.0 <= acc <= 100.0 and s.student.compute_mode == "fp32"


def test_the_driver_runs_the_task_chain_on_the_small_model(tmp_path):
    import json
    import driver_lirf
    from gslora_hip import _lib_at
    common = ["--small", "--num_class", "20", "--per_forget_cls", "4", "--num_tasks", "2", "--epochs", "1", "--batch_size", "16",
              "--samples_per_class", "4", "--dtype", "fp32", "--LIRF_T", "2", "--LIRF_alpha", "0.5"]
    rep, outdir, nets = driver_lirf.main(common + ["--outdir", str(tmp_path / "a")])
    lines = [json.loads(ln) for ln in open(os.path.join(outdir, "lirf_report.jsonl"))]
    assert len(rep) == len(lines) == 2 and [r["task"] for r in lines] == [0, 1] and all(r["method"] == "lirf" and r["steps"] >= 1 for r in rep)
    assert all(np.isfinite(r[k]) for r in rep for k in ("forget_before", "forget_after", "remain_before", "remain_after", "best_H_mean"))
    assert all(np.isfinite(v) for r in rep for e in r["epochs"] for v in e.values() if v is not None)
    assert _lib_at.loaded()
    student = nets["student_low"]
    assert [n for n, p in student.named_parameters() if p.requires_grad] == [n for n, _ in student.named_parameters() if "fn.fn.net" in n]
    assert not any(p.requires_grad for k in ("deposit_low", "teacher_low", "teacher_up") for p in nets[k].parameters())
    assert all(p.grad is None for k in ("deposit_low", "teacher_low", "teacher_up") for p in nets[k].parameters())
    rep2, _, _ = driver_lirf.main(common + ["--dropout", "0.0", "--outdir", str(tmp_path / "b")])
    rep3, _, _ = driver_lirf.main(common + ["--dropout", "0.0", "--outdir", str(tmp_path / "c")])
    assert rep2 == rep3, "without dropout: the same report twice under the same seed"


CHILD = """
import sys
sys.path[:0] = [%r, %r, %r]
from types import SimpleNamespace
import copy
import torch
import loralib as lora
from oracle import recipe
from vit_pytorch_face import ViT_face
import test_hip_ffn_train as T
from gslora_hip import _lib_at, step
from gslora_hip.optim import create_optimizer
args = SimpleNamespace(opt="adamw", weight_decay=0.05, opt_eps=1e-8, opt_betas=None, lr=1e-4)
crit = torch.nn.CrossEntropyLoss()
cfg = recipe.cfg_small(lora_rank=0)
m = T.build(cfg, "fp32")
x_r, y_r, x_f, y_f = T.batches(cfg, 3)
t = copy.deepcopy(m).eval()
assert torch.isfinite(step.ffn_reg_step(m, create_optimizer(args, m), crit, x_r, y_r)).all()
assert torch.isfinite(step.scrub_step(m, t, create_optimizer(args, m), crit, x_r, y_r, maximize=False, kd_T=2.0, sgda_gamma=0.99, sgda_alpha=0.001)).all()
for p in t.parameters():
    p.requires_grad_(False)
for method in ("lwf", "der", "fdr"):
    assert torch.isfinite(step.distill_step(m, t, create_optimizer(args, m), crit, x_f, y_f, x_r, y_r, method=method, lam=0.1, lam_aux=1.0)).all()
cfg = recipe.cfg_small()
g = ViT_face(loss_type="CosFace", GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
             dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], lora_rank=cfg["lora_rank"])
lora.mark_only_lora_as_trainable(g)
g = g.to("cuda").set_compute_dtype("fp32").train()
step.gs_lora_step(g, create_optimizer(args, g), crit, x_r, y_r, x_f, y_f, beta=0.15, alpha=0.01, BND=105.0)
torch.cuda.synchronize()
assert not _lib_at.loaded() and "libgslora_at" not in open("/proc/self/maps").read()
assert "libgslora_hip" in open("/proc/self/maps").read()
print("ok")
"""


def test_a_fresh_process_running_the_other_steps_leaves_the_sixth_library_closed():
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", CHILD % (os.path.dirname(here), os.path.join(os.path.dirname(here), "gs-lora_amd"), here)],
                       capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]
