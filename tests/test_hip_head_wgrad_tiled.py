"""GPU tests of the class-tiled head weight gradient (gsl_head_wgrad at C > 1024, head_wgrad_tiled_kernel; DESIGN.md sections 9h / 9i).

The tile constants the shapes aim at (csrc/head.hip): a workgroup owns 16 classes (C < 16384) or 64 (C >= 16384) and all D columns; the
batch is walked in K tiles of 16 images (D <= 512) or 8 (D > 512); the kernel is instantiated for D <= 128, <= 256, <= 512 and <= 1024 at
either tile. So (17, 1041, 128) is one past a class-tile edge (65 * 16 + 1) and one past a K-tile edge, (17, 16513, 512) the same for the
64-class tile (258 * 64 + 1), (130, 1027, 1024) is 16 K tiles of 8 and two images, and C = 16383 / 16384 are the two sides of the tile-size
threshold.

Gradient bar of the project: |err| <= 1e-4 * max(1, |g|) elementwise. On the CPU torch's own f32 autograd stays below a quarter of that bar
on every (shape, kind) of the float64 test below: at most 0.22 for the cosine heads ((130, 1027, 1024); 0.21 at the 16 000-class shapes) and
0.13 for the linear ones. That fixed the list: xavier-initialised rows get short at 16 000 classes and few columns (dW goes with
1 / ||W_c||), so e.g. (17, 16385, 256), (17, 16385, 512) and (5, 16385, 256) — 0.41, 0.26 and 0.32 of the bar in torch's own f32 — are not
float64 cases; the shapes at 16 000 classes were picked among those below a quarter. (19, 16384, 64) serves the bit-for-bit comparison of the
two tile sizes only."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_hip_head_large_c as lc
import test_hip_head_probe as hp
from guard_bands import Banded
from test_hip_head_probe import KINDS, S, bar_ok, label_cosines, op_inputs, reference_wgrad

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1025, 64), (7, 1100, 64), (33, 1100, 192), (65, 1153, 512), (130, 1027, 1024), (17, 1041, 128),
          (3, 16385, 128), (9, 16449, 256), (17, 16513, 512), (9, 16392, 1024)]
KIND = {k[0]: k for k in KINDS}
_cache = {}


def case_of(shape, name):
    """Inputs and the float64 reference of a (shape, kind), computed once and shared (nothing modifies them)."""
    if (shape, name) not in _cache:
        _, kind, m, easy, bias = KIND[name]
        B, C, D = shape
        emb, W, dl, label = op_inputs(B, C, D, seed=B * 1000 + C)
        cos_y = label_cosines(emb, W, label)
        _cache[(shape, name)] = SimpleNamespace(emb=emb, W=W, dl=dl, label=label, cos_y=cos_y, kind=kind, m=m, easy=easy, bias=bias,
                                                want=reference_wgrad(kind, emb, W, dl, label, cos_y, m, easy, bias))
    return _cache[(shape, name)]


def run(ops, c, dl=None, emb=None, W=None, dW=None, dbias=None, C=None):
    dev = lambda t: t.cuda().contiguous()
    dl = dev(c.dl) if dl is None else dl
    return ops.head_wgrad(dl, dev(c.emb) if emb is None else emb, dev(c.W if C is None else c.W[:C]) if W is None else W, c.kind, cos_s=S, m=c.m,
                          easy_margin=c.easy, label=dev(c.label), cos_y=dev(c.cos_y), bias=c.bias, dW=dW, dbias=dbias)


@pytest.fixture(scope="module")
def ops():
    from gslora_hip import ops
    return ops


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", list(KIND))
def test_tiled_wgrad_matches_float64_autograd(ops, shape, name):
    c = case_of(shape, name)
    B, C, D = shape
    dW = torch.full((C, D), float("nan"), device="cuda")
    db = torch.full((C,), float("nan"), device="cuda") if c.bias else None
    got_w, got_b = run(ops, c, dW=dW, dbias=db)
    assert got_w is dW and not torch.isnan(dW).any()
    assert bar_ok(got_w.cpu(), c.want[0], f"{name} {shape} dW")
    assert (got_b is not None) == c.bias
    if c.bias:
        assert got_b is db and not torch.isnan(db).any() and bar_ok(got_b.cpu(), c.want[1], f"{name} {shape} dbias")
    again_w, again_b = run(ops, c)      # fresh buffers, the same bits
    assert torch.equal(again_w, got_w) and (not c.bias or torch.equal(again_b, got_b))
    if c.kind == "arcface" and B >= 65:
        th = 0.0 if c.easy else hp.arc_constants(c.m)[2]
        assert (c.cos_y > th).any() and (c.cos_y < th).any(), "the case exercises both branches of phi"


@pytest.mark.parametrize("kind", ["cosface", "arcface"])
def test_zero_weight_row_follows_the_clamp_derivative_at_1100_classes(ops, kind):
    B, C, D = 9, 1100, 128
    emb, W, dl, label = op_inputs(B, C, D, seed=5)
    W[3] = 0.0
    label[0] = 3      # the zero row is also a label row (its cosine is 0)
    cos_y = label_cosines(emb, W, label)
    want, _ = reference_wgrad(kind, emb, W, dl, label, cos_y, 0.5, False, False)
    got, _ = ops.head_wgrad(dl.cuda(), emb.cuda(), W.cuda(), kind, cos_s=S, m=0.5, label=label.cuda(), cos_y=cos_y.cuda())
    got = got.cpu().double()
    assert torch.isfinite(got).all() and got[3].abs().max() > 1e9      # d What / 1e-12, no projection term
    # the floor of tests/test_hip_head_probe.py: an element carries ~(B + 3) * 2^-24 of the row's largest as absolute rounding error
    floor = 1e-2 * want[3].abs().max()
    err = (got[3] - want[3]).abs() / want[3].abs().clamp(min=floor)
    print(f"zero row {kind}: worst relative error {err.max().item():.3e} (bound 1e-4)")
    assert (err <= 1e-4).all()
    rest = [c for c in range(C) if c != 3]
    assert bar_ok(got[rest], want[rest], f"{kind} rows beside the zero row")


@pytest.mark.parametrize("name", ["cosface", "arcface", "linear_bias"])
@pytest.mark.parametrize("shape", [(33, 1100, 192), (9, 16392, 1024)], ids=lambda s: "x".join(map(str, s)))
def test_guard_bands_and_nan_padding(ops, shape, name):
    """NaN around every input (past B * C of dlogits, past B of emb / label / cos_y, around W), sentinels around and NaN inside the outputs:
    nothing outside is read into a sum or written, every element is stored, and the bits are those of the plain call."""
    c = case_of(shape, name)
    B, C, D = shape
    dl, emb, W = Banded((B, C), torch.float32, c.dl), Banded((B, D), torch.float32, c.emb), Banded((C, D), torch.float32, c.W)
    label, cos_y = Banded((B,), torch.int64, c.label), Banded((B,), torch.float32, c.cos_y)
    dW = Banded((C, D), torch.float32)
    db = Banded((C,), torch.float32) if c.bias else None
    dW.view.fill_(float("nan"))
    if db is not None:
        db.view.fill_(float("nan"))
    got_w, got_b = ops.head_wgrad(dl.view, emb.view, W.view, c.kind, cos_s=S, m=c.m, easy_margin=c.easy, label=label.view, cos_y=cos_y.view,
                                  bias=c.bias, dW=dW.view, dbias=None if db is None else db.view)
    torch.cuda.synchronize()
    for b in (dl, emb, W, label, cos_y, dW) + ((db,) if db is not None else ()):
        assert b.bands_intact()
    assert not torch.isnan(got_w).any() and (db is None or not torch.isnan(got_b).any())
    plain_w, plain_b = run(ops, c)
    assert torch.equal(got_w, plain_w) and (db is None or torch.equal(got_b, plain_b))


@pytest.mark.parametrize("name", list(KIND))
def test_row_c_does_not_depend_on_the_class_count(ops, name):
    """Rows [0, 1030) of a (37, 1100, 192) call against the (37, 1030, 192) call on the first 1030 columns of dlogits, bit for bit."""
    c = case_of((37, 1100, 192), name)
    if c.kind == "arcface":
        assert (c.label >= 1030).any() and (c.label < 1030).any()      # a label outside [0, C) scales no column: head_bwd_kernel's rule
    full_w, full_b = run(ops, c)
    part_w, part_b = run(ops, c, dl=c.dl[:, :1030].contiguous().cuda(), C=1030)
    assert torch.equal(full_w[:1030], part_w) and (not c.bias or torch.equal(full_b[:1030], part_b))


@pytest.mark.parametrize("name", ["cosface", "linear_bias"])
def test_row_c_does_not_depend_on_the_class_tile(ops, name):
    """C = 16383 runs 16-class tiles, C = 16384 64-class tiles: the first 16383 rows agree bit for bit."""
    c = case_of((19, 16384, 64), name)
    wide_w, wide_b = run(ops, c)
    narrow_w, narrow_b = run(ops, c, dl=c.dl[:, :16383].contiguous().cuda(), C=16383)
    assert torch.equal(wide_w[:16383], narrow_w) and (not c.bias or torch.equal(wide_b[:16383], narrow_b))
    assert torch.isfinite(wide_w).all() and wide_w.abs().max() > 0


@pytest.mark.parametrize("shape", [(128, 1100, 192), (192, 1030, 64)], ids=lambda s: "x".join(map(str, s)))
def test_the_sum_over_b_is_one_ascending_chain(ops, shape):
    """The linear kind is the plain product dlogits^T . emb; the f32 GEMM computes every element as one k-ordered fmaf chain from 0
    (tests/test_hip_gemm.py::test_f32_gemm_mfma_equals_valu_bitwise), and so does the tiled kernel: equal bits. (The per-class kernel adds 16
    wave-strided partial sums and does not pass.) torch.equal treats +0 and -0 alike, as wanted: zero padding can turn a -0 sum into +0."""
    B, C, D = shape
    c = case_of(shape, "linear")
    got, _ = run(ops, c)
    want = torch.empty(C, D, device="cuda")
    ops.gemm_nt(c.dl.cuda().t().contiguous(), c.emb.cuda().t().contiguous(), want)
    assert torch.equal(got, want)


@pytest.mark.parametrize("name", ["cosface", "linear_bias"])
def test_calls_outside_the_preconditions_fall_back_to_the_per_class_kernel(ops, name):
    """D % 4 != 0, or emb not 16-byte aligned: no refusal, the per-class kernel answers (any C, any D <= 1024, as before)."""
    c = case_of((9, 1100, 66), name)
    got_w, got_b = run(ops, c)
    assert bar_ok(got_w.cpu(), c.want[0], f"{name} D = 66") and (not c.bias or bar_ok(got_b.cpu(), c.want[1], f"{name} D = 66 dbias"))
    c = case_of((9, 1100, 64), name)
    buf = torch.empty(9 * 64 + 1, device="cuda")
    off = buf[1:].view(9, 64)
    off.copy_(c.emb)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    off_w, off_b = run(ops, c, emb=off)
    tiled_w, tiled_b = run(ops, c)
    assert bar_ok(off_w.cpu(), c.want[0], f"{name} emb + 4 bytes") and bar_ok(off_w.cpu(), tiled_w.cpu(), f"{name} emb + 4 bytes against the tiled call")
    assert not c.bias or bar_ok(off_b.cpu(), tiled_b.cpu(), f"{name} emb + 4 bytes dbias")


def golden_inputs(B, C, D):
    """numpy's legacy generator: the same stream on every machine and version."""
    r = np.random.RandomState(B * 1000 + C)
    f = lambda *s: torch.tensor(r.standard_normal(s).astype(np.float32))
    return f(B, D), f(C, D) * 0.05, f(B, C)


@pytest.mark.parametrize("shape", [(33, 100, 192), (33, 1024, 64)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", ["cosface", "linear_bias"])
def test_up_to_1024_classes_the_bits_are_the_parent_commits(ops, golden_dir, shape, name):
    """tests/golden/head_wgrad_small_c_parent.npz: what the library built from the commit before the tiled kernel returned for these inputs."""
    g = np.load(os.path.join(golden_dir, "head_wgrad_small_c_parent.npz"), allow_pickle=False)
    emb, W, dl = golden_inputs(*shape)
    key = f"{name}_{'x'.join(map(str, shape))}"
    for _ in range(2):
        got_w, got_b = ops.head_wgrad(dl.cuda(), emb.cuda(), W.cuda(), KIND[name][1], cos_s=S, m=0.35, bias=KIND[name][4])
        assert got_w.cpu().numpy().tobytes() == g[f"{key}_dW"].tobytes()
        if KIND[name][4]:
            assert got_b.cpu().numpy().tobytes() == g[f"{key}_dbias"].tobytes()


# ---------------------------------------------------------------------------------------------------------------- models
CFG = lc.CFG      # ViT_face / ViTs_face of the small geometry, num_class = 1100


def build(head="CosFace", dtype="fp32", dropout=0.0, train="head", cls=None):
    m = lc.build(head, dtype=dtype, dropout=dropout, train="lora", cls=cls)
    hp.set_trainable(m, train)
    return m


def head64(m, head, emb, y, W, b):
    """lc.head64 with the weight (and bias) as float64 leaves."""
    if head == "Softmax":
        return emb @ W.T + b
    cos = F.normalize(emb) @ F.normalize(W).T
    cy = cos.gather(1, y[:, None])
    if head == "CosFace":
        lab = cy - m.loss.m
    else:
        mm = m.loss.m
        phi = cy * math.cos(mm) - torch.sqrt(1.0 - cy * cy) * math.sin(mm)
        lab = torch.where(cy > math.cos(math.pi - mm), phi, cy - math.sin(math.pi - mm) * mm)
    return m.loss.s * cos.scatter(1, y[:, None], lab)


@pytest.mark.parametrize("head,cls,train", [("CosFace", "ViT_face", "head"), ("ArcFace", "ViT_face", "head"), ("Softmax", "ViT_face", "head"),
                                            ("CosFace", "ViT_face", "both"), ("Softmax", "ViT_face", "both"), ("ArcFace", "ViTs_face", "head")])
def test_model_head_gradient_at_1100_classes(head, cls, train):
    """loss.weight.grad (and loss.bias.grad) against the head and the mean CE in float64 autograd on the model's own emb; with LoRA also
    trainable, the LoRA gradients are bit for bit those of the frozen-head step."""
    from gslora_hip import losses
    m = build(head, train=train, cls=cls)
    x, y, _, _ = lc.batches(CFG, 37)
    logits, emb = m(x, y)
    m.zero_grad()
    (losses.ce_sum_top1(logits, y)[0] / x.shape[0]).backward()
    W = m.loss.weight.detach().double().requires_grad_(True)
    b = m.loss.bias.detach().double().requires_grad_(True) if head == "Softmax" else None
    lo64 = head64(m, head, emb.detach().double(), y, W, b)
    assert (logits.double() - lo64.detach()).abs().max() < 1e-4
    F.cross_entropy(lo64, y).backward()
    assert bar_ok(m.loss.weight.grad.cpu(), W.grad.cpu(), f"{cls} {head} {train} loss.weight")
    if b is not None:
        assert bar_ok(m.loss.bias.grad.cpu(), b.grad.cpu(), f"{cls} {head} {train} loss.bias")
    if train == "both":
        f = build(head, train="lora", cls=cls)
        logits_f, _ = f(x, y)
        (losses.ce_sum_top1(logits_f, y)[0] / x.shape[0]).backward()
        want = lc.lora_grads(f)
        assert want and any(v.abs().max() > 0 for v in want.values())
        for n, g in want.items():
            assert torch.equal(dict(m.named_parameters())[n].grad, g), n
    else:
        assert [n for n, p in m.named_parameters() if p.grad is not None] == (["loss.weight", "loss.bias"] if head == "Softmax" else ["loss.weight"])


ARGS = SimpleNamespace(opt="adamw", lr=1e-3, weight_decay=0.05, opt_eps=1e-8, opt_betas=None)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_three_probe_steps_in_16_bit_within_the_declared_tolerance(dtype):
    """6 % relative Frobenius and cosine above 0.995 on the gradient, 0.25 on what follows the logits (the loss meter)."""
    from gslora_hip.optim import create_optimizer
    from gslora_hip.step import head_probe_step
    crit = torch.nn.CrossEntropyLoss()
    data = [(torch.cat(b[0::2]), torch.cat(b[1::2])) for b in (lc.batches(CFG, 16, s) for s in range(3))]
    out = {}
    for dt in ("fp32", dtype):
        m = build("CosFace", dtype=dt)
        opt = create_optimizer(ARGS, m)
        out[dt] = []
        for x, y in data:
            meters = head_probe_step(m, opt, crit, x, y)
            out[dt].append((m.loss.weight.grad.detach().double().flatten().clone(), meters.cpu()))
    for s, ((ref, mref), (got, mgot)) in enumerate(zip(out["fp32"], out[dtype])):
        rel = ((got - ref).norm() / ref.norm()).item()
        cos = (torch.dot(got, ref) / (got.norm() * ref.norm())).item()
        print(f"{dtype} step {s + 1}: head gradient rel {rel:.5f}, cosine {cos:.6f}, loss {mgot[0].item():.4f} vs {mref[0].item():.4f}")
        assert rel <= 0.06 and cos > 0.995
        assert torch.isfinite(mgot).all() and abs(mgot[0] - mref[0]) <= 0.25


def test_graph_replay_of_the_probe_step_equals_eager_steps():
    """tests/test_hip_head_probe.py::test_graph_replay_equals_eager_steps at 1100 classes, fp16, dropout 0.1: the tiled launch captures
    (no allocation, no sync) and replays to the same bits."""
    from gslora_hip.optim import create_optimizer
    from gslora_hip.step import head_probe_step
    crit = torch.nn.CrossEntropyLoss()
    args = SimpleNamespace(opt="adamw", lr=1e-2, weight_decay=0.05, opt_eps=1e-8, opt_betas=None)
    data = [(torch.cat(b[0::2]), torch.cat(b[1::2])) for b in (lc.batches(CFG, 4, s) for s in range(4))]
    runs = {}
    for mode in ("eager", "graph"):
        torch.manual_seed(4321)      # the runner derives its dropout stream from torch's seed
        m = build("CosFace", dtype="fp16", dropout=0.1)
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
