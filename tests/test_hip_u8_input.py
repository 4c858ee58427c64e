"""uint8 image input on the GPU: ToTensor() + Normalize(mean, std) fused into the two patch gathers.

The definition is, in float32 on the CPU,  x = u.float().div(255).sub(mean[c]).div(std[c]).  Everything here compares the uint8 path with
the EXISTING float path fed this x, and the bar is bit-equality: the gathers write the only tensor that differs and every kernel behind
them is deterministic.
 (a) gsl_patchify_u8 / gsl_unfold_patches_u8, NCHW and NHWC bytes, every byte value in every channel, against the float gather of x;
 (b) the argument checks;
 (c) the models (ViT_face cls / mean pool, CosFace / ArcFace, attention adapters; ViTs_face; ModifiedViT) in train and eval mode, and one
     gs_lora_step fused and unfused;
 (d) HIP-graph replay with uint8 static inputs;  (e) the continual engine fed from host uint8 batches;  (f) the unchanged value cast."""
import copy

import pytest
import torch

from oracle import recipe

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
MODES = {"f32": "fp32", "bf16": "bf16", "fp16": "fp16"}
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
AWKWARD = ((0.1234567, 0.5, 0.9), (0.0371, 1.7, 0.333))
VITS_GEOMS = [(112, 12, 8, 4), (48, 12, 8, 4), (48, 10, 8, 1), (40, 16, 8, 4), (48, 8, 8, 0)]      # tests/test_hip_vits.py GEOMS


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    from gslora_hip import ops as _ops
    from gslora_hip import _lib
    _lib.load()
    return _ops


def definition(u, mean, std):
    mean, std = torch.tensor(mean[:u.shape[1]], dtype=torch.float32), torch.tensor(std[:u.shape[1]], dtype=torch.float32)
    return u.to(torch.float32).div(255).sub(mean[None, :, None, None]).div(std[None, :, None, None])


def all_bytes(B, C, H, W, seed):
    """Random bytes, with every byte value in every channel (the first 256 pixels of image 0 and, reversed, the last 256 of the last)."""
    g = torch.Generator().manual_seed(seed)
    u = torch.randint(0, 256, (B, C, H, W), dtype=torch.uint8, generator=g)
    ramp = torch.arange(256, dtype=torch.uint8)
    u[0].reshape(C, -1)[:, :256] = ramp
    u[-1].reshape(C, -1)[:, -256:] = ramp.flip(0)
    return u


def raw(t):
    """The storage as integers: bit-equality, not value equality (-0.0 and 0.0 differ here)."""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu()


def layouts(u):
    """(name, device tensor) of the two byte layouts of one [B, C, H, W] batch: NCHW-contiguous, and a decoder's [B, H, W, C] bytes."""
    nhwc = u.permute(0, 2, 3, 1).contiguous().cuda().permute(0, 3, 1, 2)
    return (("nchw", u.cuda()), ("nhwc", nhwc))


def table(ops, pair, C):
    return ops.u8_norm_table(pair[0][:C], pair[1][:C]).cuda()


# ------------------------------------------------------------------------------------------------------------ (a) the gathers
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("geom", [(112, 112, 8), (128, 128, 8), (48, 48, 8), (40, 56, 8), (56, 40, 8), (64, 48, 16), (40, 40, 4)])
def test_patchify_u8_equals_the_float_gather(ops, dname, geom):
    from gslora_hip import _lib as L
    dt = DTYPES[dname]
    H, W, p = geom
    for C, pair in ((3, IMAGENET), (1, AWKWARD), (2, AWKWARD)):      # (C = 2 and p = 4: the one-byte-per-load form)
        u = all_bytes(3, C, H, W, seed=H + W + C)
        ref = ops.patchify(definition(u, *pair).cuda(), p, dt)
        tab = table(ops, pair, C)
        T = 1 + (H // p) * (W // p)
        for name, src in layouts(u):
            got = ops.patchify(src, p, dt, table=tab)
            assert got.shape == ref.shape and got.dtype == dt
            assert torch.equal(raw(got), raw(ref)), (name, C)
            assert (got.view(3, T, -1)[:, 0] == 0).all()
        # through the C ABI into a NaN-filled buffer: every element is written
        out = torch.full(ref.shape, float("nan"), device="cuda", dtype=dt)
        L.check(L.load().gsl_patchify_u8(u.cuda().data_ptr(), L.U8_NCHW, tab.data_ptr(), out.data_ptr(), 3, C, H, W, p, ops.code(dt),
                                         ops._stream()), "patchify_u8")
        assert torch.equal(raw(out), raw(ref))


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("geom", VITS_GEOMS + [(56, 12, 8, 4)])
def test_unfold_u8_equals_the_float_gather(ops, dname, geom):
    from gslora_hip import _lib as L
    import torch.nn.functional as F
    dt = DTYPES[dname]
    H, k, s, pad = geom
    B = 3
    for C, pair in ((3, AWKWARD), (1, IMAGENET)):      # non-zero means: a padding tap must be 0, not normalise(0)
        u = all_bytes(B, C, H, H, seed=H + k + C)
        x = definition(u, *pair)
        ref = ops.unfold_patches(x.cuda(), k, s, pad, dt)
        tab = table(ops, pair, C)
        for name, src in layouts(u):
            got = ops.unfold_patches(src, k, s, pad, dt, table=tab)
            assert torch.equal(raw(got), raw(ref)), (name, C)
        kpad = ref.shape[1]
        out = torch.full(ref.shape, float("nan"), device="cuda", dtype=dt)
        nhwc = layouts(u)[1][1]
        L.check(L.load().gsl_unfold_patches_u8(nhwc.data_ptr(), L.U8_NHWC, tab.data_ptr(), out.data_ptr(), B, C, H, H, k, s, pad, kpad,
                                               ops.code(dt), ops._stream()), "unfold_u8")
        assert torch.equal(raw(out), raw(ref))
        # the zeros are exact zeros: cls rows, the K padding, and the out-of-image taps (F.unfold of a ones image marks them)
        o = out.cpu().float().view(B, -1, kpad)
        assert (o[:, 0] == 0).all() and (o[:, :, C * k * k:] == 0).all()
        inside = F.unfold(torch.ones(1, C, H, H), k, padding=pad, stride=s).transpose(1, 2)[0]
        assert (o[:, 1:, :C * k * k][:, inside == 0] == 0).all()
        if pad:
            assert (inside == 0).any()


@pytest.mark.parametrize("dname", list(DTYPES))
def test_u8_gathers_small_and_ragged_images(ops, dname):
    """An image whose byte count is no multiple of 8 (the last, partial word), one window per image, and a 3-channel odd size."""
    dt = DTYPES[dname]
    g = torch.Generator().manual_seed(11)
    for (B, C, H, k, s, pad) in ((1, 1, 9, 3, 3, 1), (3, 3, 9, 5, 2, 2), (5, 3, 13, 13, 1, 0), (1, 2, 7, 4, 3, 3)):
        u = torch.randint(0, 256, (B, C, H, H), dtype=torch.uint8, generator=g)
        pair = (AWKWARD[0][:C], AWKWARD[1][:C])
        ref = ops.unfold_patches(definition(u, *pair).cuda(), k, s, pad, dt)
        for name, src in layouts(u):
            assert torch.equal(raw(ops.unfold_patches(src, k, s, pad, dt, table=table(ops, pair, C))), raw(ref)), (name, B, C, H, k)


@pytest.mark.parametrize("dname", list(DTYPES))
def test_u8_two_batches_land_in_consecutive_rows(ops, dname):
    dt = DTYPES[dname]
    a, b = all_bytes(3, 3, 48, 48, seed=1), all_bytes(2, 3, 48, 48, seed=2)
    xa, xb = definition(a, *IMAGENET).cuda(), definition(b, *IMAGENET).cuda()
    tab = table(ops, IMAGENET, 3)
    ref_p, ref_u = ops.patchify((xa, xb), 8, dt), ops.unfold_patches((xa, xb), 12, 8, 4, dt)
    assert ref_u.shape == (5 * 37, 448)
    la, lb = layouts(a), layouts(b)
    for pa, pb in ((la[0][1], lb[0][1]), (la[1][1], lb[1][1]), (la[0][1], lb[1][1])):      # (also one batch of each layout)
        assert torch.equal(raw(ops.patchify((pa, pb), 8, dt, table=tab)), raw(ref_p))
        assert torch.equal(raw(ops.unfold_patches((pa, pb), 12, 8, 4, dt, table=tab)), raw(ref_u))
    with pytest.raises(ValueError, match="all uint8 or all float"):
        ops.patchify((la[0][1], xb), 8, dt, table=tab)
    with pytest.raises(RuntimeError, match="value table"):
        ops.patchify(la[0][1], 8, dt)


# ------------------------------------------------------------------------------------------------------------ (b) refusals
def test_u8_argument_checks_launch_nothing(ops):
    from gslora_hip import _lib as L
    lib = L.load()
    u = all_bytes(2, 3, 48, 48, seed=3).cuda()
    tab = table(ops, IMAGENET, 3)
    outp = torch.full((2 * 37, 192), 7.0, device="cuda", dtype=torch.float16)
    outu = torch.full((2 * 37, 448), 7.0, device="cuda", dtype=torch.float16)
    st = ops._stream()
    P, U = lib.gsl_patchify_u8, lib.gsl_unfold_patches_u8
    bad = [P(u.data_ptr(), L.U8_NCHW, None, outp.data_ptr(), 2, 3, 48, 48, 8, L.F16, st),            # null table
           P(u.data_ptr(), L.U8_NCHW, tab.data_ptr(), outp.data_ptr(), 2, 3, 48, 48, 8, 5, st),      # bad dtype
           P(u.data_ptr(), 2, tab.data_ptr(), outp.data_ptr(), 2, 3, 48, 48, 8, L.F16, st),          # bad layout code
           P(u.data_ptr(), L.U8_NHWC, tab.data_ptr(), outp.data_ptr() + 2, 2, 3, 48, 48, 8, L.F16, st),      # misaligned output
           U(u.data_ptr(), L.U8_NCHW, None, outu.data_ptr(), 2, 3, 48, 48, 12, 8, 4, 448, L.F16, st),
           U(u.data_ptr(), L.U8_NCHW, tab.data_ptr(), outu.data_ptr(), 2, 3, 48, 48, 12, 8, 4, 448, 5, st),
           U(u.data_ptr(), 7, tab.data_ptr(), outu.data_ptr(), 2, 3, 48, 48, 12, 8, 4, 448, L.F16, st),
           U(u.data_ptr(), L.U8_NHWC, tab.data_ptr(), outu.data_ptr() + 8, 2, 3, 48, 48, 12, 8, 4, 448, L.F16, st),
           U(u.data_ptr(), L.U8_NCHW, tab.data_ptr(), outu.data_ptr(), 2, 3, 48, 48, 12, 8, 12, 448, L.F16, st),      # pad >= k
           U(u.data_ptr(), L.U8_NCHW, tab.data_ptr(), outu.data_ptr(), 2, 3, 48, 48, 12, 8, 4, 444, L.F16, st)]       # ldo % 8
    assert bad == [-1] * len(bad)
    assert lib.gsl_last_error()
    torch.cuda.synchronize()
    assert (outp == 7.0).all() and (outu == 7.0).all()      # nothing was launched


# ------------------------------------------------------------------------------------------------------------ (c) the models
def build_vit(cfg, dtype, dropout=0.1, **kw):
    import loralib as lora
    from vit_pytorch_face import ViT_face
    kw.setdefault("loss_type", "CosFace")
    m = ViT_face(GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"], dim=cfg["dim"],
                 depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], dropout=dropout, emb_dropout=dropout,
                 lora_rank=cfg["lora_rank"], **kw)
    m.load_state_dict({k: torch.tensor(v) for k, v in recipe.make_state(cfg).items()}, strict=True)
    lora.mark_only_lora_as_trainable(m)
    return m.to("cuda").set_compute_dtype(dtype).train()


def build_vits(cfg, dtype, dropout=0.1):
    import loralib as lora
    from vit_pytorch_face import ViTs_face
    torch.manual_seed(5)
    m = ViTs_face(loss_type="CosFace", GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
                  ac_patch_size=12, pad=4, dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], dropout=dropout,
                  emb_dropout=dropout, lora_rank=cfg["lora_rank"])
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "lora_B" in n:
                p.normal_(0.0, 0.05)
    lora.mark_only_lora_as_trainable(m)
    return m.to("cuda").set_compute_dtype(dtype).train()


def build_vitb(cfg, dtype, dropout=0.1):
    import loralib as lora
    from util.utils import replace_ffn_with_lora
    from vit_pytorch_face import ModifiedViT
    from vit_pytorch_face.modified_VIT import vit_b_16
    vit = vit_b_16(image_size=cfg["image_size"], patch_size=cfg["patch_size"], num_layers=cfg["depth"], num_heads=cfg["heads"],
                   hidden_dim=cfg["dim"], mlp_dim=cfg["mlp_dim"], num_classes=cfg["num_class"], dropout=dropout)
    m = replace_ffn_with_lora(ModifiedViT(vit), rank=cfg["lora_rank"])
    m.load_state_dict({k: torch.tensor(v) for k, v in recipe.make_tv_state(cfg).items()}, strict=True)
    lora.mark_only_lora_as_trainable(m)
    return m.to("cuda").set_compute_dtype(dtype).train()


MODELS = {
    "vit_cls_cosface": (lambda d: build_vit(recipe.cfg_small2(), d), recipe.cfg_small2(), IMAGENET),
    "vit_mean_arcface": (lambda d: build_vit(recipe.cfg_small2(), d, pool="mean", loss_type="ArcFace"), recipe.cfg_small2(), AWKWARD),
    "vit_mean_cosface": (lambda d: build_vit(recipe.cfg_small2(), d, pool="mean"), recipe.cfg_small2(), ((0.0,) * 3, (1.0,) * 3)),
    "vit_cls_arcface": (lambda d: build_vit(recipe.cfg_small2(), d, loss_type="ArcFace"), recipe.cfg_small2(), IMAGENET),
    "vit_attention_lora": (lambda d: build_vit(recipe.cfg_small_attn(), d, lora_pos="Attention"), recipe.cfg_small_attn(), IMAGENET),
    "vits": (lambda d: build_vits(recipe.cfg_small2(), d), recipe.cfg_small2(), AWKWARD),
    "vit_b_16": (lambda d: build_vitb(recipe.cfg_vitb_small2(), d), recipe.cfg_vitb_small2(), IMAGENET),
}


def forward_at(m, calls, img, label):
    """One forward with the dropout stream at a fixed position: the same seed and forward counter give the same masks."""
    m.runner().drop_calls = calls
    out = m(img, label) if label is not None else m(img)
    return out if isinstance(out, tuple) else (None, out)


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("model", list(MODELS))
def test_model_forward_from_bytes_equals_forward_from_floats(ops, dname, model):
    mk, cfg, pair = MODELS[model]
    m = mk(MODES[dname])
    B, S = 5, cfg["image_size"]
    u = all_bytes(B, 3, S, S, seed=31)
    x = definition(u, *pair).cuda()
    y = torch.tensor(recipe.make_labels(cfg, B, seed=7)).cuda()
    assert m.set_input_norm(*pair) is m
    for training in (True, False):
        m.train(training)
        for name, src in layouts(u):
            with torch.no_grad():
                lf, ef = forward_at(m, 40, x, y)
                lu, eu = forward_at(m, 40, src, y)
                assert torch.equal(raw(lu), raw(lf)) and torch.equal(raw(eu), raw(ef)), (training, name)
                if model != "vit_b_16":      # forward(img): the embedding alone
                    assert torch.equal(raw(forward_at(m, 41, src, None)[1]), raw(forward_at(m, 41, x, None)[1])), (training, name)
    # with autograd: the LoRA gradients of a backward from the same upstream gradient
    m.train()
    grads = []
    for src in (x, layouts(u)[1][1]):
        for p in m.parameters():
            p.grad = None
        logits, emb = forward_at(m, 50, src, y)
        (logits.float().square().sum() * 1e-3 + emb.float().sum()).backward()
        grads.append(m.lora_bucket().grad.clone())
    assert grads[0].abs().max() > 0 and torch.equal(raw(grads[0]), raw(grads[1]))


def step_kw(cfg):
    return dict(beta=0.15, alpha=1e-2, BND=105.0, use_structure=True, group_type="block", use_prototype=True,
                proto_table=torch.tensor(recipe.make_prototypes(cfg)).cuda(), w_f=0.05, w_r=0.1, BND_pro=2.0)


def byte_batch(cfg, b, s, B_f=None):
    nf = max(2, cfg["num_class"] // 5)
    S = cfg["image_size"]
    return (all_bytes(b, 3, S, S, seed=100 + s), torch.tensor(recipe.make_labels(cfg, b, seed=100 + s, tag="yr", lo=0, hi=cfg["num_class"] - nf)),
            all_bytes(B_f or b, 3, S, S, seed=200 + s),
            torch.tensor(recipe.make_labels(cfg, B_f or b, seed=200 + s, tag="yf", lo=cfg["num_class"] - nf, hi=cfg["num_class"])))


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("model", ["vit_cls_cosface", "vits"])
def test_one_step_from_bytes_equals_one_step_from_floats(ops, dname, fuse, model):
    from gslora_hip.optim import FusedAdamW
    from gslora_hip.step import gs_lora_step
    mk, cfg, pair = MODELS[model]
    m1 = mk(MODES[dname])
    m2 = copy.deepcopy(m1).set_input_norm(*pair)
    mk_opt = lambda m: FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-2, weight_decay=0.05, eps=1e-8)
    o1, o2 = mk_opt(m1), mk_opt(m2)
    crit = torch.nn.CrossEntropyLoss()
    kw = step_kw(cfg)
    ur, yr, uf, yf = byte_batch(cfg, 6, 0, B_f=5)
    p1 = gs_lora_step(m1, o1, crit, definition(ur, *pair).cuda(), yr.cuda(), definition(uf, *pair).cuda(), yf.cuda(), fuse_batches=fuse, **kw)
    p2 = gs_lora_step(m2, o2, crit, layouts(ur)[1][1], yr.cuda(), uf.cuda(), yf.cuda(), fuse_batches=fuse, **kw)      # NHWC remain, NCHW forget
    assert torch.equal(raw(p1), raw(p2)), (p1.tolist(), p2.tolist())
    g1, g2 = m1.lora_bucket().grad, m2.lora_bucket().grad
    assert g1.abs().max() > 0 and torch.equal(raw(g1), raw(g2))
    assert torch.equal(raw(m1.lora_bucket().flat), raw(m2.lora_bucket().flat))
    with pytest.raises(ValueError, match="both uint8 or both float"):
        gs_lora_step(m2, o2, crit, ur.cuda(), yr.cuda(), definition(uf, *pair).cuda(), yf.cuda(), fuse_batches=fuse, **kw)


# ------------------------------------------------------------------------------------------------------------ (d) HIP graph
@pytest.mark.parametrize("dname", list(DTYPES))
def test_graph_replay_with_uint8_static_inputs_equals_eager(ops, dname):
    """The launch-bound few-shot shape (ViT-P8S8 depth 6, 112 px, batch 4 + 4): three steps through the graph stepper with uint8 inputs are
    bit-identical to eager float steps, new bytes between replays are picked up, and a changed normalisation is a new graph key."""
    from gslora_hip.optim import FusedAdamW
    from gslora_hip.step import GraphedStep, gs_lora_step
    cfg = recipe.cfg_full()
    m1 = build_vit(cfg, MODES[dname])
    m2 = copy.deepcopy(m1).set_input_norm(*IMAGENET)
    mk_opt = lambda m: FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-2, weight_decay=0.05, eps=1e-8)
    o1, o2 = mk_opt(m1), mk_opt(m2)
    crit = torch.nn.CrossEntropyLoss()
    kw = step_kw(cfg)
    g = GraphedStep(m2, o2, crit)
    packs = []
    for s in range(4):      # step 0 eager (first sighting), step 1 captured + replayed, 2 and 3 replayed
        ur, yr, uf, yf = byte_batch(cfg, 4, s)
        p1 = gs_lora_step(m1, o1, crit, definition(ur, *IMAGENET).cuda(), yr.cuda(), definition(uf, *IMAGENET).cuda(), yf.cuda(), **kw)
        p2 = g(ur.cuda(), yr.cuda(), uf.cuda(), yf.cuda(), **kw)
        assert torch.equal(raw(p1), raw(p2)), (s, p1.tolist(), p2.tolist())
        assert torch.equal(raw(m1.lora_bucket().flat), raw(m2.lora_bucket().flat)), s
        packs.append(p2.clone())
    assert (g.eager_steps, g.captures, g.replays) == (1, 1, 3)
    assert not torch.equal(packs[2], packs[3])      # the new bytes of step 3 were read
    ent = next(iter(g.graphs.values()))
    assert ent["static"][0].dtype == torch.uint8 and ent["static"][2].dtype == torch.uint8
    # a graph captured under one normalisation is not replayed under another
    m1b_pair = AWKWARD
    m2.set_input_norm(*m1b_pair)
    ur, yr, uf, yf = byte_batch(cfg, 4, 9)
    p1 = gs_lora_step(m1, o1, crit, definition(ur, *m1b_pair).cuda(), yr.cuda(), definition(uf, *m1b_pair).cuda(), yf.cuda(), **kw)
    p2 = g(ur.cuda(), yr.cuda(), uf.cuda(), yf.cuda(), **kw)
    assert g.eager_steps == 2 and torch.equal(raw(p1), raw(p2))


# ------------------------------------------------------------------------------------------------------------ (e) the engine
@pytest.mark.parametrize("dname", list(DTYPES))
def test_engine_from_host_uint8_batches_equals_engine_from_host_float_batches(ops, dname, tmp_path):
    import engine_cl
    from gslora_hip.optim import FusedAdamW
    from util.utils import AverageMeter, calculate_prototypes
    cfg, b = recipe.cfg_small2(), 5
    pair = IMAGENET
    proto_np = recipe.make_prototypes(cfg)
    proto = {c: torch.tensor(proto_np[c]) for c in range(cfg["num_class"])}
    res = {}
    for feed in ("float", "u8"):
        m = build_vit(cfg, MODES[dname])
        if feed == "u8":
            m.set_input_norm(*pair)
        # host batches; every other remain batch as NHWC bytes
        conv = (lambda u, i: definition(u, *pair)) if feed == "float" else (lambda u, i: u.to(memory_format=torch.channels_last) if i % 2 else u)
        data = [byte_batch(cfg, b, s) for s in range(4)]
        loader_r = [(conv(d[0], i), d[1]) for i, d in enumerate(data)]
        loader_f = [(conv(d[2], i + 1), d[3]) for i, d in enumerate(data)]      # (through data_prefetcher: pinned staging, copy stream)
        opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-2, weight_decay=0.05, eps=1e-8)
        crit = torch.nn.CrossEntropyLoss()
        cfgd = {"DATA_ROOT": "./data/casia100/", "BND_pro": 2.0, "MULTI_GPU": False, "WORK_PATH": str(tmp_path / feed), "BACKBONE_NAME": "VIT",
                "HIP_GRAPH": False}
        (tmp_path / feed).mkdir()
        mk = AverageMeter
        meters = dict(losses_forget=mk(), losses_remain=mk(), losses_total=mk(), losses_structure=mk(), top1_forget=mk(),
                      top1_remain=mk(), losses_prototype_forget=mk(), losses_prototype_remain=mk())
        ret = engine_cl.train_one_epoch(
            model=m, dataloader_forget=loader_f, dataloader_remain=loader_r, device=torch.device("cuda"), criterion=crit, optimizer=opt,
            epoch=0, beta=0.15, alpha=1e-2, BND=105.0, batch=0, testloader_forget=None, testloader_remain=None, forget_acc_before=0.0,
            highest_H_mean=0.0, cfg=cfgd, task_i="0", use_prototype=True, prototype_dict=proto, prototype_weight_forget=0.05,
            prototype_weight_remain=0.1, **meters)
        bucket = m.lora_bucket().flat.clone()
        grad = m.lora_bucket().grad.clone()
        acc_f = engine_cl.eval_data(m, loader_f, torch.device("cuda"), "forget")
        acc_r = engine_cl.eval_data(m, loader_r, torch.device("cuda"), "remain")
        h = engine_cl.evaluate(m, loader_f, loader_r, torch.device("cuda"), batch=3, epoch=0, forget_acc_before=100.0, highest_H_mean=-1.0,
                               cfg=cfgd, optimizer=opt, task_i="0")
        ds = torch.utils.data.TensorDataset(torch.cat([x for x, _ in loader_r]).contiguous(), torch.cat([y for _, y in loader_r]))
        protos = calculate_prototypes(m, ds, batch_size=7, device="cuda")
        res[feed] = ([ret[i].avg for i in range(2, 10)], bucket, grad, acc_f, acc_r, h, protos)
    assert res["float"][0] == res["u8"][0]
    assert torch.equal(raw(res["float"][1]), raw(res["u8"][1])) and torch.equal(raw(res["float"][2]), raw(res["u8"][2]))
    assert res["float"][3:6] == res["u8"][3:6]
    assert sorted(res["float"][6]) == sorted(res["u8"][6])
    for c in res["float"][6]:
        assert torch.equal(res["float"][6][c], res["u8"][6][c]), c


# ------------------------------------------------------------------------------------------------------------ (f) what must not move
@pytest.mark.parametrize("dname", list(DTYPES))
def test_uint8_without_set_input_norm_is_still_a_value_cast(ops, dname):
    cfg = recipe.cfg_small2()
    m = build_vit(cfg, MODES[dname], dropout=0.0)
    u = all_bytes(3, 3, 48, 48, seed=5)
    y = torch.tensor(recipe.make_labels(cfg, 3, seed=7)).cuda()
    with torch.no_grad():
        lu, eu = m(u.cuda(), y)
        lf, ef = m(u.float().cuda(), y)
    assert torch.equal(raw(lu), raw(lf)) and torch.equal(raw(eu), raw(ef))
    # and a float batch of an opted-in model is untouched by the opt-in
    m.set_input_norm(*IMAGENET)
    with torch.no_grad():
        l2, e2 = m(u.float().cuda(), y)
    assert torch.equal(raw(l2), raw(lf)) and torch.equal(raw(e2), raw(ef))
    with pytest.raises(ValueError, match="all uint8 or all float"):
        m((u.cuda(), u.float().cuda()), torch.cat([y, y]))
