"""The head above 1024 classes (csrc/head.hip, the class-tiled kernels behind gsl_head_fwd / gsl_head_bwd and their _margin twins).

 (a) op level against float64 torch autograd of the reference formulas (vit_face.py:171-208 CosFace, :110-143 ArcFace, :47-50 linear), the
     construction of tests/test_hip_heads.py. Bars: logits / emb < 1e-4 absolute in f32, gradients <= 1e-4 * max(1, |g|); a 16-bit stream or
     dxb within 1e-2 relative of the f32 gradient (the bar of test_hip_heads.py). Shapes: the smallest that can break the tiling — the
     logits tile is 64 images x 128 classes, the d e-hat tile 32 images x 64 columns with K tiles of 32 classes (and of 32 columns of D).
 (b) guard bands and NaN padding around every tensor, determinism, batch invariance, the fp16 loss scale, the C <= 1024 dispatch;
 (c) the models: LoRA gradients through the whole class loop against a float64 head on the model's own emb, the 16-bit steps, HIP-graph
     replay, evaluation."""
import copy
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from guard_bands import Banded, ptr
from oracle import recipe

pytestmark = pytest.mark.gpu

S, M_COS, M_ARC, EPS = 64.0, 0.35, 0.5, 1e-5
TH = math.cos(math.pi - M_ARC)      # -0.878
TARGETS = [0.7, 0.2, -0.5, -0.95, -0.99, 0.9, -0.2, 0.4]      # label cosines: both sides of th and of 0, none within 1e-3 of either
FORMS = ["cosface", "arcface", "arcface_easy", "linear_bias"]


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


def bar_ok(got, want, what=""):
    got, want = got.double(), want.double()
    err = ((got - want).abs() / max(1.0, want.abs().max().item())).max().item()
    print(f"{what}: max err / bar = {err / 1e-4:.4f}")
    return err <= 1e-4


def pooled_emb(x64, B, T, D, g, b, pool_mean):
    xb = x64.view(B, T, D)
    return F.layer_norm(xb.mean(1) if pool_mean else xb[:, 0], (D,), g, b, EPS)


class Case:
    """Inputs of one head call. The cosine heads' label rows of W are set so that cos(emb_b, W[y_b]) = TARGETS[(b + first) % 8]."""

    def __init__(self, form, B, C, D, T, pool_mean=False, xdt=torch.float32, seed=0, first=0, dl_scale=1.0):
        self.form, self.B, self.C, self.D, self.T, self.pool_mean = form, B, C, D, T, pool_mean
        self.linear, self.easy = form == "linear_bias", form == "arcface_easy"
        self.x = rnd(B * T, D, seed=seed + 1, scale=2.0).to(xdt)
        self.g, self.b = (1 + 0.1 * rnd(D, seed=seed + 2)).float(), (0.1 * rnd(D, seed=seed + 3)).float()
        self.y = torch.randperm(C, generator=torch.Generator().manual_seed(seed + 4))[:B]
        if self.linear:
            W = rnd(C, D, seed=seed + 5, scale=0.05)
            self.bias = rnd(C, seed=seed + 7, scale=0.5).float()
        else:
            W = rnd(C, D, seed=seed + 5)
            e = F.normalize(pooled_emb(self.x.double(), B, T, D, self.g.double(), self.b.double(), pool_mean))
            u = rnd(B, D, seed=seed + 6)
            u = F.normalize(u - (u * e).sum(1, keepdim=True) * e)
            t = torch.tensor([TARGETS[(i + first) % 8] for i in range(B)], dtype=torch.float64)[:, None]
            W[self.y] = 0.7 * (t * e + torch.sqrt(1 - t * t) * u)
            self.bias = None
        self.W = W.float()
        self.dl = rnd(B, C, seed=seed + 11, scale=dl_scale).float()
        self.de = rnd(B, D, seed=seed + 12, scale=0.5).float()

    def reference(self, use_dl=True, use_de=True):
        """float64 autograd -> logits, emb, cos_y (cosine heads), d loss / d x [B*T, D] for loss = <logits, dl> + <emb, de>."""
        B, T, D = self.B, self.T, self.D
        x64 = self.x.double().requires_grad_(True)
        emb = pooled_emb(x64, B, T, D, self.g.double(), self.b.double(), self.pool_mean)
        W, yy, cy = self.W.double(), self.y[:, None], None
        if self.linear:
            logits = emb @ W.T + self.bias.double()
        else:
            cos = F.normalize(emb) @ F.normalize(W).T
            cy = cos.gather(1, yy)
            if self.form == "cosface":
                lab = cy - M_COS
            else:
                phi = cy * math.cos(M_ARC) - torch.sqrt(1.0 - cy * cy) * math.sin(M_ARC)
                lab = torch.where(cy > 0, phi, cy) if self.easy else torch.where(cy > TH, phi, cy - math.sin(math.pi - M_ARC) * M_ARC)
            logits = S * cos.scatter(1, yy, lab)
        loss = (emb * 0).sum()
        if use_dl:
            loss = loss + (logits * self.dl.double()).sum()
        if use_de:
            loss = loss + (emb * self.de.double()).sum()
        (dx,) = torch.autograd.grad(loss, x64)
        return logits.detach(), emb.detach(), (cy.detach()[:, 0] if cy is not None else None), dx

    def forward(self, ops):
        """-> (logits, emb, mean, rstd, cos_y, Wn) on the device"""
        c = lambda t: None if t is None else t.cuda()
        Wn = c(self.W) if self.linear else ops.cosface_prep(c(self.W))
        ln = (c(self.x), self.B, self.T, self.D, c(self.g), c(self.b), EPS, Wn)
        if self.linear:
            out = ops.head_fwd(*ln, None, 1.0, 0.0, head_bias=c(self.bias), linear=True, pool_mean=self.pool_mean) + (None,)
        elif self.form == "cosface":
            out = ops.head_fwd(*ln, c(self.y), S, M_COS, pool_mean=self.pool_mean) + (None,)
        else:
            out = ops.head_fwd_margin(*ln, c(self.y), S, 0.0, "arcface", m=M_ARC, easy_margin=self.easy, pool_mean=self.pool_mean)
        return out + (Wn,)

    def backward(self, ops, fwd, dt=torch.float32, use_dl=True, use_de=True, **kw):
        logits, emb, mean, rstd, cos_y, Wn = fwd
        dl, de = (self.dl.cuda() if use_dl else None), (self.de.cuda() if use_de else None)
        args = (dl, de, self.x.cuda(), self.B, self.T, self.D, self.g.cuda(), mean, rstd, emb, Wn, 1.0 if self.linear else S, dt)
        kw = dict(dict(linear=self.linear, pool_mean=self.pool_mean), **kw)
        if self.form.startswith("arcface"):
            return ops.head_bwd_margin(*args, "arcface", m=M_ARC, easy_margin=self.easy, cos_y=cos_y, label=self.y.cuda(), **kw)
        return ops.head_bwd(*args, **kw)

    def check_branches(self, cy):
        """A condition on the inputs: the label cosines lie on both sides of the threshold in use, none within 1e-3 of it."""
        if not self.form.startswith("arcface"):
            return
        th = 0.0 if self.easy else TH
        assert ((cy - th).abs() > 1e-3).all()
        if self.B >= 5:
            assert (cy > th).any() and (cy < th).any()


# ------------------------------------------------------------------------------------------------------------ (a) op level
# (B, C, D, T, pool, demb): C = 1025 the first tiled size, 1151 / 1153 around 9 class tiles of 128 (and 36 K tiles of 32), 2049 one past 16;
# B around the 32- and 64-image tiles; D = 64 one column tile, 192 ragged in the 64-column tile, 1024 the most; T = 2, 5
SHAPES = [(1, 1025, 64, 2, "cls_compact", True), (31, 1100, 192, 5, "mean", False), (33, 1151, 512, 2, "cls_dense", True),
          (63, 1153, 64, 5, "cls_compact", False), (65, 2049, 1024, 2, "mean", True), (37, 1100, 512, 5, "cls_dense", False)]


def check_forward(case, fwd, ref):
    logits, emb, mean, rstd, cos_y, _ = fwd
    lo_r, emb_r, cy_r, _ = ref
    e_emb, e_lo = (emb.cpu().double() - emb_r).abs().max().item(), (logits.cpu().double() - lo_r).abs().max().item()
    print(f"{case.form}: emb err {e_emb:.3e}, logits err {e_lo:.3e}")
    assert e_emb < 1e-4 and e_lo < 1e-4
    if case.form.startswith("arcface"):
        assert (cos_y.cpu().double() - cy_r).abs().max() < 1e-4 / S      # the logits' bar, before the scale s
    else:
        assert cos_y is None


def check_backward(ops, case, got, ref_dx, compact, dt=torch.float32, p_drop=0.25, seed=5, site=3, what=""):
    B, T, D = case.B, case.T, case.D
    dx, dxb = got
    ref = ref_dx.view(B, T, D)[:, 0] if compact else ref_dx
    assert dx.shape == ref.shape
    assert bar_ok(dx.cpu(), ref, f"{case.form} {what} dx")
    keep = ops.dropout_mask(B * T * D, p_drop, seed, site, "cuda").cpu().view(B, T, D).float()
    keep = keep[:, 0] if compact else keep.view(B * T, D)
    want = dx.cpu().float() * keep * (1.0 / (1.0 - p_drop))
    tol = 1e-6 if dt == torch.float32 else 1e-2
    assert ((dxb.cpu().float() - want).abs() - tol * want.abs()).max() <= 1e-6
    if not compact and not case.pool_mean:
        assert (dx.view(B, T, D)[:, 1:] == 0).all() and (dxb.view(B, T, D)[:, 1:] == 0).all()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:4])))
@pytest.mark.parametrize("form", FORMS)
def test_op_matches_float64_autograd(ops, form, shape):
    B, C, D, T, pool, with_de = shape
    pool_mean, compact = pool == "mean", pool == "cls_compact"
    # a single image cannot straddle a threshold: B = 1 runs once on each side
    for first in ((0, 3) if B == 1 else (0,)):
        case = Case(form, B, C, D, T, pool_mean, seed=C + B, first=first)
        ref = case.reference(use_de=with_de)
        if ref[2] is not None:
            case.check_branches(ref[2])
            if B == 1 and form.startswith("arcface"):
                assert (ref[2].item() > max(TH, 0.0)) == (first == 0)
        fwd = case.forward(ops)
        check_forward(case, fwd, ref)
        got = case.backward(ops, fwd, use_de=with_de, p_drop=0.25, seed=5, site=3, compact=compact)
        check_backward(ops, case, got, ref[3], compact, what=str(shape[:4]))


@pytest.mark.parametrize("form", ["cosface", "arcface", "linear_bias"])
def test_demb_only_backward_skips_the_class_loop(ops, form):
    """dlogits == NULL: the gradient of emb alone (the embedding losses), no stage 1."""
    case = Case(form, 33, 1100, 192, 2, seed=50)
    ref = case.reference(use_dl=False)
    fwd = case.forward(ops)
    got = case.backward(ops, fwd, use_dl=False, p_drop=0.25, seed=5, site=3, compact=True)
    check_backward(ops, case, got, ref[3], True, what="demb only")


@pytest.mark.parametrize("xname", ["bf16", "f16"])
@pytest.mark.parametrize("form", FORMS)
def test_16_bit_stream_and_gradients(ops, form, xname):
    """x in a 16-bit format (emb and logits stay f32 arithmetic on the rounded x), dxb in the operand format, dx f32 or 16-bit."""
    xdt = {"bf16": torch.bfloat16, "f16": torch.float16}[xname]
    case = Case(form, 37, 1100, 192, 5, seed=60, xdt=xdt, dl_scale=0.1)
    ref = case.reference()
    case.check_branches(ref[2]) if ref[2] is not None else None
    fwd = case.forward(ops)
    check_forward(case, fwd, ref)
    for compact in (True, False):
        dx32, dxb = got = case.backward(ops, fwd, dt=xdt, p_drop=0.25, seed=5, site=3, compact=compact)
        assert dx32.dtype == torch.float32 and dxb.dtype == xdt
        check_backward(ops, case, got, ref[3], compact, dt=xdt, what=f"{xname} x")
        dx16, dxb16 = case.backward(ops, fwd, dt=xdt, p_drop=0.25, seed=5, site=3, compact=compact, stream_dtype=xdt)
        assert dx16.dtype == xdt and torch.equal(dxb16, dxb)
        assert ((dx16.float() - dx32).abs() - 1e-2 * dx32.abs()).max() <= 1e-6


# ------------------------------------------------------------------------------------------------------------ (b) edges
def raw_forward(ops, case, x, g, b, Wn, y, bias, emb, mean, rstd, logits, cos_y):
    """The C entry points on raw addresses (the tensors live inside guard bands)."""
    from gslora_hip import _lib as L
    B, T, D, C = case.B, case.T, case.D, case.C
    head = (x, ops.code(case.x.dtype), T, g, b, EPS, Wn, y, emb, mean, rstd, logits, B, D, C)
    st = torch.cuda.current_stream().cuda_stream
    if case.linear:
        rc = L.load().gsl_head_fwd(*head, 1.0, 0.0, bias, 1, int(case.pool_mean), st)
    elif case.form == "cosface":
        rc = L.load().gsl_head_fwd(*head, S, M_COS, None, 0, int(case.pool_mean), st)
    else:
        rc = L.load().gsl_head_fwd_margin(*head, S, 0.0, None, 0, int(case.pool_mean), 1, M_ARC, int(case.easy), cos_y, st)
    L.check(rc, "head forward")


def raw_backward(ops, case, dl, de, x, g, mean, rstd, emb, Wn, dx, dxb, dt, stream_dt, p_drop, seed, site, compact, gscale, ws, cos_y, y):
    from gslora_hip import _lib as L
    B, T, D, C = case.B, case.T, case.D, case.C
    head = (dl, de, x, ops.code(case.x.dtype), T, g, mean, rstd, emb, Wn, dx, dxb, B, D, C, 1.0 if case.linear else S, ops.code(dt),
            ops.code(stream_dt), float(p_drop), int(seed), int(site), int(case.linear), int(case.pool_mean), int(compact), gscale, ws, 0)
    st = torch.cuda.current_stream().cuda_stream
    if case.form.startswith("arcface"):
        return L.load().gsl_head_bwd_margin(*head, 1, M_ARC, int(case.easy), cos_y, y, st)
    return L.load().gsl_head_bwd(*head, st)


@pytest.mark.parametrize("form", ["cosface", "arcface", "linear_bias"])
def test_guard_bands_and_nan_padding(ops, form):
    """Every tensor sits between two bands: NaN around the inputs (Wn, head_bias and dlogits continue in NaN past C, emb and x past B),
    a sentinel around the outputs, whose own elements start as NaN. Nothing outside a view changes, every element of a view is stored,
    and the results are those of the plain call bit for bit."""
    from gslora_hip import _lib as L
    case = Case(form, 33, 1100, 192, 2, seed=70)
    B, T, D, C = case.B, case.T, case.D, case.C
    fwd = case.forward(ops)
    want_dx, want_dxb = case.backward(ops, fwd, p_drop=0.25, seed=5, site=3, compact=False)
    logits, emb, mean, rstd, cos_y, Wn = fwd
    f32 = torch.float32
    i = {k: Banded(v.shape, v.dtype, src=v.cuda()) for k, v in
         dict(x=case.x, g=case.g, b=case.b, y=case.y, dl=case.dl, de=case.de).items()}
    i["Wn"] = Banded(Wn.shape, f32, src=Wn)
    if case.linear:
        i["bias"] = Banded((C,), f32, src=case.bias.cuda())
    o = dict(emb=Banded((B, D), f32), mean=Banded((B,), f32), rstd=Banded((B,), f32), logits=Banded((B, C), f32), cos_y=Banded((B,), f32),
             dx=Banded((B * T, D), f32), dxb=Banded((B * T, D), f32), ws=Banded((B * (D + 1),), f32))
    for k in ("emb", "mean", "rstd", "logits", "dx", "dxb"):
        o[k].view.fill_(float("nan"))
    raw_forward(ops, case, ptr(i["x"]), ptr(i["g"]), ptr(i["b"]), ptr(i["Wn"]), ptr(i["y"]), ptr(i.get("bias")), ptr(o["emb"]), ptr(o["mean"]),
                ptr(o["rstd"]), ptr(o["logits"]), ptr(o["cos_y"]))
    for k, t in dict(emb=emb, mean=mean, rstd=rstd, logits=logits).items():
        assert torch.equal(o[k].view, t), k
    if form == "arcface":
        assert torch.equal(o["cos_y"].view, cos_y) and o["cos_y"].unwritten() == 0
    # the backward reads the forward's outputs from banded INPUTS: emb, mean, rstd, cos_y continue in NaN past B
    for k in ("emb", "mean", "rstd", "cos_y"):
        i[k] = Banded(o[k].view.shape, f32, src=o[k].view)
    rc = raw_backward(ops, case, ptr(i["dl"]), ptr(i["de"]), ptr(i["x"]), ptr(i["g"]), ptr(i["mean"]), ptr(i["rstd"]), ptr(i["emb"]), ptr(i["Wn"]),
                      ptr(o["dx"]), ptr(o["dxb"]), f32, f32, 0.25, 5, 3, False, None, ptr(o["ws"]), ptr(i["cos_y"]), ptr(i["y"]))
    L.check(rc, "head backward")
    torch.cuda.synchronize()
    assert torch.equal(o["dx"].view, want_dx) and torch.equal(o["dxb"].view, want_dxb)
    assert torch.isfinite(o["dx"].view).all() and torch.isfinite(o["logits"].view).all()
    # d e-hat: every element behind the B maxima (which only the loss-scaled form writes) is stored
    assert int((o["ws"].view.view(torch.int32)[B:] == o["ws"].sent).sum()) == 0
    for k, band in {**i, **o}.items():
        assert band.bands_intact(), k


@pytest.mark.parametrize("form", FORMS)
def test_bit_repeatable_and_row_b_does_not_depend_on_the_batch(ops, form):
    case = Case(form, 37, 1100, 192, 5, seed=80)
    B, T, D = case.B, case.T, case.D
    fwd = case.forward(ops)
    dx, _ = case.backward(ops, fwd, compact=True)
    fwd2 = case.forward(ops)
    dx2, _ = case.backward(ops, fwd2, compact=True)
    assert torch.equal(fwd[0], fwd2[0]) and torch.equal(fwd[1], fwd2[1]) and torch.equal(dx, dx2)
    for b in (0, 17, 36):
        one = copy.copy(case)
        one.B, one.x, one.y, one.dl, one.de = 1, case.x[b * T:(b + 1) * T], case.y[b:b + 1], case.dl[b:b + 1], case.de[b:b + 1]
        f1 = one.forward(ops)
        d1, _ = one.backward(ops, f1, compact=True)
        assert torch.equal(f1[0][0], fwd[0][b]) and torch.equal(f1[1][0], fwd[1][b]), (form, b)
        if fwd[4] is not None:
            assert torch.equal(f1[4][0], fwd[4][b])
        assert torch.equal(d1[0], dx[b]), (form, b)


@pytest.mark.parametrize("form", ["arcface", "cosface"])
def test_fp16_loss_scaled_backward_at_1100_classes(ops, form):
    """The two-pass loss scale around ONE run of the class loop: S is the power of two with S * max|dx| in [2^10, 2^11), gscale[3] = 11,
    gscale[2] is cleared, and dx / S is the unscaled gradient (the bar of test_hip_heads.test_arcface_fp16_loss_scaled_backward)."""
    case = Case(form, 33, 1100, 192, 2, seed=90, xdt=torch.float16, dl_scale=1e-2)
    case.de = case.de * 2e-3
    ref = case.reference()
    fwd = case.forward(ops)
    dx_u, _ = case.backward(ops, fwd, dt=torch.float16, compact=True)
    for start in ([0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 700.0, 11.0]):
        gscale = torch.tensor(start, device="cuda")
        dx_s, dxb_s = case.backward(ops, fwd, dt=torch.float16, compact=True, gscale=gscale)
        Sg = gscale[0].item()
        assert Sg == 2.0 ** round(math.log2(Sg)) and gscale[1].item() == 1.0 / Sg
        assert 1024.0 <= Sg * dx_u.abs().max().item() < 2048.0
        assert gscale[3].item() == 11.0 and gscale[2].item() == 0.0
        assert torch.equal(dx_s, dx_u * Sg)
        assert ((dxb_s.float() - dx_s).abs() - 1e-2 * dx_s.abs()).max() <= 1e-6
    want = ref[3].view(case.B, case.T, case.D)[:, 0]
    assert ((dx_s.cpu().double() / Sg) - want).abs().max() < 2e-5 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("C", [100, 1024])
def test_up_to_1024_classes_nothing_moved(ops, C):
    """The dispatch guard: at C <= 1024 the workspace contract is the old one — amax_ws [B] with gscale (a band behind it stays intact: the
    tiled backward would put d e-hat there), NULL without — and the results are the plain calls'. At C = 1024 the logits are NOT the bits
    of the tiled kernel (the first 1024 columns of a 1025-class call on the same rows): the per-image kernel sums in another order."""
    from gslora_hip import _lib as L
    case = Case("cosface", 33, C, 192, 2, seed=100, xdt=torch.float16, dl_scale=1e-2)
    B, T, D = case.B, case.T, case.D
    fwd = case.forward(ops)
    logits, emb, mean, rstd, _, Wn = fwd
    ref = case.reference()
    check_forward(case, fwd, ref)
    cu = lambda t: t.cuda()
    f16, f32 = torch.float16, torch.float32
    # f32 stream gradients, no loss scale: amax_ws = NULL is accepted
    dx = torch.empty(B, D, device="cuda")
    dxb = torch.empty(B, D, device="cuda", dtype=f16)
    x, g, dl, de = cu(case.x), cu(case.g), cu(case.dl), cu(case.de)
    a = lambda t: t.data_ptr()
    rc = raw_backward(ops, case, a(dl), a(de), a(x), a(g), a(mean), a(rstd), a(emb), a(Wn), a(dx), a(dxb), f16, f32, 0.0, 0, 0, True, None, None,
                      None, None)
    L.check(rc, "gsl_head_bwd")
    want = case.backward(ops, fwd, dt=f16, compact=True)
    assert torch.equal(dx, want[0]) and torch.equal(dxb, want[1])
    assert bar_ok(dx.cpu(), ref[3].view(B, T, D)[:, 0], f"C = {C} dx")
    # loss-scaled: the workspace is B floats
    ws = Banded((B,), f32)
    gs1, gs2 = torch.zeros(4, device="cuda"), torch.zeros(4, device="cuda")
    rc = raw_backward(ops, case, a(dl), a(de), a(x), a(g), a(mean), a(rstd), a(emb), a(Wn), a(dx), a(dxb), f16, f32, 0.0, 0, 0, True, a(gs1), ptr(ws),
                      None, None)
    L.check(rc, "gsl_head_bwd")
    want = case.backward(ops, fwd, dt=f16, compact=True, gscale=gs2)
    assert torch.equal(dx, want[0]) and torch.equal(dxb, want[1]) and torch.equal(gs1, gs2)
    assert ws.bands_intact() and ws.unwritten() == 0
    if C == 1024:
        wide = copy.copy(case)
        wide.C, wide.W = C + 1, torch.cat((case.W, case.W[:1]))
        tiled = wide.forward(ops)[0][:, :C]
        assert (tiled - logits).abs().max() < 1e-4 and not torch.equal(tiled, logits)


# ------------------------------------------------------------------------------------------------------------ (c) models
# (40 px in 8 px patches: 25 patches, the fewest the constructors accept above their floor of 16)
CFG = dict(image_size=40, patch_size=8, dim=64, depth=2, heads=1, dim_head=64, mlp_dim=128, num_class=1100, lora_rank=4, channels=3)


def head_state(cfg, head):
    st = recipe.make_state(cfg)
    if head == "Softmax":
        st["loss.bias"] = recipe.uniform("loss.bias", (cfg["num_class"],), 1337, -0.5, 0.5)
    return st


def build(head="CosFace", dtype="fp32", dropout=0.0, train="lora", cls=None, cfg=CFG):
    import loralib as lora
    from vit_pytorch_face import ViT_face, ViTs_face
    kw = dict(loss_type=head, GPU_ID=[0], num_class=cfg["num_class"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
              dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], mlp_dim=cfg["mlp_dim"], dropout=dropout, emb_dropout=dropout,
              lora_rank=cfg["lora_rank"])
    if cls == "ViTs_face":
        torch.manual_seed(7)
        m = ViTs_face(ac_patch_size=12, pad=4, **kw)
        with torch.no_grad():      # loralib zero-initialises lora_B: give the adapters' A side a gradient
            for n, p in m.named_parameters():
                if "lora_B" in n:
                    p.normal_(0.0, 0.02)
    else:
        m = ViT_face(**kw)
        m.load_state_dict({k: torch.tensor(v) for k, v in head_state(cfg, head).items()}, strict=True)
    if train == "lora":
        lora.mark_only_lora_as_trainable(m)
    else:
        for n, p in m.named_parameters():
            p.requires_grad = "loss" in n
    return m.to("cuda").set_compute_dtype(dtype).train()


def batches(cfg, batch, s=0):
    nf = max(2, cfg["num_class"] // 5)
    mk = lambda a: torch.tensor(a).cuda()
    return (mk(recipe.make_images(cfg, batch, seed=100 + s, tag="xr")),
            mk(recipe.make_labels(cfg, batch, seed=100 + s, tag="yr", lo=0, hi=cfg["num_class"] - nf)),
            mk(recipe.make_images(cfg, batch, seed=200 + s, tag="xf")),
            mk(recipe.make_labels(cfg, batch, seed=200 + s, tag="yf", lo=cfg["num_class"] - nf, hi=cfg["num_class"])))


def lora_grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.requires_grad}


def head64(m, head, emb, y):
    """logits of the model's head in float64 from its (differentiable) emb: vit_face.py:171-208, 110-143, 47-50."""
    W = m.loss.weight.detach().double()
    if head == "Softmax":
        return emb @ W.T + m.loss.bias.detach().double()
    cos = F.normalize(emb) @ F.normalize(W).T
    cy = cos.gather(1, y[:, None])
    if head == "CosFace":
        lab = cy - m.loss.m
    else:
        mm = m.loss.m
        phi = cy * math.cos(mm) - torch.sqrt(1.0 - cy * cy) * math.sin(mm)
        lab = torch.where(cy > math.cos(math.pi - mm), phi, cy - math.sin(math.pi - mm) * mm)
    return m.loss.s * cos.scatter(1, y[:, None], lab)


@pytest.mark.parametrize("head,cls", [("CosFace", "ViT_face"), ("ArcFace", "ViT_face"), ("Softmax", "ViT_face"), ("CosFace", "ViTs_face")])
def test_model_lora_gradients_through_1100_classes(head, cls):
    """Reference: the model's own emb, the head and the mean CE in float64 autograd, d emb sent back through emb.backward() — a route that
    never enters the class loop. Under test: model(x, y) -> ce_sum_top1 -> backward."""
    from gslora_hip import losses
    m = build(head, cls=cls)
    x, y, _, _ = batches(CFG, 37)
    emb = m(x)
    e64 = emb.detach().double().requires_grad_(True)
    lo64 = head64(m, head, e64, y)
    F.cross_entropy(lo64, y).backward()
    emb.backward(e64.grad.float())
    want = lora_grads(m)
    assert any(v.abs().max() > 0 for v in want.values())
    m.zero_grad()
    logits, emb2 = m(x, y)
    assert torch.equal(emb2, emb.detach())
    assert (logits.double() - lo64.detach()).abs().max() < 1e-4
    (losses.ce_sum_top1(logits, y)[0] / x.shape[0]).backward()
    for n, g in lora_grads(m).items():
        assert bar_ok(g.cpu(), want[n].cpu(), f"{cls} {head} {n}")


HY = dict(beta=0.15, alpha=1e-2, BND=105.0)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_steps_in_16_bit_within_the_declared_tolerance(dtype):
    """One gs_lora_step and one head_probe_step at 1100 classes against the f32 step: DESIGN.md section 1 (6 % relative Frobenius, cosine
    above 0.995 on the gradient; the meters follow the logits' 0.25)."""
    from gslora_hip.optim import create_optimizer
    from gslora_hip.step import gs_lora_step, head_probe_step
    args = SimpleNamespace(opt="adamw", lr=1e-3, weight_decay=0.05, opt_eps=1e-8, opt_betas=None)
    crit = torch.nn.CrossEntropyLoss()
    xr, yr, xf, yf = batches(CFG, 16)
    out = {}
    for dt in ("fp32", dtype):
        m = build("CosFace", dtype=dt)
        meters = gs_lora_step(m, create_optimizer(args, m), crit, xr, yr, xf, yf, **HY)
        g_lora = m.lora_bucket().grad.detach().double().clone()
        p = build("CosFace", dtype=dt, train="head")
        pm = head_probe_step(p, create_optimizer(args, p), crit, torch.cat((xr, xf)), torch.cat((yr, yf)))
        out[dt] = (g_lora, p.loss.weight.grad.detach().double().flatten().clone(), meters.cpu(), pm.cpu())
    for k, what in ((0, "LoRA gradient"), (1, "head gradient")):
        ref, got = out["fp32"][k], out[dtype][k]
        rel = ((got - ref).norm() / ref.norm()).item()
        cos = (torch.dot(got, ref) / (got.norm() * ref.norm())).item()
        print(f"{dtype} {what}: rel {rel:.5f}, cosine {cos:.6f}")
        assert rel <= 0.06 and cos > 0.995
    assert torch.isfinite(out[dtype][2]).all() and torch.isfinite(out[dtype][3]).all()
    assert (out[dtype][2][:4] - out["fp32"][2][:4]).abs().max() <= 0.25 and abs(out[dtype][3][0] - out["fp32"][3][0]) <= 0.25


def test_graph_replay_of_the_step_is_bit_identical_to_eager():
    """torch.cuda.graph capture of the whole step at 1100 classes: no allocation or sync crept into the tiled path."""
    from gslora_hip.optim import FusedAdamW
    from gslora_hip.step import GraphedStep, gs_lora_step
    m1 = build("ArcFace", "fp16", dropout=0.1)
    m2 = copy.deepcopy(m1)
    mk_opt = lambda m: FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-2, weight_decay=0.05, eps=1e-8)
    o1, o2 = mk_opt(m1), mk_opt(m2)
    crit = torch.nn.CrossEntropyLoss()
    g = GraphedStep(m2, o2, crit)
    for s in range(3):
        xr, yr, xf, yf = batches(CFG, 6, s)
        p1 = gs_lora_step(m1, o1, crit, xr, yr, xf, yf, **HY)
        p2 = g(xr, yr, xf, yf, **HY)
        assert torch.equal(p1, p2) and torch.isfinite(p1).all(), (s, p1.tolist(), p2.tolist())
        for (n, a), (_, c) in zip(m1.named_parameters(), m2.named_parameters()):
            if a.requires_grad:
                assert torch.equal(a, c), (s, n)
    assert (g.eager_steps, g.captures, g.replays) == (1, 1, 2)


def test_evaluation_agrees_with_torch_max_on_the_logits():
    import engine_cl
    m = build("CosFace")
    xr, yr, xf, yf = batches(CFG, 37)
    # an untrained model gets nothing right: make the class row of one image its own embedding (cosine 1 beats the margin; one image
    # only, because the embeddings of an untrained model are nearly parallel and a second such row would beat the first)
    m.eval()
    with torch.no_grad():
        m.loss.weight[yr[0]] = m(xr)[0]
    loader = [(xr.cpu(), yr.cpu()), (xf.cpu(), yf.cpu())]
    hits, total, ccount, chit = 0, 0, torch.zeros(1100, dtype=torch.int64), torch.zeros(1100, dtype=torch.int64)
    with torch.no_grad():
        for x, y in loader:
            logits = m(x.cuda(), y.cuda())[0]
            assert logits.shape == (x.shape[0], 1100)
            ok = (torch.max(logits, 1)[1].cpu() == y)
            hits, total = hits + int(ok.sum()), total + y.numel()
            ccount += torch.bincount(y, minlength=1100)
            chit += torch.bincount(y[ok], minlength=1100)
    assert 0 < hits < total
    acc = engine_cl.eval_data(m, loader, torch.device("cuda"), "large-C")
    assert acc == 100 * hits / total
    res = engine_cl.eval_data_per_class(m, loader, torch.device("cuda"), "large-C", num_classes=1100)
    assert res["accuracy"] == acc and torch.equal(res["class_total"].cpu(), ccount) and torch.equal(res["class_correct"].cpu(), chit)
