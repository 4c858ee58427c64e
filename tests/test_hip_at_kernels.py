"""The kernels of libgslora_at.so alone (csrc/at.hip): gsa_at_fwd and gsa_at_bwd through gslora_hip._lib_at / gslora_hip.at, every output
between guard bands (tests/guard_bands.py).

The reference is a float64 restatement of the reference's at / at_loss (baselines/LIRFtrain.py:42-55) written here, on the inputs as the
element type holds them; the table G and the boundary gradient come from autograd on it (G = d loss / d q * 2 / T with q the token mean of
squares; the gradient of the stream is d loss / d xs).

Bars:
  value      |got - want| <= 1e-4 * max(1, |want|), and — the loss is far below 1, so that bar alone says little — the bound that follows from
             the f32 sums: every at entry carries a relative error of at most k E, E = 2^-24, k = T + 40 (T sequential adds at worst, the
             division by T, the norm's D-term sum over 4 per thread + 6 butterfly levels + 4 waves, root, quotient), so
             |loss - want| <= 2 k E * sum((|at_s| + |at_t|) * |at_s - at_t|) / (B D) + E |want|, evaluated in float64 by the test.
  G, f32 increments of dmid     within 1e-4 of the reference tensor's largest element.
  16-bit dmid  got = rn16(fl32(old + inc32)): against the float64 value old + inc the error is the increment's (the f32 bar above), the f32
             add's (E |want|) and the store's (u |want|, u = 2^-11 for fp16 and 2^-8 for bf16, half an ulp; fp16 below its normal range:
             2^-25 absolute), summed: u |want| * (1 + 2^-10) + 2^-25 + 1e-4 * max|inc| + E |want|.
No tolerance is tuned to the output.

The threshold branch. The gradient that arrives at a student entry the threshold zeroed is exactly zero at the threshold's stage (asserted
on the reference); through F.normalize the entry still receives -raw * <g, raw> / n, the gradient through the norm it contributes to, and
autograd on the reference gives exactly that. G of those entries is therefore tiny but not zero, and the test holds it to the rounding
bound of that one term, 3 k E * (raw / n) * (2 / T) * sum|g raw| + 3 k E |G| (the dot product's terms, the entry and the quotient), which
the test first shows to be a thousand times below the 1e-4 bar of the whole table: a threshold the backward ignored misses it by orders
of magnitude."""
import pytest
import torch

from guard_bands import NAN_SENTINEL, Banded

pytestmark = pytest.mark.gpu

F32, F16, BF16, F64 = torch.float32, torch.float16, torch.bfloat16, torch.float64
E = 2.0 ** -24
SHAPES = ((1, 26, 64), (3, 37, 128), (5, 26, 576), (2, 197, 512), (1, 1025, 1024))
DTYPES = (F32, F16, BF16)
# (stream, gradient stream): fp32 modes; fp16 mode; bf16 mode with its fp16 or bf16 forward stream; a 16-bit stream under f32 gradients
PAIRS = ((F32, F32), (F16, F16), (F16, BF16), (BF16, BF16), (F16, F32), (BF16, F32))
U16 = {F16: 2.0 ** -11, BF16: 2.0 ** -8}
SENT = NAN_SENTINEL[F32]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    from gslora_hip import _lib_at
    _lib_at.load()
    return _lib_at


def streams(B, T, D, dtype, seed, extra_rows=0, pad=0, spread=0.5):
    """(xs, xt): the student's stream [(B * T + extra_rows), D] as a column block of rows D + pad long, the teacher's [B * T, D]; values
    with a per-channel scale in [1 - spread, 1 + spread] so that the at entries differ."""
    g = torch.Generator().manual_seed(seed)
    ch = 1 - spread + 2 * spread * torch.rand(D, generator=g)
    xs = (torch.randn(B * T + extra_rows, D, generator=g) * ch).to(dtype)
    xt = (torch.randn(B * T, D, generator=g) * (1 - spread + 2 * spread * torch.rand(D, generator=g))).to(dtype)
    full = torch.full((B * T + extra_rows, D + pad), float("nan"), dtype=dtype)
    full[:, :D] = xs
    return full.cuda()[:, :D], xt.cuda()


def at64(x):
    """at(x) of the reference in float64 on a [B, T, D] tensor; returns (at, at before the threshold, q)."""
    q = x.pow(2).mean(1)
    raw = torch.nn.functional.normalize(q.view(x.size(0), -1))
    if q.requires_grad:
        q.retain_grad()
        raw.retain_grad()
    a = torch.where(raw < 0.005, torch.zeros_like(raw), raw)
    return a, raw, q


def reference(xs, xt, B, T):
    """-> dict: loss, at_s, at_t, their values raw_s, raw_t before the threshold, G [B, D], dx [B * T, D] (d loss / d xs), g_raw (d loss /
    d raw_s) and n_s (the norms [B, 1] of the student's q), all float64 on the device."""
    D = xs.shape[1]
    x = xs[:B * T].to(F64).reshape(B, T, D).clone().requires_grad_(True)
    a_s, raw_s, q = at64(x)
    with torch.no_grad():
        a_t, raw_t, _ = at64(xt.to(F64).reshape(B, T, D))
    loss = (a_s - a_t).pow(2).mean()
    loss.backward()
    return dict(loss=loss.detach(), at_s=a_s.detach(), at_t=a_t, raw_s=raw_s.detach(), raw_t=raw_t, G=q.grad * (2.0 / T),
                dx=x.grad.reshape(B * T, D), g_raw=raw_s.grad, n_s=q.detach().norm(dim=1, keepdim=True))


def value_bound(ref, T):
    k = T + 40
    a_s, a_t = ref["at_s"], ref["at_t"]
    return float(2 * k * E * ((a_s.abs() + a_t.abs()) * (a_s - a_t).abs()).sum() / a_s.numel() + E * ref["loss"].abs())


def run_fwd(lib, xs, xt, B, T, tables=True):
    """gsa_at_fwd with every output between bands -> (loss, G, at_s, at_t, bands)."""
    D = xs.shape[1]
    loss = Banded((1,), F32, sentinel=SENT)
    G = Banded((B, D), F32, sentinel=SENT)
    a_s = Banded((B, D), F32, sentinel=SENT) if tables else None
    a_t = Banded((B, D), F32, sentinel=SENT) if tables else None
    ws = Banded((lib.at_ws_elems(B, T, D),), F32, sentinel=SENT)
    lib.at_fwd(xs, xt, B, T, loss.view, G.view, ws.view, None if a_s is None else a_s.view, None if a_t is None else a_t.view)
    torch.cuda.synchronize()
    bands = [b for b in (loss, G, a_s, a_t, ws) if b is not None]
    for b in bands[:-1]:
        assert b.bands_intact() and b.unwritten() == 0
    assert ws.bands_intact()
    return loss.view[0].clone(), G.view.clone(), None if a_s is None else a_s.view.clone(), None if a_t is None else a_t.view.clone()


def check_fwd(ref, loss, G, a_s, a_t, T):
    want = float(ref["loss"])
    err = abs(float(loss) - want)
    print(f"loss {float(loss):.9e} want {want:.9e} err {err:.2e} bound {value_bound(ref, T):.2e}")
    assert err <= 1e-4 * max(1.0, abs(want))
    assert err <= value_bound(ref, T)
    gmax = float(ref["G"].abs().max())
    gerr = float((G.to(F64) - ref["G"]).abs().max())
    print(f"G max {gmax:.3e} err {gerr:.2e}")
    assert torch.isfinite(G).all() and gerr <= 1e-4 * gmax
    if a_s is not None:
        k = (T + 40) * E
        for got, w in ((a_s, ref["at_s"]), (a_t, ref["at_t"])):
            assert bool(((got == 0) == (w == 0)).all()), "the same entries are under the threshold"
            assert float((got.to(F64) - w).abs().max()) <= k * float(w.abs().max())


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_value_tables_and_G_against_float64(lib, shape, dtype):
    B, T, D = shape
    xs, xt = streams(B, T, D, dtype, seed=B * 1000 + T, extra_rows=2 * T, pad=8)
    assert xs.stride(0) == D + 8
    ref = reference(xs, xt, B, T)
    for raw in (ref["raw_s"], ref["raw_t"]):
        assert float(((raw - 0.005).abs() / 0.005).min()) > 1e-3, "no entry sits on the threshold"
    loss, G, a_s, a_t = run_fwd(lib, xs, xt, B, T)
    check_fwd(ref, loss, G, a_s, a_t, T)
    loss2, G2, _, _ = run_fwd(lib, xs, xt, B, T, tables=False)
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)) and torch.equal(G.view(torch.int32), G2.view(torch.int32)), "two calls, same bits"


@pytest.mark.parametrize("shape", ((3, 37, 128), (2, 26, 576)), ids=lambda s: "x".join(map(str, s)))
def test_the_threshold_branch_on_crafted_columns(lib, shape):
    B, T, D = shape
    xs, xt = streams(B, T, D, F32, seed=7, spread=0.1)      # (unscaled entries stay well above the threshold: about 1 / sqrt(D))
    xs, xt = xs.contiguous(), xt.clone()
    cs = torch.arange(D) < int(0.3 * D)                                     # the student's scaled channels
    ct = (torch.arange(D) >= int(0.2 * D)) & (torch.arange(D) < int(0.45 * D))      # the teacher's: overlap and difference on both sides
    xs[:, cs.cuda()] *= 1e-2
    xt[:, ct.cuda()] *= 1e-2
    ref = reference(xs, xt, B, T)
    for a in (ref["at_s"], ref["at_t"]):
        frac = float((a == 0).double().mean())
        assert 0.10 <= frac <= 0.50, frac
    for raw in (ref["raw_s"], ref["raw_t"]):
        assert float(((raw - 0.005).abs() / 0.005).min()) > 1e-3
    ms, mt = ref["at_s"] == 0, ref["at_t"] == 0
    assert bool((ms & ~mt).any()) and bool((~ms & mt).any())
    loss, G, a_s, a_t = run_fwd(lib, xs, xt, B, T)
    check_fwd(ref, loss, G, a_s, a_t, T)
    assert bool((a_s[ms] == 0).all()) and bool((a_t[mt] == 0).all())
    # the masked student entries: only the path through the norm is left (module docstring)
    assert bool((ref["g_raw"][ms] == 0).all()), "the reference: no gradient arrives at a zeroed entry"
    k = (T + 40) * E
    absdot = (ref["g_raw"] * ref["raw_s"]).abs().sum(1, keepdim=True)
    bound = (3 * k * (ref["raw_s"] / ref["n_s"]) * (2.0 / T) * absdot + 3 * k * ref["G"].abs())[ms]
    want = ref["G"][ms]
    err = (G[ms].to(F64) - want).abs()
    print(f"masked entries: max |G| {float(want.abs().max()):.3e} of {float(ref['G'].abs().max()):.3e} overall, max err {float(err.max()):.2e}, "
          f"max bound {float(bound.max()):.2e}")
    assert float(bound.max()) < 1e-3 * 1e-4 * float(ref["G"].abs().max()), "a bar a thousand times below the whole table's"
    assert bool((err <= bound).all())


def test_an_all_zero_image_and_equal_streams(lib):
    B, T, D = 3, 26, 128
    xs, xt = streams(B, T, D, F32, seed=11)
    xs = xs.contiguous()
    xs[T:2 * T] = 0                    # the student's second image
    xt[2 * T:] = 0                     # the teacher's third
    ref = reference(xs, xt, B, T)
    loss, G, a_s, a_t = run_fwd(lib, xs, xt, B, T)
    assert torch.isfinite(loss) and torch.isfinite(G).all() and torch.isfinite(a_s).all() and torch.isfinite(a_t).all()
    assert bool((a_s[1] == 0).all()) and bool((G[1] == 0).all()) and bool((a_t[2] == 0).all())
    check_fwd(ref, loss, G, a_s, a_t, T)
    for dtype in DTYPES:
        x, _ = streams(B, T, D, dtype, seed=12, extra_rows=T, pad=8)
        loss, G, a_s, a_t = run_fwd(lib, x, x[:B * T].contiguous(), B, T)
        assert float(loss) == 0.0 and bool((G == 0).all()) and torch.equal(a_s, a_t)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "-".join(str(d).replace("torch.", "") for d in p))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backward_accumulates_the_scaled_gradient_on_the_forget_rows_only(lib, shape, pair):
    from gslora_hip import at as AT
    B, T, D = shape
    xdt, ddt = pair
    extra = 2 * T
    xs, xt = streams(B, T, D, xdt, seed=B + T, extra_rows=extra, pad=8)
    ref = reference(xs, xt, B, T)
    loss, G = AT.at_loss_value_and_table(xs, B, T, xt)
    assert abs(float(loss) - float(ref["loss"])) <= value_bound(ref, T)
    coef = torch.tensor([-300.0 * 0.37], device="cuda")
    S = torch.tensor([256.0 if ddt == F16 else 0.5], device="cuda")
    g = torch.Generator().manual_seed(3)
    inc = ref["dx"] * float(coef) * float(S)
    old = (torch.randn(B * T + extra, D, generator=g) * float(inc.abs().max())).to(ddt)
    dm = Banded((B * T + extra, D), ddt, old, ld=D + 16)
    before = dm.view.clone()
    AT.at_inject(dm.view, xs, G, coef, S, T=T)
    torch.cuda.synchronize()
    assert dm.outside_intact(), "pad columns and bands"
    assert torch.equal(dm.view[B * T:].view(torch.int16 if ddt != F32 else torch.int32),
                       before[B * T:].view(torch.int16 if ddt != F32 else torch.int32)), "rows behind the forget images are untouched"
    want = before[:B * T].to(F64) + inc
    got = dm.view[:B * T].to(F64)
    imax = float(inc.abs().max())
    err = (got - want).abs()
    if ddt == F32:
        bound = 1e-4 * imax + E * want.abs()
    else:
        bound = U16[ddt] * want.abs() * (1 + 2.0 ** -10) + 2.0 ** -25 + 1e-4 * imax + E * want.abs()
    print(f"max |inc| {imax:.3e}, max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    # the increment alone (f32 gradient stream): 1e-4 of its largest element
    if ddt == F32:
        assert float((dm.view[:B * T].to(F64) - before[:B * T].to(F64) - inc).abs().max()) <= 1e-4 * imax + 2 * E * float(want.abs().max())
    # a second call on the same start gives the same bits
    dm2 = Banded((B * T + extra, D), ddt, old, ld=D + 16)
    AT.at_inject(dm2.view, xs, G, coef, S, T=T)
    assert torch.equal(dm.view.view(torch.int16 if ddt != F32 else torch.int32), dm2.view.view(torch.int16 if ddt != F32 else torch.int32))


def test_reference_named_wrappers_and_three_dimensional_views(lib):
    from gslora_hip import at as AT
    B, T, D = 3, 37, 128
    xs, xt = streams(B, T, D, F32, seed=5)
    x3, y3 = xs.contiguous().reshape(B, T, D), xt.reshape(B, T, D)
    ref = reference(xs, xt, B, T)
    assert abs(float(AT.at_loss(x3, y3)) - float(ref["loss"])) <= value_bound(ref, T)
    a = AT.at(x3)
    assert a.shape == (B, D) and float((a.to(F64) - ref["at_s"]).abs().max()) <= (T + 40) * E * float(ref["at_s"].abs().max())
    assert not AT.at_loss(x3.requires_grad_(True), y3).requires_grad, "the wrappers are values, not autograd nodes"
    dm = torch.zeros(B, T, D, device="cuda")
    loss, G = AT.at_loss_value_and_table(x3.detach(), B, T, y3)
    AT.at_inject(dm, x3.detach(), G, torch.ones(1, device="cuda"), None)
    assert float((dm.reshape(B * T, D).to(F64) - ref["dx"]).abs().max()) <= 1e-4 * float(ref["dx"].abs().max())


def test_refusals_name_the_argument(lib):
    from gslora_hip import at as AT
    x = torch.zeros(2, 26, 128, device="cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        AT.at_loss(x.cpu(), x.cpu())
    with pytest.raises(ValueError, match="multiple of 64"):
        AT.at_loss(torch.zeros(2, 26, 96, device="cuda"), torch.zeros(2, 26, 96, device="cuda"))
    with pytest.raises(ValueError, match="does not match"):
        AT.at_loss_value_and_table(x, 2, 26, torch.zeros(2, 25, 128, device="cuda"))
    with pytest.raises(ValueError, match="the teacher's torch.float16"):
        AT.at_loss(x, x.half())
    with pytest.raises(RuntimeError, match="16-byte aligned rows"):
        lib.at_fwd(x.reshape(52, 128).view(-1)[1:1 + 51 * 128].view(51, 128)[:26], x.reshape(52, 128)[:26], 1, 26, x, x, x)
