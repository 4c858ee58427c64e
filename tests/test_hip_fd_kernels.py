"""The kernels of libgslora_fd.so alone (csrc/fd.hip): gsf_rowdist_fwd / gsf_rowdist_bwd on both kernels of gsf_rowdist_plan, both modes,
every tensor between NaN bands (tests/guard_bands.py), and the autograd node gslora_hip.fd.row_dist.

References are float64 restatements of the definitions of include/gslora_fd.h on the same f32 inputs. The difference fl(a - t) is the
correctly rounded f32 one, as in the kernels — IEEE subtraction has one result — and everything behind it is float64. Bounds are worst-case
linear counts of the roundings on the kernels' longest path, in units of E = 2^-24 relative to the (non-negative) sums:

  S_b        one rounding per square, then the adds: a thread sums n_t = 4 * ceil(ceil(W / 4) / STRIDE) elements in order (STRIDE 64 lanes or
             256 threads), 6 butterfly levels, and in the workgroup kernel 4 more adds of the wave sums: k_S = n_t + 12 covers 1 + (n_t - 1)
             + 6 + 4 with two to spare for the second-order terms (k_S E < 3e-5 at the widest row here).
  batch sum  256 threads stride the rows (ceil(B / 256) adds), 6 levels, 4 wave sums: k_R = ceil(B / 256) + 10.
  GSF_SQ     out = n * n, n = sqrtf(sum_b S_b): the sum (k_S + k_R) E, the root halves that and adds at most one ulp (2 E), the square
             doubles it and rounds once: (k_S + k_R + 5) E |out|.
  GSF_ROWNORM out = (sum_b sqrtf(S_b)) / B: the roots (k_S / 2 + 2) E, the sum k_R E, the division E: (k_S / 2 + k_R + 3) E |out|.
  d, GSF_SQ  fl(a - t) * (2 * (g * coef)): the product g * coef, the doubling (exact), the product: 2 E |d|; 3 E is asserted.
  d, GSF_ROWNORM  fl(a - t) * (((g * coef) / B) / sqrtf(S_b)): g * coef, / B, the root of S_b ((k_S / 2 + 2) E), the quotient, the product:
             (k_S / 2 + 6) E |d|.
  accumulate + E |old + d|, and the stored bits are exactly fl(old + value) of the plain call's value.
No tolerance is tuned to the output."""
import functools
import math

import numpy as np
import pytest
import torch

from guard_bands import NAN_SENTINEL, Banded

pytestmark = pytest.mark.gpu

F32 = torch.float32
NF = np.float32
E = 2.0 ** -24
ROWS = (1, 3, 4, 5, 9)
WIDTHS = (1, 2, 63, 64, 65, 1000, 1024, 1025, "thr-1", "thr", "thr+1")
SQ, ROWNORM = 0, 1
SENT = NAN_SENTINEL[F32]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    from gslora_hip import _lib_fd
    _lib_fd.load()
    return _lib_fd


@functools.lru_cache(None)
def threshold():
    from gslora_hip import _lib_fd as LF
    lo, hi = 1, 1 << 20
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if LF.rowdist_plan(4, mid)[0] == LF.FD_WAVE else (lo, mid)
    return hi


def width(W):
    return W if isinstance(W, int) else threshold() + {"thr-1": -1, "thr": 0, "thr+1": 1}[W]


def stream():
    return torch.cuda.current_stream().cuda_stream


class Placed:
    """A [B, W] block at column `off` of rows `ld` floats long, inside a banded buffer: the pad columns in front of and behind the block
    belong to the bands (NaN for an input, the sentinel for an output). off = 1..3 takes the block's rows off their 16-byte alignment."""

    def __init__(self, B, W, ld, off, src=None):
        assert off + W <= ld
        self.B, self.W, self.ld, self.off = B, W, ld, off
        if src is None:
            self.b = Banded((B, ld), F32, sentinel=SENT)
        else:
            full = np.full((B, ld), np.nan, dtype=NF)
            full[:, off:off + W] = src
            self.b = Banded((B, ld), F32, torch.from_numpy(full))
            self.before = self.bits().copy()

    @property
    def ptr(self):
        return self.b.view.data_ptr() + 4 * self.off

    def bits(self):
        return self.b.view.view(torch.int32).cpu().numpy()

    def block(self):
        return self.b.view[:, self.off:self.off + self.W].cpu().numpy().copy()

    def pads(self, bits):
        return np.delete(bits, np.arange(self.off, self.off + self.W), axis=1)

    def input_intact(self):
        return self.b.bands_intact()

    def output_ok(self):
        """Bands and pad columns untouched, every element of the block written."""
        bits = self.bits()
        return self.b.bands_intact() and (self.pads(bits) == SENT).all() and not (bits[:, self.off:self.off + self.W] == SENT).any()

    def accumulated_ok(self):
        return self.b.outside_intact() and np.array_equal(self.pads(self.bits()), self.pads(self.before))


def run(lib, a, t, mode, coef=1.0, g=1.0, old=None, pads=(0, 0, 0), offs=(0, 0, 0), backward=True):
    """Both entry points, banded. pads: extra elements of the row strides of a, t and d; offs: column offsets of the three blocks.
    -> (out, d or None, ws)"""
    B, W = a.shape
    ld = [W + p + o for p, o in zip(pads, offs)]
    A, T_ = Placed(B, W, ld[0], offs[0], a), Placed(B, W, ld[1], offs[1], t)
    out, ws = Banded((1,), F32, sentinel=SENT), Banded((lib.rowdist_ws_elems(B, W),), F32, sentinel=SENT)
    G = Banded((1,), F32, torch.tensor([g], dtype=F32))
    L = lib.load()
    lib.check(L.gsf_rowdist_fwd(A.ptr, ld[0], T_.ptr, ld[1], B, W, mode, out.view.data_ptr(), ws.view.data_ptr(), stream()), "gsf_rowdist_fwd")
    D = None
    if backward:
        D = Placed(B, W, ld[2], offs[2], old)
        lib.check(L.gsf_rowdist_bwd(A.ptr, ld[0], T_.ptr, ld[1], ws.view.data_ptr(), G.view.data_ptr(), B, W, mode, coef, D.ptr, ld[2],
                                    0 if old is None else 1, stream()), "gsf_rowdist_bwd")
    torch.cuda.synchronize()
    assert A.input_intact() and T_.input_intact() and G.bands_intact()
    assert out.bands_intact() and out.unwritten() == 0 and ws.bands_intact() and ws.unwritten() == 0
    if D is not None:
        assert D.output_ok() if old is None else D.accumulated_ok()
    return float(out.view.cpu().numpy()[0]), None if D is None else D.block(), ws.view.cpu().numpy().copy()


# ---------------------------------------------------------------------------------------------------------------- reference and bounds
def k_rows(W):
    stride = 64 if W < threshold() else 256
    return 4 * math.ceil(math.ceil(W / 4) / stride) + 12


def reference(a, t, mode, coef=1.0, g=1.0):
    """float64 on the f32 inputs. -> dict(out, b_out, S [B], b_S [B], d [B, W], b_d [B, W])"""
    B, W = a.shape
    with np.errstate(invalid="ignore"):
        diff = (a - t).astype(np.float64)      # a - t in f32 first: the kernels' difference
        S = (diff * diff).sum(1)
        kS, kR = k_rows(W), math.ceil(B / 256) + 10
        gc = float(NF(g)) * float(NF(coef))
        if mode == SQ:
            out = S.sum()
            b_out = (kS + kR + 5) * E * abs(out)
            d = diff * (2.0 * gc)
            b_d = 3 * E * np.abs(d)
        else:
            root = np.sqrt(S)
            out = root.sum() / B
            b_out = (kS / 2 + kR + 3) * E * abs(out)
            d = np.where(S[:, None] == 0, 0.0, diff * (gc / B) / np.where(root == 0, 1.0, root)[:, None])
            b_d = (kS / 2 + 6) * E * np.abs(d)
    return dict(out=out, b_out=b_out, S=S, b_S=kS * E * S, d=d, b_d=b_d)


def under(what, got, ref, bound):
    got, ref, bound = (np.asarray(v, dtype=np.float64) for v in (got, ref, bound))
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref)), what
    ok = ~np.isnan(ref)
    err = np.abs(got - ref)[ok]
    ratio = float((err / np.maximum(bound[ok], 1e-300)).max()) if err.size and err.max() > 0 else 0.0
    print(f"RATIO {what} {ratio:.3f}")
    assert (err <= bound[ok]).all(), (what, ratio)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def rows(B, W, seed, spread=3.0):
    g = np.random.default_rng(seed)
    return (g.standard_normal((B, W)) * spread).astype(NF), (g.standard_normal((B, W)) * spread).astype(NF)


# ---------------------------------------------------------------------------------------------------------------- against float64
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("B", ROWS)
def test_rowdist_against_float64(lib, B, W):
    """Aligned rows (the 16-byte path), odd padded strides (rows lose their alignment: the 4-byte path) and base pointers 1 to 3 floats off;
    the three placements give the same bits (the element ownership does not depend on the load width)."""
    W = width(W)
    a, t = rows(B, W, 1000 * B + W)
    old = np.random.default_rng(7).standard_normal((B, W)).astype(NF)
    for mode in (SQ, ROWNORM):
        coef, g = (0.1, 1.0) if mode == SQ else (0.37, 0.5)
        r = reference(a, t, mode, coef, g)
        first = None
        for pads, offs in (((0, 4, 8), (0, 0, 0)), ((3, 5, 7), (0, 0, 0)), ((0, 0, 0), (1, 2, 3)), ((4, 0, 1), (0, 3, 0))):
            tag = f"B{B} W{W} mode{mode} pads{pads} offs{offs}"
            out, d, ws = run(lib, a, t, mode, coef, g, pads=pads, offs=offs)
            under(f"out {tag}", out, r["out"], r["b_out"])
            under(f"S {tag}", ws, r["S"], r["b_S"])
            under(f"d {tag}", d, r["d"], r["b_d"])
            if first is None:
                first = (out, d, ws)
            assert out == first[0] and same_bits(d, first[1]) and same_bits(ws, first[2]), "the placement does not change a bit"
            out_a, d_a, _ = run(lib, a, t, mode, coef, g, old=old, pads=pads, offs=offs)
            assert out_a == out
            under(f"accumulate {tag}", d_a, old.astype(np.float64) + r["d"], r["b_d"] + E * np.abs(old + r["d"]))
            assert same_bits(d_a, old + d), "accumulate is fl(old + value), the value formed first"
        # the reference's expressions, evaluated by torch on the CPU in f32
        x, y = torch.from_numpy(a), torch.from_numpy(t)
        want = float(torch.norm(x - y, p=2) ** 2) if mode == SQ else float(torch.norm(x - y, 2, 1).mean())
        assert abs(first[0] - want) <= r["b_out"] + abs(want - r["out"])


@pytest.mark.parametrize("mode", [SQ, ROWNORM])
def test_decomposition(lib, mode):
    """The same rows through both kernels: width thr - 1 (a wave per row) and the same rows with one more column in which a == t (a workgroup
    per row; the column adds an exact +0): each is within the bound of the one float64 value, so they agree within twice the bound."""
    thr = threshold()
    a, t = rows(5, thr - 1, 99)
    a2, t2 = np.concatenate([a, np.ones((5, 1), NF)], 1), np.concatenate([t, np.ones((5, 1), NF)], 1)
    assert lib.rowdist_plan(5, thr - 1)[0] == lib.FD_WAVE and lib.rowdist_plan(5, thr)[0] == lib.FD_BLOCK
    r = reference(a, t, mode, 0.3, 1.0)
    o1, d1, s1 = run(lib, a, t, mode, 0.3)
    o2, d2, s2 = run(lib, a2, t2, mode, 0.3)
    assert abs(o1 - o2) <= 2 * r["b_out"]
    assert (np.abs(s1.astype(np.float64) - s2) <= 2 * r["b_S"]).all()
    assert (np.abs(d1.astype(np.float64) - d2[:, :-1]) <= 2 * r["b_d"]).all() and not d2[:, -1].any()


@pytest.mark.parametrize("W", [65, "thr+1"])
def test_exact_cases(lib, W):
    W = width(W)
    a, t = rows(5, W, 3)
    for mode in (SQ, ROWNORM):      # a == t: value 0, an all-zero gradient
        out, d, ws = run(lib, a, a.copy(), mode, 0.5)
        assert out == 0.0 and not d.any() and not ws.any() and not np.isnan(d).any()
    t0 = t.copy()
    t0[2] = a[2]      # one zero row among non-zero rows
    r = reference(a, t0, ROWNORM, 0.5)
    out, d, ws = run(lib, a, t0, ROWNORM, 0.5)
    assert ws[2] == 0.0 and not d[2].any() and d[[0, 1, 3, 4]].all()
    under("zero row: out", out, r["out"], r["b_out"])
    under("zero row: d", d, r["d"], r["b_d"])
    old = np.full((5, W), 2.5, NF)
    _, d_a, _ = run(lib, a, t0, ROWNORM, 0.5, old=old)
    assert (d_a[2] == 2.5).all()
    # integer-valued inputs: every square and every partial sum is an integer below 2^24, so S_b is exact whatever the order
    g = np.random.default_rng(5)
    ai, ti = g.integers(-8, 9, (5, W)).astype(NF), g.integers(-8, 9, (5, W)).astype(NF)
    want = ((ai.astype(np.int64) - ti.astype(np.int64)) ** 2).sum(1)
    assert want.max() < 2 ** 24
    out, d, ws = run(lib, ai, ti, SQ, 0.5)
    assert np.array_equal(ws.astype(np.int64), want)
    assert np.array_equal(d, (ai - ti) * NF(1.0)), "2 * (1 * 0.5) = 1: the gradient is the difference, exactly"
    n = np.sqrt(NF(want.sum()))
    assert out == float(n * n), "n = sqrtf(sum), n * n — not the sum"


@pytest.mark.parametrize("W", [65, "thr"])
def test_nan_and_determinism(lib, W):
    W = width(W)
    a, t = rows(5, W, 11)
    a[3, W // 2] = np.nan
    for mode in (SQ, ROWNORM):
        out, d, ws = run(lib, a, t, mode, 0.5)
        assert np.isnan(out) and np.isnan(ws[3]) and not np.isnan(ws[[0, 1, 2, 4]]).any()
        assert not np.isnan(d[[0, 1, 2, 4]]).any(), "no other row is touched"
        if mode == ROWNORM:
            assert np.isnan(d[3]).all(), "the row's norm is NaN: so is its whole gradient"
        else:
            assert np.isnan(d[3, W // 2]) and np.isnan(d[3]).sum() == 1
        out2, d2, ws2 = run(lib, a, t, mode, 0.5)
        assert same_bits(np.array([out]), np.array([out2])) and same_bits(d, d2) and same_bits(ws, ws2), "two calls, the same bits"


@pytest.mark.parametrize("mode", ["sq", "rownorm"])
@pytest.mark.parametrize("W", [64, "thr+1"])
def test_autograd_node_over_a_row_range(lib, mode, W):
    from gslora_hip import fd
    W = width(W)
    a, t = rows(7, W, 21)
    full = torch.from_numpy(a).cuda().requires_grad_(True)
    teacher = torch.from_numpy(t[2:5]).cuda().requires_grad_(True)
    coef = 0.25
    dist, part = fd.row_dist(full, 2, 3, teacher, mode, coef)
    assert not dist.requires_grad and part.requires_grad and dist.dim() == 0 and part.dim() == 0
    (1.5 * part).backward()
    assert teacher.grad is None, "the teacher receives no gradient"
    got = full.grad.cpu().numpy()
    assert not got[:2].any() and not got[5:].any(), "rows outside the range come back exactly zero"
    m = SQ if mode == "sq" else ROWNORM
    r = reference(a[2:5], t[2:5], m, coef, 1.5)
    under(f"node value {mode}", dist.item(), r["out"], r["b_out"])
    assert abs(part.item() - coef * r["out"]) <= coef * r["b_out"] + 2 * E * abs(coef * r["out"])
    under(f"node gradient {mode}", got[2:5], r["d"], r["b_d"])
    x = torch.from_numpy(a).cuda().requires_grad_(True)
    y = torch.from_numpy(t[2:5]).cuda()
    want = torch.norm(x[2:5] - y, p=2) ** 2 if mode == "sq" else torch.norm(x[2:5] - y, 2, 1).mean()
    (1.5 * (coef * want)).backward()
    tg = x.grad.cpu().numpy().astype(np.float64)
    assert (np.abs(got[2:5] - tg[2:5]) <= r["b_d"] + np.abs(tg[2:5] - r["d"])).all(), "torch autograd on the same expression"
    with pytest.raises(ValueError, match="are not a non-empty range"):
        fd.row_dist(full, 5, 3, teacher, mode, coef)
    with pytest.raises(ValueError, match="does not match rows"):
        fd.row_dist(full, 0, 2, teacher, mode, coef)
    with pytest.raises(ValueError, match="mode must be one of"):
        fd.row_dist(full, 2, 3, teacher, "l1", coef)
    with pytest.raises(RuntimeError, match="no CPU\\s+fallback"):
        fd.row_dist(full.detach().cpu(), 2, 3, teacher, mode, coef)
