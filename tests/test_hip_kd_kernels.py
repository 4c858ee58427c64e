"""The kernels of libgslora_kd.so alone (csrc/kd.hip): gsk_kd_ce_fwd / gsk_kd_ce_bwd on both kernels of gsk_kd_plan and
gsk_param_dist_fwd / gsk_param_dist_bwd, every tensor between NaN bands (tests/guard_bands.py).

References are float64 restatements of the definitions of include/gslora_kd.h on the same f32 inputs (a = ys / T and t = yt / T are the
correctly rounded f32 quotients, as in the kernels, everything behind them is float64). Bounds are worst-case linear counts of the
roundings on the kernels' longest path, with E = 2^-24 and the expf / logf accuracy U_EXP / U_LOG of oracle/loss_probes.py, whose row
bounds are reused where the kernels share the row walk of loss.hip:

  lse(a), lse(t), lse(ys)   loss_probes.bound_lse (lane-strided sums of NPL = ceil(C / 64) elements and 6 butterfly levels; the
                            workgroup-per-row kernel sums ceil(C / 256) elements per thread, 6 levels and a 4-wave combine: fewer
                            roundings for every C it serves, C > 1024 — the same bound holds)
  KD_b                      loss_probes.bound_kl of the rows (a_b, t_b): the term exp(l) (l - q) on the shifted logs, as proto_row
  CE_b                      loss_probes.bound_loss
  batch sums                loss_probes.bound_sum (256 threads stride the rows, 6 levels, 4-wave combine)
  out[0]                    bound_sum * T^2 / B + 3 E |out[0]|: fl(T T), the product, the division
  out[1]                    bound_sum / B + E |out[1]|
  out[2]                    |c_kd| b0 + |c_ce| b1 + E (|c_kd out0| + |c_ce out1|) + E |out2|
  d                         |k1| (bp_a + bp_t) + 5 E |k1 dp|: the two exponentials under the stored log-sum-exps' bounds (_bound_p), T / B,
                            c_kd ., g ., the subtraction, the product;  + |k2| bp_s + 4 E |k2 dq|: c_ce / B, g ., the subtraction, the
                            product;  + E |d| for the add of the two parts, + E |old + d| in accumulate mode
  param_dist                S_k: the f64 per-thread sums round once (E), then 6 levels + 4-wave combine + ceil(nblk / 256) strided adds +
                            10 more: (ceil(nblk / 256) + 20) E relative; the root halves it and rounds: (.. / 2 + 1) E |norm|; the running
                            total: n_entries E sum |norm|; p .: E. Gradient: the norm's bound through the quotient, plus p - q, gout p,
                            the quotient and the product: 4 E."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from guard_bands import NAN_SENTINEL, Banded, ptr
from oracle import loss_probes as P

pytestmark = pytest.mark.gpu

F32 = torch.float32
NF = np.float32
E = P.E
ROWS = (1, 3, 4, 5, 9)
TEMPS = (1.0, 2.0, 4.5)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a ROCm device (no CPU fallback exists)")
    from gslora_hip import _lib_kd
    _lib_kd.load()
    return _lib_kd


@functools.lru_cache(None)
def threshold():
    from gslora_hip import _lib_kd as LK
    lo, hi = 1, 1 << 20
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if LK.kd_plan(4, mid)[0] == LK.KD_WAVE else (lo, mid)
    return hi


# widths: fixed ones, and the plan's threshold - 1, threshold, threshold + 1 — resolved inside the tests (nothing opens the library at collection)
WIDTHS = (1, 2, 63, 64, 65, 1000, 1024, 1025, "thr-1", "thr", "thr+1")


def width(C):
    return C if isinstance(C, int) else threshold() + {"thr-1": -1, "thr": 0, "thr+1": 1}[C]


def stream():
    return torch.cuda.current_stream().cuda_stream


def In(a, ld=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return Banded(t.shape, t.dtype, t) if ld is None else Banded(t.shape, t.dtype, t, ld=ld)


def Out(*shape, ld=None):
    return Banded(shape, F32, sentinel=NAN_SENTINEL[F32]) if ld is None else Banded(shape, F32, ld=ld, sentinel=NAN_SENTINEL[F32])


def host(b):
    return b.view.cpu().numpy()


def under(what, got, ref, bound):
    r = P.ratio(got, ref, bound)
    print(f"RATIO {what} {r:.3f}")
    assert r <= 1.0, (what, r)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def logits(B, C, seed, spread=3.0):
    g = np.random.default_rng(seed)
    return (g.standard_normal((B, C)) * spread).astype(NF), (g.standard_normal((B, C)) * spread).astype(NF), g.integers(0, C, B).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- reference and bounds
def reference(ys, yt, y, T, c_kd, c_ce, g=1.0):
    """float64 on the f32 inputs. -> dict(out [3], bound [3], d [B, C], bound_d [B, C], rows ..)."""
    B, C = ys.shape
    T32 = NF(T)
    a, t = ys / T32, yt / T32      # the kernels' quotients: correctly rounded f32 divisions
    T64, ck, cc, g64 = float(T32), float(NF(c_kd)), float(NF(c_ce)), float(NF(g))
    rows = np.arange(B)
    k = P.kl(a, t, rows)
    b_kd_rows = P.bound_kl(a, t, rows)
    o0 = k["row"].sum() * T64 * T64 / B
    b0 = P.bound_sum(k["row"], b_kd_rows) * T64 * T64 / B + 3 * E * abs(o0)
    with_ce = cc != 0.0
    if with_ce:
        ok = (y >= 0) & (y < C)
        c = P.ce(ys, np.where(ok, y, 0))
        loss = np.where(ok, c["loss"], np.nan)
        o1 = loss.sum() / B
        b1 = P.bound_sum(c["loss"], P.bound_loss(ys, np.where(ok, y, 0))) / B + E * abs(o1)
    else:
        o1, b1 = 0.0, 0.0
    o2 = ck * o0 + cc * o1
    b2 = abs(ck) * b0 + abs(cc) * b1 + E * (abs(ck * o0) + abs(cc * o1)) + E * abs(o2)
    a64, t64, s64 = a.astype(np.float64), t.astype(np.float64), ys.astype(np.float64)
    k1 = g64 * ck * T64 / B
    dp = np.exp(a64 - k["la"][:, None]) - np.exp(t64 - k["lt"][:, None])
    d = k1 * dp
    bd = abs(k1) * (P._bound_p(a64, k["la"], P.bound_lse(a)) + P._bound_p(t64, k["lt"], P.bound_lse(t))) + 5 * E * np.abs(d)
    if with_ce:
        k2 = g64 * cc / B
        dq = np.exp(s64 - c["lse"][:, None])
        dq[rows, np.where(ok, y, 0)] -= 1.0
        part = k2 * dq
        bd = bd + abs(k2) * P._bound_p(s64, c["lse"], P.bound_lse(ys)) + 4 * E * np.abs(part)
        d = d + part
        bd = bd + E * np.abs(d)
        d[~ok] = np.nan
    return dict(out=np.array([o0, o1, o2]), bound=np.array([b0, b1, b2]), d=d, bound_d=bd, la=k["la"], lt=k["lt"], kd_rows=k["row"])


def run(lib, ys, yt, y, T, c_kd, c_ce, g=1.0, old=None, pads=(0, 0, 0)):
    """Both entry points, banded; pads: extra elements of the row strides of ys, yt and d."""
    B, C = ys.shape
    t = dict(ys=In(ys, C + pads[0]), yt=In(yt, C + pads[1]), y=None if y is None else In(y), out=Out(3), ws=Out(lib.kd_ws_elems(B, C)),
             g=In(np.array([g], dtype=NF)))
    if old is None:
        t["d"] = Out(B, C, ld=C + pads[2])
    else:
        t["d"] = In(old, C + pads[2])
    L = lib.load()
    lib.check(L.gsk_kd_ce_fwd(ptr(t["ys"]), C + pads[0], ptr(t["yt"]), C + pads[1], ptr(t["y"]), B, C, T, c_kd, c_ce, ptr(t["out"]),
                              ptr(t["ws"]), stream()), "gsk_kd_ce_fwd")
    lib.check(L.gsk_kd_ce_bwd(ptr(t["ys"]), C + pads[0], ptr(t["yt"]), C + pads[1], ptr(t["y"]), ptr(t["ws"]), ptr(t["g"]), B, C, T, c_kd,
                              c_ce, ptr(t["d"]), C + pads[2], 0 if old is None else 1, stream()), "gsk_kd_ce_bwd")
    torch.cuda.synchronize()      # (the launches return, whatever the values)
    for n in ("ys", "yt", "y", "g", "out", "ws"):
        assert t[n] is None or t[n].bands_intact(), n
    assert t["out"].unwritten() == 0 and t["ws"].unwritten() == 0
    if old is None:
        assert t["d"].bands_intact() and t["d"].unwritten() == 0
    else:
        assert t["d"].outside_intact()
    return host(t["out"]).copy(), host(t["d"]).copy(), host(t["ws"]).copy()


def torch_cpu(ys, yt, T):
    """The reference's formula, evaluated by torch on the CPU in f32."""
    a, b = torch.from_numpy(ys), torch.from_numpy(yt)
    return float(F.kl_div(F.log_softmax(a / T, dim=1), F.softmax(b / T, dim=1), reduction="sum") * T ** 2 / ys.shape[0])


# ---------------------------------------------------------------------------------------------------------------- gsk_kd_ce_*
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("B", ROWS)
def test_kd_ce_against_float64(lib, B, C):
    C = width(C)
    ys, yt, y = logits(B, C, 1000 * B + C)
    pads = (3, 5, 7)      # odd strides: rows lose their 16-byte alignment
    old = np.random.default_rng(7).standard_normal((B, C)).astype(NF)
    for T in TEMPS:
        for c_kd, c_ce, g in ((0.001, 0.99, 1.0), (-1.0, 0.0, 0.37)):
            r = reference(ys, yt, y, T, c_kd, c_ce, g)
            labels = y if c_ce else None
            out, d, ws = run(lib, ys, yt, labels, T, c_kd, c_ce, g, pads=pads)
            tag = f"B{B} C{C} T{T} ce{c_ce}"
            under(f"out {tag}", out, r["out"], r["bound"])
            under(f"d {tag}", d, r["d"], r["bound_d"])
            under(f"la {tag}", ws[:B], r["la"], P.bound_lse(ys / NF(T)))
            under(f"lt {tag}", ws[B:2 * B], r["lt"], P.bound_lse(yt / NF(T)))
            if not c_ce:
                assert out[1] == 0.0 and not ws[2 * B:3 * B].any() and not ws[4 * B:].any()
            want = torch_cpu(ys, yt, T)
            assert abs(out[0] - want) <= r["bound"][0] + abs(want - r["out"][0]), "the reference formula in f32 on the CPU"
            out_a, d_a, _ = run(lib, ys, yt, labels, T, c_kd, c_ce, g, old=old, pads=pads)
            assert same_bits(out_a, out)
            under(f"accumulate {tag}", d_a, old.astype(np.float64) + r["d"], r["bound_d"] + E * np.abs(old + r["d"]))
            assert same_bits(d_a, old + d), "accumulate is fl(old + value), the value formed first"


@pytest.mark.parametrize("C", [65, "thr-1", "thr+1"])
def test_decomposition(lib, C):
    C = width(C)
    from gslora_hip import _lib
    B = 5
    ys, yt, y = logits(B, C, 11 + C)
    out, _, _ = run(lib, ys, yt, None, 2.0, 1.0, 0.0)
    assert out[2] == out[0] and out[1] == 0.0, "c_kd = 1, c_ce = 0: the part IS the KL"
    out, d, _ = run(lib, ys, yt, y, 2.0, 0.0, 1.0, g=0.37)
    L = _lib.load()
    x, yy, o2, ws, coef, g = In(ys), In(y), Out(2), Out(2 * B), In(np.array([0.37], dtype=NF)), Out(B, C)
    _lib.check(L.gsl_ce_fwd(ptr(x), ptr(yy), ptr(o2), ptr(ws), B, C, stream()), "gsl_ce_fwd")
    _lib.check(L.gsl_ce_bwd(ptr(x), ptr(yy), ptr(coef), 1.0 / B, ptr(g), B, C, 0, stream()), "gsl_ce_bwd")
    torch.cuda.synchronize()
    r = reference(ys, yt, y, 2.0, 0.0, 1.0, 0.37)
    # two kernels under the same bound against the same float64 value are within twice the bound of each other
    assert abs(out[1] - host(o2)[0] / B) <= 2 * r["bound"][1]
    assert out[2] == out[1], "c_kd = 0, c_ce = 1: 0 * kd + 1 * ce"
    assert (np.abs(d - host(g)) <= 2 * r["bound_d"]).all()


@pytest.mark.parametrize("C", [64, "thr+1"])
def test_edge_rows(lib, C):
    C = width(C)
    B = 5
    ys, yt, y = logits(B, C, 5 + C)
    yt[1, :] = 0.25
    yt[1, C // 2] = 500.25      # every other teacher probability of row 1 underflows
    yt[3] = ys[3]               # identical rows
    for T in TEMPS:
        r = reference(ys, yt, y, T, 1.0, 0.5)
        out, d, ws = run(lib, ys, yt, y, T, 1.0, 0.5)
        assert np.isfinite(out).all() and np.isfinite(d).all() and np.isfinite(torch_cpu(ys, yt, T))
        under(f"underflow out C{C} T{T}", out, r["out"], r["bound"])
        under(f"underflow d C{C} T{T}", d, r["d"], r["bound_d"])
        kd_rows, b_rows = ws[3 * B:4 * B], P.bound_kl(ys / NF(T), yt / NF(T), np.arange(B))
        under(f"kd rows C{C} T{T}", kd_rows, r["kd_rows"], b_rows)
        assert abs(kd_rows[3]) <= b_rows[3], "identical rows: KD is 0 within the bound"
        _, d_kd, _ = run(lib, ys, yt, None, T, 1.0, 0.0)
        assert (np.abs(d_kd[3]) <= reference(ys, yt, None, T, 1.0, 0.0)["bound_d"][3]).all(), "... and so is its gradient"


@pytest.mark.parametrize("C", [65, "thr"])
@pytest.mark.parametrize("bad", [-1, "C"])
def test_label_out_of_range(lib, C, bad):
    C = width(C)
    B = 5
    ys, yt, y = logits(B, C, 3 + C)
    y[2] = C if bad == "C" else bad
    r = reference(ys, yt, y, 2.0, 0.001, 0.99)
    out, d, ws = run(lib, ys, yt, y, 2.0, 0.001, 0.99, pads=(1, 2, 3))      # (run() checks the bands)
    assert np.isfinite(out[0]) and np.isnan(out[1]) and np.isnan(out[2])
    assert np.isnan(d[2]).all() and np.isfinite(np.delete(d, 2, 0)).all()
    under("neighbours", np.delete(d, 2, 0), np.delete(r["d"], 2, 0), np.delete(r["bound_d"], 2, 0))
    assert np.isnan(ws[4 * B + 2]) and np.isfinite(np.delete(ws[4 * B:], 2)).all()
    out0, d0, _ = run(lib, ys, yt, None, 2.0, 0.001, 0.0)      # without the cross-entropy the labels are not read
    assert np.isfinite(out0).all() and np.isfinite(d0).all()


@pytest.mark.parametrize("C", [65, "thr"])
def test_nan_logit_and_determinism(lib, C):
    C = width(C)
    B = 9
    ys, yt, y = logits(B, C, 17 + C)
    a = run(lib, ys, yt, y, 4.5, 0.001, 0.99, g=0.37)
    b = run(lib, ys, yt, y, 4.5, 0.001, 0.99, g=0.37)
    assert all(same_bits(u, v) for u, v in zip(a, b)), "the same inputs give the same bits"
    ys[4, C - 1] = np.nan
    out, d, _ = run(lib, ys, yt, y, 4.5, 0.001, 0.99)      # the launches return (run() synchronizes)
    assert np.isnan(out).all() and np.isnan(d[4]).all() and np.isfinite(np.delete(d, 4, 0)).all()
    ys[4, C - 1] = 0.0
    yt[0, 0] = np.nan
    out, d, _ = run(lib, ys, yt, y, 4.5, 0.001, 0.99)
    assert np.isnan(out[0]) and np.isfinite(out[1]) and np.isnan(out[2]) and np.isnan(d[0]).all()


def test_autograd_node_and_distillkl(lib):
    from gslora_hip import kd
    B, C = 5, 100
    ys, yt, y = logits(B, C, 99)
    s = torch.from_numpy(ys).cuda().requires_grad_()
    t = torch.from_numpy(yt).cuda().requires_grad_()
    k, ce, part = kd.kd_ce(s, t, torch.from_numpy(y).cuda(), 2.0, 0.001, 0.99)
    assert not k.requires_grad and not ce.requires_grad and part.requires_grad
    (part * 0.37).backward()
    assert t.grad is None, "the teacher's logits never receive a gradient"
    r = reference(ys, yt, y, 2.0, 0.001, 0.99, 0.37)
    under("autograd values", torch.stack((k, ce, part)).detach().cpu().numpy(), r["out"], r["bound"])
    under("autograd gradient", s.grad.cpu().numpy(), r["d"], r["bound_d"])
    s2 = torch.from_numpy(ys).cuda().requires_grad_()
    loss = kd.DistillKL(2.0)(s2, t)
    assert loss.item() == kd.kd_ce(s2, t, None, 2.0, 1.0, 0.0)[0].item()
    loss.backward()
    r = reference(ys, yt, None, 2.0, 1.0, 0.0)
    under("DistillKL gradient", s2.grad.cpu().numpy(), r["d"], r["bound_d"])


# ---------------------------------------------------------------------------------------------------------------- gsk_param_dist_*
SIZES = (1, 3, 4, 1023, 1024, 1025, 70001)


def dist_case(lib, sizes, train, offsets, p, gout, equal=()):
    """One table: tensor k has sizes[k] elements, starts offsets[k] floats behind a 16-byte boundary, trains if train[k]; tensors named in
    `equal` have q == p. -> what the kernels gave and the float64 reference with its bounds."""
    rng = np.random.default_rng(sum(sizes) + len(sizes))
    hp = [rng.standard_normal(n).astype(NF) for n in sizes]
    hq = [hp[k].copy() if k in equal else (hp[k] + 0.01 * rng.standard_normal(sizes[k])).astype(NF) for k in range(len(sizes))]

    def place(arrs):      # every tensor in ONE banded buffer, at its own offset modulo 4 floats
        starts, pos = [], 0
        for k, a in enumerate(arrs):
            pos = (pos + 3) // 4 * 4 + offsets[k]
            starts.append(pos)
            pos += len(a)
        flat = np.full(pos, np.nan, dtype=NF)
        for s, a in zip(starts, arrs):
            flat[s:s + len(a)] = a
        return In(flat), starts
    bp, sp = place(hp)
    bq, sq = place(hq)
    entries = [(ptr(bp) + 4 * sp[k], ptr(bq) + 4 * sq[k], sizes[k], train[k]) for k in range(len(sizes))]
    table, total, bwd, g_elems = lib.param_dist_layout(entries)
    tab = lib.table_to_device(table, "cuda")
    out, norms, ws, g_in = Out(1), Out(len(sizes)), Out(total), In(np.array([gout], dtype=NF))
    lib.param_dist_fwd(tab, len(sizes), total, p, out.view, norms.view, ws.view)
    g = None
    if bwd:
        g = In(np.zeros(g_elems, dtype=NF))
        lib.param_dist_bwd(tab, len(sizes), bwd, p, g_in.view, norms.view, g.view)
    torch.cuda.synchronize()
    for b in (bp, bq, out, norms, ws, g_in):
        assert b.bands_intact()
    assert out.unwritten() == 0 and norms.unwritten() == 0 and ws.unwritten() == 0
    assert g is None or g.outside_intact()
    # float64
    p64, g64 = float(NF(p)), float(NF(gout))
    nrm = np.array([np.sqrt(((a.astype(np.float64) - b.astype(np.float64)) ** 2).sum()) for a, b in zip(hp, hq)])
    nblk = np.array([min(1024, -(-n // 1024)) for n in sizes])
    b_nrm = ((-(-nblk // 256) + 20) / 2 + 1) * E * nrm
    want = p64 * nrm.sum()
    b_out = abs(p64) * (b_nrm.sum() + len(sizes) * E * nrm.sum()) + E * abs(want)
    grads, b_grads, spans = [], [], []
    for k in range(len(sizes)):
        if not train[k]:
            continue
        diff = hp[k].astype(np.float64) - hq[k].astype(np.float64)
        if nrm[k] == 0:
            grads.append(np.zeros(sizes[k])); b_grads.append(np.zeros(sizes[k]))
        else:
            gk = g64 * p64 / nrm[k] * diff
            grads.append(gk); b_grads.append(np.abs(gk) * (b_nrm[k] / nrm[k] + 4 * E))
        spans.append((table[k].goff, sizes[k]))
    return dict(out=host(out)[0], norms=host(norms).copy(), g=None if g is None else host(g).copy(), want=want, b_out=b_out, nrm=nrm, b_nrm=b_nrm,
                grads=grads, b_grads=b_grads, spans=spans, g_elems=g_elems)


def check_dist(r, tag):
    under(f"param_dist value {tag}", r["out"], r["want"], r["b_out"])
    under(f"param_dist norms {tag}", r["norms"], r["nrm"], r["b_nrm"] + P.TINY)
    if r["g"] is None:
        return
    rest = r["g"].copy()
    for (off, n), want, bound in zip(r["spans"], r["grads"], r["b_grads"]):
        got = r["g"][off:off + n]
        assert np.isfinite(got).all()
        if not want.any():
            assert not got.any(), "p_k == q_k: the gradient is exactly 0"
        else:
            under(f"param_dist gradient {tag}", got, want, bound)
        rest[off:off + n] = 0
    assert not rest.any(), "the gradient buffer outside the trainable views is zero"


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_param_dist_one_tensor(lib, n, offset):
    check_dist(dist_case(lib, [n], [True], [offset], 0.1, 1.0), f"n{n} +{offset}")


def test_param_dist_two_and_seven_tensors(lib):
    check_dist(dist_case(lib, [1025, 3], [False, True], [1, 0], 0.1, 0.5), "two")
    check_dist(dist_case(lib, [70001, 4], [True, False], [0, 3], 0.25, 1.0), "two, the second frozen")
    sizes = list(SIZES)
    r = dist_case(lib, sizes, [True, False, True, True, False, True, True], [0, 1, 2, 3, 0, 1, 2], 0.1, 0.37, equal=(2, 5))
    check_dist(r, "seven")
    assert r["norms"][2] == 0.0 and r["norms"][5] == 0.0
    r2 = dist_case(lib, sizes, [True, False, True, True, False, True, True], [0, 1, 2, 3, 0, 1, 2], 0.1, 0.37, equal=(2, 5))
    assert same_bits(np.float32(r["out"]), np.float32(r2["out"])) and same_bits(r["norms"], r2["norms"]) and same_bits(r["g"], r2["g"])
    check_dist(dist_case(lib, [5, 1024], [False, False], [0, 0], 0.1, 1.0), "nothing trains")


def test_param_dist_autograd_node(lib):
    from gslora_hip import kd
    torch.manual_seed(3)
    model = torch.nn.Sequential(torch.nn.Linear(37, 29), torch.nn.Linear(29, 5)).cuda()
    avg = torch.nn.Sequential(torch.nn.Linear(37, 29), torch.nn.Linear(29, 5)).cuda()
    model[0].bias.requires_grad_(False)
    with torch.no_grad():
        avg[1].weight.copy_(model[1].weight)      # a zero distance among the trainable ones
    d = kd.ParamDist(model, avg, 0.1)
    (d.loss() * 2.0).backward()
    want = 0.1 * sum(torch.norm(a.double() - b.double()) for a, b in zip(model.parameters(), avg.parameters()))
    assert abs(d.loss().item() - want.item()) <= 1e-6 * want.item()
    ps = [q.detach().double().requires_grad_() for q in model.parameters()]
    (0.2 * sum(torch.norm(a - b.double()) for a, b in zip(ps, avg.parameters()))).backward()
    assert model[0].bias.grad is None and not model[1].weight.grad.any()
    for a, b in ((model[0].weight, ps[0]), (model[1].bias, ps[3])):
        assert (a.grad.double() - b.grad).abs().max().item() <= 1e-6 * b.grad.abs().max().item()
    assert d.rebuilds == 0
    model[1].bias.data = model[1].bias.data.clone()      # a tensor moved: the table is rebuilt
    d.loss()
    assert d.rebuilds == 1
    z = kd.ParamDist(model, avg, 0.0).loss()
    assert z.dim() == 0 and z.item() == 0.0 and not z.requires_grad
