"""Loss-kernel probes, float64 references, error bounds, an f32 emulation and fault models for csrc/loss.hip
(tests/test_loss_probes_host.py, tests/test_hip_loss_edges.py; measured ratios: profiles/loss_kernel_tests.md).

Everything here is numpy on the CPU. A case of TABLE names a shape and a value regime; make(case) builds, from a seed that depends on the
case alone: logits x [B, n] with labels y, and embeddings a [B, n] with a prototype table t [CP_OF(n), n] and labels py. n is the class
count C of the cross entropy and the width D of the prototype distances (the same lane-strided row code serves both).

Regimes: unit (N(0, 1), the row maximum planted at 0 / 63 / 64 / n - 1 in turn, labels at those places in another turn), plus1e4 / minus1e4
(unit shifted), spread200 (every exp but the maximum's underflows), cosface (64 cos, the label's cosine 0.85 .. 0.95 and the others below 0.7: the
row loss is 1e-7 .. 1e-2), neginf (-inf in a third of the non-label places), tie_lane (the maximum twice, at c and c + 64: one lane),
tie_cross (twice in different lanes, c and c + 3 on even rows pairs, c and c + 67 on the others), ints (small integers: ties at every
place, for top-k).

References (float64): ce(), kl(), l2() with their gradients for an upstream k, topk_hits() by the header's rule, tail64() for the scalar
tail; tail32() restates the tail in float32, one rounding per operation, in the order of the reference's torch expression
(engine_cl.py:65-125 of the project this one follows: sum / n, BND - mean, relu, loss_forget * beta + loss_remain + structure * alpha +
(w_f relu(..) + w_r mean)).

Bounds, with E = 2^-24 (half an ulp of f32, relative), NPL = ceil(n / 64) elements per lane, U_EXP / U_LOG the accuracy of the device's
expf / logf in ulps (an ulp = 2 E relative). They are worst-case linear counts: every rounding at its largest, all with one sign.

  lse      S = sum exp(x - m): the subtraction (E |x - m|) and expf (2 U_EXP E) on each term, NPL - 1 adds per lane and 6 butterfly
           levels on the sum: rho = sum_c e_c (E |x_c - m| + 2 U_EXP E) / S + (NPL + 6) E relative on S, absolute on log S;
           logf: 2 U_LOG E |log S|; the add of m: E |lse|.
  loss     bound_lse + E |loss|: the subtraction lse - x[y] rounds once, but its operand lse carries E |lse| from the add above — THAT
           term dominates a confident row (|lse| = 64, loss = 1e-4: 4e-6 absolute). It is inside bound_lse and stays there.
  dlogits  p = expf(x - lse'): lse' is off by bound_lse, the subtraction by E |x - lse|, expf by 2 U_EXP E: |k| p (.. + .. + ..);
           k = coef * scale, the subtraction of the one-hot and the product: 3 E |g|; an underflowing p: |k| 2^-126.
  kl row   term_d = e_d (l_d - q_d), l = t - lt, q = a - la, e = expf(l): l is off by bound_lse(t) + E |l|, q by bound_lse(a) + E |q|, the
           difference rounds (E |l - q|), e is relative (err l + 2 U_EXP E), the product rounds; (NPL + 6) E on the sum of magnitudes.
  demb kl  as dlogits with two exponentials.
  l2 row   (a - t) rounds, the square and the add are one fma, NPL + 6 adds, the division: (NPL + 10) E l2.
  demb l2  2/D, a - t, two products, k: 6 E |g|.
  sums     sum_r of the row bounds + (ceil(B / 256) + 9) E sum_r |v_r|: the 256-thread stride, 6 butterfly levels, the 4-wave combine.
  tail     8 E times the sum of the magnitudes each output is made of (bound_tail), plus the bounds of the sums times |d out / d sum|.

emulate_*() restate the kernels' summation order in float32 numpy (64 lanes, lane-strided elements, the xor butterfly, the 256-thread row
stride and the fixed-order combine): the host test shows that they stay under every bound on every case, and that each fault model
(fault_*) exceeds one or changes an exact output on every case it is named for.

U_EXP / U_LOG. No copy of ROCm's accuracy tables for its device math library is installed next to the compiler, so the constants are
chosen from the CPU: the largest error of torch's CPU float32 exp / log against float64
on the arguments the table's cases produce (cpu_exp_log_ulps(): 0.56 and 0.50 ulp, asserted by the host test), doubled and rounded up to
2 — the measured device ratios of profiles/loss_kernel_tests.md are the record of whether that holds."""
import collections
import functools

import numpy as np

E = 2.0 ** -24
U_EXP = 2.0
U_LOG = 2.0
TINY = 2.0 ** -126
F = np.float32
POS = (0, 63, 64, -1)                      # label / maximum places (-1: n - 1); clipped to n - 1
WIDTHS = (1, 2, 63, 64, 65, 127, 129, 1000, 1023, 1024, 1025, 2049)
ROWS = (1, 3, 4, 5, 255, 257, 513, 1027)
REGIMES = ("plus1e4", "minus1e4", "spread200", "cosface", "neginf", "tie_lane", "tie_cross", "ints")
SUM_THREADS = 256

Case = collections.namedtuple("Case", "name B n regime")
TABLE = (tuple(Case(f"w{n}_b5", 5, n, "unit") for n in WIDTHS)
         + tuple(Case(f"w65_b{B}", B, 65, "unit") for B in ROWS if B != 5)
         + tuple(Case(f"{r}_w129_b8", 8, 129, r) for r in REGIMES)
         + (Case("cosface_w1000_b64", 64, 1000, "cosface"), Case("plus1e4_w1025_b5", 5, 1025, "plus1e4"), Case("big", 1027, 2049, "unit")))
BY_NAME = {c.name: c for c in TABLE}


def cp_of(n):
    """Rows of the prototype table of a case: never n itself (Cp != C in both directions over the table)."""
    return 7 if n != 7 and n >= 4 else 11


def npl(n):
    return (n + 63) // 64


def place(p, n):
    return n - 1 if p < 0 else min(p, n - 1)


@functools.lru_cache(maxsize=None)
def _make(case):
    B, n, regime = case.B, case.n, case.regime
    g = np.random.default_rng(100003 * B + 1009 * n + 17 * (REGIMES.index(regime) + 1 if regime in REGIMES else 0))
    r = np.arange(B)
    y = np.array([place(POS[i % 4], n) for i in r], dtype=np.int64)
    mpos = np.array([place(POS[(i + i // 4) % 4], n) for i in r], dtype=np.int64)
    x = g.standard_normal((B, n)).astype(F)
    first = np.full(B, -1, dtype=np.int64)            # tie cases: the first / second of the equals
    second = np.full(B, -1, dtype=np.int64)
    if regime in ("unit", "plus1e4", "minus1e4"):
        x[r, mpos] = np.abs(x).max(1) + F(2.0)
        if regime != "unit":
            x = x + F(1e4 if regime == "plus1e4" else -1e4)
    elif regime == "spread200":
        x = (x * F(5.0)).astype(F)
        x[r, mpos] = F(200.0) + np.abs(x).max(1)
    elif regime == "cosface":
        cos = g.uniform(-1.0, 0.7, (B, n))
        cos[r, y] = 0.9 + 0.05 * g.uniform(-1, 1, B)
        x = (64.0 * cos).astype(F)
    elif regime == "neginf":
        hole = g.uniform(0, 1, (B, n)) < 0.33
        hole[r, y] = False
        hole[r, mpos] = False
        x[r, mpos] = np.abs(x).max(1) + F(2.0)
        x[hole] = -np.inf
    elif regime in ("tie_lane", "tie_cross"):
        assert n >= 129
        first = (r * 7) % 60
        second = first + (64 if regime == "tie_lane" else np.where(r % 4 < 2, 3, 67))
        top = np.abs(x).max(1) + F(1.5)
        x[r, first] = top
        x[r, second] = top
        y = np.where(r % 2 == 0, first, second)
    elif regime == "ints":
        x = g.integers(-3, 4, (B, n)).astype(F)
    a = g.standard_normal((B, n)).astype(F)
    Cp = cp_of(n)
    t = (g.standard_normal((Cp, n)) * 1.5).astype(F)
    py = ((r * 3 + 1) % Cp).astype(np.int64)
    return dict(x=x, y=y, a=a, t=t, py=py, first=first, second=second, mpos=mpos)


def make(case):
    """A fresh copy of the case's arrays (the cached originals are never handed out)."""
    return {k: v.copy() for k, v in _make(case).items()}


# ---------------------------------------------------------------------------------------------------------------- float64 references
def lse64(x):
    """(m, S, lse) per row in float64; x [B, n]."""
    x = np.asarray(x, dtype=np.float64)
    m = x.max(1)
    with np.errstate(invalid="ignore"):
        S = np.exp(x - m[:, None]).sum(1)
    return m, S, m + np.log(S)


def ce(x, y, k=None):
    """-> dict(loss, lse, amax, hit [, g = k (softmax - onehot)]) in float64; amax the FIRST index of the row maximum."""
    x64 = np.asarray(x, dtype=np.float64)
    B = x64.shape[0]
    m, S, lse = lse64(x64)
    r = np.arange(B)
    out = dict(lse=lse, loss=(m - x64[r, y]) + np.log(S), amax=x64.argmax(1))
    out["hit"] = (out["amax"] == y).astype(np.float64)
    if k is not None:
        p = np.exp(x64 - lse[:, None])
        p[r, y] -= 1.0
        out["g"] = float(k) * p
    return out


def kl(a, t, py, k=None):
    """Per-row KL(softmax(t[py]) || softmax(a)) [, g = k (softmax(a) - softmax(t[py]))]."""
    a64, t64 = np.asarray(a, dtype=np.float64), np.asarray(t, dtype=np.float64)[py]
    la, lt = lse64(a64)[2], lse64(t64)[2]
    l, q = t64 - lt[:, None], a64 - la[:, None]
    out = dict(row=(np.exp(l) * (l - q)).sum(1), la=la, lt=lt)
    if k is not None:
        out["g"] = float(k) * (np.exp(q) - np.exp(l))
    return out


def l2(a, t, py, k=None):
    a64, t64 = np.asarray(a, dtype=np.float64), np.asarray(t, dtype=np.float64)[py]
    out = dict(row=((a64 - t64) ** 2).mean(1))
    if k is not None:
        out["g"] = float(k) * (2.0 / a64.shape[1]) * (a64 - t64)
    return out


def topk_hits(x, y, ks):
    """The header's rule: a row is a hit for k when fewer than k logits are strictly greater than the label's; a label outside [0, n)
    is never a hit. -> int64 [len(ks)]."""
    x = np.asarray(x)
    B, n = x.shape
    ok = (y >= 0) & (y < n)
    yv = x[np.arange(B), np.where(ok, y, 0)]
    cnt = (x > yv[:, None]).sum(1)
    return np.array([int((ok & (cnt < k)).sum()) for k in ks], dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------------- the scalar tail
Hyper = collections.namedtuple("Hyper", "beta BND alpha w_f w_r BND_pro")
Sums = collections.namedtuple("Sums", "ce_r ce_f kl_f kl_r hit_r hit_f")


def _relu(v):
    return v if (v > 0 or v != v) else type(v)(0)      # torch's relu: a NaN stays a NaN, relu(-1) is +0


def tail64(s, n_r, n_f, structure, h, has_proto=True):
    """(total, meters [8], coefs [5]) in float64 from the six batch sums (include/gslora_hip.h at gsl_loss_combine)."""
    f = np.float64
    s, h = Sums(*map(f, s)), Hyper(*map(f, h))
    n_r, n_f = f(n_r), f(n_f)
    st = f(0.0 if structure is None else structure)
    with np.errstate(all="ignore"):
        loss_remain = s.ce_r / n_r
        hinge_f = h.BND - s.ce_f / n_f
        loss_forget = _relu(hinge_f)
        pl_f, pl_r = (s.kl_f / n_f, s.kl_r / n_r) if has_proto else (f(0.0), f(0.0))
        hinge_p = h.BND_pro - pl_f
        pro_f = h.w_f * _relu(hinge_p)
        pro_r = pl_r * h.w_r
        total = h.beta * loss_forget + loss_remain + h.alpha * st + ((pro_f + pro_r) if has_proto else 0.0)
        meters = [h.beta * loss_forget, loss_remain, total, h.alpha * st, s.hit_f * 100.0 / n_f, s.hit_r * 100.0 / n_r, pro_f, pro_r]
        coefs = [1.0 / n_r, -h.beta / n_f if hinge_f > 0 else 0.0, (-h.w_f / n_f if hinge_p > 0 else 0.0) if has_proto else 0.0,
                 h.w_r / n_r if has_proto else 0.0, h.alpha]
    return f(total), np.array(meters, dtype=f), np.array(coefs, dtype=f)


def tail32(s, n_r, n_f, structure, h, has_proto=True):
    """The same in float32, every operation rounded on its own, in the order of the reference's torch expression: the criterion's mean
    (sum / n), F.relu(BND - loss), weight * relu(BND_pro - loss) + weight * loss, loss_forget * beta + loss_remain + structure * alpha +
    prototype_loss, added left to right; accuracy = hits * (100 / n) as util/utils.py's correct_k.mul_(100.0 / batch_size)."""
    s, h = Sums(*map(F, s)), Hyper(*map(F, h))
    n_r, n_f = F(n_r), F(n_f)
    st = F(0.0 if structure is None else structure)
    zero = F(0.0)
    with np.errstate(all="ignore"):
        loss_remain = s.ce_r / n_r
        hinge_f = h.BND - s.ce_f / n_f
        loss_forget = _relu(hinge_f)
        if has_proto:
            hinge_p = h.BND_pro - s.kl_f / n_f
            pro_f = h.w_f * _relu(hinge_p)
            pro_r = h.w_r * (s.kl_r / n_r)
            proto = pro_f + pro_r
        else:
            hinge_p, pro_r, proto = h.BND_pro - zero, zero, zero
            pro_f = h.w_f * _relu(hinge_p)                      # logged only
        total = loss_forget * h.beta + loss_remain + st * h.alpha + proto
        meters = [h.beta * loss_forget, loss_remain, total, h.alpha * st, s.hit_f * (F(100.0) / n_f), s.hit_r * (F(100.0) / n_r), pro_f, pro_r]
        coefs = [F(1.0) / n_r, -h.beta / n_f if hinge_f > 0 else zero, (-h.w_f / n_f if hinge_p > 0 else zero) if has_proto else zero,
                 h.w_r / n_r if has_proto else zero, h.alpha]
    return F(total), np.array(meters, dtype=F), np.array(coefs, dtype=F)


def bound_tail(s, n_r, n_f, structure, h, has_proto=True, sum_bounds=None):
    """(b_total, b_meters [8], b_coefs [5]): 8 E times the sum of the magnitudes an output is made of (no output takes more than 8
    roundings), plus — when the sums themselves come from the device — sum_bounds (a Sums of absolute bounds) times |d output / d sum|
    with the hinges taken as active."""
    f = np.float64
    s, h = Sums(*map(f, s)), Hyper(*map(f, h))
    sb = Sums(*map(f, sum_bounds)) if sum_bounds is not None else Sums(*([f(0.0)] * 6))
    st = abs(f(0.0 if structure is None else structure))
    K = 8 * E
    m_lf = abs(h.beta) * (abs(h.BND) + abs(s.ce_f) / n_f)
    m_lr = abs(s.ce_r) / n_r
    m_pf = abs(h.w_f) * (abs(h.BND_pro) + (abs(s.kl_f) / n_f if has_proto else 0.0))
    m_pr = abs(h.w_r) * abs(s.kl_r) / n_r if has_proto else f(0.0)
    d_lf, d_lr = abs(h.beta) * sb.ce_f / n_f, sb.ce_r / n_r
    d_pf, d_pr = (abs(h.w_f) * sb.kl_f / n_f, abs(h.w_r) * sb.kl_r / n_r) if has_proto else (f(0.0), f(0.0))
    m_st = abs(h.alpha) * st
    m_tot = m_lf + m_lr + m_st + (m_pf + m_pr if has_proto else 0.0)
    d_tot = d_lf + d_lr + d_pf + d_pr
    b_m = np.array([K * m_lf + d_lf, K * m_lr + d_lr, K * m_tot + d_tot, K * m_st, K * abs(s.hit_f) * 100.0 / n_f, K * abs(s.hit_r) * 100.0 / n_r,
                    K * m_pf + d_pf, K * m_pr + d_pr])
    b_c = K * np.array([1.0 / n_r, abs(h.beta) / n_f, abs(h.w_f) / n_f, abs(h.w_r) / n_r, abs(h.alpha)])
    return K * m_tot + d_tot, b_m, b_c


# hyper-parameters and sums of the scalar-tail grid: (name, Sums, n_r, n_f, Hyper): both hinges active / inactive / exactly zero
H_ACTIVE = Hyper(0.15, 7.5, 0.01, 0.3, 0.7, 4.0)
TAIL_GRID = (
    ("active", Sums(13.25, 9.125, 2.75, 5.5, 4.0, 1.0), 6.0, 3.0, H_ACTIVE),
    ("inactive", Sums(13.25, 39.5, 20.75, 5.5, 5.0, 0.0), 6.0, 3.0, H_ACTIVE),
    ("zero", Sums(13.25, 6.0, 12.0, 5.5, 6.0, 3.0), 6.0, 3.0, Hyper(0.15, 2.0, 0.01, 0.3, 0.7, 4.0)),
    ("odd_sizes", Sums(101.3, 18.77, 3.1, 55.9, 37.0, 2.0), 41.0, 7.0, Hyper(0.37, 5.3, 0.013, 1.7, 0.9, 1.9)),
)
STRUCTURE = 23.4375


# ---------------------------------------------------------------------------------------------------------------- bounds
def _rho(x64, m, S, n):
    """Relative error bound of S = sum exp(x - m) as the kernels compute it."""
    with np.errstate(invalid="ignore"):
        d = x64 - m[:, None]
        e = np.exp(d)
        w = np.where(e > 0, e * (E * np.abs(d) + 2 * U_EXP * E), 0.0)
    return w.sum(1) / S + (npl(n) + 6) * E


def bound_lse(x):
    x64 = np.asarray(x, dtype=np.float64)
    m, S, lse = lse64(x64)
    return _rho(x64, m, S, x64.shape[1]) + 2 * U_LOG * E * np.abs(np.log(S)) + E * np.abs(lse)


def bound_loss(x, y):
    """bound_lse (which holds E |lse|, the rounding of m + log S that the subtraction then exposes) + E |loss|."""
    ref = ce(x, y)
    return bound_lse(x) + E * np.abs(ref["loss"])


def _bound_p(v64, lse, b_lse):
    """Absolute bound of expf(v - lse') per element."""
    with np.errstate(invalid="ignore"):
        u = v64 - lse[:, None]
        p = np.exp(u)
        return np.where(p > 0, p * (b_lse[:, None] + E * np.abs(u) + 2 * U_EXP * E), 0.0) + TINY


def bound_dlogits(x, y, k):
    x64 = np.asarray(x, dtype=np.float64)
    ref = ce(x64, y, k)
    return abs(float(k)) * _bound_p(x64, ref["lse"], bound_lse(x64)) + 3 * E * np.abs(ref["g"])


def bound_kl(a, t, py):
    a64, t64 = np.asarray(a, dtype=np.float64), np.asarray(t, dtype=np.float64)[py]
    n = a64.shape[1]
    ref = kl(a, t, py)
    b_la, b_lt = bound_lse(a64)[:, None], bound_lse(t64)[:, None]
    l, q = t64 - ref["lt"][:, None], a64 - ref["la"][:, None]
    e = np.exp(l)
    err_l = b_lt + E * np.abs(l)
    err_diff = err_l + b_la + E * np.abs(q) + E * np.abs(l - q)
    term = np.abs(e * (l - q))
    return (e * err_diff + term * (err_l + 2 * U_EXP * E + E)).sum(1) + (npl(n) + 7) * E * term.sum(1)


def bound_demb_kl(a, t, py, k):
    a64, t64 = np.asarray(a, dtype=np.float64), np.asarray(t, dtype=np.float64)[py]
    ref = kl(a, t, py, k)
    return abs(float(k)) * (_bound_p(a64, ref["la"], bound_lse(a64)) + _bound_p(t64, ref["lt"], bound_lse(t64))) + 3 * E * np.abs(ref["g"])


def bound_l2(a, t, py):
    return (npl(np.asarray(a).shape[1]) + 10) * E * l2(a, t, py)["row"]


def bound_demb_l2(a, t, py, k):
    return 6 * E * np.abs(l2(a, t, py, k)["g"])


def bound_sum(rows64, row_bounds):
    """Bound of the batch sum of per-row values: the rows' own bounds and the summation's roundings."""
    B = len(rows64)
    return float(np.sum(row_bounds) + ((B + SUM_THREADS - 1) // SUM_THREADS + 9) * E * np.abs(rows64).sum())


def ratio(got, ref, bound):
    """Largest |got - ref| / bound; inf where got is not finite or a bound is missed by a NaN; 0 on an exact element."""
    got, ref, bound = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (got, ref, bound))
    with np.errstate(all="ignore"):
        r = np.abs(got - ref) / bound
    r = np.where(np.isfinite(r), r, np.inf)
    r = np.where(got == ref, 0.0, r)
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------------------- f32 emulation
_LANE = np.arange(64)


def _wave(v):
    """The xor butterfly over the last axis (64 lanes); every lane ends with the same bits, lane 0 is returned."""
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANE ^ o]
    return v[..., 0]


def _lanes(v, fill):
    """[B, n] -> [B, NPL, 64]: [.., i, lane] = element lane + 64 i (fill behind the row's end) and the mask of real elements."""
    B, n = v.shape
    p = npl(n) * 64
    out = np.full((B, p), fill, dtype=v.dtype)
    out[:, :n] = v
    mask = np.zeros((B, p), dtype=bool)
    mask[:, :n] = True
    return out.reshape(B, -1, 64), mask.reshape(B, -1, 64)


def _seq(v):
    """Per-lane sequential sum over the passes, from 0."""
    s = np.zeros_like(v[:, 0])
    for i in range(v.shape[1]):
        s = s + v[:, i]
    return s


def emulate_lse(x, passes=None, drop_last=False, no_max=False):
    """row_softmax_stats / row_lse in float32: (lse, first arg-max). passes / drop_last / no_max: fault models."""
    x = np.asarray(x, dtype=F)
    B, n = x.shape
    v, mask = _lanes(x, F(0))
    if drop_last:
        mask.reshape(B, -1)[:, n - 1] = False
    if passes is not None:
        mask[:, passes:] = False
    xm = np.where(mask, v, F(-3.0e38))
    m = xm.reshape(B, -1).max(1)
    amax = xm.reshape(B, -1).argmax(1)
    if no_max:
        m = np.zeros(B, dtype=F)
    with np.errstate(all="ignore"):
        e = np.where(mask, np.exp(v - m[:, None, None]), F(0))
        return (m + np.log(_wave(_seq(e)))).astype(F), amax


def emulate_sum(rows, stop=None):
    """sum_rows_kernel in float32: 256 threads stride the rows, butterfly per wave, the waves combined in order from 0."""
    rows = np.asarray(rows, dtype=F)[:stop]
    B = len(rows)
    p = (B + SUM_THREADS - 1) // SUM_THREADS * SUM_THREADS
    v = np.zeros(p, dtype=F)
    v[:B] = rows
    part = _seq(v.reshape(1, -1, SUM_THREADS))[0]              # thread t: rows t, t + 256, ...
    w = _wave(part.reshape(4, 64))
    t = F(0)
    for i in range(4):
        t = t + w[i]
    return F(t)


def emulate_ce(x, y, k=None, **fault):
    """-> dict(loss, lse, hit [, g]) float32."""
    x = np.asarray(x, dtype=F)
    B = x.shape[0]
    lse, amax = emulate_lse(x, **fault)
    r = np.arange(B)
    with np.errstate(all="ignore"):
        out = dict(lse=lse, loss=lse - x[r, y], hit=(amax == y).astype(F), amax=amax)
        if k is not None:
            p = np.exp(x - lse[:, None])
            p[r, y] = p[r, y] - F(1)
            out["g"] = F(k) * p
    return out


def emulate_kl(a, t, py, k=None, swapped=False):
    a, tt = np.asarray(a, dtype=F), np.asarray(t, dtype=F)[py]
    if swapped:
        a, tt = tt, a
    la, lt = emulate_lse(a)[0], emulate_lse(tt)[0]
    l, q = tt - lt[:, None], a - la[:, None]
    term = np.exp(l) * (l - q)
    tv, mask = _lanes(term.astype(F), F(0))
    out = dict(row=_wave(_seq(tv)).astype(F))
    if k is not None:
        out["g"] = F(k) * (np.exp(q) - np.exp(l))
    return out


def emulate_l2(a, t, py, k=None, grad_scale=2.0):
    a, tt = np.asarray(a, dtype=F), np.asarray(t, dtype=F)[py]
    n = a.shape[1]
    df, _ = _lanes(a - tt, F(0))
    s = np.zeros_like(df[:, 0])
    for i in range(df.shape[1]):                                # fmaf(df, df, acc): one rounding
        s = (df[:, i].astype(np.float64) ** 2 + s.astype(np.float64)).astype(F)
    out = dict(row=(_wave(s) / F(n)).astype(F))
    if k is not None:
        out["g"] = F(k) * ((F(grad_scale) / F(n)) * (a - tt))
    return out


def cpu_exp_log_ulps():
    """The largest error, in f32 ulps of the result, of torch's CPU float32 exp / log against float64 on the arguments the table's cases
    hand to them (x - m of every logits row; the row sums of exponentials)."""
    import torch
    worst_e = worst_l = 0.0
    for case in TABLE:
        d = _make(case)
        for v in (d["x"], d["a"], d["t"]):
            v = v[:64]
            m = v.max(1, keepdims=True)
            arg = (v - m).astype(F)
            arg = arg[np.isfinite(arg) & (arg > -80)]
            got = torch.exp(torch.from_numpy(arg)).numpy().astype(np.float64)
            ref = np.exp(arg.astype(np.float64))
            worst_e = max(worst_e, float((np.abs(got - ref) / np.spacing(ref.astype(F)).astype(np.float64)).max()))
            S = np.exp(v.astype(np.float64) - m).sum(1).astype(F)
            got = torch.log(torch.from_numpy(S)).numpy().astype(np.float64)
            ref = np.log(S.astype(np.float64))
            ulp = np.spacing(np.maximum(np.abs(ref), TINY).astype(F)).astype(np.float64)
            worst_l = max(worst_l, float((np.abs(got - ref) / ulp).max()))
    return worst_e, worst_l


# ---------------------------------------------------------------------------------------------------------------- fault models
# Each returns what a kernel with one fault would have produced from the same inputs, as float32 / float64 arrays that the host test holds
# against the same bounds (or exact outputs) as the device test holds the kernels. FAULT_CASES names the table cases that can show it.
def fault_last_element_dropped(d):
    return emulate_ce(d["x"], d["y"], drop_last=True)


def fault_pass17_dropped(d):
    return emulate_ce(d["x"], d["y"], passes=16)


def fault_no_max_subtraction(d):
    return emulate_ce(d["x"], d["y"], no_max=True)


def fault_label_off_by_one(d):
    return emulate_ce(d["x"], (d["y"] + 1) % d["x"].shape[1], k=1.0)


def fault_row_stride_plus_one(d):
    """Row r read at r (C + 1) of the flat buffer; behind the tensor lies the NaN band."""
    B, n = d["x"].shape
    flat = np.concatenate([d["x"].reshape(-1), np.full(B, np.nan, dtype=F)])
    x = np.lib.stride_tricks.as_strided(flat, (B, n), ((n + 1) * 4, 4)).copy()
    return emulate_ce(x, d["y"])


def fault_sum_stops_at_256(rows):
    return emulate_sum(rows, stop=256)


def fault_swapped_sizes(s, n_r, n_f, structure, h, has_proto=True):
    """1/n_r and 1/n_f swapped in the coefficients (the hinge decisions and the total are the right ones)."""
    total, meters, coefs = tail32(s, n_r, n_f, structure, h, has_proto)
    c = coefs.copy()
    c[0] = F(1.0) / F(n_f)
    c[1] = -F(h.beta) / F(n_r) if coefs[1] != 0 else F(0)
    c[2] = -F(h.w_f) / F(n_r) if coefs[2] != 0 else F(0)
    c[3] = F(h.w_r) / F(n_f) if has_proto else F(0)
    return total, meters, c


def fault_mean_for_sum(rows):
    return F(emulate_sum(rows) / F(len(rows)))


def fault_relu_grad_one_at_zero(s, n_r, n_f, structure, h, has_proto=True):
    total, meters, coefs = tail32(s, n_r, n_f, structure, h, has_proto)
    coefs = coefs.copy()
    if F(h.BND) - F(s.ce_f) / F(n_f) >= 0:
        coefs[1] = -F(h.beta) / F(n_f)
    if has_proto and F(h.BND_pro) - F(s.kl_f) / F(n_f) >= 0:
        coefs[2] = -F(h.w_f) / F(n_f)
    return total, meters, coefs


def fault_tie_to_last(d):
    x = d["x"]
    n = x.shape[1]
    last = n - 1 - x[:, ::-1].argmax(1)
    return (last == d["y"]).astype(F)


def fault_kl_direction(d):
    return emulate_kl(d["a"], d["t"], d["py"], swapped=True)


def fault_l2_grad_half(d, k):
    return emulate_l2(d["a"], d["t"], d["py"], k=k, grad_scale=1.0)


def fault_forget_rows_take_remain_coef(d, nr, c_remain, c_forget):
    """dlogits of the one-launch tail with coefficient 0 on every row."""
    return emulate_ce(d["x"], d["y"], k=c_remain)["g"]


def fault_neighbour_label_prototype(d):
    return emulate_kl(d["a"], d["t"], np.roll(d["py"], -1)), emulate_l2(d["a"], d["t"], np.roll(d["py"], -1))


def _names(pred):
    return tuple(c.name for c in TABLE if pred(c))


FAULT_CASES = {
    "last_element_dropped": _names(lambda c: c.n % 64 == 1 and c.n > 1 and c.regime == "unit" and c.name != "big"),
    "pass17_dropped": _names(lambda c: c.n >= 1025 and c.name != "big"),
    "no_max_subtraction": _names(lambda c: c.regime in ("plus1e4", "minus1e4")),
    "label_off_by_one": _names(lambda c: c.regime == "unit" and c.n >= 2 and c.name != "big"),
    "row_stride_plus_one": _names(lambda c: c.regime == "unit" and c.B >= 2 and c.name != "big"),
    "sum_stops_at_256": _names(lambda c: c.B > 256 and c.name != "big"),
    "mean_for_sum": _names(lambda c: c.B >= 2 and c.regime == "unit" and c.name != "big"),
    "tie_to_last": _names(lambda c: c.regime in ("tie_lane", "tie_cross")),
    "kl_direction": _names(lambda c: c.regime == "unit" and c.n >= 2 and c.name != "big"),
    "l2_grad_half": _names(lambda c: c.regime == "unit" and c.name != "big"),
    "forget_rows_take_remain_coef": _names(lambda c: c.regime == "unit" and c.B >= 2 and c.n >= 2 and c.name != "big"),      # n = 1: g = 0
    "neighbour_label_prototype": _names(lambda c: c.regime == "unit" and c.B >= 2 and c.name != "big"),
}
