"""Head-kernel probes, float64 references, error bounds, an f32 emulation and fault models for csrc/head.hip
(tests/test_head_probes_host.py, tests/test_hip_head_edges.py; measured ratios: profiles/head_kernel_tests.md).

Everything here is numpy on the CPU. A case of TABLE names a kernel, a shape (B, T, D, C), a head form, a pool and a value regime;
make(case) builds every input from a seed that depends on the case's name alone.

  kernel   fwd (head_fwd_kernel), bwd (head_bwd_kernel), wgrad (head_wgrad_kernel), logits_t / de_t / wgrad_t (the class-tiled kernels)
  form     cosface (s = 64, m = 0.35), arcface (m = 1.5: th = -0.07 puts random label cosines on both sides of the branch), arcface_easy
           (m = 0.5, easy margin), arcface_m05 (m = 0.5 plain: the planted cases), linear, linear_bias
  regime   unit (N(0, 1)), shift1e3 (x + 1000), zero_emb (row 1 of x constant and beta = 0: a zero embedding), zero_w (class row 1 of W
           zero), parallel (the label rows of Wn are +e-hat on even images and -e-hat on odd ones), planted (cos_y of the backward and of
           the weight gradient planted at PLANTED), pow2 (the loss-scaled form with max |dx| exactly 4), tiny_emb / tiny_w (embeddings / row 1
           of W of norm 1e-13: below F.normalize's clamp but not zero)
  opt      words: compact, p0.1 (dxb with dropout), dl / de (dlogits only / demb only), scaled (loss-scaled form), t_<T><S><X> dtypes

Labels walk through (0, 63, 64, C - 1, -1, C, 2^32 + 3) (places beyond C - 1 clipped to it), starting at a place that depends
on the case, so the batch of 129 has every one and the batches of 3 have them between them.

References (float64), written from the formulas in the header of head.hip (vit_face.py:540-546 pool + LayerNorm, :171-208 CosFace,
:72-143 ArcFace, :47-50 Softmax): fwd64(), bwd64(), loss_scale(), wgrad64(). Every constant a kernel holds in f32 (1e-12, 1e-6, the four
ArcFace constants, 1 / (1 - p)) enters the reference as that f32 value. The ArcFace branch is the one the f32 cos_y selects: the
comparison the forward made. F.normalize's clamp has derivative 0 below it: d e-hat / d e = I / 1e-12 where ||e|| < 1e-12.

Bounds, E = 2^-24 (half an ulp of f32, relative). Worst-case linear counts: every rounding at its largest, all with one sign, first order
in E. n_block(D, nt) = ceil(D / nt) + 6 + nt / 64 is the number of roundings of a block_sum on nt threads (the thread's strided
fma chain, six butterfly levels, the wave-order combine).

  pool     mean: T E sum_t |x_t| / T (T - 1 adds and the division)
  mu       bound(p) averaged + (n_block + 1) E mean|p|
  var      c = p - mu carries bound(p) + bound(mu) + E |c|; sum 2 |c| bound(c) / D + (n_block + 2) E var
  rstd     rs (bound(var) + E (var + eps)) / (2 (var + eps)) + 2 U_RSQRT E rs
  emb      |rs gamma| bound(c) + |c gamma| bound(rs) + 2 E |c rs gamma| + E |emb|
  1/||e||  relative: sum |e| bound(e) / ||e||^2 + (n_block + 2) E / 2 + 2 E (sqrtf and the division: correctly rounded, see below)
  dot      sum_d bound(e_d) |w_d| + (ceil(D / 64) + 6) E sum |e| |w|   (the row dot products; MFMA chain: K rounded up to the K tile)
  cos      bound(dot) / ||e|| + |cos| (rel(1/||e||) + E)
  margin   phi = c cos_m - sqrt(1 - c^2) sin_m: |phi'(c)| bound(cos), phi' = cos_m + sin_m c / sine — the condition number of the square
           root — plus sin_m (E (c^2 + |1 - c^2|) / (2 sine) + 2 E sine) + 2 E |c cos_m| + E |phi|
  backward G = s dlogits (E |G|), the label column times phi' (bound_dphi); d e-hat = sum_c G_c Wn_c, a chain of C fma: C E sum |G| |w|;
           the projection (e . d e-hat) / ||e||^2, the division by ||e||, gamma, the two LayerNorm-backward means and the final
           rs (g - c1 - xh c2), each with its operands' bounds and one E per operation (bwd64)
  dW       d What = sum_b G e-hat: (ceil(B / 16) + 16) E sum |G e-hat| (a wave's chain and the 16-wave sum; tiled: B rounded up to the K tile),
           the epilogue's two sums and its four operations (wgrad64)
  stores   a 16-bit store adds 2^-8 (bf16) or 2^-11 (fp16; 2^-25 absolute below the normal range) of the value

Division and sqrtf are taken as CORRECTLY ROUNDED: gslora_hip/build.py compiles with -O3 and nothing else that touches floating point, and
hipcc's default is -fhip-fp32-correctly-rounded-divide-sqrt (no -ffast-math, no -fno-hip-fp32-correctly-rounded-divide-sqrt on the line).
Contraction to fma is on by default; an fma rounds once where the count above has two, so the bounds hold either way. rsqrtf is not
correctly rounded: U_RSQRT ulps (an ulp = 2 E relative), chosen like U_EXP of oracle/loss_probes.py — twice the largest error of the CPU's
float32 torch.rsqrt against float64 on the arguments the table produces (cpu_rsqrt_ulps(): 1.40 ulp, asserted by the host test), rounded up
to 3.
The measured device ratios of profiles/head_kernel_tests.md are the record of whether that holds.

Ill-conditioned places: an ArcFace label cosine with 1 - cos^2 < 2^-19 on the phi branch of the FORWARD (the bound of phi exceeds what
the margin changes). Only the `parallel` regime plants them. There the check is: finite, the sign of the reference, and inside the
interval phi takes over [cos - bound, cos + bound] with 1 - c^2 clamped at 0 (exempt_interval()). The backward reads cos_y as an exact f32
input, so its bound stays below the value at every planted cosine and nothing is exempt there.

emulate_*() restate each kernel's summation order in float32 numpy: lane stride 64, the xor butterfly, the wave-order combine, the
5-class rounds of the forward, the 16-wave sum of the weight gradient, the ascending-k chain of the MFMA forms with zero-filled tails.
`fault` changes one line of an emulation (FAULTS); `reverse` sums the same terms with the lanes in reverse order — the negative control:
a legal reordering must stay under every bound."""
import collections
import functools
import math
import zlib

import numpy as np

E = 2.0 ** -24
F = np.float32
CLAMP = float(F(1e-12))
FLOOR = float(F(1e-6))
U_RSQRT = 3.0
COS_S, COS_M, EPS = 64.0, 0.35, 1e-5
ARC_M = {"arcface": (1.5, 0), "arcface_easy": (0.5, 1), "arcface_m05": (0.5, 0)}
STORE_U = {"f32": 0.0, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}
HEAD_TILED_C = 1024

Case = collections.namedtuple("Case", "name kernel B T D C form pool regime opt")
Arc = collections.namedtuple("Arc", "cos_m sin_m th mm easy")


def arc_constants(form):
    """head.hip's arc_margin(): math.cos / math.sin in double, then float."""
    m, easy = ARC_M[form]
    return Arc(*(float(F(v)) for v in (math.cos(m), math.sin(m), math.cos(math.pi - m), math.sin(math.pi - m) * m)), easy)


def is_arc(form):
    return form in ARC_M


def is_linear(form):
    return form.startswith("linear")


# ---------------------------------------------------------------------------------------------------------------- the case table
def _c(name, kernel, B, T, D, C, form="cosface", pool="cls", regime="unit", opt=""):
    return Case(name, kernel, B, T, D, C, form, pool, regime, opt)


FORMS4 = ("cosface", "arcface", "arcface_easy", "linear_bias")
FWD_D = (4, 60, 64, 68, 252, 256, 260, 1020, 1024)
FWD_C_1024T = (1, 15, 16, 17, 79, 80, 81, 100, 161, 1024)
FWD_C_256T = (1, 3, 4, 5, 19, 20, 21, 41, 100)
PLANTED = ("one", "minus_one", "below_one", "th", "above_th", "plus_zero", "minus_zero", "tiny", "above_one")
ROW_TRIPLES = ("fff", "bff", "bfb", "bfh", "bbf", "bbb", "bbh", "hff", "hfh", "hhf", "hhh")      # T S X of check_row_dtypes' eleven rows


def _table():
    t = []
    t += [_c(f"fwd_d{D}", "fwd", 3, 2, D, 17, FORMS4[i % 4]) for i, D in enumerate(FWD_D)]
    t += [_c(f"fwd_c{C}", "fwd", 3, 2, 64, C, FORMS4[i % 4]) for i, C in enumerate(FWD_C_1024T)]
    t += [_c(f"fwd_c{C}_{f}", "fwd", 3, 1, 64, C, f) for C in (80, 81) for f in ("arcface", "cosface")]
    t += [_c(f"fwd_b129_c{C}", "fwd", 129, 1, 64, C, FORMS4[(i + 1) % 4]) for i, C in enumerate(FWD_C_256T)]
    t += [_c(f"fwd_t{T}_{pool}", "fwd", 3, T, 68, 21, FORMS4[T % 4], pool) for T in (1, 2, 5) for pool in ("cls", "mean")]
    t += [_c(f"fwd_x{x}", "fwd", 5, 3, 68, 21, "arcface", "mean", opt=f"x_{x}") for x in ("bf16", "f16")]
    t += [_c(f"fwd_shift_{f}", "fwd", 3, 2, 68, 21, f, "mean", "shift1e3") for f in ("cosface", "linear_bias")]
    t += [_c(f"fwd_zero_emb_{f}", "fwd", 3, 2, 64, 21, f, regime="zero_emb") for f in ("cosface", "arcface", "arcface_easy")]
    t += [_c(f"fwd_zero_w_{f}", "fwd", 3, 1, 64, 21, f, regime="zero_w") for f in ("cosface", "arcface")]
    t += [_c(f"fwd_parallel_{f}", "fwd", 4, 1, 64, 21, f, regime="parallel") for f in ("cosface", "arcface_m05", "arcface_easy")]
    # backward, C <= 1024: six images, labels 0 / 255 / 256 / C - 1 / -1 / C
    t += [_c(f"bwd_c{C}", "bwd", 6, 2, 64, C, ("arcface", "arcface_easy", "cosface")[i % 3]) for i, C in enumerate((1, 255, 256, 257, 1023, 1024))]
    t += [_c(f"bwd_c{C}_arc", "bwd", 6, 1, 64, C, "arcface") for C in (257, 1024)]
    t += [_c(f"bwd_dense_t{T}", "bwd", 3, T, 68, 21, "arcface", opt="p0.1") for T in (1, 2, 5)]
    t += [_c("bwd_compact", "bwd", 3, 5, 68, 21, "cosface", opt="compact p0.1"), _c("bwd_compact_p0", "bwd", 3, 2, 64, 21, "arcface", opt="compact")]
    t += [_c(f"bwd_mean_t{T}", "bwd", 3, T, 68, 21, "cosface", "mean", opt="p0.1") for T in (2, 5)]
    t += [_c(f"bwd_only_{o}", "bwd", 3, 2, 64, 21, "arcface", opt=o) for o in ("dl", "de")]
    t += [_c(f"bwd_linear_{o or 'both'}", "bwd", 3, 2, 64, 21, "linear", opt=o) for o in ("", "de")]
    t += [_c(f"bwd_t_{tr}", "bwd", 3, 2, 64, 21, "cosface", opt=f"t_{tr} p0.1") for tr in ROW_TRIPLES if tr != "fff"]
    t += [_c(f"bwd_d{D}", "bwd", 2, 2, D, 5, "arcface") for D in (4, 252, 260, 1024)]
    t += [_c(f"bwd_planted_{f}", "bwd", 9, 1, 64, 300, f, regime="planted") for f in ("arcface_m05", "arcface_easy")]
    t += [_c("bwd_zero_emb", "bwd", 3, 2, 64, 21, "cosface", regime="zero_emb"), _c("bwd_tiny_emb", "bwd", 3, 1, 64, 21, "cosface", regime="tiny_emb")]
    t += [_c("bwd_shift", "bwd", 3, 2, 68, 21, "cosface", "mean", "shift1e3")]
    t += [_c("bwd_scaled", "bwd", 5, 2, 64, 21, "arcface", opt="scaled t_hff"), _c("bwd_scaled_h", "bwd", 5, 2, 64, 21, "cosface", opt="scaled t_hhh p0.1"),
          _c("bwd_scaled_mean", "bwd", 3, 3, 68, 21, "cosface", "mean", opt="scaled t_hff"),
          _c("bwd_scaled_pow2", "bwd", 2, 1, 4, 3, "linear", regime="pow2", opt="scaled t_hff de")]
    # weight gradient, per-class form
    t += [_c(f"wg_c{C}", "wgrad", 5, 1, 8, C, ("cosface", "arcface", "linear_bias")[i % 3]) for i, C in enumerate((1, 2, 255, 256, 257, 258, 1024))]
    t += [_c(f"wg_d{D}", "wgrad", 17, 1, D, 3, ("cosface", "arcface", "arcface_easy", "linear")[i % 4])
          for i, D in enumerate((1, 3, 4, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024))]
    t += [_c(f"wg_ct2_d{D}", "wgrad", 17, 1, D, 258, "arcface") for D in (257, 513)]
    t += [_c(f"wg_b{B}", "wgrad", B, 1, 64, 3, ("cosface", "arcface", "linear_bias")[i % 3]) for i, B in enumerate((1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130))]
    t += [_c(f"wg_km16_b{B}", "wgrad", B, 1, 1023, 2, "arcface") for B in (31, 32, 33)]
    t += [_c(f"wg_zero_w_{f}", "wgrad", 9, 1, 64, 7, f, regime="zero_w") for f in ("cosface", "arcface")]
    t += [_c("wg_zero_emb", "wgrad", 9, 1, 64, 7, "cosface", regime="zero_emb"), _c("wg_tiny_w", "wgrad", 9, 1, 64, 7, "cosface", regime="tiny_w"),
          _c("wt_tiny_w", "wgrad_t", 9, 1, 8, 1041, "cosface", regime="tiny_w")]
    t += [_c(f"wg_planted_{f}", "wgrad", 9, 1, 64, 300, f, regime="planted") for f in ("arcface_m05", "arcface_easy")]
    t += [_c("wg_linear", "wgrad", 17, 1, 64, 7, "linear"), _c("wg_linear_bias", "wgrad", 17, 1, 64, 7, "linear_bias")]
    t += [_c(f"wg_fallback_c{C}_d6", "wgrad", 5, 1, 6, C, "arcface") for C in (1025, 1100)]
    t += [_c(f"wg_fallback_c{C}_off4", "wgrad", 5, 1, 8, C, "cosface", opt="off4") for C in (1025, 1100)]
    # the class-tiled kernels at their tile edges
    t += [_c(f"lt_b{B}", "logits_t", B, 1, 32, 1025, ("cosface", "arcface", "linear_bias")[i % 3]) for i, B in enumerate((1, 63, 64, 65))]
    t += [_c(f"lt_c{C}", "logits_t", 3, 1, 32, C, "arcface") for C in (1152, 1153)]
    t += [_c(f"lt_d{D}", "logits_t", 3, 1, D, 1025, "cosface") for D in (4, 28, 36)]
    t += [_c(f"dt_b{B}", "de_t", B, 1, 64, 1025, "arcface") for B in (31, 32, 33)]
    t += [_c(f"dt_d{D}", "de_t", 3, 1, D, 1153, "cosface") for D in (4, 60, 68)]
    t += [_c("dt_c1152", "de_t", 3, 1, 64, 1152, "arcface_easy")]
    t += [_c(f"wt_d{D}_c{C}", "wgrad_t", 9, 1, D, C, "arcface" if D == 4 else "cosface") for D in (4, 132, 260, 516) for C in (1041, 16449)]
    t += [_c(f"wt_b{B}", "wgrad_t", B, 1, 4, 1041, ("cosface", "arcface", "linear_bias")[i % 3]) for i, B in enumerate((1, 7, 8, 15, 16, 17, 33))]
    names = [c.name for c in t]
    assert len(set(names)) == len(names)
    return tuple(t)


TABLE = _table()
BY_NAME = {c.name: c for c in TABLE}


def cases(kernel):
    return [c for c in TABLE if c.kernel == kernel]


def opt(case, word):
    return word in case.opt.split()


def triple(case):
    """(T, S, X) element types of a backward case: dxb, dx, x."""
    names = {"f": "f32", "b": "bf16", "h": "f16"}
    for w in case.opt.split():
        if w.startswith("t_"):
            return tuple(names[ch] for ch in w[2:])
    for w in case.opt.split():
        if w.startswith("x_"):
            return ("f32", "f32", w[2:])
    return ("f32", "f32", "f32")


def round_to(x, fmt):
    """x (f32) rounded to nearest even in a 16-bit format, returned as f32."""
    x = np.asarray(x, dtype=F)
    if fmt == "f32":
        return x.copy()
    if fmt == "f16":
        return x.astype(np.float16).astype(F)
    u = x.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(F).reshape(x.shape)


def labels_of(case):
    B, C = case.B, case.C
    if case.kernel == "bwd" and case.B == 6:
        lab = [0, min(255, C - 1), min(256, C - 1), C - 1, -1, C]
    elif case.regime == "planted":
        lab = [257, 0, 255, 256, 299, 63, 64, 258, 1]
    else:
        places = (0, min(63, C - 1), min(64, C - 1), C - 1, -1, C, 2 ** 32 + 3)
        k = zlib.crc32(case.name.encode()) % 7
        lab = [places[(i + k) % 7] for i in range(B)]
        if case.regime == "parallel":
            lab = [0, 5, C - 1, 7]      # four different rows of Wn
        if case.regime in ("zero_w", "tiny_w") and C > 1:
            lab[0] = 1      # the zero row is also a label row (its cosine is 0)
    return np.array(lab[:B], dtype=np.int64)


def planted_cos(form):
    a = arc_constants(form)
    th = F(a.th)
    v = dict(one=F(1), minus_one=F(-1), below_one=F(1) - F(2.0 ** -24), th=th, above_th=np.nextafter(th, F(2)), plus_zero=F(0.0),
             minus_zero=F(-0.0), tiny=F(1e-30), above_one=np.nextafter(F(1), F(2)))
    return np.array([v[k] for k in PLANTED], dtype=F)


@functools.lru_cache(maxsize=None)
def _make(case):
    B, T, D, C = case.B, case.T, case.D, case.C
    g = np.random.default_rng(zlib.crc32(case.name.encode()))
    x = g.standard_normal((B, T, D)).astype(F)
    gamma = (1.0 + 0.2 * g.standard_normal(D)).astype(F)
    beta = (0.1 * g.standard_normal(D)).astype(F)
    W = (g.uniform(-1, 1, (C, D)) * math.sqrt(6.0 / (C + D))).astype(F)
    bias = g.uniform(-0.5, 0.5, C).astype(F)
    dl = g.standard_normal((B, C)).astype(F)
    demb = g.standard_normal((B, D)).astype(F)
    label = labels_of(case)
    eps = EPS
    if case.regime == "shift1e3":
        x = (x + F(1000.0)).astype(F)
    if case.regime == "zero_emb":
        x[1] = F(3.0)
        beta[:] = 0
    if case.regime == "zero_w":
        W[1] = 0
    if case.regime == "tiny_w":
        W[1] = (g.standard_normal(D) * 1e-14).astype(F)
    if case.regime == "pow2":      # every operation of the backward is exact: max |dx| = 4 and 2 on the two images
        x = np.tile(np.array([1, -1, 1, -1], dtype=F), (B, T, 1))
        gamma[:], beta[:], eps = 1, 0, 0.0
        demb = np.zeros((B, D), F)
        demb[0, 0], demb[1, 0] = 8, 4
    x = round_to(x, triple(case)[2])
    if is_linear(case.form):
        Wn = W.copy()
    else:
        n = np.sqrt((W.astype(np.float64) ** 2).sum(1, keepdims=True))
        Wn = (W / np.maximum(n, CLAMP)).astype(F)
    d = dict(x=x, gamma=gamma, beta=beta, W=W, Wn=Wn, bias=bias if case.form == "linear_bias" else None, dl=dl, demb=demb, label=label, eps=eps)
    f = fwd64(d, case)
    if case.regime == "parallel":
        eh = f["emb"] / np.maximum(np.sqrt((f["emb"] ** 2).sum(1, keepdims=True)), CLAMP)
        for b in range(B):
            Wn[label[b]] = ((1 if b % 2 == 0 else -1) * eh[b]).astype(F)
    # what a backward or a weight gradient reads of the forward: its f32 outputs
    emb = f["emb"].astype(F)
    if case.regime == "tiny_emb":
        emb = (emb * F(1e-14)).astype(F)
    if case.regime == "pow2":
        emb = np.zeros((B, D), F)
    cos_y = np.where((label >= 0) & (label < C), f["cos"][np.arange(B), np.clip(label, 0, C - 1)], 0.0).astype(F)
    if case.regime == "planted":
        cos_y = planted_cos(case.form)[:B]
    d.update(mean=f["mu"].astype(F), rstd=f["rs"].astype(F), emb=emb, cos_y=cos_y)
    return d


def make(case):
    """A fresh copy of the case's arrays (the cached originals are never handed out)."""
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in _make(case).items()}


# ---------------------------------------------------------------------------------------------------------------- float64 references
def n_block(D, nt):
    return -(-D // nt) + 6 + nt // 64


def fwd_threads(B):
    return 1024 if B <= 128 else 256


def valid_labels(label, C):
    return (label >= 0) & (label < C)


def phi64(c, a, above):
    """phi of the label column where `above` (the branch the f32 comparison took), else the other branch."""
    sine = np.sqrt(np.maximum(1.0 - c * c, 0.0))
    return np.where(above, c * a.cos_m - sine * a.sin_m, c if a.easy else c - a.mm)


def branch32(cos_y32, a):
    return np.asarray(cos_y32, dtype=F) > (F(0.0) if a.easy else F(a.th))


def dphi64(cos_y32, a):
    c = np.asarray(cos_y32, dtype=np.float64)
    sine = np.maximum(np.sqrt(np.maximum(1.0 - c * c, 0.0)), FLOOR)
    return np.where(branch32(cos_y32, a), a.cos_m + a.sin_m * c / sine, 1.0)


def bound_dphi(cos_y32, a):
    """Error bound of arc_dphi() in f32 on an exact f32 argument."""
    c = np.asarray(cos_y32, dtype=np.float64)
    s2 = np.maximum(1.0 - c * c, 0.0)
    err_s2 = np.where(s2 == 0.0, 0.0, E * (c * c + s2))
    sine = np.sqrt(s2)
    with np.errstate(all="ignore"):
        err_sine = np.where(sine > 0, err_s2 / (2 * np.maximum(sine, 1e-300)) * 1.5 + E * sine, 0.0)
    lo = np.maximum(sine - err_sine, FLOOR)
    q = a.sin_m * np.abs(c)
    b = q * (1.0 / lo - 1.0 / np.maximum(sine, FLOOR)) + 2 * E * q / lo + E * np.abs(dphi64(cos_y32, a))
    return np.where(branch32(cos_y32, a), b, 0.0)


def pool64(x, pool):
    x = np.asarray(x, dtype=np.float64)
    return x[:, 0] if pool == "cls" else x.sum(1) / x.shape[1]


def fwd64(d, case, cos_y32=None):
    """The forward in float64 with every intermediate. cos_y32: the f32 label cosines whose comparison picks the ArcFace branch (the
    device's, or an emulation's); None: the float64 cosine's own."""
    B, D, C = case.B, case.D, case.C
    Wn, label = d["Wn"].astype(np.float64), d["label"]
    p = pool64(d["x"], case.pool)
    mu = p.mean(1)
    c = p - mu[:, None]
    var = (c * c).mean(1)
    rs = 1.0 / np.sqrt(var + float(F(d["eps"])))
    emb = c * rs[:, None] * d["gamma"].astype(np.float64) + d["beta"].astype(np.float64)
    nrm = np.maximum(np.sqrt((emb * emb).sum(1)), CLAMP)
    dot = emb @ Wn.T
    out = dict(p=p, mu=mu, c=c, var=var, rs=rs, emb=emb, nrm=nrm, dot=dot)
    ok = valid_labels(label, C)
    r, y = np.arange(B)[ok], label[ok]
    if is_linear(case.form):
        out["cos"] = dot
        out["logits"] = dot + (d["bias"].astype(np.float64) if d["bias"] is not None else 0.0)
        return out
    cos = dot / nrm[:, None]
    out["cos"] = cos
    z = cos.copy()
    if case.form == "cosface":
        z[r, y] -= float(F(COS_M))
    else:
        a = arc_constants(case.form)
        cy = cos[r, y]
        above = branch32(cy.astype(F) if cos_y32 is None else np.asarray(cos_y32)[ok], a)
        z[r, y] = phi64(cy, a, above)
        out["above"] = above
    out["logits"] = COS_S * z
    return out


def fwd_bounds(d, case, f):
    """Per-output bounds of the forward: dict(mean, rstd, emb, cos_y [B], logits [B, C]) and ill [B]: the exempt label places."""
    B, T, D, C = case.B, case.T, case.D, case.C
    nb = n_block(D, fwd_threads(B))
    x64 = np.abs(d["x"].astype(np.float64))
    gam, Wn = np.abs(d["gamma"].astype(np.float64)), np.abs(d["Wn"].astype(np.float64))
    b_p = T * E * x64.sum(1) / T if case.pool == "mean" else np.zeros((B, D))
    b_mu = b_p.mean(1) + (nb + 1) * E * np.abs(f["p"]).mean(1)
    c, rs, var, emb = np.abs(f["c"]), f["rs"], f["var"], np.abs(f["emb"])
    b_c = b_p + b_mu[:, None] + E * c
    b_var = (2 * c * b_c).mean(1) + (nb + 2) * E * var
    ve = var + float(F(d["eps"]))
    b_rs = rs * (b_var + E * ve) / (2 * ve) + 2 * U_RSQRT * E * rs
    b_e = rs[:, None] * gam * b_c + c * gam * b_rs[:, None] + 2 * E * c * rs[:, None] * gam + E * emb
    nn = (emb * emb).sum(1)
    with np.errstate(all="ignore"):
        r_inv = np.where(nn > 0, (emb * b_e).sum(1) / np.maximum(nn, 1e-300), 0.0) + (nb + 2) * E / 2 + 2 * E
    ndot = -(-D // 32) * 32 if case.kernel == "logits_t" else -(-D // 64) + 6      # the MFMA chain over the K tiles, or a wave's row dot
    b_dot = b_e @ Wn.T + ndot * E * (emb @ Wn.T)
    out = dict(mean=b_mu, rstd=b_rs, emb=b_e, ill=np.zeros(B, bool))
    if is_linear(case.form):
        out["logits"] = b_dot + 2 * E * np.abs(f["logits"]) + E * np.abs(f["dot"])
        return out
    cos = f["cos"]
    b_cos = b_dot / f["nrm"][:, None] + np.abs(cos) * (r_inv[:, None] + E)
    b_l = COS_S * b_cos + E * np.abs(f["logits"])
    label = d["label"]
    ok = valid_labels(label, C)
    r, y = np.arange(B)[ok], label[ok]
    out["cos_y"] = np.where(ok, b_cos[np.arange(B), np.clip(label, 0, C - 1)], 0.0)
    cy, bcy = cos[r, y], b_cos[r, y]
    if case.form == "cosface":
        b_l[r, y] = COS_S * (bcy + E * np.abs(cy - COS_M)) + E * np.abs(f["logits"][r, y])
    else:
        a = arc_constants(case.form)
        above = f["above"]
        s2 = np.maximum(1.0 - cy * cy, 0.0)
        ill = above & (s2 < 2.0 ** -19)
        sine = np.sqrt(np.maximum(s2, 2.0 ** -19))
        dphi = np.abs(a.cos_m + a.sin_m * cy / sine)
        local = a.sin_m * (E * (cy * cy + s2) / (2 * sine) + 2 * E * sine) + 2 * E * np.abs(cy * a.cos_m)
        phi = f["logits"][r, y] / COS_S
        b_phi = np.where(above, 1.5 * dphi * bcy + local + E * np.abs(phi), bcy + E * np.abs(phi))
        b_l[r, y] = COS_S * b_phi + E * np.abs(f["logits"][r, y])
        out["ill"][r] = ill
    out["logits"] = b_l
    return out


def exempt_interval(d, case, f, bounds):
    """[lo, hi] of the label logit at the ill-conditioned places: phi over [cos - bound, cos + bound], 1 - c^2 clamped at 0."""
    a = arc_constants(case.form)
    B = case.B
    y = np.clip(d["label"], 0, case.C - 1)
    cy, b = f["cos"][np.arange(B), y], bounds["cos_y"]
    phi = lambda c: c * a.cos_m - np.sqrt(np.maximum(1.0 - c * c, 0.0)) * a.sin_m
    lo, hi = COS_S * phi(cy - b), COS_S * phi(cy + b)
    pad = 8 * E * COS_S
    return np.minimum(lo, hi) - pad, np.maximum(lo, hi) + pad


def loss_scale(am, tex=11):
    """S = 2^(E - ex), am = m 2^ex with m in [0.5, 1) (frexp), the exponent clamped to +-60; 1 for am = 0 or am >= 3e38."""
    am = float(am)
    if not (am > 0.0 and am < 3.0e38):
        return 1.0
    ex = math.frexp(am)[1]
    return math.ldexp(1.0, min(max(tex - ex, -60), 60))


def bwd_G(d, case):
    """(G [B, C] float64, its bound): s dlogits, the ArcFace label column times d phi / d cos at the f32 cos_y."""
    lin = is_linear(case.form)
    G = (1.0 if lin else COS_S) * d["dl"].astype(np.float64)
    bG = (0.0 if lin else E) * np.abs(G)
    if is_arc(case.form):
        a = arc_constants(case.form)
        ok = valid_labels(d["label"], case.C)
        r, y = np.arange(case.B)[ok], d["label"][ok]
        dp, bdp = dphi64(d["cos_y"][ok], a), bound_dphi(d["cos_y"][ok], a)
        bG[r, y] = bG[r, y] * np.abs(dp) + np.abs(G[r, y]) * bdp + E * np.abs(G[r, y] * dp)
        G[r, y] *= dp
    return G, bG


def bwd64(d, case, chain=None):
    """-> dict(g [B, D]: d loss / d pooled row, unscaled, float64; bound [B, D]; amax [B] as pass 1 defines it). chain: the number of
    roundings of d e-hat's class sum (the per-image kernel: C; the tiled kernel: C rounded up to its K tile)."""
    B, D, C = case.B, case.D, case.C
    use_dl, use_de = not opt(case, "de"), not opt(case, "dl")
    lin = is_linear(case.form)
    nb = n_block(D, 256)
    er = d["emb"].astype(np.float64)
    gam = d["gamma"].astype(np.float64)
    Wn = d["Wn"].astype(np.float64)
    if use_dl:
        G, bG = bwd_G(d, case)
        de = G @ Wn
        b_de = bG @ np.abs(Wn) + (C if chain is None else chain) * E * (np.abs(G) @ np.abs(Wn))
    else:
        de, b_de = np.zeros((B, D)), np.zeros((B, D))
    raw = np.sqrt((er * er).sum(1))
    nrm = np.maximum(raw, CLAMP)[:, None]
    r_n = (nb + 1) * E / 2 + E
    if lin:
        g, b_g = de, b_de
    else:
        dotp = (de * er).sum(1)
        b_dotp = (b_de * np.abs(er)).sum(1) + (nb + 1) * E * (np.abs(de * er)).sum(1)
        live = (raw >= CLAMP)[:, None]      # the clamp's derivative is 0 below it: no projection term
        proj = np.where(live, dotp[:, None] / nrm ** 2, 0.0)
        b_proj = np.where(live, b_dotp[:, None] / nrm ** 2 + np.abs(proj) * (2 * r_n + 2 * E), 0.0)
        t = de - er * proj
        g = t / nrm
        b_g = (b_de + np.abs(er) * b_proj + E * np.abs(er * proj) + E * np.abs(t)) / nrm + np.abs(g) * (r_n + E)
    if use_de:
        g = g + d["demb"].astype(np.float64)
        b_g = b_g + E * np.abs(g)
    dg = g * gam
    b_dg = b_g * np.abs(gam) + E * np.abs(dg)
    xp = pool64(d["x"], case.pool)
    b_xp = case.T * E * np.abs(d["x"].astype(np.float64)).sum(1) / case.T if case.pool == "mean" else 0.0
    mu, rs = d["mean"].astype(np.float64)[:, None], d["rstd"].astype(np.float64)[:, None]
    xh = (xp - mu) * rs
    b_xh = (b_xp + E * np.abs(xp - mu)) * rs + E * np.abs(xh)
    c1 = dg.mean(1, keepdims=True)
    b_c1 = b_dg.mean(1, keepdims=True) + (nb + 1) * E * np.abs(dg).mean(1, keepdims=True)
    c2 = (dg * xh).mean(1, keepdims=True)
    b_c2 = (b_dg * np.abs(xh) + np.abs(dg) * b_xh + E * np.abs(dg * xh)).mean(1, keepdims=True) + (nb + 1) * E * np.abs(dg * xh).mean(1, keepdims=True)
    out = rs * (dg - c1 - xh * c2)
    b = rs * (b_dg + b_c1 + b_xh * np.abs(c2) + np.abs(xh) * b_c2 + 3 * E * (np.abs(dg) + np.abs(c1) + np.abs(xh * c2))) + 2 * E * np.abs(out)
    amax = np.abs(out).max(1)
    if case.pool == "mean":
        amax = amax / case.T
    return dict(g=out, bound=b, amax=amax, b_amax=b.max(1))


def bwd_layout(case, g, b, S=1.0, keep=None, p=0.0):
    """dx and dxb as the kernel lays them out, with their bounds: (dx, b_dx, dxb, b_dxb). keep: the dense dropout mask [B * T * D] as
    ops.dropout_mask gives it (1 = kept)."""
    B, T, D = case.B, case.T, case.D
    tT, tS, _ = triple(case)
    g, b = S * g, S * b
    if case.pool == "mean":
        dense = np.repeat((g / T)[:, None, :], T, 1)
        bd = np.repeat((b / T + E * np.abs(g / T))[:, None, :], T, 1)
    else:
        dense, bd = np.zeros((B, T, D)), np.zeros((B, T, D))
        dense[:, 0], bd[:, 0] = g, b
    scale = float(F(1.0) / (F(1.0) - F(p))) if p > 0 else 1.0
    m = np.ones((B, T, D)) if keep is None else np.asarray(keep, dtype=np.float64).reshape(B, T, D)
    dxb, b_dxb = dense * m * scale, (bd * scale + E * np.abs(dense * scale)) * m
    if opt(case, "compact"):
        dense, bd, dxb, b_dxb = dense[:, 0], bd[:, 0], dxb[:, 0], b_dxb[:, 0]
    store = lambda v, bv, fmt: bv + STORE_U[fmt] * np.abs(v) + (2.0 ** -25 if fmt == "f16" else 0.0)
    return dense, store(dense, bd, tS), dxb, store(dxb, b_dxb, tT)


def wgrad_tile(case):
    """(per-class kernel?, K tile of the batch chain) by head_wgrad_rule: tiled above 1024 classes when D % 4 == 0 and emb is aligned."""
    tiled = case.C > HEAD_TILED_C and case.D % 4 == 0 and not opt(case, "off4")
    return tiled, (8 if case.D > 512 else 16)


def wgrad64(d, case):
    """-> dict(dW, b_dW [C, D], dbias, b_dbias [C] (linear_bias))."""
    B, D, C = case.B, case.D, case.C
    lin = is_linear(case.form)
    tiled, bk = wgrad_tile(case)
    G, bG = bwd_G(d, case)
    er = d["emb"].astype(np.float64)
    nchain = (-(-B // bk) * bk) if tiled else (-(-B // 16) + 16)
    if lin:
        eh, r_e = er, 0.0
    else:
        eh = er / np.maximum(np.sqrt((er * er).sum(1)), CLAMP)[:, None]
        r_e = (-(-D // 64) + 4 + 6 + 2) * E / 2 + 3 * E
    f = G.T @ eh
    b_f = bG.T @ np.abs(eh) + (nchain + 1) * E * (np.abs(G).T @ np.abs(eh)) + r_e * (np.abs(G).T @ np.abs(eh))
    out = {}
    if case.form == "linear_bias":
        out["dbias"] = d["dl"].astype(np.float64).sum(0)
        out["b_dbias"] = (nchain + 16) * E * np.abs(d["dl"].astype(np.float64)).sum(0)
    if lin:
        out.update(dW=f, b_dW=b_f)
        return out
    W = d["W"].astype(np.float64)
    n_epi = (1 + 6 + 16) if not tiled else (-(-D // 64) + 6)
    raw = np.sqrt((W * W).sum(1))[:, None]
    nrm = np.maximum(raw, CLAMP)
    r_w = (n_epi + 1) * E / 2 + E
    dot = (W * f).sum(1, keepdims=True)
    b_dot = (np.abs(W) * b_f).sum(1, keepdims=True) + (n_epi + 1) * E * np.abs(W * f).sum(1, keepdims=True)
    wh, dh = W / nrm, dot / nrm
    b_wh, b_dh = np.abs(wh) * (r_w + E), b_dot / nrm + np.abs(dh) * (r_w + E)
    t = f - wh * dh
    b_t = b_f + b_wh * np.abs(dh) + np.abs(wh) * b_dh + E * np.abs(wh * dh) + E * np.abs(t)
    live = raw >= CLAMP
    out["dW"] = np.where(live, t / nrm, f / nrm)
    out["b_dW"] = np.where(live, b_t, b_f) / nrm + np.abs(out["dW"]) * (r_w + E)
    return out


def ratio(got, ref, bound):
    """Largest |got - ref| / bound; inf where got is not finite or a bound is missed by a NaN; 0 on an exact element."""
    got, ref, bound = np.broadcast_arrays(*(np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (got, ref, bound)))
    with np.errstate(all="ignore"):
        r = np.abs(got - ref) / bound
    r = np.where(np.isfinite(r), r, np.inf)
    r = np.where(got == ref, 0.0, r)
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------------------- dropout (csrc/gsl_common.h)
def drop_mix(seed, site):
    M = (1 << 64) - 1
    z = (seed * 0x9E3779B97F4A7C15 + site * 0xBF58476D1CE4E5B9 + 0x94D049BB133111EB) & M
    z ^= z >> 29
    z = (z * 0xD6E8FEB86659FD93) & M
    z ^= z >> 32
    return z & 0xFFFFFFFF


def drop_keep(idx, p, seed, site):
    """1 where element `idx` of the dense tensor is kept (drop_mul of gsl_common.h, restated)."""
    idx = np.asarray(idx, dtype=np.uint64)
    thr = int(float(F(p) * F(65536.0) + F(0.5))) if p > 0 else 0
    if thr == 0:
        return np.ones(idx.shape, np.uint8)
    key = drop_mix(seed, site)
    w = (((idx >> np.uint64(1)) + np.uint64(key)) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    w ^= w >> np.uint64(15)
    h = (w * np.uint64(0x85EBCA77)) & np.uint64(0xFFFFFFFF)
    s = np.where(idx & np.uint64(1), h >> np.uint64(16), h & np.uint64(0xFFFF))
    return (s >= thr).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- f32 emulation
FAULTS = ("round_last_dropped", "dead_slot_stored", "label_truncated", "margin_at_column0", "branch_ge", "no_max0", "no_floor", "cos_y_after_margin",
          "mean_div_tm1", "mean_from_token1", "var_div_dm1", "rstd_no_eps", "no_projection", "dphi_at_y_and_255", "zero_fill_short",
          "compact_counter", "mean_grad_undivided", "scale_pow2_off", "gscale_inverse", "wave15_dropped", "dead_row_contributes",
          "zero_w_projected", "emb_clamp_projected", "ktile_tail_not_zeroed")
_LANE = np.arange(64)
NAN32 = F(np.nan)


def _wave(v):
    """The xor butterfly over the last axis (64 lanes); every lane ends with the same bits, lane 0 is returned."""
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANE ^ o]
    return v[..., 0]


def _strided(v, nt, reverse=False):
    """Thread t of nt adds the elements t, t + nt, ... of the last axis in ascending order (reverse: the elements mirrored)."""
    v = np.asarray(v, dtype=F)
    if reverse:
        v = v[..., ::-1]
    D = v.shape[-1]
    K = -(-D // nt)
    pad = np.zeros(v.shape[:-1] + (K * nt,), F)
    pad[..., :D] = v
    pad = pad.reshape(v.shape[:-1] + (K, nt))
    acc = np.zeros(v.shape[:-1] + (nt,), F)
    for k in range(K):
        acc = acc + pad[..., k, :]
    return acc


def wave_sum(v, reverse=False):
    return _wave(_strided(v, 64, reverse))


def block_sum(v, nt, reverse=False, skip_wave=None):
    part = _strided(v, nt, reverse)
    sm = _wave(part.reshape(part.shape[:-1] + (nt // 64, 64)))
    t = np.zeros(sm.shape[:-1], F)
    for i in range(nt // 64):
        if i != skip_wave:
            t = t + sm[..., i]
    return t


def _pool32(x, pool, fault):
    x = np.asarray(x, dtype=F)
    T = x.shape[1]
    if pool == "cls":
        return x[:, 0]
    first = 1 if fault == "mean_from_token1" and T > 1 else 0
    p = x[:, first]
    for t in range(first + 1, T):
        p = p + x[:, t]
    return p / F(T - 1 if fault == "mean_div_tm1" else T)


def _labels(label, C, fault):
    """The class a label selects, -1 where it selects none."""
    lab = np.asarray(label, dtype=np.int64)
    if fault == "label_truncated":
        lab = lab.astype(np.int32).astype(np.int64)      # cast before the range test
    ok = (lab >= 0) & (lab < C)
    return np.where(ok, lab, 0 if fault == "margin_at_column0" else -1)


def _above32(c, a, fault):
    th = F(0.0) if a.easy else F(a.th)
    return (c >= th) if fault == "branch_ge" else (c > th)


def arc_phi32(c, a, fault=None):
    s2 = F(1.0) - c * c
    with np.errstate(invalid="ignore"):
        sine = np.sqrt(s2 if fault == "no_max0" else np.maximum(s2, F(0.0)))
    phi = c * F(a.cos_m) - sine * F(a.sin_m)
    return np.where(_above32(c, a, fault), phi, c if a.easy else c - F(a.mm)).astype(F)


def arc_dphi32(c, a, fault=None):
    with np.errstate(all="ignore"):
        s2 = F(1.0) - c * c
        sine = np.sqrt(s2 if fault == "no_max0" else np.maximum(s2, F(0.0)))
        if fault != "no_floor":
            sine = np.maximum(sine, F(1e-6))
        v = F(a.cos_m) + F(a.sin_m) * c / sine
    return np.where(_above32(c, a, fault), v, F(1.0)).astype(F)


def _finish_logits(dots, inv, lab, case, d, fault):
    """The store of one logit per (image, class) from its dot product: (logits [B, C], cos_y [B])."""
    B, C = dots.shape
    cos_y = np.full(B, NAN32, F)
    if is_linear(case.form):
        return (dots + (d["bias"][None, :] if d["bias"] is not None else F(0.0))).astype(F), cos_y
    dk = dots * inv[:, None]
    hit = np.arange(C)[None, :] == lab[:, None]
    if case.form == "cosface":
        return (F(COS_S) * np.where(hit, dk - F(COS_M), dk)).astype(F), cos_y
    a = arc_constants(case.form)
    phi = arc_phi32(dk, a, fault)
    rows = hit.any(1)
    cos_y[rows] = (phi if fault == "cos_y_after_margin" else dk)[hit]
    return (F(COS_S) * np.where(hit, phi, dk)).astype(F), cos_y


def emulate_fwd(d, case, fault=None, reverse=False):
    """head_fwd_kernel: dict(emb, mean, rstd, logits, cos_y); an element the kernel does not store is NaN."""
    B, D, C = case.B, case.D, case.C
    nt = fwd_threads(B)
    nwv = nt // 64
    p = _pool32(d["x"], case.pool, fault)
    mu = block_sum(p, nt, reverse) / F(D)
    c = p - mu[:, None]
    var = block_sum(c * c, nt, reverse) / F(D - 1 if fault == "var_div_dm1" and D > 1 else D)
    rs = (F(1.0) / np.sqrt(var + (F(0.0) if fault == "rstd_no_eps" else F(d["eps"])))).astype(F)
    v = (c * rs[:, None] * d["gamma"] + d["beta"]).astype(F)
    inv = F(1.0) / np.maximum(np.sqrt(block_sum(v * v, nt, reverse)), F(1e-12))
    dots = wave_sum(v[:, None, :] * d["Wn"][None, :, :], reverse)
    lab = _labels(d["label"], C, fault)
    logits, cos_y = _finish_logits(dots, inv, lab, case, d, fault)
    # the rounds: wave w owns classes w + nwv k, five of them a round; a dead slot computes class C - 1 again and is masked at the store
    reached = np.zeros(C, bool)
    for wave in range(nwv):
        for c0 in range(wave, C, nwv * 5):
            for k in range(5):
                cl = c0 + nwv * k
                if fault == "round_last_dropped" and k == 4:
                    continue
                if cl < C:
                    reached[cl] = True
                elif fault == "dead_slot_stored":      # the clamped slot's value (class C - 1, no margin: its c is not the label) lands on C - 1
                    plain, _ = _finish_logits(dots, inv, np.full(B, -1), case, d, fault)
                    logits[:, C - 1] = plain[:, C - 1]
    logits[:, ~reached] = NAN32
    return dict(emb=v, mean=mu, rstd=rs, logits=logits, cos_y=cos_y)


def _chain(a, b, ktile, fault=None):
    """acc[i, j] = sum_k a[i, k] b[j, k] as ONE chain over ascending k from 0, over zero-filled padding to the K tile's end (the MFMA
    forms). fault ktile_tail_not_zeroed: the padding holds what the clamped address holds, the last k."""
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    K = a.shape[1]
    acc = np.zeros((a.shape[0], b.shape[0]), F)
    for k in range(-(-K // ktile) * ktile):
        if k < K:
            acc = acc + a[:, k, None] * b[None, :, k]
        elif fault == "ktile_tail_not_zeroed":
            acc = acc + a[:, K - 1, None] * b[None, :, K - 1]
    return acc


def emulate_logits_tiled(d, case, fault=None, reverse=False):
    """head_logits_tiled_kernel behind head_fwd_kernel(logits = NULL)."""
    B, D, C = case.B, case.D, case.C
    nt = fwd_threads(B)
    p = _pool32(d["x"], case.pool, fault)
    mu = block_sum(p, nt, reverse) / F(D)
    c = p - mu[:, None]
    rs = (F(1.0) / np.sqrt(block_sum(c * c, nt, reverse) / F(D) + F(d["eps"]))).astype(F)
    v = (c * rs[:, None] * d["gamma"] + d["beta"]).astype(F)
    inv = F(1.0) / np.maximum(np.sqrt(wave_sum(v * v, reverse)), F(1e-12))
    dots = _chain(v, d["Wn"], 32, fault)
    logits, cos_y = _finish_logits(dots, inv, _labels(d["label"], C, fault), case, d, fault)
    return dict(emb=v, mean=mu, rstd=rs, logits=logits, cos_y=cos_y)


def _G32(d, case, fault):
    lin = is_linear(case.form)
    G = d["dl"].astype(F) if lin else (F(COS_S) * d["dl"]).astype(F)
    if is_arc(case.form):
        a = arc_constants(case.form)
        lab = _labels(d["label"], case.C, fault)
        for b in np.nonzero(lab >= 0)[0]:
            col = (lab[b] & 255) if fault == "dphi_at_y_and_255" else lab[b]
            G[b, col] = G[b, col] * arc_dphi32(d["cos_y"][b:b + 1], a, fault)[0]
    return G


def emulate_bwd(d, case, fault=None, reverse=False, keep=None, p=0.0, tiled=False):
    """head_bwd_kernel (tiled: behind head_de_tiled_kernel): dict(dx, dxb in the case's layout, NaN where nothing is stored; gscale [2])."""
    B, T, D, C = case.B, case.T, case.D, case.C
    use_dl, use_de = not opt(case, "de"), not opt(case, "dl")
    lin = is_linear(case.form)
    er = d["emb"].astype(F)
    raw = np.sqrt(block_sum(er * er, 256, reverse))[:, None]
    nrm = np.maximum(raw, F(1e-12))
    de = np.zeros((B, D), F)
    if use_dl:
        G = _G32(d, case, fault)
        if tiled:
            de = _chain(G, d["Wn"].T, 128, fault)
        else:
            for c in range(C):
                de = de + G[:, c, None] * d["Wn"][None, c, :]
    proj = (block_sum(de * er, 256, reverse)[:, None] / (nrm * nrm)).astype(F)
    if fault != "emb_clamp_projected":
        proj = np.where(raw < F(1e-12), F(0.0), proj)
    xp = _pool32(d["x"], case.pool, None)
    with np.errstate(all="ignore"):
        g = de if lin else ((de if fault == "no_projection" else de - er * proj) / nrm).astype(F)
    if use_de:
        g = g + d["demb"]
    g = (g * d["gamma"]).astype(F)
    mu, rs = d["mean"][:, None], d["rstd"][:, None]
    xh = ((xp - mu) * rs).astype(F)
    c1 = (block_sum(g, 256, reverse) / F(D))[:, None]
    c2 = (block_sum(g * xh, 256, reverse) / F(D))[:, None]
    out = (rs * (g - c1 - xh * c2)).astype(F)
    gs = F(1.0)
    gscale = None
    if opt(case, "scaled"):
        am = np.abs(out).max(1)
        if case.pool == "mean":
            am = am / F(T)
        amx = float(am.max())
        if fault == "scale_pow2_off" and amx > 0 and math.frexp(amx)[0] == 0.5:
            amx = amx / 2      # ceil(log2) in place of frexp's exponent
        gs = F(loss_scale(amx))
        gscale = np.array([gs, F(1.0) / gs if fault != "gscale_inverse" else gs], dtype=F)
    out = (gs * out).astype(F)
    dense = np.full((B, T, D), NAN32, F)
    if case.pool == "mean":
        gt = out if fault == "mean_grad_undivided" else (out / F(T)).astype(F)
        dense[:] = gt[:, None, :]
    else:
        n4 = (T - 1) * D // 4 - (1 if fault == "zero_fill_short" and T > 1 else 0)
        dense.reshape(B, T * D)[:, D:D + 4 * n4] = 0
        dense[:, 0] = out
    idx = np.arange(B * T * D, dtype=np.uint64).reshape(B, T, D)
    if fault == "compact_counter" and opt(case, "compact"):
        idx[:, 0] = np.arange(B * D, dtype=np.uint64).reshape(B, D)
    scale = (F(1.0) / (F(1.0) - F(p))) if p > 0 else F(1.0)
    m = drop_keep(idx, p, *DROP_SEED_SITE).astype(F) * scale
    dxb = (dense * m).astype(F)
    if opt(case, "compact"):
        dense, dxb = dense[:, 0], dxb[:, 0]
    tT, tS, _ = triple(case)
    return dict(dx=round_to(dense, tS), dxb=round_to(dxb, tT), gscale=gscale)


DROP_SEED_SITE = (0x1234567, 9)


def emulate_wgrad(d, case, fault=None, reverse=False):
    """head_wgrad_kernel (per class) or head_wgrad_tiled_kernel, by head_wgrad_rule: dict(dW [, dbias])."""
    B, D, C = case.B, case.D, case.C
    lin = is_linear(case.form)
    tiled, bk = wgrad_tile(case)
    G = _G32(d, case, fault)
    er = d["emb"].astype(F)
    if not lin:
        inv = F(1.0) / np.maximum(np.sqrt(wave_sum(er * er, reverse)), F(1e-12))
    out = {}
    if tiled:
        eh = er if lin else (er * inv[:, None]).astype(F)
        f = _chain(G.T, eh.T, bk, fault)
        if case.form == "linear_bias":
            out["dbias"] = _chain(G.T, np.ones((1, B), F), bk, fault)[:, 0]
    else:
        part = np.zeros((16, C, D), F)
        bsum = np.zeros((16, C), F)
        nround = 16 * (2 if D > 512 else 4)
        for b in range(B):
            w = b % 16
            gi = G[b] if lin else (G[b] * inv[b]).astype(F)
            part[w] = part[w] + gi[:, None] * er[b][None, :]
            bsum[w] = bsum[w] + G[b]
        if fault == "dead_row_contributes":      # a dead slot of the last round reads row b0 (the redirected address) and adds it
            for b in range(B, -(-B // nround) * nround):
                b0 = (b // nround) * nround + b % 16
                if b0 < B:
                    gi = G[b0] if lin else (G[b0] * inv[b0]).astype(F)
                    part[b % 16] = part[b % 16] + gi[:, None] * er[b0][None, :]
        f = np.zeros((C, D), F)
        s = np.zeros(C, F)
        for w in range(16):
            if fault == "wave15_dropped" and w == 15:
                continue
            f = f + part[w]
            s = s + bsum[w]
        if case.form == "linear_bias":
            out["dbias"] = s
    if lin:
        out["dW"] = f
        return out
    W = d["W"].astype(F)
    if tiled:
        raw, dot = np.sqrt(wave_sum(W * W, reverse)), wave_sum(W * f, reverse)
    else:
        raw, dot = np.sqrt(block_sum(W * W, 1024, reverse)), block_sum(W * f, 1024, reverse)
    nrm = np.maximum(raw, F(1e-12))[:, None]
    with np.errstate(all="ignore"):
        full = ((f - (W / nrm) * (dot[:, None] / nrm)) / nrm).astype(F)
        live = (raw >= F(1e-12))[:, None] | (fault == "zero_w_projected")
        out["dW"] = np.where(live, full, (f / nrm).astype(F))
    return out


# ---------------------------------------------------------------------------------------------------------------- judging a set of outputs
def judge_fwd(d, case, got):
    """error / bound ratios of a forward's outputs (the device's or an emulation's): dict name -> largest ratio, inf for a missed exact
    check. got: emb, mean, rstd, logits (None: not asked for), cos_y [B] (read at the valid labels only). -> (ratios, exempt rows)."""
    B, C = case.B, case.C
    ok = valid_labels(d["label"], C)
    arc = is_arc(case.form)
    f = fwd64(d, case, cos_y32=np.where(ok, got["cos_y"], 0).astype(F) if arc and got.get("logits") is not None else None)
    bd = fwd_bounds(d, case, f)
    r = {k: ratio(got[k], f[{"mean": "mu", "rstd": "rs", "emb": "emb"}[k]], bd[k]) for k in ("mean", "rstd", "emb")}
    zero = (f["emb"] == 0).all(1)      # a zero embedding is exact on both sides: equality, whatever the bound
    if zero.any() and not (np.asarray(got["emb"])[zero] == 0).all():
        r["emb"] = np.inf
    if got.get("logits") is None:
        return r, np.zeros(B, bool)
    lg = np.asarray(got["logits"], dtype=np.float64)
    ill = bd["ill"]
    keep = np.ones((B, C), bool)
    keep[np.nonzero(ill)[0], d["label"][ill]] = False
    r["logits"] = ratio(lg[keep], f["logits"][keep], bd["logits"][keep])
    if zero.any() and not (lg[zero] == f["logits"][zero]).all():
        r["logits"] = np.inf
    if arc:
        r["cos_y"] = ratio(np.asarray(got["cos_y"])[ok], f["cos"][np.arange(B)[ok], d["label"][ok]], bd["cos_y"][ok])
    if ill.any():
        lo, hi = exempt_interval(d, case, f, bd)
        v, ref = lg[np.nonzero(ill)[0], d["label"][ill]], f["logits"][np.nonzero(ill)[0], d["label"][ill]]
        good = np.isfinite(v) & (np.sign(v) == np.sign(ref)) & (v >= lo[ill]) & (v <= hi[ill])
        r["exempt"] = 0.0 if good.all() else np.inf
    return r, ill


def allowed_scales(amax, b_amax):
    """The loss scales the rule allows for a largest gradient known to within its bound."""
    return {loss_scale(max(float(amax.max()) - float(b_amax.max()), 0.0)), loss_scale(float(amax.max())), loss_scale(float(amax.max()) + float(b_amax.max()))}


def judge_bwd(d, case, got, keep=None, p=0.0):
    """Ratios of a backward's dx / dxb (in the case's layout; an element the kernel must not leave unwritten arrives as NaN and misses),
    and of gscale[0..1] in the loss-scaled form: S a power of two the rule allows for the reference's maximum, gscale[1] = 1 / S exactly."""
    chain = -(-case.C // 128) * 128 if case.kernel == "de_t" else None
    ref = bwd64(d, case, chain)
    r, S = {}, 1.0
    if opt(case, "scaled"):
        S, inv = float(got["gscale"][0]), float(got["gscale"][1])
        allowed = {loss_scale(ref["amax"].max())} if case.regime == "pow2" else allowed_scales(ref["amax"], ref["b_amax"])      # pow2: exact
        r["gscale"] = 0.0 if (S in allowed and math.frexp(S)[0] == 0.5 and inv == 1.0 / S) else np.inf
    dx, b_dx, dxb, b_dxb = bwd_layout(case, ref["g"], ref["bound"], S if math.isfinite(S) else 1.0, keep, p)
    r["dx"] = ratio(got["dx"], dx, b_dx)
    if got.get("dxb") is not None:
        r["dxb"] = ratio(got["dxb"], dxb, b_dxb)
    return r


def judge_wgrad(d, case, got):
    ref = wgrad64(d, case)
    r = dict(dW=ratio(got["dW"], ref["dW"], ref["b_dW"]))
    if case.form == "linear_bias":
        r["dbias"] = ratio(got["dbias"], ref["dbias"], ref["b_dbias"])
    return r


def emulate(d, case, fault=None, reverse=False):
    """The emulation of the case's kernel and the judgement of its outputs: dict name -> ratio."""
    if fault is not None:      # a fault may divide by zero or carry a NaN on purpose
        with np.errstate(all="ignore"):
            return _emulate(d, case, fault, reverse)
    return _emulate(d, case, fault, reverse)


def _emulate(d, case, fault, reverse):
    if case.kernel in ("fwd", "logits_t"):
        got = (emulate_fwd if case.kernel == "fwd" else emulate_logits_tiled)(d, case, fault, reverse)
        return judge_fwd(d, case, got)[0]
    if case.kernel in ("bwd", "de_t"):
        p = 0.1 if opt(case, "p0.1") else 0.0
        keep = drop_keep(np.arange(case.B * case.T * case.D, dtype=np.uint64), p, *DROP_SEED_SITE)
        return judge_bwd(d, case, emulate_bwd(d, case, fault, reverse, p=p, tiled=case.kernel == "de_t"), keep, p)
    return judge_wgrad(d, case, emulate_wgrad(d, case, fault, reverse))


def cpu_rsqrt_ulps():
    """The largest error, in f32 ulps of the result, of torch's CPU float32 rsqrt against float64 on the arguments the forward cases
    produce (var + eps)."""
    import torch
    worst = 0.0
    for case in cases("fwd"):
        d = _make(case)
        arg = (fwd64(d, case)["var"] + float(F(d["eps"]))).astype(F)
        got = torch.rsqrt(torch.from_numpy(arg)).numpy().astype(np.float64)
        ref = 1.0 / np.sqrt(arg.astype(np.float64))
        worst = max(worst, float((np.abs(got - ref) / np.spacing(ref.astype(F)).astype(np.float64)).max()))
    return worst
