"""LayerNorm probes, float64 references, error bounds and fault models (tests/test_norm_probes_host.py, tests/test_hip_norm_edges.py).

An absolute tolerance cannot hold a LayerNorm kernel: on N(0.5, 2) rows 1e-5 is a thousand ulps, and on a constant row of -1234.567 any
correct f32 kernel is off by about 5e-2 (the rounding of the mean times rsqrt(eps)). Here every comparison is per element against a bound
that follows the roundings of the kernels of csrc/norm.hip, on rows chosen so that a dropped element, a wrong 1/D or a wrong row shows.

Inputs. Row m of x is of kind m % 7 (ROW_KINDS): N(0.5, 2), N(1000, 1), N(-300, 0.01), the constant rows 3.0 and -1234.567, N(0, 1e-4),
and N(0, 1) with one element times 3000. gamma = 1 + 0.1 N and beta = 0.1 N are not symmetric in d (a permuted lane mapping shows),
eps = 1e-5. A 16-bit x is rounded to its type first and the reference sees the widened values.

References (float64, on the device of their arguments): forward(), backward() — a function of (dy, x, gamma, mean, rstd, dres) with mean
and rstd TAKEN AS GIVEN: the f32 values the forward kernel wrote, widened, which is how the ABI defines the backward —, dropout_copy().

Bounds, with e = 2^-24 (half an ulp of f32, relative), NPL = D / 64 elements per lane, h(ref) = half an ulp of the stored type at ref
(0 for f32, 2^-8 |ref| for bf16, max(2^-11 |ref|, 2^-25) for fp16). The counts are worst-case linear ones: every rounding at its
largest, all with one sign.

  mean    (NPL + 7) e max|x|                       NPL - 1 adds per lane, 6 butterfly levels, the multiply by 1/D (and 1/D itself)
  rstd    (NPL + 8) e (1 + max|x| rstd64), relative: the centred values carry the mean's error and their own subtraction,
          2 d_i err / D summed is at most 2 sigma err: relative err / sigma = err rstd on rstd (the square root halves, the factor 2
          doubles); the "1 +" holds the sum of squares' own NPL + 7 roundings, the add of eps and rsqrt's ulp. On a constant row the
          mean's error enters squared, delta^2 / (2 eps) relative: below the linear term as long as that term is below 2.
  y       (NPL + 8) e max|x| rstd64 |gamma_d| + 8 e |ref| + h(ref)      the mean's error and the subtraction, times rstd gamma;
          rstd's own error, the two multiplies and the add of beta are relative to the terms of ref
  dx      (NPL + 8) e rstd (G + H |xhat_i|)                              c1 = mean(gy), c2 = mean(gy xhat): NPL + 5 adds, gy's product
          + 8 e rstd (|gy_i| + |c1| + |xhat_i c2|) + 2 e rstd |xhat_i| H    with gamma, the product with xhat, 1/D; G = max|gy|,
          + e |ref| + h(ref)                                              H = max|gy xhat|. Second line: the final expression (gy's
          own rounding, xhat's two, the product, two subtractions, the multiply by rstd: 7 <= 8) and xhat's two roundings inside the
          sum of c2. Third line: the add of dres and the store.
  dxb     the same with h of the operand type; under dropout p = 0.5 a kept element is exactly 2 dx: the bound of 2 ref.

emulate_forward() / emulate_backward() / emulate_forward_lora() restate the kernels' summation order (per-lane sequential sums in
RowIO's element order, the xor butterfly, times 1/D) in f32 torch: the host test shows with them that a correct implementation stays under
every bound with slack, and the fault models (fault_*) each exceed one or break a guard band."""
import collections

import numpy as np
import torch

EPS = 1e-5
E = 2.0 ** -24
WIDTHS = (64, 128, 256, 512, 768, 1024)
SMALL_M = (1, 3, 4, 5, 37)
ROWS_PER_TRIP = 4 * 2048                   # ln_fwd_kernel / ln_bwd_kernel: min(ceil(M / 4), 2048) blocks of four one-row waves
LORA_ROWS_PER_TRIP = 16 * 4 * 1024         # ln_fwd_lora_kernel: min(ceil(M / 64), 1024) blocks of four 16-row waves
TRIP2_M = ROWS_PER_TRIP + 5
CLS_T = 7                                  # tokens per image of the cls placements
P_DROP = 0.5
ROW_KINDS = ("n0.5_2", "n1000_1", "n-300_0.01", "const3", "const-1234.567", "n0_1e-4", "outlier3000")

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
# (T, X) of gsl_layernorm_fwd and (T, S, X) of gsl_layernorm_bwd: T operands (y, dy, dxb), S the gradient stream (dres, dx), X the saved x
FWD_INSTANCES = ((F16, F16), (F16, F32), (BF16, F16), (BF16, BF16), (BF16, F32), (F32, F32))
BWD_INSTANCES = ((F16, F16, F16), (F16, F16, F32), (F16, F32, F16), (F16, F32, F32),
                 (BF16, BF16, F16), (BF16, F32, F16), (BF16, BF16, BF16), (BF16, BF16, F32), (BF16, F32, BF16), (BF16, F32, F32),
                 (F32, F32, F32))

# kind: small (all widths x the row counts around one block), trip2 (a second grid-stride trip), inst (the instantiation table),
# lora (gsl_layernorm_fwd_lora; r = the adapter rank)
Case = collections.namedtuple("Case", "name kind M D r")
TABLE = (tuple(Case(f"d{D}_m{M}", "small", M, D, 0) for D in WIDTHS for M in SMALL_M)
         + tuple(Case(f"trip2_d{D}", "trip2", TRIP2_M, D, 0) for D in (64, 768))
         + tuple(Case(f"inst_d{D}", "inst", 9, D, 0) for D in (128, 256))
         + tuple(Case(f"lora_d{D}_r{r}_m{M}", "lora", M, D, r) for D in (512, 768) for r in (4, 16) for M in (1, 15, 16, 17, 63, 65))
         + (Case("lora_trip2", "lora", LORA_ROWS_PER_TRIP + 17, 512, 4),))
BY_NAME = {c.name: c for c in TABLE}


def npl(D):
    return D // 64


def _gen(case, salt=0):
    return torch.Generator().manual_seed(1000003 * case.M + 1009 * case.D + 7919 * salt + 17)


def make(case, xdtype=F32):
    """x [M, D] (rounded to xdtype, returned as float32), gamma, beta, dy, dres: float32 CPU tensors. dy ~ N(0, 1) with rows scaled
    1, 8, 1/8 in turn; dres ~ N(0, 1)."""
    g = _gen(case)
    M, D = case.M, case.D
    n = torch.randn(M, D, generator=g)
    kind = torch.arange(M) % len(ROW_KINDS)
    mu = torch.tensor([0.5, 1000.0, -300.0, 3.0, -1234.567, 0.0, 0.0])[kind][:, None]
    sd = torch.tensor([2.0, 1.0, 0.01, 0.0, 0.0, 1e-4, 1.0])[kind][:, None]
    x = mu + sd * n
    out = (kind == 6).nonzero().flatten()
    col = torch.randint(0, D, (len(out),), generator=g)
    x[out, col] *= 3000.0
    d = dict(x=x.to(xdtype).float())
    d["gamma"] = 1 + 0.1 * torch.randn(D, generator=g)
    d["beta"] = 0.1 * torch.randn(D, generator=g)
    d["dy"] = torch.randn(M, D, generator=g) * torch.tensor([1.0, 8.0, 0.125])[torch.arange(M) % 3][:, None]
    d["dres"] = torch.randn(M, D, generator=g)
    if case.kind == "lora":
        P = torch.zeros(16, D)
        P[:case.r] = torch.randn(case.r, D, generator=g) * D ** -0.5
        d["P"] = P.bfloat16().float()
    return d


# ---------------------------------------------------------------------------------------------------------------- float64 references
def forward(x, gamma, beta, eps=EPS):
    """(mean, rstd, y) in float64."""
    x = x.double()
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    return mean, rstd, (x - mean[:, None]) * rstd[:, None] * gamma.double() + beta.double()


def backward(dy, x, gamma, mean, rstd, dres=None, parts=False):
    """dx = dres + LN'(dy) in float64 with mean / rstd as given. parts: also (rstd, gy, xhat, c1, c2), what the bound is made of."""
    rs = rstd.double()[:, None]
    xhat = (x.double() - mean.double()[:, None]) * rs
    gy = dy.double() * gamma.double()
    c1, c2 = gy.mean(1, keepdim=True), (gy * xhat).mean(1, keepdim=True)
    dx = rs * (gy - c1 - xhat * c2)
    if dres is not None:
        dx = dx + dres.double()
    return (dx, (rs, gy, xhat, c1, c2)) if parts else dx


def expand_compact(dres_c, M, T):
    """The dense incoming stream gradient of the compact form: row m receives dres_c[m / T] when m % T == 0 and nothing otherwise."""
    dense = torch.zeros(M, dres_c.shape[1], dtype=dres_c.dtype, device=dres_c.device)
    dense[::T] = dres_c[:(M + T - 1) // T]
    return dense


def dropout_copy(dx, keep, p=P_DROP):
    return dx.double() * keep.double() / (1.0 - p)


def keep_rows(keep_flat, M, D, drop_row_stride):
    """keep [M, D] out of the dense counter space: element (row, d) has counter row * drop_row_stride + d."""
    idx = torch.arange(M, device=keep_flat.device)[:, None] * drop_row_stride + torch.arange(D, device=keep_flat.device)[None, :]
    return keep_flat[idx]


def dropout_keep(n, p, seed, site):
    """The documented hash of gsl_dropout_mask (csrc/gsl_common.h) in numpy: uint8 CPU tensor [n], 1 = kept."""
    U, M64 = np.uint64, (1 << 64) - 1
    z = (seed * 0x9E3779B97F4A7C15 + site * 0xBF58476D1CE4E5B9 + 0x94D049BB133111EB) & M64
    z ^= z >> 29
    z = (z * 0xD6E8FEB86659FD93) & M64
    z ^= z >> 32
    i = np.arange(n, dtype=np.uint64)
    w = (((i >> U(1)) + U(z & 0xFFFFFFFF)) * U(0x9E3779B1)) & U(0xFFFFFFFF)
    h = ((w ^ (w >> U(15))) * U(0x85EBCA77)) & U(0xFFFFFFFF)
    sample = np.where((i & U(1)) == 0, h & U(0xFFFF), h >> U(16))
    return torch.from_numpy((sample >= U(int(p * 65536.0 + 0.5))).astype(np.uint8))


# ---------------------------------------------------------------------------------------------------------------- bounds
def half_ulp(ref, dtype):
    a = ref.abs()
    if dtype == BF16:
        return a * 2.0 ** -8
    if dtype == F16:
        return torch.clamp(a * 2.0 ** -11, min=2.0 ** -25)
    return torch.zeros_like(a)


def bound_mean(x, D):
    return (npl(D) + 7) * E * x.double().abs().amax(1)


def bound_rstd(x, rstd64, D):
    """Absolute (the relative bound of the module docstring times rstd64)."""
    return (npl(D) + 8) * E * (1.0 + x.double().abs().amax(1) * rstd64) * rstd64


def bound_y(x, gamma, rstd64, ref, D, dtype):
    xm = x.double().abs().amax(1, keepdim=True)
    return (npl(D) + 8) * E * xm * rstd64[:, None] * gamma.double().abs() + 8 * E * ref.abs() + half_ulp(ref, dtype)


def bound_dx(parts, ref, D, dtype, scale=1.0):
    """parts from backward(..., parts=True); ref the float64 dx (with dres); dtype the stored type. scale 2: the kept elements of the
    dropout copy at p = 0.5 (ref then is 2 dx)."""
    rs, gy, xhat, c1, c2 = parts
    G, H = gy.abs().amax(1, keepdim=True), (gy * xhat).abs().amax(1, keepdim=True)
    ax = xhat.abs()
    b = ((npl(D) + 8) * E * rs * (G + H * ax) + 8 * E * rs * (gy.abs() + c1.abs() + ax * c2.abs()) + 2 * E * rs * ax * H) * scale
    return b + E * ref.abs() + half_ulp(ref, dtype)


def lora_u(y, P, alpha, D):
    """(float64 reference, bound) of u[:, :16] = alpha * y P[:16]^T from the bf16 rows y the kernel itself wrote: D products summed in f32 in
    whatever order the matrix core takes (D e of the sum of the magnitudes), the multiply by alpha, the bf16 store."""
    yd, Pd = y.double(), P.double()[:16]
    ref = alpha * (yd @ Pd.t())
    return ref, D * E * alpha * (yd.abs() @ Pd.abs().t()) + E * ref.abs() + half_ulp(ref, BF16)


def ratio(got, ref, bound):
    """Largest |got - ref| / bound; inf where got is not finite or the bound is missed by a NaN."""
    r = (got.double() - ref).abs() / bound
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    r = torch.where((got.double() == ref), torch.zeros_like(r), r)      # 0 / 0 on an exact element of bound 0
    return float(r.max()) if r.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------------- f32 emulation
def _lanes(t, D):
    """[M, D] -> [M, NPL, 64]: [.., i, lane] is the i-th element lane `lane` holds (RowIO<NPL>::idx)."""
    M, n = t.shape[0], npl(D)
    if n % 4 == 0:
        return t.view(M, n // 4, 64, 4).permute(0, 1, 3, 2).reshape(M, n, 64)
    return t.view(M, n, 64)


def _unlanes(v, D):
    M, n = v.shape[0], npl(D)
    if n % 4 == 0:
        return v.view(M, n // 4, 4, 64).permute(0, 1, 3, 2).reshape(M, D)
    return v.reshape(M, D)


def _wave_sum(v):
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    return v[:, 0]


def _seq(v):
    s = torch.zeros_like(v[:, 0])
    for i in range(v.shape[1]):
        s = s + v[:, i]
    return s


def emulate_forward(x, gamma, beta, D, eps=EPS, inv_d=None, drop=None):
    """ln_fwd_kernel in f32 torch: (mean, rstd, y) float32. inv_d: another 1/D (fault model); drop: the element left out of the mean."""
    inv = torch.tensor(1.0 / D if inv_d is None else inv_d, dtype=F32)
    v = _lanes(x.float(), D)
    vs = v
    if drop is not None:
        vs = _lanes(torch.cat([x[:, :drop], torch.zeros_like(x[:, :1]), x[:, drop + 1:]], 1).float(), D)
    mu = _wave_sum(_seq(vs)) * inv
    c = v - mu[:, None, None]
    rs = torch.rsqrt(_wave_sum(_seq(c * c)) * inv + torch.tensor(eps, dtype=F32))
    y = c * rs[:, None, None] * _lanes(gamma.float()[None], D) + _lanes(beta.float()[None], D)
    return mu, rs, _unlanes(y, D)


def emulate_backward(dy, x, gamma, mean, rstd, dres, D):
    """ln_bwd_kernel in f32 torch: dx float32 (before the store's rounding)."""
    inv = torch.tensor(1.0 / D, dtype=F32)
    mu, rs = mean.float()[:, None, None], rstd.float()[:, None, None]
    xh = (_lanes(x.float(), D) - mu) * rs
    gy = _lanes(dy.float(), D) * _lanes(gamma.float()[None], D)
    c1 = (_wave_sum(_seq(gy)) * inv)[:, None, None]
    c2 = (_wave_sum(_seq(gy * xh)) * inv)[:, None, None]
    out = rs * (gy - c1 - xh * c2)
    if dres is not None:
        out = out + _lanes(dres.float(), D)
    return _unlanes(out, D)


def emulate_forward_lora(x, gamma, beta, D, eps=EPS):
    """ln_fwd_lora_kernel's statistics in f32 torch (x bf16 values): lane kc of the four lanes of a row holds the 8-element chunks
    32 s + 8 kc, adds them pair by pair (sum += a + b), then two xor levels. (mean, rstd, y) float32."""
    M = x.shape[0]
    inv = torch.tensor(1.0 / D, dtype=F32)
    v = x.float().view(M, D // 32, 4, 4, 2)          # [M, s, kc, pair, half]
    s = torch.zeros(M, 4)
    for k in range(D // 32):
        for i in range(4):
            s = s + (v[:, k, :, i, 0] + v[:, k, :, i, 1])
    s = s + s[:, [1, 0, 3, 2]]
    s = s + s[:, [2, 3, 0, 1]]
    mu = s[:, 0] * inv
    c = v - mu[:, None, None, None, None]
    q = torch.zeros(M, 4)
    for k in range(D // 32):
        for i in range(4):
            a, b = c[:, k, :, i, 0], c[:, k, :, i, 1]
            q = q + (a * a + b * b)
    q = q + q[:, [1, 0, 3, 2]]
    q = q + q[:, [2, 3, 0, 1]]
    rs = torch.rsqrt(q[:, 0] * inv + torch.tensor(eps, dtype=F32))
    y = c.reshape(M, D) * rs[:, None] * gamma.float() + beta.float()
    return mu, rs, y


# ---------------------------------------------------------------------------------------------------------------- fault models
# Each turns the inputs of a correct call into what a kernel with one fault would have written (float32 / float64 tensors the host test
# holds against the same bounds and bands as the device test holds the kernels).
def neighbour_width(D):
    return WIDTHS[WIDTHS.index(D) - 1] if D != WIDTHS[0] else WIDTHS[1]


def fault_dropped_element(d, D):
    """The last element of every row left out of the sum of the mean."""
    return emulate_forward(d["x"], d["gamma"], d["beta"], D, drop=D - 1)


def fault_inv_d(d, D):
    """1 / D of the neighbouring width (a width dispatched to the wrong NPL's constant)."""
    return emulate_forward(d["x"], d["gamma"], d["beta"], D, inv_d=1.0 / neighbour_width(D))


def fault_row_stride(buf, first, M, D):
    """Row m read at first + m D of the flat buffer that holds x as a strided view (instead of first + m x_row_stride)."""
    return buf.as_strided((M, D), (D, 1), first)


def fault_trip_skipped(out, sentinel, rows_per_trip=ROWS_PER_TRIP):
    """The rows of the second grid-stride trip left as the output buffer held them."""
    out = out.clone()
    out[rows_per_trip:] = sentinel
    return out


def fault_dres_every_row(dx_wo_dres, dres_c, T):
    """Compact mode with the row test missing: every row m receives dres_c[m / T]."""
    M = dx_wo_dres.shape[0]
    return dx_wo_dres + dres_c[torch.arange(M) // T].to(dx_wo_dres.dtype)


def fault_drop_counter(keep_flat, M, D):
    """The dropout counter row * D where the call says row * drop_row_stride."""
    return keep_rows(keep_flat, M, D, D)


def fault_swapped_casts(x_bits, dres_bits, M, D, xdtype, sdtype):
    """The S and X casts of one line of the instantiation chain swapped: x's bytes read as the stream type and dres' bytes as x's type
    (the buffers are [M, D] of their own types; a wider read runs into what follows them, here NaN). Returns (x, dres) as float32."""
    def reread(t, as_dtype):
        raw = t.contiguous().view(torch.uint8).flatten()
        need = M * D * torch.empty(0, dtype=as_dtype).element_size()
        if raw.numel() < need:
            pad = torch.full((need - raw.numel(),), 0xFF, dtype=torch.uint8)      # 0xFFFF / 0xFFFFFFFF: NaN in every format
            raw = torch.cat([raw, pad])
        return raw[:need].view(as_dtype).view(M, D).float()
    return reread(x_bits, sdtype), reread(dres_bits, xdtype)


def fault_gmax_first_trip(dy, dx, rows_per_trip=ROWS_PER_TRIP):
    """gmax without the rows of the second trip."""
    return max(float(dy[:rows_per_trip].abs().max()), float(dx[:rows_per_trip].abs().max()))


def gmax_reference(dy, dx):
    return max(float(dy.abs().max()), float(dx.abs().max()))
