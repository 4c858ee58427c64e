"""Probes, references and fault models of the four patch gathers of csrc/patch.hip: gsl_patchify, gsl_patchify_u8, gsl_unfold_patches,
gsl_unfold_patches_u8 (tests/test_input_probes_host.py on the CPU, tests/test_hip_patch_edges.py on the device).

A gather computes nothing: every output element is one input element (or 0) in the stored format. So there is no tolerance here, only
bits. The references are written on the layout functions of torch (reshape / permute, torch.nn.functional.unfold); the host test holds
them against index arithmetic of a second kind (a four-loop gather, and gather_index() below).

References
  patchify_ref(img, p)                   einops' `b c (h p1) (w p2) -> b (h w) (p1 p2 c)` with a zero cls row per image: [B*T, p*p*C]
  unfold_ref(img, k, stride, pad, ldo)   F.unfold(...).transpose(1, 2), a zero cls row per image, zero K padding up to ldo: [B*T, ldo]
  store(ref32, dtype)                    the stored format: f32 as is, bf16 rounded to nearest even, fp16 with finite values clamped to
                                         +-65504 first (the saturating convert of csrc/gsl_common.h; Inf and NaN stay)
  u8_image(u, table)                     the float image a byte batch stands for: table[c][u], a lookup, whatever the table holds
The zeros of a cls row, a padding tap and the K padding are +0 by construction (torch.zeros, F.unfold's padding).

Inputs. make(case) builds everything from the case's seed. The f32 outputs are compared on the INDEX image: element i of the image holds
the integer i + 1 (at most 2^23 + 1 < 2^24, exact in f32; 0 never occurs), so every output element names its source pixel and a 0 is
a cls row, a padding tap or the K padding. The 16-bit outputs use the VALUE image (3 N(0, 1): integers above 2048 would collide in
11 or 8 bits of significand). Bytes come as `leak` bytes (drawn from the 255 values other than the guard bands' 0x5A: with
table[c][0x5A] = NaN a tap on a band byte is a NaN) and as `all` bytes (every byte value in every channel). Two tables: `affine`
((u / 255 - mean_c) / std_c with awkward means, so table[c][0] != 0: a padding zero is a zero, not the value of byte 0) and `arbitrary`
(random entries, no order, no relation between neighbours).

The case table. Shapes are the smallest that reach the path named; each row says what it reaches. Derived sizes:
  * a grid sweep of the patchify kernels is 4096 workgroups x 256 threads = 1048576 threads. The narrow thread map (one thread per
    (token, p1, p2)) runs B T p p threads: with C = 1, p = 4 that needs B T > 65536; one 1024 x 1024 image has T = 1 + 256 * 256 =
    65537: 1048592 threads, 16 in the second trip. The wide map of the u8 form (p % 8 == 0, C = 1 or 3: one thread per 8 pixels) runs
    B T p p / 8: with C = 1, p = 8 that needs B T > 131072; one 2048 x 4096 image has T = 1 + 256 * 512 = 131073: 1048584 threads, 8 in
    the second trip (the float form walks the same image in eight trips).
  * the row-count cases use k = 2, stride 1, no padding on an (Lh + 1) x (Lw + 1) image of one channel: B T = 1 * 31, 2 * 16, 3 * 11, 5 * 13.
  * the wide-row ladder: C = 3, k = 26 (2028 columns) at ldo 2040 / 2048 / 2056 (nch 255 / 256 / 257), k = 36 (3888) at 4096 (nch 512), on
    26 x 28 and 36 x 38 images with stride 2 and pad 1 (2 x 3 windows, padding taps on every side). Each runs once more with the zero
    fill 64 columns longer: 2104 / 2112 / 2120, and — 4096 + 64 is beyond the entry's limit of 4096 — 3952 = 3888 + 64 for k = 36.

Fault models (FAULTS): wrong restatements that return an output of the right shape; FAULT_TARGET names the case each is aimed at."""
import collections

import numpy as np
import torch
import torch.nn.functional as Fn

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = (F32, BF16, F16)
BAND_BYTE = 0x5A                      # tests/guard_bands.py SENTINEL[1]
UNF_ROWS = 32                         # csrc/patch.hip
GRID_SWEEP = 4096 * 256
U8_LDS_MAX_C = 16
SPECIALS = (65520.0, -1e6, float("inf"), float("-inf"), float("nan"), -0.0)

# op: "patchify" (a = p; stride, pad, ldo unused) or "unfold" (a = k). tags: "nonsquare" (also run through the Python wrappers),
# "sweep" (large: one placement only), "ladder"
Case = collections.namedtuple("Case", "name op B C H W a stride pad ldo tags")


def kpad(C, k, to=64):
    return -(-C * k * k // to) * to


def _p(name, B, C, H, W, p, tags=()):
    return Case(name, "patchify", B, C, H, W, p, 0, 0, 0, tuple(tags))


def _u(name, B, C, H, W, k, s, pad, ldo=None, tags=()):
    return Case(name, "unfold", B, C, H, W, k, s, pad, kpad(C, k) if ldo is None else ldo, tuple(tags))


TABLE = (
    _p("p_wide_16x24", 2, 3, 16, 24, 8, ["nonsquare"]),            # wide u8 form, H < W
    _p("p_wide_24x16", 2, 3, 24, 16, 8, ["nonsquare"]),            # wide u8 form, H > W
    _p("p_one_patch", 1, 1, 8, 8, 8),                              # one patch, wide C = 1
    _p("p_c4_narrow", 2, 4, 16, 8, 8),                             # p % 8 == 0 but C = 4: narrow form
    _p("p_narrow_12x20", 2, 2, 12, 20, 4, ["nonsquare"]),          # narrow form
    _p("p_odd_p3", 1, 3, 6, 9, 3, ["nonsquare"]),                  # odd p
    _p("p_p1", 1, 3, 3, 5, 1, ["nonsquare"]),                      # p = 1
    _p("p_c17_global", 1, 17, 4, 4, 2),                            # C > U8_LDS_MAX_C: the value table stays in global memory
    _p("p_p16", 1, 3, 32, 32, 16),                                 # p = 16: two 8-pixel segments per patch row
    _p("p_sweep_narrow", 1, 1, 1024, 1024, 4, ["sweep"]),          # narrow map, 16 threads in a second grid-stride trip
    _p("p_sweep_wide", 1, 1, 2048, 4096, 8, ["sweep"]),            # wide map, 8 threads in a second trip
    _u("u_20x28", 2, 3, 20, 28, 6, 4, 2, tags=["nonsquare"]),      # Lh = 5, Lw = 7
    _u("u_28x20", 2, 3, 28, 20, 6, 4, 2, tags=["nonsquare"]),      # Lh = 7, Lw = 5
    _u("u_stride_gt_k", 1, 1, 17, 13, 3, 5, 1, tags=["nonsquare"]),
    _u("u_stride1_padk1", 1, 3, 7, 9, 3, 1, 2, tags=["nonsquare"]),       # stride = 1, pad = k - 1
    _u("u_k1_nch1", 2, 3, 5, 6, 1, 1, 0, ldo=8, tags=["nonsquare"]),      # k = 1, one chunk per row; 5 x 6 x 3 x 2: NCHW image of 180 bytes
    _u("u_one_window", 3, 1, 4, 4, 4, 1, 0),                       # one window per image
    _u("u_nch5", 1, 2, 7, 7, 4, 3, 3, ldo=40),                     # nch odd; 98 bytes: no multiple of 8; C = 2 in NHWC
    _u("u_c4", 2, 4, 6, 5, 3, 2, 1, ldo=40, tags=["nonsquare"]),   # C = 4 in NHWC (added: the table above it has none), nch = 5
    _u("u_c17_global", 1, 17, 5, 5, 2, 1, 0),                      # C = 17: value table in global memory
    _u("u_rows31", 1, 1, 6, 7, 2, 1, 0, ldo=16),                   # B T = 31, 32, 33, 65 around UNF_ROWS
    _u("u_rows32", 2, 1, 4, 6, 2, 1, 0, ldo=16),
    _u("u_rows33", 3, 1, 3, 6, 2, 1, 0, ldo=16),
    _u("u_rows65", 5, 1, 4, 5, 2, 1, 0, ldo=16),
) + tuple(_u(f"u_ldo{ldo}", 2, 3, k, k + 2, k, 2, 1, ldo=ldo, tags=["ladder"])
          for k, ldo in ((26, 2040), (26, 2048), (26, 2056), (36, 4096), (26, 2104), (26, 2112), (26, 2120), (36, 3952)))
BY_NAME = {c.name: c for c in TABLE}
SATURATION = ("p_wide_16x24", "u_stride1_padk1")      # the cases that also run with SPECIALS planted
HOLE = _u("u_h32767", 1, 1, 32767, 8, 3, 1, 1, ldo=16)      # H + pad = 32768: the K-padding hole of gsl_unfold_patches (not in TABLE: one test of its own)


def geometry(case):
    """(T, row length) of the output."""
    if case.op == "patchify":
        return 1 + (case.H // case.a) * (case.W // case.a), case.a * case.a * case.C
    Lh, Lw = (case.H + 2 * case.pad - case.a) // case.stride + 1, (case.W + 2 * case.pad - case.a) // case.stride + 1
    return 1 + Lh * Lw, case.ldo


def seed_of(case):
    return 7919 * case.B + 104729 * case.C + 1009 * case.H + 31 * case.W + 17 * case.a + 5 * case.stride + 3 * case.pad + case.ldo


# ---------------------------------------------------------------------------------------------------------------- references
def patchify_ref(img, p):
    B, C, H, W = img.shape
    hp, wp = H // p, W // p
    x = img.reshape(B, C, hp, p, wp, p).permute(0, 2, 4, 3, 5, 1).reshape(B, hp * wp, p * p * C)
    return torch.cat([torch.zeros(B, 1, p * p * C, dtype=img.dtype), x], 1).reshape(B * (1 + hp * wp), p * p * C)


def unfold_ref(img, k, stride, pad, ldo):
    B, C = img.shape[:2]
    x = Fn.unfold(img, k, padding=pad, stride=stride).transpose(1, 2)          # [B, L, C k k]
    out = torch.zeros(B, 1 + x.shape[1], ldo, dtype=img.dtype)
    out[:, 1:, :C * k * k] = x
    return out.reshape(-1, ldo)


def reference(case, img):
    return patchify_ref(img, case.a) if case.op == "patchify" else unfold_ref(img, case.a, case.stride, case.pad, case.ldo)


def store(ref32, dtype):
    if dtype == F32:
        return ref32
    if dtype == BF16:
        return ref32.to(BF16)
    return torch.where(torch.isfinite(ref32), ref32.clamp(-65504.0, 65504.0), ref32).to(F16)


def bits(t):
    """The storage as integers, every NaN as one pattern (the converts are free in the payload they give a NaN)."""
    i = t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)
    return torch.where(torch.isnan(t), torch.full_like(i, -1), i)


def u8_image(u, table):
    C = u.shape[1]
    return table[torch.arange(C)[None, :, None, None], u.long()]


# ---------------------------------------------------------------------------------------------------------------- inputs
def index_image(case):
    n = case.B * case.C * case.H * case.W
    assert n + 1 < 2 ** 24
    return torch.arange(1, n + 1, dtype=F32).reshape(case.B, case.C, case.H, case.W)


def value_image(case, specials=False):
    g = torch.Generator().manual_seed(seed_of(case))
    x = 3.0 * torch.randn(case.B, case.C, case.H, case.W, generator=g)
    if specials:
        plant(x.view(-1), g)
    return x


def plant(flat, g):
    """SPECIALS at known places: the first and the last element and random ones between."""
    n = flat.numel()
    at = torch.cat([torch.tensor([0, n - 1]), torch.randperm(n - 2, generator=g)[:2 * len(SPECIALS) - 2] + 1])
    flat[at] = torch.tensor(SPECIALS * 2)
    return at


def leak_bytes(case):
    g = torch.Generator().manual_seed(seed_of(case) + 1)
    u = torch.randint(0, 255, (case.B, case.C, case.H, case.W), generator=g)
    return (u + (u >= BAND_BYTE).long()).to(torch.uint8)            # 0 .. 255 without 0x5A


def all_bytes(case):
    """Random bytes with every value in every channel where the channel has 256 pixels, a ramp through as many as fit otherwise."""
    g = torch.Generator().manual_seed(seed_of(case) + 2)
    u = torch.randint(0, 256, (case.B, case.C, case.H, case.W), dtype=torch.uint8, generator=g)
    n = min(256, case.H * case.W)
    ramp = torch.arange(256, dtype=torch.uint8)
    u[0].reshape(case.C, -1)[:, :n] = ramp[:n]
    u[-1].reshape(case.C, -1)[:, -n:] = ramp.flip(0)[:n]
    return u


def affine_table(C):
    c = torch.arange(C, dtype=F32)
    mean, std = 0.1234567 + 0.0377 * c, 0.0371 + 0.29 * ((c * 7) % 5)
    return torch.arange(256, dtype=F32)[None, :].div(255).sub(mean[:, None]).div(std[:, None])


def arbitrary_table(C, seed, leak=True, specials=False):
    g = torch.Generator().manual_seed(seed + 3)
    t = 3.0 * torch.randn(C, 256, generator=g)
    t[:, 0] = 1.5 + torch.arange(C)                 # byte 0 is not 0
    if specials:
        for c in range(C):
            plant(t[c], g)
    if leak:
        t[:, BAND_BYTE] = float("nan")
    return t


def nhwc_bytes(u):
    """The decoder's [B, H, W, C] bytes of a [B, C, H, W] batch, flat."""
    return u.permute(0, 2, 3, 1).contiguous().reshape(-1)


def make(case, what):
    """what: "index" / "value" / "value_sat" -> the float image; "leak" / "all" / "leak_sat" -> (bytes [B, C, H, W], table [C, 256])."""
    if what == "index":
        return index_image(case)
    if what in ("value", "value_sat"):
        return value_image(case, what == "value_sat")
    if what == "all":
        return all_bytes(case), affine_table(case.C)
    return leak_bytes(case), arbitrary_table(case.C, seed_of(case), leak=True, specials=what == "leak_sat")


# ---------------------------------------------------------------------------------------------------------------- index arithmetic
def gather_index(case, fault=None):
    """The gather as explicit index arithmetic (numpy, no layout function of torch): for every output element the flat index of its source
    in the NCHW batch, -1 for a zero. `fault` (a name of FAULTS) restates it wrongly; the result keeps its shape and every index stays
    inside the batch (a real kernel would read next to it: here the index wraps around)."""
    B, C, H, W, a = case.B, case.C, case.H, case.W, case.a
    T, cols = geometry(case)
    b = np.arange(B)[:, None, None]
    t = np.arange(T - 1)[None, :, None]
    j = np.arange(cols)[None, None, :]
    HH, WW = (W, H) if fault == "hw_swapped" else (H, W)             # the extents the source index is built with
    if case.op == "patchify":
        hp, wp = H // a, W // a
        c, p2, p1 = j % C, (j // C) % a, j // (C * a)
        wdiv = hp if fault == "lw_for_lh" else wp
        h, w = (t // wdiv) * a + p1, (t % wdiv) * a + p2
        if fault == "one_stride_off":
            w = w + a
        ok = np.ones((B, T - 1, cols), bool)
        inside = (h < H) & (w < W)
    else:
        k, s, pad = a, case.stride, case.pad
        Lh, Lw = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
        wdiv = Lh if fault == "lw_for_lh" else Lw
        wh, ww = t // wdiv, t % wdiv
        if fault == "one_stride_off":
            ww = ww + 1
        c, kh, kw = j // (k * k), (j // k) % k, j % k
        ok = np.broadcast_to(j < C * k * k, (B, T - 1, cols)).copy()
        if fault == "kpad_copies_col0":
            c, kh, kw = np.where(j < C * k * k, c, 0), np.where(j < C * k * k, kh, 0), np.where(j < C * k * k, kw, 0)
            ok[:] = True
        h, w = wh * s - pad + kh, ww * s - pad + kw
        inside = (h >= 0) & (h < H) & (w >= 0) & (w < W)
        if fault == "pad_clamps":
            h, w, inside = np.clip(h, 0, H - 1), np.clip(w, 0, W - 1), np.ones_like(inside)
    src = ((b * C + c) * HH + h) * WW + w
    src = np.where(ok & inside, src % (B * C * H * W), -1)
    cls = src[:, :1] if fault == "cls_is_window0" else np.full((B, 1, cols), -1)
    return np.concatenate([cls, src], 1).reshape(B * T, cols)


def gather(case, img, fault=None):
    """The output of gather_index() on img: float32 [B*T, cols]."""
    idx = torch.from_numpy(gather_index(case, fault))
    flat = torch.cat([img.reshape(-1), torch.zeros(1, dtype=img.dtype)])      # index -1: the zero
    return flat[idx]


def four_loops(img, p):
    """gsl_patchify as the loops one would write first."""
    B, C, H, W = img.shape
    hp, wp = H // p, W // p
    out = torch.zeros(B, 1 + hp * wp, p * p * C, dtype=img.dtype)
    for b in range(B):
        for t in range(hp * wp):
            for p1 in range(p):
                for p2 in range(p):
                    out[b, 1 + t, (p1 * p + p2) * C:(p1 * p + p2 + 1) * C] = img[b, :, (t // wp) * p + p1, (t % wp) * p + p2]
    return out.reshape(-1, p * p * C)


# ---------------------------------------------------------------------------------------------------------------- fault models
def fault_nhwc_as_nchw(case, u, table):
    """The NHWC bytes gathered with the NCHW index (the layout flag ignored)."""
    wrong = nhwc_bytes(u).reshape(u.shape)
    return reference(case, u8_image(wrong, table))


def fault_last_chunk_dropped(out, sentinel=float("nan")):
    """The last 8 columns of every row left as the output buffer held them."""
    out = out.clone()
    out[:, -8:] = sentinel
    return out


def fault_last_block_dropped(out, sentinel=float("nan")):
    """The rows of the last block of UNF_ROWS left as the output buffer held them."""
    out = out.clone()
    out[(out.shape[0] - 1) // UNF_ROWS * UNF_ROWS:] = sentinel
    return out


FAULTS = ("hw_swapped", "lw_for_lh", "one_stride_off", "pad_clamps", "kpad_copies_col0", "cls_is_window0")      # of gather_index()
# the case(s) each fault model is aimed at (tests/test_input_probes_host.py shows that it changes an element there)
FAULT_TARGET = {
    "hw_swapped": ("p_wide_16x24", "p_wide_24x16", "u_20x28", "u_28x20"),
    "lw_for_lh": ("p_wide_16x24", "p_narrow_12x20", "u_20x28", "u_28x20", "u_stride_gt_k"),
    "one_stride_off": ("p_odd_p3", "u_stride_gt_k", "u_k1_nch1"),
    "pad_clamps": ("u_stride1_padk1", "u_nch5", "u_ldo2040"),
    "kpad_copies_col0": ("u_k1_nch1", "u_nch5", "u_ldo2040", "u_ldo3952"),
    "cls_is_window0": ("p_one_patch", "u_one_window", "u_rows33"),
    "nhwc_as_nchw": ("p_wide_16x24", "p_c4_narrow", "u_nch5", "u_c4"),
    "last_chunk_dropped": ("u_nch5", "u_k1_nch1", "u_ldo2056", "u_ldo4096"),
    "last_block_dropped": ("u_rows31", "u_rows33", "u_rows65", "u_ldo2048"),
}
