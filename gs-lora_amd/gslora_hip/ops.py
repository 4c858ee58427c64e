"""Thin torch-tensor wrappers over the C ABI (include/gslora_hip.h). PyTorch supplies device
memory and the stream; every FLOP of the step runs in libgslora_hip.so. No fallbacks."""
import collections
import ctypes

import torch

from . import _lib as L

# Longest sequence the attention entry points accept (include/gslora_hip.h, GSL_ATTN_MAX_T): a 32 x 32 patch grid plus the cls token.
ATTN_MAX_T = 1025


def check_num_tokens(model, T):
    """Refuse, at construction, a geometry whose token count the attention kernels do not serve."""
    if T > ATTN_MAX_T:
        raise NotImplementedError(f"{model}: this geometry gives {T} tokens per image; the gs-lora_amd attention kernels take at most "
                                  f"{ATTN_MAX_T} (GSL_ATTN_MAX_T: a 32 x 32 patch grid plus the cls token)")


LORA_MAX_RANK = 64      # the LoRA K segment of the GEMMs is 64 columns wide (PADK in vit_runner.py)


def check_lora_rank(model, rank, attention_site=False):
    """Refuse, at construction, a LoRA rank the 64-column LoRA K segment of the GEMMs does not hold."""
    if rank > LORA_MAX_RANK:
        raise NotImplementedError(f"{model}: lora_rank {rank} exceeds {LORA_MAX_RANK}, the width of the LoRA K segment of the gs-lora_amd "
                                  f"GEMMs (64 columns)")
    if attention_site and 3 * rank > LORA_MAX_RANK:
        raise NotImplementedError(f"{model}: 3 * lora_rank = {3 * rank} must not exceed {LORA_MAX_RANK} for lora_pos Attention: the q / k / v "
                                  f"adapters share the one 64-column LoRA K segment of the QKV GEMM (lora_rank <= {LORA_MAX_RANK // 3})")


DT = {torch.float32: L.F32, torch.bfloat16: L.BF16, torch.float16: L.F16}      # (fp16: MFMA operand format of the "fp16" mode; also the forward residual stream of both 16-bit modes)


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _need(*ts, rows_ok=False):
    """rows_ok: 2-D row slices / column blocks (unit inner stride) are accepted — the entry point takes the leading dimension."""
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("gslora_hip: tensors must live on a ROCm GPU (the HIP path has no CPU fallback)")
        if not (t.is_contiguous() or (rows_ok and t.dim() == 2 and t.stride(1) == 1)):
            raise RuntimeError("gslora_hip: tensors must be contiguous")


def code(dtype):
    try:
        return DT[dtype]
    except KeyError:
        raise RuntimeError(f"gslora_hip: unsupported compute dtype {dtype}")


F32_MODES = (None, "x3")      # how a GEMM multiplies float32 tensors: None = the exact-f32 kernels, "x3" = GSL_F32X3


def gemm_code(dtype, f32_mode=None):
    """The gsl_dtype of a gsl_gemm_nt call on tensors of `dtype` under `f32_mode`."""
    if f32_mode is None:
        return code(dtype)
    if f32_mode != "x3":
        raise ValueError(f"gslora_hip: unknown f32_mode {f32_mode!r}; allowed: {F32_MODES}")
    if dtype != torch.float32:
        raise RuntimeError(f"gslora_hip: f32_mode='x3' multiplies float32 tensors, not {dtype} (the 16-bit modes are matrix-core modes already)")
    return L.F32X3


def f32x3_split_reference(x):
    """The split rule of GSL_F32X3 (include/gslora_hip.h, gsl_dtype), restated on the host: x (float32 numpy array or CPU tensor) ->
    (hi, mid, lo), float32 arrays whose values are bf16-representable, with hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid) and
    bf16() = round to nearest even, saturating (a finite value that would round up to Inf, |x| >= 2^128 - 2^119, becomes the largest finite bf16:
    what the kernel's conversion does under the FP16_OVFL mode bit). Both subtractions are exact in f32, and hi + mid + lo == x bit for bit for 0 and
    every finite |x| >= 2^-110 (smaller magnitudes: to 2^-134 absolute, bf16's denormal grid). Inf and NaN stay themselves in hi, and mid = x - hi is
    then NaN — the flag the kernel keeps per operand row."""
    import numpy as np
    x = np.ascontiguousarray(x.numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float32)

    def bf16_rne(v):
        u = v.view(np.uint32).astype(np.uint64)
        r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
        r = np.where(np.isfinite(v) & ((r & 0x7FFFFFFF) == 0x7F800000), (r & 0x80000000) | 0x7F7F0000, r)              # finite overflow saturates
        r = np.where(np.isnan(v), (v.view(np.uint32) | np.uint32(0x00400000)) & np.uint32(0xFFFF0000), r)      # a NaN stays a (quiet) NaN
        return r.astype(np.uint32).view(np.float32)

    with np.errstate(invalid="ignore", over="ignore"):
        hi = bf16_rne(x)
        r1 = (x - hi).astype(np.float32)
        mid = bf16_rne(r1)
        lo = bf16_rne((r1 - mid).astype(np.float32))
    return hi, mid, lo


# the piece products GSL_F32X3 adds up, (piece of A, piece of W), and the five-product set without mid * mid (the yardstick of the tests: one product
# too few is visible at f32 accuracy)
F32X3_PRODUCTS = (("hi", "hi"), ("hi", "mid"), ("mid", "hi"), ("mid", "mid"), ("hi", "lo"), ("lo", "hi"))
F32X3_FIVE = tuple(p for p in F32X3_PRODUCTS if p != ("mid", "mid"))


def f32x3_product_reference(A, W, products=F32X3_PRODUCTS):
    """Host emulation of a piece-product set: sum over `products` of piece(A) @ piece(W)^T, accumulated in float64 (what the choice of products
    costs, without what an f32 accumulator adds). A [M, K], W [N, K] float32 -> float64 numpy [M, N]."""
    import numpy as np
    pa = dict(zip(("hi", "mid", "lo"), (t.astype(np.float64) for t in f32x3_split_reference(A))))
    pw = dict(zip(("hi", "mid", "lo"), (t.astype(np.float64) for t in f32x3_split_reference(W))))
    return sum(pa[a] @ pw[w].T for a, w in products)


# ---- uint8 image batches (gsl_patchify_u8 / gsl_unfold_patches_u8): ToTensor() + Normalize(mean, std) happen inside the gather
# named (mean, std) pairs: the face drivers use ToTensor() alone, the ImageNet-100 driver the ImageNet constants
INPUT_NORM_TOTENSOR = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
INPUT_NORM_IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
INPUT_NORMS = {"totensor": INPUT_NORM_TOTENSOR, "imagenet": INPUT_NORM_IMAGENET}


def u8_reference(u, mean, std):
    """The float32 image a uint8 batch stands for: ToTensor() then Normalize(mean, std), in torchvision's operation order. This expression
    is the definition; u8_norm_table() evaluates it for every (channel, byte) and the gathers look the result up."""
    mean = torch.as_tensor(mean, dtype=torch.float32, device=u.device)
    std = torch.as_tensor(std, dtype=torch.float32, device=u.device)
    return u.to(torch.float32).div(255).sub(mean[None, :, None, None]).div(std[None, :, None, None])


def u8_norm_table(mean, std):
    """[C, 256] float32 (host): row c holds u8_reference() of the bytes 0 .. 255 in channel c."""
    mean, std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
    if len(mean) != len(std) or not mean:
        raise ValueError(f"input norm: mean and std need one entry per channel, got {len(mean)} and {len(std)}")
    if any(v == 0.0 or v != v for v in std):
        raise ValueError(f"input norm: std must be non-zero, got {std}")
    u = torch.arange(256, dtype=torch.uint8).reshape(256, 1, 1, 1).expand(256, len(mean), 1, 1)
    return u8_reference(u, mean, std).reshape(256, len(mean)).t().contiguous()


def _u8_source(t):
    """(layout code, tensor the kernel can read) of one [B, C, H, W] uint8 batch: NCHW-contiguous bytes, or NHWC bytes (a tensor that is
    contiguous in torch.channels_last: what a decoder produces, permuted to the logical shape); anything else is copied to NCHW."""
    if t.is_contiguous():
        return L.U8_NCHW, t
    if t.is_contiguous(memory_format=torch.channels_last):
        return L.U8_NHWC, t
    return L.U8_NCHW, t.contiguous()


def _image_parts(img, table, what):
    parts = list(img) if isinstance(img, (tuple, list)) else [img]
    u8 = parts[0].dtype == torch.uint8
    if any((t.dtype == torch.uint8) != u8 for t in parts):
        raise ValueError(f"{what}: the batches of one call must be all uint8 or all float")
    if not u8:
        _need(*parts)
        return parts, None
    if table is None:
        raise RuntimeError(f"{what}: a uint8 image needs the [C, 256] value table of its normalisation (ops.u8_norm_table)")
    _need(table)
    if not all(t.is_cuda for t in parts):
        raise RuntimeError("gslora_hip: tensors must live on a ROCm GPU (the HIP path has no CPU fallback)")
    if table.dtype != torch.float32 or tuple(table.shape) != (parts[0].shape[1], 256):
        raise ValueError(f"{what}: the value table must be float32 [{parts[0].shape[1]}, 256], got {table.dtype} {tuple(table.shape)}")
    src = []
    for t in parts:
        lay, t = _u8_source(t)
        if t.data_ptr() % 8:      # (a view at an odd byte offset: the wide loads want 8-byte alignment)
            t = t.clone(memory_format=torch.preserve_format)
        src.append((lay, t))
    return parts, src


def _gather_parts(entry, parts, src, table, out, T, *geom):
    """The per-batch launches of patchify / unfold_patches: batch i lands in its row range of `out` (T rows per image) through `entry`
    (float images) or `entry`_u8 (bytes, their layout code and the value table in front of the same arguments)."""
    row = 0
    for i, t in enumerate(parts):
        if src is None:
            L.check(getattr(L.load(), entry)(_p(t), _p(out[row:]), t.shape[0], *geom, _stream()), entry)
        else:
            L.check(getattr(L.load(), entry + "_u8")(_p(src[i][1]), src[i][0], _p(table), _p(out[row:]), t.shape[0], *geom, _stream()),
                    entry + "_u8")
        row += t.shape[0] * T
    return out


def patchify(img, p, dtype, table=None):
    """img: one [B, C, H, W] batch or a list of batches of one image shape; the batches land in consecutive row ranges of the output.
    float32 batches are gathered as they are; uint8 batches (NCHW-contiguous or channels_last) are normalised through `table` on the way."""
    parts, src = _image_parts(img, table, "patchify")
    _, Cc, H, W = parts[0].shape
    T = 1 + (H // p) * (W // p)
    out = torch.empty(sum(t.shape[0] for t in parts) * T, p * p * Cc, device=parts[0].device, dtype=dtype)
    return _gather_parts("gsl_patchify", parts, src, table, out, T, Cc, H, W, p, code(dtype))


def unfold_geometry(H, W, k, stride, pad):
    """(Lh, Lw) windows of nn.Unfold(k, stride=stride, padding=pad) over an H x W image."""
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def unfold_patches(img, k, stride, pad, dtype, table=None):
    """nn.Unfold(k, stride, pad)(img).transpose(1, 2) with a zero cls row per image and the feature dimension zero-padded to a multiple
    of 64 (the patch GEMM's K): [B*T, Kpad], T = 1 + Lh*Lw, Kpad = ceil(C*k*k / 64)*64. img: one [B, C, H, W] batch or a list of batches
    of one image shape; the batches land in consecutive row ranges of the output. uint8 batches: as patchify (padding taps stay 0)."""
    parts, src = _image_parts(img, table, "unfold_patches")
    _, Cc, H, W = parts[0].shape
    Lh, Lw = unfold_geometry(H, W, k, stride, pad)
    T = 1 + Lh * Lw
    kpad = -(-Cc * k * k // 64) * 64
    out = torch.empty(sum(t.shape[0] for t in parts) * T, kpad, device=parts[0].device, dtype=dtype)
    return _gather_parts("gsl_unfold_patches", parts, src, table, out, T, Cc, H, W, k, stride, pad, kpad, code(dtype))


_ws_cache = {}
_ws_retired = []


def _workspace(key, need, device, floor=0):
    """The f32 scratch buffer of `key`, grown to `need` elements (at least `floor` when it is created or grown). A buffer that is
    outgrown is retired, never freed: a captured HIP graph may still launch with it."""
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < need:
        if ws is not None:
            _ws_retired.append(ws)
        ws = _ws_cache[key] = torch.empty(max(need, floor), device=device, dtype=torch.float32)
    return ws


# optional per-kernel timing hook used by bench.py: {tag: [(start_event, end_event), ...]} recorded on the
# stream the kernel is launched on (torch's current stream == the hipStream_t handed to the C ABI)
PROFILE = None


def _profiled(tag, shape_of):
    """bench.py: when PROFILE holds `tag`, bracket the launch with HIP events on the launch stream and record (ev0, ev1, *shape_of(args)).
    tag None: the tag is the call's own `tag=` keyword (the GEMM wrappers are tagged per call site; the fixed tags are the memory-bound
    kernels of the step: LayerNorm and attention)."""
    def deco(fn):
        def wrapped(*a, **kw):
            if PROFILE is None:
                return fn(*a, **kw)
            t = tag or kw.get("tag")
            if t not in PROFILE:
                return fn(*a, **kw)
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
            out = fn(*a, **kw)
            ev[1].record()
            PROFILE[t].append((ev[0], ev[1]) + tuple(shape_of(*a, **kw)))
            return out
        wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
        return wrapped
    return deco


def _gemm_shape(A, W, *a, A2=None, **kw):
    return A.shape[0], W.shape[0], A.shape[1], 0 if A2 is None else A2.shape[1]      # M, N, K1, K2


def gemm_tile_choice(M, N, K, dtype, has_out2=False, in_kernel_lora=False, f32_mode=None):
    """The kernel gemm_nt (or gemm_nt_lora) launches for this shape: one of _lib.TILE_* (gsl_gemm_tile_choice; K = K1 + K2)."""
    return int(L.load().gsl_gemm_tile_choice(int(M), int(N), int(K), gemm_code(dtype, f32_mode), 1 if has_out2 else 0, 1 if in_kernel_lora else 0))


def attention_kernel(B, T, H, dtype, layout=0, direction="fwd"):
    """The kernel(s) attention_fwd / attention_bwd / attention_fwd_cls / attention_bwd_cls (direction "fwd", "bwd", "cls_fwd", "cls_bwd")
    launch for this shape in the product library: one of _lib.ATTN_* (gsl_attention_kernel_choice), -1 where the entry point refuses."""
    return int(L.load().gsl_attention_kernel_choice(int(B), int(T), int(H), code(dtype), int(layout), L.ATTN_DIRECTIONS[direction]))


def _share_ldo(what, epilogue, out, res, aux, out2):
    """The kernels index res, the aux of EPI_MUL and the out2 of EPI_BIAS_GELU with the row stride of `out` (ldo): row slices and column
    blocks are accepted for them, a row stride that differs from out's is refused. Every other aux / out2 (the LayerNorm column vector,
    the 8-bit GELU' code tensor, the compact [M, 16] copy of STORE) has a layout of its own and must be contiguous."""
    with_ldo = {"res": res, "aux": aux if epilogue == L.EPI_MUL else None, "out2": out2 if epilogue == L.EPI_BIAS_GELU else None}
    _need(*(t for t in (res, aux, out2) if not any(t is v for v in with_ldo.values())))
    for name, t in with_ldo.items():
        if t is None:
            continue
        _need(t, rows_ok=True)
        if t.dim() < 2 or (t.numel() > t.shape[-1] and t.stride(-2) != out.stride(0)):
            raise RuntimeError(f"{what}: {name} and out must share one row stride (the kernel indexes {name} with out's leading dimension)")


@_profiled(None, _gemm_shape)
def gemm_nt(A1, W1, out, *, epilogue=L.EPI_STORE, A2=None, W2=None, alpha=1.0, bias=None, res=None, aux=None, out2=None,
            pos=None, cls=None, T=0, p_drop=0.0, seed=0, site=0, tag=None, f32_mode=None):
    """f32_mode: None, or "x3" — float32 tensors only: the products as three bf16 pieces per operand on the bf16 matrix cores (GSL_F32X3;
    f32x3_split_reference states the split). Same tensors, epilogues and dropout masks as the exact-f32 call."""
    _need(bias, pos, cls)
    _need(A1, W1, A2, W2, out, rows_ok=True)      # lda / ldw of both K segments and ldo travel with the call
    _share_ldo("gemm_nt", epilogue, out, res, aux, out2)
    M, K1 = A1.shape
    N = W1.shape[0]
    K2 = 0 if A2 is None else A2.shape[1]
    L.check(L.load().gsl_gemm_nt(_p(A1), A1.stride(0), _p(W1), W1.stride(0), K1, _p(A2), 0 if A2 is None else A2.stride(0),
                                 _p(W2), 0 if W2 is None else W2.stride(0), K2, M, N, gemm_code(A1.dtype, f32_mode), epilogue, float(alpha),
                                 _p(bias), _p(res), _p(aux), _p(out), _p(out2), out.stride(0), _p(pos), _p(cls), int(T),
                                 float(p_drop), int(seed), int(site), _stream()), "gsl_gemm_nt")
    return out


@_profiled(None, _gemm_shape)
def gemm_nt_lora(A, W, P, Q, lora_scale, tout, out, *, epilogue=L.EPI_STORE, bias=None, res=None, aux=None, out2=None, p_drop=0.0,
                 seed=0, site=0, tag=None):
    """out = epilogue(A W^T + t Q^T), t = lora_scale * A P^T computed inside the kernel and stored to tout [M,64] (bf16)."""
    _need(P, Q, tout, bias)
    _need(A, W, out, rows_ok=True)
    _share_ldo("gemm_nt_lora", epilogue, out, res, aux, out2)
    M, K = A.shape
    N = W.shape[0]
    L.check(L.load().gsl_gemm_nt_lora(_p(A), A.stride(0), _p(W), W.stride(0), K, _p(P), P.stride(0), _p(Q), Q.stride(0),
                                      float(lora_scale), _p(tout), 0 if tout is None else tout.stride(0), M, N, code(A.dtype), epilogue,
                                      _p(bias), _p(res), _p(aux), _p(out), _p(out2), out.stride(0), float(p_drop), int(seed), int(site),
                                      _stream()), "gsl_gemm_nt_lora")
    return out


@_profiled(None, _gemm_shape)
def gemm_nt_lora_mulgrad(A, W, P, Q, lora_scale, tout, out, aux, U1, G1, g1s, Y2, G2, g2s, r, accumulate=True, tag=None, p_drop=0.0, gscale=None):
    """out = (A W^T + t Q^T) * aux with t = lora_scale * A P^T (as gemm_nt_lora, epilogue MUL) and, from the same tiles,
    G1[n*g1s[0] + j*g1s[1]] (+)= sum_m out[m,n] U1[m,j] and G2[n*g2s[0] + j*g2s[1]] (+)= sum_m Y2[m,n] t[m,j].
    A uint8 aux is the 8-bit GELU' code of EPI_BIAS_GELU_G8; p_drop is then the dropout rate of the forward that wrote it.
    gscale: device {S, 1/S} of a loss-scaled (fp16) backward — G1 / G2 receive the sums multiplied by 1/S."""
    aux_u8 = aux.dtype == torch.uint8
    _need(P, Q, tout, gscale)
    _need(A, W, out, U1, Y2, rows_ok=True)      # row slices / column blocks: lda, ldw, ldo (out, aux and Y2 share it) and ldu1 travel with the call
    _need(aux, rows_ok=not aux_u8)               # the 8-bit code tensor is slab-major [N/64][M][64] whatever ldo is: contiguous, no row stride to share
    M, K = A.shape
    N = W.shape[0]
    if aux_u8 and aux.numel() != M * N:
        raise RuntimeError("gemm_nt_lora_mulgrad: the 8-bit aux is the code tensor of EPI_BIAS_GELU_G8, M * N bytes")
    if not (out.stride(0) == Y2.stride(0) and (aux_u8 or aux.stride(0) == out.stride(0)) and U1.stride(1) == 1):
        raise RuntimeError("gemm_nt_lora_mulgrad: out / aux / Y2 must share one row stride")
    lib = L.load()
    need = lib.gsl_gemm_mulgrad_ws_elems(M, N, r)
    ws = _workspace((A.device.index, "mulgrad"), need, A.device)
    L.check(lib.gsl_gemm_nt_lora_mulgrad(_p(A), A.stride(0), _p(W), W.stride(0), K, _p(P), P.stride(0), _p(Q), Q.stride(0),
                                         float(lora_scale), _p(tout), 0 if tout is None else tout.stride(0), M, N, _p(aux), _p(out),
                                         out.stride(0), _p(U1), U1.stride(0), G1.data_ptr(), g1s[0], g1s[1], _p(Y2), G2.data_ptr(),
                                         g2s[0], g2s[1], r, 1 if accumulate else 0, _p(ws), 1 if aux.dtype == torch.uint8 else 0,
                                         float(p_drop), code(A.dtype), _p(gscale), _stream()), "gsl_gemm_nt_lora_mulgrad")
    return out


@_profiled("ln_fwd", lambda x, row_stride, M, D, *a, **k: (M, D, 0, 0))
def layernorm_fwd(x, row_stride, M, D, gamma, beta, eps, dtype):
    """x: the residual stream, f32 or (bf16 mode) bf16 — its dtype is handed to the kernel."""
    _need(x, gamma, beta)
    y = torch.empty(M, D, device=x.device, dtype=dtype)
    mean = torch.empty(M, device=x.device, dtype=torch.float32)
    rstd = torch.empty(M, device=x.device, dtype=torch.float32)
    L.check(L.load().gsl_layernorm_fwd(_p(x), row_stride, _p(gamma), _p(beta), float(eps), _p(y), _p(mean), _p(rstd), M, D,
                                       code(dtype), code(x.dtype), _stream()), "gsl_layernorm_fwd")
    return y, mean, rstd


@_profiled("ln_stats", lambda x, row_stride, M, D, *a, **k: (M, D, 0, 0))
def layernorm_stats(x, row_stride, M, D, gamma, beta, eps, dtype):
    """(mean, rstd) of the rows of x — gsl_layernorm_fwd without its output: the row statistics a GEMM with a consumer-side LayerNorm
    (EPI_STORE_LN) finishes the normalisation with, and what the LayerNorm backward needs. One read of x, no write of LN(x)."""
    _need(x, gamma, beta)
    mean = torch.empty(M, device=x.device, dtype=torch.float32)
    rstd = torch.empty(M, device=x.device, dtype=torch.float32)
    L.check(L.load().gsl_layernorm_fwd(_p(x), row_stride, _p(gamma), _p(beta), float(eps), None, _p(mean), _p(rstd), M, D,
                                       code(dtype), code(x.dtype), _stream()), "gsl_layernorm_fwd(stats)")
    return mean, rstd


def layernorm_fwd_lora(x, row_stride, M, D, gamma, beta, eps, P, alpha, pad=64):
    """bf16 mode: (LN(x), mean, rstd, u) with u = alpha * LN(x) P[:16]^T in a [M, 64] K-segment buffer (columns >= 16 zero): LayerNorm and
    the LoRA down-projection of the layer that consumes it in one pass over x (gsl_layernorm_fwd_lora)."""
    _need(x, gamma, beta, P)
    if x.dtype != torch.bfloat16 or P.dtype != torch.bfloat16 or P.shape[0] < 16 or P.shape[1] != D or pad != 64:
        raise ValueError("layernorm_fwd_lora: bf16 x, P [>= 16, D] bf16, 64-column u")
    y = torch.empty(M, D, device=x.device, dtype=torch.bfloat16)
    u = torch.empty(M, pad, device=x.device, dtype=torch.bfloat16)
    mean = torch.empty(M, device=x.device, dtype=torch.float32)
    rstd = torch.empty(M, device=x.device, dtype=torch.float32)
    L.check(L.load().gsl_layernorm_fwd_lora(_p(x), row_stride, _p(gamma), _p(beta), float(eps), _p(y), _p(mean), _p(rstd), M, D,
                                            _p(P), P.stride(0), float(alpha), _p(u), _stream()), "gsl_layernorm_fwd_lora")
    return y, mean, rstd, u


@_profiled("ln_bwd", lambda dy, *a, **k: (dy.shape[0], dy.shape[1], 0, 0))
def layernorm_bwd(dy, x, row_stride, gamma, mean, rstd, dres, want_copy=True, p_drop=0.0, seed=0, site=0, dx=None,
                  io_row_stride=0, drop_row_stride=0, dres_cls_T=0, gmax=None):
    """dx = dres + LN'(dy). gmax: f32 device element (gscale[2:] of head_bwd) raised to the largest |dy| read / |dx| stored: the overflow guard. With dx given (and io_row_stride), the rows of an existing buffer are updated in place. The dtype of the
    residual-gradient stream (dres / dx: f32, or bf16 in bf16 mode) is taken from dres / dx, the dtype of the saved forward stream from x.
    dres_cls_T > 0: dres holds the cls rows only ([M / T, D]); the other rows of the incoming stream gradient are zero."""
    _need(dy, x, gamma, mean, rstd)
    M, D = dy.shape
    sdt = dx.dtype if dx is not None else (dres.dtype if dres is not None else torch.float32)
    own_dx = dx is None
    if dx is None:
        _need(dres)
        dx = torch.empty(M, D, device=dy.device, dtype=sdt)
    elif dres is not None and dres.dtype != dx.dtype:
        raise RuntimeError("layernorm_bwd: dres and dx must share one dtype")
    # the masked operand copy IS dx when no mask applies (dropout 0: ViT-B/16, eval-free training runs) and the stream already has the
    # operand dtype: one [M, D] write less per LayerNorm backward
    alias = bool(want_copy) and float(p_drop) == 0.0 and sdt == dy.dtype and own_dx and not io_row_stride
    dxb = torch.empty(M, D, device=dy.device, dtype=dy.dtype) if (want_copy and not alias) else None
    L.check(L.load().gsl_layernorm_bwd(_p(dy), _p(x), row_stride, _p(gamma), _p(mean), _p(rstd), _p(dres), _p(dx),
                                       int(io_row_stride), _p(dxb), M, D, code(dy.dtype), code(sdt), code(x.dtype), float(p_drop),
                                       int(seed), int(site), int(drop_row_stride), int(dres_cls_T), _p(gmax), _stream()), "gsl_layernorm_bwd")
    return dx, (dx if alias else dxb)


@_profiled("attn_fwd", lambda qkv, B, T, H, *a, **k: (B * T, H * 64, T, H))
def attention_fwd(qkv, B, T, H, scale, layout=0):
    """layout: 0 = qkv token-major [B*T, 3*H*64], 1 = head-major [B][H][3][T][64] (bf16; see gemm_nt(epilogue=EPI_STORE_QKV_HM)).
    2 <= T <= ATTN_MAX_T: up to 224 tokens one LDS panel holds an item's K / V; above, 64-key panels stream with an online softmax.
    o [B*T, H*64] token-major, lse f32 [B, H, T] (natural-log logsumexp of the scaled scores) in both regimes."""
    _need(qkv)
    o = torch.empty(B * T, H * 64, device=qkv.device, dtype=qkv.dtype)
    lse = torch.empty(B, H, T, device=qkv.device, dtype=torch.float32)
    L.check(L.load().gsl_attention_fwd(_p(qkv), _p(o), _p(lse), B, T, H, float(scale), code(qkv.dtype), int(layout), _stream()),
            "gsl_attention_fwd")
    return o, lse


@_profiled("attn_bwd", lambda qkv, o, d_o, lse, B, T, H, *a, **k: (B * T, H * 64, T, H))
def attention_bwd(qkv, o, d_o, lse, B, T, H, scale, layout=0):
    """dqkv is token-major [B*T, 3*H*64] whatever the layout of the qkv input. 2 <= T <= ATTN_MAX_T; deterministic (no atomics) at
    every T. `delta` [B, H, T] is the rowsum(dO o) hand-off between the dQ and the dK / dV kernels of the split forms (T <= 64, T > 224)."""
    _need(qkv, o, d_o, lse)
    dqkv = torch.empty_like(qkv)
    delta = torch.empty(B, H, T, device=qkv.device, dtype=torch.float32)
    L.check(L.load().gsl_attention_bwd(_p(qkv), _p(o), _p(d_o), _p(lse), _p(dqkv), _p(delta), B, T, H, float(scale),
                                       code(qkv.dtype), int(layout), _stream()), "gsl_attention_bwd")
    return dqkv


def attention_fwd_cls(qkv, B, T, H, scale, layout=0, q_cls=None):
    """Attention output of the cls query alone (the last block under pool='cls'): o_cls [B, H*64], lse_cls [B, H].
    layout 2: `qkv` is kv [B*T, 2*H*64] (k | v, token-major) and q_cls [B, H*64] holds the queries. 2 <= T <= ATTN_MAX_T (above 256
    keys the softmax runs over 256-key chunks with an online max / sum)."""
    _need(qkv, q_cls)
    o = torch.empty(B, H * 64, device=qkv.device, dtype=qkv.dtype)
    lse = torch.empty(B, H, device=qkv.device, dtype=torch.float32)
    L.check(L.load().gsl_attention_fwd_cls(_p(qkv), _p(q_cls), _p(o), _p(lse), B, T, H, float(scale), code(qkv.dtype), int(layout),
                                           _stream()), "gsl_attention_fwd_cls")
    return o, lse


def attention_bwd_cls(qkv, o, d_o_cls, lse, B, T, H, scale, layout=0, q_cls=None):
    """o / lse: either the full forward tensors ([B*T, H*64] / [B, H, T]) or the compact ones of attention_fwd_cls ([B, H*64] / [B, H]).
    layout 0 / 1 -> dqkv [B*T, 3*H*64]; layout 2 (kv + q_cls) -> (dkv [B*T, 2*H*64], dq_cls [B, H*64]). Any T >= 2 (it walks the keys
    in steps of 32)."""
    _need(qkv, o, d_o_cls, lse, q_cls)
    nw = 2 if layout == 2 else 3
    dqkv = torch.empty(B * T, nw * H * 64, device=qkv.device, dtype=qkv.dtype)
    dq = torch.empty(B, H * 64, device=qkv.device, dtype=qkv.dtype) if layout == 2 else None
    compact = o.shape[0] == B and lse.dim() == 2
    L.check(L.load().gsl_attention_bwd_cls(_p(qkv), _p(q_cls), _p(o), _p(d_o_cls), _p(lse), _p(dqkv), _p(dq), B, T, H, float(scale),
                                           code(qkv.dtype), int(layout), 1 if compact else 0, _stream()), "gsl_attention_bwd_cls")
    return (dqkv, dq) if layout == 2 else dqkv




def lora_grad(Y, U, G, gsn, gsj, r, accumulate=True, gscale=None):
    """G[n*gsn + j*gsj] (+)= sum_m Y[m,n] U[m,j]; G is a view into the flat f32 gradient bucket. Y / U may be column blocks of wider
    row-major tensors (unit column stride). gscale: device {S, 1/S} of a loss-scaled (fp16) backward: the sum is multiplied by 1/S."""
    if not (Y.is_cuda and U.is_cuda and Y.stride(1) == 1 and U.stride(1) == 1):
        raise RuntimeError("lora_grad: operands must be CUDA tensors with unit column stride")
    M, N = Y.shape
    lib = L.load()
    need = lib.gsl_lora_grad_ws_elems(M, N, r)
    ws = _workspace((Y.device.index,), need, Y.device, floor=1 << 22)
    L.check(lib.gsl_lora_grad(_p(Y), Y.stride(0), _p(U), U.stride(0), G.data_ptr(), gsn, gsj, M, N, r, code(Y.dtype),
                              1 if accumulate else 0, _p(ws), _p(gscale), _stream()), "gsl_lora_grad")


class _LgradDesc(ctypes.Structure):      # mirrors struct gsl_lgrad_desc (include/gslora_hip.h), 72 bytes
    _fields_ = [("Y", ctypes.c_void_p), ("ldy", ctypes.c_long), ("U", ctypes.c_void_p), ("ldu", ctypes.c_int), ("M", ctypes.c_int),
                ("N", ctypes.c_int), ("r", ctypes.c_int), ("accumulate", ctypes.c_int), ("pad_", ctypes.c_int), ("G", ctypes.c_void_p),
                ("gsn", ctypes.c_long), ("gsj", ctypes.c_long)]


class _LgradPlan(ctypes.Structure):      # mirrors struct gsl_lgrad_plan
    _fields_ = [(n, ctypes.c_int) for n in ("form", "R", "bx", "nsplit", "rps", "CG", "reduce")]


class _LgradBatchPlan(ctypes.Structure):      # mirrors struct gsl_lgrad_batch_plan
    _fields_ = [(n, ctypes.c_int) for n in ("R", "bx", "nsplit", "rps")]


LgradPlan = collections.namedtuple("LgradPlan", "form R bx nsplit rps CG reduce")
LgradBatchPlan = collections.namedtuple("LgradBatchPlan", "R bx nsplit rps")
_PLAN_ADDR = 1 << 20      # the made-up, 16-byte aligned operand address of a plan asked for by shape


def lora_grad_plan_args(M, N, r, dtype, ldy=None, ldu=64, y_addr=_PLAN_ADDR, u_addr=_PLAN_ADDR):
    """How gsl_lora_grad runs a call with these operand arguments (gsl_lora_grad_plan: host code, no device needed, nothing is dereferenced):
    form / reduce are _lib.LGRAD_*. Raises RuntimeError where the launch refuses, with the launch's message."""
    out = _LgradPlan()
    L.check(L.load().gsl_lora_grad_plan(y_addr, N if ldy is None else ldy, u_addr, ldu, M, N, r, code(dtype), ctypes.byref(out)), "gsl_lora_grad_plan")
    return LgradPlan(*(getattr(out, n) for n in LgradPlan._fields))


def lora_grad_plan(Y, U, r):
    """The plan of lora_grad(Y, U, G, ..., r) on these very tensors (their strides and addresses count)."""
    return lora_grad_plan_args(Y.shape[0], Y.shape[1], r, Y.dtype, Y.stride(0), U.stride(0), Y.data_ptr(), U.data_ptr())


def _lgrad_descs(entries):
    """entries as for lora_grad_batch — or (M, N, r) shapes, placed at made-up aligned addresses with dense Y and a 64-wide U."""
    arr = (_LgradDesc * len(entries))()
    for k, e in enumerate(entries):
        if isinstance(e[0], int):
            M, N, r = e
            arr[k] = _LgradDesc(_PLAN_ADDR, N, _PLAN_ADDR, 64, M, N, r, 0, 0, _PLAN_ADDR, r, 1)
        else:
            Y, U, G, gsn, gsj, r, acc = e
            arr[k] = _LgradDesc(Y.data_ptr(), Y.stride(0), U.data_ptr(), U.stride(0), Y.shape[0], Y.shape[1], r, 1 if acc else 0, 0,
                                G.data_ptr(), gsn, gsj)
    return arr


def lora_grad_batch_plan(entries):
    """Per entry of lora_grad_batch(entries): (R, bx, nsplit, rps) of its aligned MFMA body (gsl_lora_grad_batch_plan, host code)."""
    arr = _lgrad_descs(entries)
    out = (_LgradBatchPlan * len(entries))()
    L.check(L.load().gsl_lora_grad_batch_plan(arr, len(entries), out), "gsl_lora_grad_batch_plan")
    return [LgradBatchPlan(o.R, o.bx, o.nsplit, o.rps) for o in out]


def lora_grad_batchable(Y, U, r):
    """Can this reduction ride in gsl_lora_grad_batch (16-bit MFMA form: 256-column blocks, 16-byte rows)? The form reads columns 0..15
    of U up to rank 16 and the 8-column chunks [0, 8 * ceil(r / 8)) above: a row of U must be at least that long."""
    ucols = 16 if r <= 16 else -(-r // 8) * 8
    return (Y.dtype in (torch.bfloat16, torch.float16) and U.dtype == Y.dtype and Y.is_cuda and Y.stride(1) == 1 and U.stride(1) == 1
            and Y.shape[1] % 256 == 0 and Y.stride(0) % 8 == 0 and U.stride(0) % 8 == 0 and U.stride(0) >= ucols and 1 <= r <= LORA_MAX_RANK
            and Y.data_ptr() % 16 == 0 and U.data_ptr() % 16 == 0)


def lora_grad_batch(entries, gscale=None):
    """entries: [(Y, U, G, gsn, gsj, r, accumulate)] as for lora_grad — all of them in two launches (gsl_lora_grad_batch). The
    descriptors travel in the kernel arguments: nothing to keep alive on the host, HIP-graph capture friendly."""
    if not entries:
        return
    assert ctypes.sizeof(_LgradDesc) == 72
    arr = _lgrad_descs(entries)
    lib = L.load()
    need = lib.gsl_lora_grad_batch_ws_elems(arr, len(entries))
    if need < 0:
        L.check(int(need), "gsl_lora_grad_batch_ws_elems")
    dev = entries[0][0].device
    ws = _workspace((dev.index,), need, dev, floor=1 << 22)
    L.check(lib.gsl_lora_grad_batch(arr, len(entries), _p(ws), code(entries[0][0].dtype), _p(gscale), _stream()), "gsl_lora_grad_batch")


def _tail14(out):
    """The 14 floats every form of the scalar tail writes -> (total [0-dim], meters [8], coefs [5])."""
    return out[0], out[1:9], out[9:14]


def loss_combine(ce_r_sum, ce_f_sum, kl_f_sum, kl_r_sum, structure, hit_r, hit_f, n_r, n_f, beta, BND, alpha, w_f, w_r, BND_pro):
    """-> (total [0-dim], meters [8], coefs [5]) — see gsl_loss_combine."""
    _need(ce_r_sum, ce_f_sum, kl_f_sum, kl_r_sum, structure, hit_r, hit_f)
    dev = ce_r_sum.device
    out = torch.empty(14, device=dev, dtype=torch.float32)
    L.check(L.load().gsl_loss_combine(_p(ce_r_sum), _p(ce_f_sum), _p(kl_f_sum), _p(kl_r_sum), _p(structure), _p(hit_r), _p(hit_f),
                                      float(n_r), float(n_f), float(beta), float(BND), float(alpha), float(w_f), float(w_r),
                                      float(BND_pro), out.data_ptr(), out.data_ptr() + 4, out.data_ptr() + 36, _stream()),
            "gsl_loss_combine")
    return _tail14(out)


def loss_tail_max_rows():
    return int(L.load().gsl_loss_tail_max_rows())


def _loss_tail(entry, logits, labels, nr, emb, proto, structure, beta, BND, alpha, w_f, w_r, BND_pro):
    """gsl_loss_tail or gsl_loss_tail_l2 (same arguments): -> (total, meters [8], coefs [5], dlogits, demb or None)."""
    _need(logits, labels, emb, proto, structure)
    N, C = logits.shape
    out = torch.empty(14, device=logits.device, dtype=torch.float32)
    dlogits = torch.empty_like(logits)
    demb = None if emb is None else torch.empty_like(emb)
    L.check(getattr(L.load(), entry)(_p(logits), _p(labels), N, int(nr), C, _p(emb), _p(proto), 0 if emb is None else emb.shape[1],
                                     0 if proto is None else proto.shape[0], _p(structure), float(beta), float(BND), float(alpha), float(w_f),
                                     float(w_r), float(BND_pro), _p(out), _p(dlogits), _p(demb), _stream()), entry)
    return _tail14(out) + (dlogits, demb)


def loss_tail(logits, labels, nr, emb, proto, structure, beta, BND, alpha, w_f, w_r, BND_pro):
    """The loss section of a single-process step in one launch (gsl_loss_tail): -> (total, meters [8], coefs [5], dlogits, demb or None)."""
    return _loss_tail("gsl_loss_tail", logits, labels, nr, emb, proto, structure, beta, BND, alpha, w_f, w_r, BND_pro)


def loss_tail_l2(logits, labels, nr, emb, proto, structure, beta, BND, alpha, w_f, w_r, BND_pro):
    """loss_tail with the l2 prototype distance (gsl_loss_tail_l2; the prototype term is required): same five results."""
    if emb is None or proto is None:
        raise RuntimeError("gslora_hip: loss_tail_l2 needs the embeddings and the prototype table (without a prototype term use loss_tail)")
    return _loss_tail("gsl_loss_tail_l2", logits, labels, nr, emb, proto, structure, beta, BND, alpha, w_f, w_r, BND_pro)


def loss_combine_pack(pack8, structure, has_proto, beta, BND, alpha, w_f, w_r, BND_pro):
    """Data-parallel scalar tail from the all-reduced 8-float pack -> (total [0-dim], meters [8], coefs [5]) — see gsl_loss_combine_pack."""
    _need(pack8, structure)
    out = torch.empty(14, device=pack8.device, dtype=torch.float32)
    L.check(L.load().gsl_loss_combine_pack(_p(pack8), _p(structure), 1 if has_proto else 0, float(beta), float(BND), float(alpha),
                                           float(w_f), float(w_r), float(BND_pro), out.data_ptr(), out.data_ptr() + 4,
                                           out.data_ptr() + 36, _stream()), "gsl_loss_combine_pack")
    return _tail14(out)


def cosface_prep(W):
    _need(W)
    Wn = torch.empty_like(W)
    L.check(L.load().gsl_cosface_prep(_p(W), _p(Wn), W.shape[0], W.shape[1], _stream()), "gsl_cosface_prep")
    return Wn


HEAD_KINDS = {"cosface": 0, "arcface": 1}      # head_kind of gsl_head_fwd_margin / gsl_head_bwd_margin
HEAD_TILED_C = 1024      # more classes than this: the class-tiled head kernels (csrc/head.hip), whose backward needs B * (D + 1) workspace floats


def _head_fwd(entry, margin, x, B, T, D, gamma, beta, eps, Wn, label, cos_s, cos_m, head_bias, linear, pool_mean):
    """gsl_head_fwd, or (margin = (kind, m, easy_margin)) gsl_head_fwd_margin, which takes those three and cos_y behind the same arguments."""
    _need(x, gamma, beta, Wn, label, head_bias)
    dev = x.device
    emb = torch.empty(B, D, device=dev, dtype=torch.float32)
    mean = torch.empty(B, device=dev, dtype=torch.float32)
    rstd = torch.empty(B, device=dev, dtype=torch.float32)
    C = Wn.shape[0] if Wn is not None else 0
    logits = torch.empty(B, C, device=dev, dtype=torch.float32) if (label is not None or linear) else None
    cos_y = torch.empty(B, device=dev, dtype=torch.float32) if (margin and margin[0] and logits is not None) else None
    tail = (margin[0], float(margin[1]), 1 if margin[2] else 0, _p(cos_y)) if margin else ()
    L.check(getattr(L.load(), entry)(_p(x), code(x.dtype), T, _p(gamma), _p(beta), float(eps), _p(Wn), _p(label), _p(emb), _p(mean),
                                     _p(rstd), _p(logits), B, D, C, float(cos_s), float(cos_m), _p(head_bias), 1 if linear else 0,
                                     1 if pool_mean else 0, *tail, _stream()), entry)
    return logits, emb, mean, rstd, cos_y


def head_fwd(x, B, T, D, gamma, beta, eps, Wn, label, cos_s, cos_m, head_bias=None, linear=False, pool_mean=False):
    return _head_fwd("gsl_head_fwd", None, x, B, T, D, gamma, beta, eps, Wn, label, cos_s, cos_m, head_bias, linear, pool_mean)[:4]


def head_fwd_margin(x, B, T, D, gamma, beta, eps, Wn, label, cos_s, cos_m, head_kind, m=0.5, easy_margin=False, head_bias=None,
                    linear=False, pool_mean=False):
    """head_fwd with the margin head chosen by head_kind ("cosface" | "arcface"; gsl_head_fwd_margin). m / easy_margin: the ArcFace
    margin (cos_m is CosFace's). Returns (logits, emb, mean, rstd, cos_y): cos_y [B] is the label column's cosine before the margin
    (ArcFace with labels; None otherwise), which head_bwd_margin needs."""
    return _head_fwd("gsl_head_fwd_margin", (HEAD_KINDS[head_kind], m, easy_margin), x, B, T, D, gamma, beta, eps, Wn, label, cos_s, cos_m,
                     head_bias, linear, pool_mean)


def _head_bwd(entry, margin, dlogits, demb, x, B, T, D, gamma, mean, rstd, emb, Wn, cos_s, dtype, p_drop, seed, site, linear, pool_mean,
              stream_dtype, compact, gscale, target_exp):
    """gsl_head_bwd, or (margin = (kind, m, easy_margin, cos_y, label)) gsl_head_bwd_margin, which takes those five behind the same arguments."""
    _need(dlogits, demb, x, gamma, mean, rstd, emb, Wn, gscale, *(margin[3:] if margin else ()))
    if gscale is not None and (gscale.numel() < 4 or gscale.dtype != torch.float32):
        raise RuntimeError(f"{entry[4:]}: gscale must be a float32 tensor of 4 elements {{S, 1/S, seen maximum, exponent}}")
    C = Wn.shape[0] if Wn is not None else 0
    # above HEAD_TILED_C classes the workspace is required in every mode and also carries d e-hat [B, D] behind the B maxima (gsl_head_bwd)
    ws_elems = B * (D + 1) if C > HEAD_TILED_C else (B if gscale is not None else 0)
    amax_ws = torch.empty(ws_elems, device=x.device, dtype=torch.float32) if ws_elems else None
    rows = B if compact else B * T
    dx = torch.empty(rows, D, device=x.device, dtype=stream_dtype)
    dxb = torch.empty(rows, D, device=x.device, dtype=dtype)
    tail = (margin[0], float(margin[1]), 1 if margin[2] else 0, _p(margin[3]), _p(margin[4])) if margin else ()
    L.check(getattr(L.load(), entry)(_p(dlogits), _p(demb), _p(x), code(x.dtype), T, _p(gamma), _p(mean), _p(rstd), _p(emb), _p(Wn), _p(dx),
                                     _p(dxb), B, D, C, float(cos_s), code(dtype), code(stream_dtype), float(p_drop), int(seed), int(site),
                                     1 if linear else 0, 1 if pool_mean else 0, 1 if compact else 0, _p(gscale), _p(amax_ws),
                                     int(target_exp), *tail, _stream()), entry)
    return dx, dxb


def head_bwd(dlogits, demb, x, B, T, D, gamma, mean, rstd, emb, Wn, cos_s, dtype, p_drop=0.0, seed=0, site=0, linear=False,
             pool_mean=False, stream_dtype=torch.float32, compact=False, gscale=None, target_exp=0):
    """compact (pool='cls' only): dx / dxb are [B, D] — the cls rows alone, nothing zero-filled.
    gscale: f32 [4] device tensor that persists across steps (zeroed once) -> loss-scaled gradients (fp16 operands): dx / dxb come out
    multiplied by the power of two S the kernel picks from their largest magnitude; gscale receives {S, 1/S} for the LoRA-gradient
    reductions, [2] is cleared for the overflow guard of this backward (layernorm_bwd(gmax=gscale[2:])) and [3] carries the exponent in use
    (gsl_head_bwd). target_exp: 0 = the default 11."""
    return _head_bwd("gsl_head_bwd", None, dlogits, demb, x, B, T, D, gamma, mean, rstd, emb, Wn, cos_s, dtype, p_drop, seed, site, linear,
                     pool_mean, stream_dtype, compact, gscale, target_exp)


def head_bwd_margin(dlogits, demb, x, B, T, D, gamma, mean, rstd, emb, Wn, cos_s, dtype, head_kind, m=0.5, easy_margin=False, cos_y=None,
                    label=None, p_drop=0.0, seed=0, site=0, linear=False, pool_mean=False, stream_dtype=torch.float32, compact=False,
                    gscale=None, target_exp=0):
    """head_bwd with the margin head chosen by head_kind (gsl_head_bwd_margin). ArcFace with dlogits needs the forward's cos_y and the
    labels; everything else as head_bwd."""
    return _head_bwd("gsl_head_bwd_margin", (HEAD_KINDS[head_kind], m, easy_margin, cos_y, label), dlogits, demb, x, B, T, D, gamma, mean,
                     rstd, emb, Wn, cos_s, dtype, p_drop, seed, site, linear, pool_mean, stream_dtype, compact, gscale, target_exp)


HEAD_WGRAD_KINDS = {"cosface": 0, "arcface": 1, "linear": 2, "softmax": 2}      # head_kind of gsl_head_wgrad


def head_wgrad(dlogits, emb, W, head_kind, cos_s=64.0, m=0.5, easy_margin=False, label=None, cos_y=None, bias=False, dW=None, dbias=None):
    """d loss / d W of the head from the upstream dlogits [B, C] (gsl_head_wgrad): emb [B, D] is the head forward's (un-normalised)
    embedding, W [C, D] the raw weight. head_kind "cosface" | "arcface" (needs the forward's label and cos_y) | "linear" / "softmax"
    (bias=True: also d loss / d bias). Returns (dW, dbias or None): freshly allocated unless given, every element stored.
    Dispatch inside the library, on the call alone: C <= 1024 (HEAD_TILED_C) runs the per-class kernel; C > 1024 the class-tiled
    matrix-core kernel when D % 4 == 0 and emb is 16-byte aligned (every element one chain over ascending b: the linear kind equals
    gemm_nt(dlogits.T, emb.T) bit for bit), and the per-class kernel otherwise — never a refusal. Any C, D <= 1024."""
    kind = HEAD_WGRAD_KINDS[head_kind]
    _need(dlogits, emb, W, label, cos_y, dW, dbias)
    B, C = dlogits.shape
    D = emb.shape[1]
    if emb.shape[0] != B or tuple(W.shape) != (C, D) or any(t.dtype != torch.float32 for t in (dlogits, emb, W)):
        raise RuntimeError(f"head_wgrad: float32 dlogits [B, C], emb [B, D], W [C, D] expected, got {tuple(dlogits.shape)}, {tuple(emb.shape)}, {tuple(W.shape)}")
    if not (dlogits.is_contiguous() and emb.is_contiguous() and W.is_contiguous()):
        raise RuntimeError("head_wgrad: dlogits, emb and W must be contiguous")
    if kind == 1 and (label is None or cos_y is None or label.dtype != torch.int64 or label.numel() != B or cos_y.numel() != B
                      or cos_y.dtype != torch.float32 or not label.is_contiguous() or not cos_y.is_contiguous()):
        raise RuntimeError("head_wgrad: the ArcFace head needs the forward's contiguous int64 label [B] and float32 cos_y [B]")
    if dW is None:
        dW = torch.empty(C, D, device=W.device, dtype=torch.float32)
    elif tuple(dW.shape) != (C, D) or dW.dtype != torch.float32 or not dW.is_contiguous():      # (the kernel stores all C * D elements)
        raise RuntimeError(f"head_wgrad: dW must be a contiguous float32 [{C}, {D}] buffer, got {dW.dtype} {tuple(dW.shape)}")
    if kind == 2 and (bias or dbias is not None):
        if dbias is None:
            dbias = torch.empty(C, device=W.device, dtype=torch.float32)
        elif tuple(dbias.shape) != (C,) or dbias.dtype != torch.float32 or not dbias.is_contiguous():
            raise RuntimeError(f"head_wgrad: dbias must be a contiguous float32 [{C}] buffer, got {dbias.dtype} {tuple(dbias.shape)}")
    else:
        dbias = None
    L.check(L.load().gsl_head_wgrad(_p(dlogits), _p(emb), _p(W), _p(label) if kind == 1 else None, _p(cos_y) if kind == 1 else None, _p(dW),
                                    _p(dbias), B, C, D, kind, float(cos_s), float(m), 1 if easy_margin else 0, _stream()), "gsl_head_wgrad")
    return dW, dbias


def ce_fwd(logits, labels):
    _need(logits, labels)
    out = torch.empty(2, device=logits.device, dtype=torch.float32)
    ws = torch.empty(2 * logits.shape[0], device=logits.device, dtype=torch.float32)
    L.check(L.load().gsl_ce_fwd(_p(logits), _p(labels), _p(out), _p(ws), logits.shape[0], logits.shape[1], _stream()), "gsl_ce_fwd")
    return out


def ce_bwd(logits, labels, coef, scale, dlogits=None, accumulate=None):
    _need(logits, labels, coef, dlogits)
    acc = (dlogits is not None) if accumulate is None else bool(accumulate)
    if dlogits is None:
        dlogits = torch.empty_like(logits)
    L.check(L.load().gsl_ce_bwd(_p(logits), _p(labels), _p(coef), float(scale), _p(dlogits), logits.shape[0], logits.shape[1],
                                1 if acc else 0, _stream()), "gsl_ce_bwd")
    return dlogits


def _proto_fwd(entry, emb, labels, proto):
    """gsl_proto_kl_fwd or gsl_proto_l2_fwd (same arguments) -> [1] f32, the sum of the row distances."""
    _need(emb, labels, proto)
    out = torch.empty(1, device=emb.device, dtype=torch.float32)
    ws = torch.empty(emb.shape[0], device=emb.device, dtype=torch.float32)
    L.check(getattr(L.load(), entry)(_p(emb), _p(labels), _p(proto), _p(out), _p(ws), emb.shape[0], emb.shape[1], proto.shape[0], _stream()), entry)
    return out


def _proto_bwd(entry, emb, labels, proto, coef, scale, demb, accumulate):
    """gsl_proto_kl_bwd or gsl_proto_l2_bwd (same arguments); a passed demb is accumulated into unless accumulate says otherwise."""
    _need(emb, labels, proto, coef, demb)
    acc = (demb is not None) if accumulate is None else bool(accumulate)
    if demb is None:
        demb = torch.empty_like(emb)
    L.check(getattr(L.load(), entry)(_p(emb), _p(labels), _p(proto), _p(coef), float(scale), _p(demb), emb.shape[0], emb.shape[1],
                                     proto.shape[0], 1 if acc else 0, _stream()), entry)
    return demb


def proto_kl_fwd(emb, labels, proto):
    return _proto_fwd("gsl_proto_kl_fwd", emb, labels, proto)


def proto_kl_bwd(emb, labels, proto, coef, scale, demb=None, accumulate=None):
    return _proto_bwd("gsl_proto_kl_bwd", emb, labels, proto, coef, scale, demb, accumulate)


def proto_l2_fwd(emb, labels, proto):
    """-> [1] f32: sum_i mean_d (emb[i] - proto[labels[i]])^2 (gsl_proto_l2_fwd)."""
    return _proto_fwd("gsl_proto_l2_fwd", emb, labels, proto)


def proto_l2_bwd(emb, labels, proto, coef, scale, demb=None, accumulate=None):
    return _proto_bwd("gsl_proto_l2_bwd", emb, labels, proto, coef, scale, demb, accumulate)


def topk_max_k():
    return int(L.load().gsl_topk_max_k())


def topk_hits(logits, labels, ks):
    """-> int32 [len(ks)] device tensor: for each k the number of rows whose label is among the k largest logits (gsl_topk_hits, one launch)."""
    _need(logits, labels)
    ks = [int(k) for k in ks]
    if not ks or len(ks) > topk_max_k() or min(ks) < 1:
        raise ValueError(f"topk_hits: between 1 and {topk_max_k()} positive values of k, got {ks}")
    hits = torch.empty(len(ks), device=logits.device, dtype=torch.int32)
    arr = (ctypes.c_int * len(ks))(*ks)
    L.check(L.load().gsl_topk_hits(_p(logits), _p(labels), logits.shape[0], logits.shape[1], arr, len(ks), _p(hits), _stream()), "gsl_topk_hits")
    return hits


# ---- per-class evaluation (csrc/classstat.hip; engine_cl.eval_data_per_class, util.utils.calculate_prototypes)
class ClassStats:
    """The per-class counters of one evaluation, in ONE zeroed int64 device buffer so that one host read serves it:
    count [C] | hit [C] | bad [1] | acc [C] (f64 bits, written by finish()) | confusion [C, C] (int32 pairs, only if asked for).
    The views are plain integer buffers: under data parallelism one sum all_reduce of `buf` would combine the ranks."""

    def __init__(self, C, device, confusion=False):
        self.C = C = int(C)
        if C <= 0:
            raise ValueError(f"ClassStats: the number of classes must be positive, got {C}")
        self.buf = torch.zeros(3 * C + 1 + ((C * C + 1) // 2 if confusion else 0), device=device, dtype=torch.int64)
        _need(self.buf)
        self.count, self.hit, self.bad = self.buf[:C], self.buf[C:2 * C], self.buf[2 * C:2 * C + 1]
        self.acc = self.buf[2 * C + 1:3 * C + 1].view(torch.float64)
        self.confusion = self.buf[3 * C + 1:].view(torch.int32)[:C * C].view(C, C) if confusion else None

    def add(self, logits, labels):
        class_stats(logits, labels, self.count, self.hit, self.bad, self.confusion)

    def finish(self):
        """-> dict of CPU tensors (count, hit int64 [C]; acc f64 [C], NaN where count == 0; confusion int32 [C, C] or None) and bad (int)."""
        class_finish(self.count, self.hit, acc=self.acc)
        host, C = self.buf.cpu(), self.C
        return dict(count=host[:C], hit=host[C:2 * C], bad=int(host[2 * C]), acc=host[2 * C + 1:3 * C + 1].view(torch.float64),
                    confusion=host[3 * C + 1:].view(torch.int32)[:C * C].view(C, C) if self.confusion is not None else None)


def _labels_i64(labels, n, what):
    _need(labels)
    if labels.dtype != torch.int64 or labels.dim() != 1 or labels.shape[0] != n:
        raise RuntimeError(f"gslora_hip: {what} takes int64 labels [{n}], got {labels.dtype} {tuple(labels.shape)}")
    return labels


def _counter(t, n, dtype, what):
    _need(t)
    if t.dtype != dtype or t.numel() != n:
        raise RuntimeError(f"gslora_hip: {what} must be a contiguous {dtype} device buffer of {n} elements")
    return t


def class_stats(logits, labels, count, hit, bad, confusion=None):
    """count[label] += 1, hit[label] += (first arg-max of the row == label), confusion[label, arg-max] += 1 for one batch of f32 logits
    [B, C] (row slices are taken with their stride); labels outside [0, C) add to bad[0] only (gsl_class_stats). In place; returns None."""
    logits = _rows_f32(logits, "logits")
    B, C = logits.shape
    _labels_i64(labels, B, "class_stats")
    _counter(count, C, torch.int64, "count"), _counter(hit, C, torch.int64, "hit"), _counter(bad, 1, torch.int64, "bad")
    if confusion is not None:
        _counter(confusion, C * C, torch.int32, "confusion")
    if B == 0:
        return
    L.check(L.load().gsl_class_stats(_p(logits), logits.stride(0), _p(labels), B, C, _p(count), _p(hit), _p(bad), _p(confusion), _stream()),
            "gsl_class_stats")


def class_embed_sum(emb, labels, sums, count, bad):
    """sums[c] += emb[i] over the rows with labels[i] == c in increasing i (sequential f32 adds: the reference's summation order), count[c]
    += their number; labels outside [0, C) add to bad[0] only (gsl_class_embed_sum). In place; returns None."""
    emb = _rows_f32(emb, "emb")
    B, D = emb.shape
    _need(sums)
    if sums.dtype != torch.float32 or sums.dim() != 2 or sums.shape[1] != D:
        raise RuntimeError(f"gslora_hip: class_embed_sum takes sums f32 [C, {D}], got {sums.dtype} {tuple(sums.shape)}")
    C = sums.shape[0]
    _labels_i64(labels, B, "class_embed_sum")
    _counter(count, C, torch.int64, "count"), _counter(bad, 1, torch.int64, "bad")
    if B == 0:
        return
    L.check(L.load().gsl_class_embed_sum(_p(emb), emb.stride(0), _p(labels), B, D, C, _p(sums), _p(count), _p(bad), _stream()),
            "gsl_class_embed_sum")


def class_finish(count, hit=None, sums=None, acc=None, proto=None):
    """acc [C] f64 = 100 * hit / count and / or proto [C, D] f32 = sums / count, NaN for a class without samples (gsl_class_finish). The
    outputs are allocated when not given; returns (acc, proto) with None for the one not asked for (acc needs hit, proto needs sums)."""
    _need(count, hit, sums, acc, proto)
    C = count.numel()
    _counter(count, C, torch.int64, "count")
    if hit is not None:
        _counter(hit, C, torch.int64, "hit")
        acc = _counter(acc, C, torch.float64, "acc") if acc is not None else torch.empty(C, device=count.device, dtype=torch.float64)
    D = 0
    if sums is not None:
        if sums.dtype != torch.float32 or sums.dim() != 2 or sums.shape[0] != C:
            raise RuntimeError(f"gslora_hip: class_finish takes sums f32 [{C}, D], got {sums.dtype} {tuple(sums.shape)}")
        D = sums.shape[1]
        proto = _counter(proto, C * D, torch.float32, "proto") if proto is not None else torch.empty_like(sums)
    L.check(L.load().gsl_class_finish(_p(count), _p(hit), _p(sums), C, D, _p(acc) if hit is not None else None,
                                      _p(proto) if sums is not None else None, _stream()), "gsl_class_finish")
    return (acc if hit is not None else None), (proto if sums is not None else None)


def group_norms_fwd(flat, toff, tnumel, tgroup, ngroups, tau=0.0):
    _need(flat, toff, tnumel, tgroup)
    dev = flat.device
    nt = toff.numel()
    ws = torch.empty(nt * L.NORM_SPLIT, device=dev, dtype=torch.float32)
    tss = torch.empty(nt, device=dev, dtype=torch.float32)
    gn = torch.empty(ngroups, device=dev, dtype=torch.float32)
    cn = torch.empty(ngroups, device=dev, dtype=torch.float32)
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    mask = torch.empty(ngroups, device=dev, dtype=torch.uint8)
    L.check(L.load().gsl_group_norms_fwd(_p(flat), _p(toff), _p(tnumel), _p(tgroup), nt, ngroups, float(tau), _p(ws), _p(tss),
                                         _p(gn), _p(cn), _p(loss), _p(mask), _stream()), "gsl_group_norms_fwd")
    return dict(tensor_sumsq=tss, group_norm=gn, cal_norm=cn, loss=loss, mask=mask)


def group_norms_bwd(flat, toff, tnumel, tgroup, group_norm, coef, scale, gradflat):
    _need(flat, toff, tnumel, tgroup, group_norm, coef, gradflat)
    L.check(L.load().gsl_group_norms_bwd(_p(flat), _p(toff), _p(tnumel), _p(tgroup), toff.numel(), _p(group_norm), _p(coef),
                                         float(scale), _p(gradflat), _stream()), "gsl_group_norms_bwd")


def adamw_flat(p, g, m, v, lr, beta1, beta2, eps, wd, step, guard=None):
    """guard: f32 device element (gscale[2:] of the backward that produced g): the update is skipped when it holds >= 65504 or a non-finite value."""
    _need(p, g, m, v, guard)
    L.check(L.load().gsl_adamw_flat(_p(p), _p(g), _p(m), _p(v), p.numel(), float(lr), float(beta1), float(beta2), float(eps),
                                    float(wd), int(step), _p(guard), _stream()), "gsl_adamw_flat")


def adamw_flat_dev(p, g, m, v, lr_dev, b1, b2, eps, wd, step_dev, guard=None):
    """Same update with the step count (int64) and learning rate (f32) read from device memory (HIP-graph replays)."""
    _need(p, g, m, v, lr_dev, step_dev, guard)
    L.check(L.load().gsl_adamw_flat_dev(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(lr_dev), float(b1), float(b2), float(eps), float(wd),
                                        _p(step_dev), _p(guard), _stream()), "gsl_adamw_flat_dev")


def cast(x, dtype):
    _need(x)
    out = torch.empty(x.shape, device=x.device, dtype=dtype)
    L.check(L.load().gsl_cast(_p(x), _p(out), x.numel(), code(dtype), _stream()), "gsl_cast")
    return out


def transpose_cast(W, dtype):
    _need(W)
    R, Cc = W.shape
    out = torch.empty(Cc, R, device=W.device, dtype=dtype)
    L.check(L.load().gsl_transpose_cast(_p(W), _p(out), R, Cc, code(dtype), _stream()), "gsl_transpose_cast")
    return out


def pack_pad(src, si, sj, rows, cols, rows_out, ld_out, dtype, scale=1.0, out=None):
    """out given: that [rows_out, ld_out] buffer is rewritten in place (the persistent LoRA packs of the runner)."""
    _need(src, out)
    if out is None:
        out = torch.empty(rows_out, ld_out, device=src.device, dtype=dtype)
    L.check(L.load().gsl_pack_pad(_p(src), si, sj, rows, cols, float(scale), _p(out), rows_out, ld_out, code(dtype), _stream()),
            "gsl_pack_pad")
    return out


PACK_DESC = None


def pack_desc_table(entries, device):
    """entries: list of (src f32 tensor, si, sj, rows, cols, scale, out tensor). -> (uint8 device tensor holding gsl_pack_desc[n], max_elems)"""
    import numpy as np
    global PACK_DESC
    if PACK_DESC is None:   # mirrors struct gsl_pack_desc (include/gslora_hip.h), 56 bytes
        PACK_DESC = np.dtype([("in", "<u8"), ("si", "<i8"), ("sj", "<i8"), ("rows", "<i4"), ("cols", "<i4"), ("scale", "<f4"),
                              ("pad_", "<i4"), ("out", "<u8"), ("rows_out", "<i4"), ("ld_out", "<i4")], align=False)
        assert PACK_DESC.itemsize == 56
    arr = np.zeros(len(entries), dtype=PACK_DESC)
    mx = 0
    for k, (src, si, sj, rows, cols, scale, out) in enumerate(entries):
        arr[k] = (src.data_ptr(), si, sj, rows, cols, scale, 0, out.data_ptr(), out.shape[0], out.shape[1])
        mx = max(mx, out.numel())
    return torch.from_numpy(arr.view(np.uint8).copy()).to(device), mx


def pack_pad_batch(table, n, max_elems, dtype):
    _need(table)
    L.check(L.load().gsl_pack_pad_batch(_p(table), int(n), int(max_elems), code(dtype), _stream()), "gsl_pack_pad_batch")


def dropout_mask(n, p_drop, seed, site, device):
    keep = torch.empty(n, device=device, dtype=torch.uint8)
    L.check(L.load().gsl_dropout_mask(_p(keep), n, float(p_drop), int(seed), int(site), _stream()), "gsl_dropout_mask")
    return keep


# ---- face verification on pairs (csrc/verif.hip; util/verification.py, util.utils.perform_val)
def _rows_f32(t, what):
    """A 2-D f32 device tensor with unit inner stride (row slices such as emb[0::2] are taken with their stride, not copied)."""
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"gslora_hip: {what} must be a torch tensor on a ROCm GPU (the HIP path has no CPU fallback)")
    _need(t, rows_ok=True)
    if t.dim() != 2 or t.dtype != torch.float32:
        raise RuntimeError(f"gslora_hip: {what} must be a 2-D float32 tensor")
    return t


def verif_pair_dist(e0, e1, want_normed=False):
    """perform_val's middle (utils.py:205-216 + verification.py:67-68): e0, e1 [2P, D] = the embeddings of the original and of the flipped
    images. Returns (dist [P], xnorm [1], the normalised embeddings [2P, D] or None)."""
    e0, e1 = _rows_f32(e0, "e0"), _rows_f32(e1, "e1")
    if e0.shape != e1.shape or e0.shape[0] % 2 or e0.stride(0) != e1.stride(0):
        raise ValueError(f"verif_pair_dist: e0 and e1 must be [2P, D] of one shape and row stride, not {tuple(e0.shape)} / {tuple(e1.shape)}")
    P, D = e0.shape[0] // 2, e0.shape[1]
    dist = torch.empty(P, device=e0.device, dtype=torch.float32)
    xnorm = torch.empty(1, device=e0.device, dtype=torch.float32)
    ws = torch.empty(P, device=e0.device, dtype=torch.float32)
    nemb = torch.empty(2 * P, D, device=e0.device, dtype=torch.float32) if want_normed else None
    L.check(L.load().gsl_verif_pair_dist(_p(e0), _p(e1), e0.stride(0), P, D, L.VERIF_FLIP_SUM, _p(dist), _p(xnorm), _p(ws), _p(nemb), _stream()),
            "gsl_verif_pair_dist")
    return dist, xnorm, nemb


def verif_sq_dist(a, b):
    """dist[p] = sum (a[p] - b[p])^2 of two [P, D] embedding arrays (verification.py:67-68, 159-160)."""
    a, b = _rows_f32(a, "embeddings1"), _rows_f32(b, "embeddings2")
    if a.shape != b.shape or a.stride(0) != b.stride(0):
        raise ValueError(f"verif_sq_dist: the two embedding arrays must share shape and row stride, not {tuple(a.shape)} / {tuple(b.shape)}")
    dist = torch.empty(a.shape[0], device=a.device, dtype=torch.float32)
    L.check(L.load().gsl_verif_pair_dist(_p(a), _p(b), a.stride(0), a.shape[0], a.shape[1], L.VERIF_PLAIN, _p(dist), None, None, None, _stream()),
            "gsl_verif_pair_dist")
    return dist


def verif_fold_counts(dist, issame, thresholds, nrof_folds):
    """dist [P] f32, issame [P] uint8, thresholds [Tn] f64 (device) -> (counts int32 [F, Tn, 2] = true / false accepts of each KFold test
    fold, fold_tot int32 [F, 2] = same / different pairs of each fold)."""
    _need(dist, issame, thresholds)
    if dist.dtype != torch.float32 or issame.dtype != torch.uint8 or thresholds.dtype != torch.float64 or issame.numel() != dist.numel():
        raise RuntimeError("verif_fold_counts: dist f32 [P], issame uint8 [P], thresholds f64 [Tn]")
    F, Tn = int(nrof_folds), thresholds.numel()
    counts = torch.empty(F, Tn, 2, device=dist.device, dtype=torch.int32)
    tot = torch.empty(F, 2, device=dist.device, dtype=torch.int32)
    L.check(L.load().gsl_verif_fold_counts(_p(dist), _p(issame), dist.numel(), _p(thresholds), Tn, F, _p(counts), _p(tot), _stream()),
            "gsl_verif_fold_counts")
    return counts, tot


def verif_select(counts, fold_tot, thresholds, xnorm=None):
    """-> f64 [2F + 2Tn + 1]: accuracy [F], best_thresholds [F], tpr [Tn], fpr [Tn], xnorm (0 if not given)."""
    _need(counts, fold_tot, thresholds, xnorm)
    F, Tn = counts.shape[0], counts.shape[1]
    out = torch.zeros(2 * F + 2 * Tn + 1, device=counts.device, dtype=torch.float64)
    L.check(L.load().gsl_verif_select(_p(counts), _p(fold_tot), _p(thresholds), Tn, F, _p(xnorm), _p(out), _stream()), "gsl_verif_select")
    return out
