/* gslora_hip.h — C ABI of libgslora_hip.so: the MI355X (gfx950) kernels behind the GS-LoRA
 * forgetting train step.
 *
 * Boundary contract:
 *  - plain C: pointers + sizes, no C++/torch types. All pointers are DEVICE pointers owned by
 *    the caller (torch tensors' data_ptr()); the library allocates nothing.
 *  - every call is asynchronous on the given hipStream_t (passed as void*; NULL = default stream).
 *  - return 0 on success, negative gsl_status on error; message via gsl_last_error()
 *    (thread-local). Never aborts.
 *  - dtype selects the operand/activation element type: GSL_F32 (parity mode, exact-f32 kernels),
 *    GSL_BF16 or GSL_F16 (speed mode: 16-bit operands, f32 accumulate on MFMA; "bf16" in the comments below means either 16-bit
 *    format unless a comment says otherwise). LayerNorm statistics, biases,
 *    LoRA master weights, losses and optimizer state are always f32; the residual stream and its
 *    gradient are f32 or — in speed mode, per call (x_dtype / stream_dtype) — bf16.
 *
 * Each entry point names the reference code it replaces (paths relative to bjzhb666/GS-LoRA).
 * The reference has no FFI of its own (it is pure PyTorch); the "binding a maintainer would add"
 * is the ctypes stub in gs-lora_amd/gslora_hip/_lib.py, shown in INTEGRATION.md.
 */
#ifndef GSLORA_HIP_H
#define GSLORA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: exactly the entry points declared here are exported. */
#define GSL_API __attribute__((visibility("default")))

typedef void* gsl_stream_t;

/* GSL_F16 (round 5): the speed mode with IEEE fp16 operands — the same kernels, bytes and MFMA rate as GSL_BF16 (v_mfma_f32_16x16x32_f16),
 * an 11-bit significand instead of 8. Activations saturate at +-65504 on store (NaN / Inf stay visible); the backward runs on gradients
 * multiplied by a power-of-two loss scale chosen on the device by gsl_head_bwd (gscale = {S, 1/S}) which the LoRA-gradient reductions
 * divide out again, exactly. As an x_dtype it is also the forward residual stream format of the GSL_BF16 mode (round 4). */
/* GSL_F32X3: a third way to compute on f32 tensors, accepted by gsl_gemm_nt ONLY (every other entry point rejects it with GSL_ERR_ARG). All
 * tensors are f32 exactly as for GSL_F32 — same shapes, epilogues and dropout masks — but the products run on the bf16 matrix cores at f32
 * accuracy (gfx950 has no xf32; the exact-f32 MFMA runs at 1/16 of the bf16 rate):
 *  - split rule: every operand element x is split in registers into three bf16 pieces, hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid),
 *    bf16() = ROUND TO NEAREST EVEN, SATURATING: a finite value that would round up to Inf (|x| >= 2^128 - 2^119, f32 bits 0x7f7f8000) becomes
 *    the largest finite bf16 instead (the kernel runs with the wave's FP16_OVFL mode bit set, which governs v_cvt_pk_bf16_f32 too; Inf and NaN
 *    stay Inf and NaN). Both subtractions are exact and hi + mid + lo == x bit for bit for 0 and every finite |x| >= 2^-110, the largest finite
 *    values included; below 2^-110 the last piece can fall under bf16's denormal grid of 2^-133, an absolute error <= 2^-134 per element;
 *  - product set: hi*hi, hi*mid, mid*hi, mid*mid, hi*lo, lo*hi (six bf16 MFMAs per K tile of 32, f32 accumulate). The dropped mid*lo, lo*mid,
 *    lo*lo are <= 2^-26 |a w|: below the rounding of an f32 accumulation of the same products;
 *  - the result is NOT the k-ordered fmaf chain of GSL_F32 bit for bit (it is as close to the exact product as that chain is). It is
 *    deterministic: a fixed order of accumulation, the same bits on every call and under HIP-graph replay;
 *  - non-finite rule: a NaN or Inf in row m of A1 | A2 makes every element of output row m NaN, one
 *    in row n of W1 | W2 every element of output column n (NaN also where the f32 kernel would produce Inf); nothing else is touched. (A 16-bit
 *    MFMA by itself drops a NaN operand's k-group and clamps Inf.)
 * Shapes outside the matrix-core kernel's (N < 128 or M < 64) run the exact-f32 VALU kernel of GSL_F32. */
enum gsl_dtype { GSL_F32 = 0, GSL_BF16 = 1, GSL_F16 = 2, GSL_F32X3 = 3 };

enum gsl_status {
  GSL_OK = 0,
  GSL_ERR_ARG = -1,      /* bad shape / alignment / unsupported size */
  GSL_ERR_LAUNCH = -2,   /* hipLaunch / runtime error */
  GSL_ERR_UNSUPPORTED = -3
};

/* GEMM epilogues (gsl_gemm_nt). acc = alpha * (A1*W1^T + A2*W2^T)  */
enum gsl_epilogue {
  GSL_EPI_STORE = 0,        /* out[dtype]  = acc (+ bias); out2 (nullable; 16-bit operands, 16 <= N <= 128, no bias): a COMPACT [M,16] copy
                               (row stride 16) of output columns 0..15 — the 16-column operand form of a LoRA down-projection for
                               gsl_gemm_nt_lora_mulgrad's U1 (32 rows = one contiguous 1 KB read)                                   */
  GSL_EPI_BIAS_RES_F32 = 1, /* outf32      = dropout(acc + bias) + res                          */
  GSL_EPI_BIAS_GELU = 2,    /* out[dtype]  = dropout(gelu(acc+bias)); out2[dtype] = gelu'(acc+bias)*dropmask */
  GSL_EPI_MUL = 3,          /* out[dtype]  = acc * aux[dtype]                                   */
  GSL_EPI_PATCH = 4,        /* outf32      = dropout((tok==0 ? cls : acc + bias) + pos[tok]),  tok = m % T */
  GSL_EPI_STORE_F32 = 5,    /* outf32      = acc (+ bias)                                       */
  GSL_EPI_STORE_QKV_HM = 6, /* bf16 only: STORE of a QKV projection (N = 3*H*64, rows m = b*T + t, T = tokens per image) into the
                               head-major layout [B][H][3][T][64] that the attention entry points read with qkv_layout = 1 */
  GSL_EPI_BIAS_RES_BF16 = 7,/* bf16 only, the forward residual stream carried in bf16: out[bf16] = bf16(dropout(acc + bias) + f32(res[bf16]))
                               — f32 arithmetic on the f32 accumulator, one rounding on store; same dropout mask as BIAS_RES_F32 */
  GSL_EPI_PATCH_BF16 = 8,   /* bf16 only: PATCH with a bf16 output */
  GSL_EPI_MUL_G8 = 9,       /* bf16 only: MUL with aux = the 8-bit GELU' code tensor (slab-major, see below) written by BIAS_GELU_G8;
                               p_drop = the dropout rate of the forward that wrote it (decode scale 1/(1-p); no mask is applied here) */
  GSL_EPI_BIAS_RES_F16 = 11,/* bf16 only: BIAS_RES_BF16 with the forward residual stream (res in, out) in IEEE fp16 (clamped to +-65504 on store) */
  GSL_EPI_PATCH_F16 = 12,   /* bf16 only: PATCH with an fp16 output */
  GSL_EPI_STORE_LN = 13,    /* STORE with a CONSUMER-SIDE LayerNorm (reference vit_face.py:316-323 PreNorm + :358-360 to_qkv; modified_VIT.py: ln_1 -> in_proj): A1 is the RAW
                               residual stream x (not LN(x)), W1 the weight with gamma folded in (W'[n,k] = W[n,k] gamma[k], operand format), and
                               out[dtype] = rstd[m] * (acc - mean[m] * c[n]) + d[n]   with pos = mean [M], cls = rstd [M] (gsl_layernorm_fwd with
                               y = NULL), aux = c [N] = rowsum_k W' (f32, of the ROUNDED W'), bias = d [N] = W beta (+ the layer's bias) (f32).
                               One pass over x replaces LayerNorm's read + write and the GEMM reads the stream itself. alpha = 1, no out2. T > 0: row m takes
                               mean[m*T], rstd[m*T] — the statistics of every T-th row of a larger tensor (A1 = its cls rows at lda1 = T*D). */
  GSL_EPI_STORE_QKV_HM_LN = 14, /* the same with the head-major copy-out of GSL_EPI_STORE_QKV_HM */
  GSL_EPI_BIAS_GELU_G8 = 10 /* bf16 only: BIAS_GELU whose second output is the 8-bit fixed-point code of gelu'(acc+bias)*dropmask:
                               q = round(gelu' * keep * 200 + 26), decoded as (q - 26) * 0.005 / (1 - p); gelu' lies in [-0.129, 1.129]:
                               absolute error <= 0.0025/(1-p), a dropped element decodes to exactly 0. out2 is M*N bytes in SLAB-MAJOR
                               order [N/64][M][64] (element (m, n) at ((n/64)*M + m)*64 + n%64; N % 64 == 0): a tensor private to this
                               epilogue and its reader, laid out so that both touch consecutive memory */
};

GSL_API int gsl_version(void);
GSL_API const char* gsl_last_error(void);

/* ---- K1 patch gather: einops 'b c (h p1) (w p2) -> b (h w) (p1 p2 c)' (vit_face.py:530).
 * img f32 [B,C,H,W] -> out[dtype] [B*T, p*p*C], T = 1 + (H/p)*(W/p); row b*T (cls slot) is zero. */
GSL_API int gsl_patchify(const float* img, void* out, int B, int C, int H, int W, int p, int dtype, gsl_stream_t s);

/* ---- K1s overlapping patch gather of ViTs_face: nn.Unfold(k, stride, pad)(img).transpose(1, 2) (vits_face.py:446-450, 489-491).
 * img f32 [B,C,H,W] -> out[dtype] [B*T, ldo], T = 1 + Lh*Lw, Lh = (H + 2*pad - k)/stride + 1 (Lw likewise). Row b*T (cls slot) is zero,
 * row b*T + 1 + t holds window t (row-major over Lh x Lw) in Unfold's order j = c*k*k + kh*k + kw; taps outside the image and the K padding
 * C*k*k <= j < ldo are zero. Every element of out is written. 0 <= pad < k, ldo % 8 == 0, C*k*k <= ldo <= 4096, out 16-byte aligned. */
GSL_API int gsl_unfold_patches(const float* img, void* out, int B, int C, int H, int W, int k, int stride, int pad, int ldo, int dtype,
                               gsl_stream_t s);

/* ---- K1 / K1s from uint8 images: the dataset transform ToTensor() + Normalize(mean, std) of the drivers (train/train_own_forget_cl.py:131-147)
 * fused into the two gathers above, so that a batch crosses the host boundary as the decoder's bytes. img u8 in layout GSL_U8_NCHW
 * ([B,C,H,W]) or GSL_U8_NHWC ([B,H,W,C]); table f32 [C][256] on the device: table[c*256 + u] is the value of byte u in channel c (the
 * caller builds it with the expression it wants to match, ((u / 255) - mean[c]) / std[c] in f32). out is exactly what the float gather
 * writes for the image of those values: cls rows, out-of-image taps and the K padding are 0 (not table[c][0]). img 8-byte aligned
 * (gsl_unfold_patches_u8; gsl_patchify_u8 takes any address and loads 8 bytes at a time when p % 8 == 0, C is 1 or 3 and img is 8-byte
 * aligned), out 16-byte aligned, k < 256; otherwise the float forms' conditions. */
enum gsl_u8_layout { GSL_U8_NCHW = 0, GSL_U8_NHWC = 1 };
GSL_API int gsl_patchify_u8(const uint8_t* img, int layout, const float* table, void* out, int B, int C, int H, int W, int p, int dtype,
                            gsl_stream_t s);
GSL_API int gsl_unfold_patches_u8(const uint8_t* img, int layout, const float* table, void* out, int B, int C, int H, int W, int k, int stride,
                                  int pad, int ldo, int dtype, gsl_stream_t s);

/* ---- K3/K5/K6/K7/K8 dense NT GEMM with an optional second K segment (the LoRA rank-r term)
 * and a fused epilogue. Replaces F.linear + loralib.Linear.forward (vit_face.py:330-334,349-356)
 * and their autograd dX.
 *   A1 [M,K1] (lda1), W1 [N,K1] (ldw1); A2 [M,K2] (lda2), W2 [N,K2] (ldw2)  — all `dtype` (GSL_F32X3: f32 tensors, see gsl_dtype);
 *   K1 % 64 == 0, K2 % 64 == 0 (K2 may be 0). bias/pos/cls f32; res f32 (bf16 for GSL_EPI_BIAS_RES_BF16). out/out2/aux per epilogue.
 *   dropout: p_drop in [0,1); mask = hash(seed, site, m*N+n) (see gsl_dropout_keep in DESIGN.md).
 *   Every (seed, site) pair of this ABI: when bit 31 of `site` (GSL_SEED_ON_DEVICE) is set, `seed` is not the value but a device
 *   pointer to a uint64 holding it — the kernels load it, so a captured HIP graph replays with the value current at replay time. */
#define GSL_SEED_ON_DEVICE 0x80000000u
GSL_API int gsl_gemm_nt(const void* A1, int lda1, const void* W1, int ldw1, int K1,
                const void* A2, int lda2, const void* W2, int ldw2, int K2,
                int M, int N, int dtype, int epilogue, float alpha,
                const float* bias, const void* res, const void* aux,
                void* out, void* out2, int ldo,
                const float* pos, const float* cls, int T,
                float p_drop, uint64_t seed, uint32_t site, gsl_stream_t s);

/* Leading dimensions (elements) of both entry points: lda >= K and ldw >= K of every segment, ldo >= N (STORE_QKV_HM: ldo == N);
 * a smaller one fails with GSL_ERR_ARG. aux and out2 of the MUL / BIAS_GELU epilogues are indexed with ldo, like res. */

/* The tile rule: the kernel gsl_gemm_nt (in_kernel_lora = 0) or gsl_gemm_nt_lora (in_kernel_lora = 1) launches for a shape — a function
 * of the shape alone, the same one the launches call. K = K1 + K2; has_out2: GSL_EPI_STORE with the compact second output. The
 * development build's variant knobs apply after it. Returns a gsl_gemm_tile, or -1 for a dtype the entry point does not take. */
enum gsl_gemm_tile {
  GSL_TILE_RING64 = 0,         /* 16-bit: 64x64 tiles, LDS-DMA ring (few rows: up to 256 tiles of 128x128)                 */
  GSL_TILE_RING64_WIDE = 1,    /* 16-bit: the ring kernel on 64x128 tiles (more 64x64 tiles than resident workgroups)      */
  GSL_TILE_RING64_KSPLIT = 2,  /* 16-bit: the ring kernel, two wave groups split K (K >= 1024, at most 256 tiles of 64x64)  */
  GSL_TILE_128 = 3,            /* 16-bit: 128x128 single stage                                                             */
  GSL_TILE_RING256X128 = 4,    /* 16-bit: 256x128 three-stage ring (N < 512; STORE with out2)                              */
  GSL_TILE_P8 = 5,             /* 16-bit: 256x256 8-phase                                                                  */
  GSL_TILE_F32_VALU = 6,       /* f32 / f32x3: 64x64 VALU kernel (N < 128 or M < 64)                                       */
  GSL_TILE_F32_MFMA = 7,       /* f32: 128x128 matrix-core kernel                                                          */
  GSL_TILE_F32X3_MFMA = 8      /* f32x3: 128x128 tiles, three bf16 pieces per operand                                      */
};
GSL_API int gsl_gemm_tile_choice(int M, int N, int K, int dtype, int has_out2, int in_kernel_lora);

/* Same GEMM with the LoRA rank-r term produced INSIDE the kernel (bf16 only; replaces the two-launch form
 * t = s*(A P^T) [gsl_gemm_nt, N=64] ; out = A W^T + t Q^T [gsl_gemm_nt with a K segment], and saves one full read of A):
 *   out = epilogue(A*W^T + t*Q^T),  t = lora_scale * (A*P^T)
 *   A [M,K] (lda), W [N,K] (ldw), P [16,K] (ldp; rows >= r zero), Q [N,32] (ldq >= 32; cols >= r zero), K % 64 == 0.
 *   tout (nullable) [M, ldt >= 64] receives t in bf16, zero padded to 64 columns (input of gsl_lora_grad).
 * Epilogues: STORE, BIAS_RES_F32, BIAS_RES_BF16, BIAS_GELU, BIAS_GELU_G8, MUL, MUL_G8. */
GSL_API int gsl_gemm_nt_lora(const void* A, int lda, const void* W, int ldw, int K,
                     const void* P, int ldp, const void* Q, int ldq, float lora_scale, void* tout, int ldt,
                     int M, int N, int dtype, int epilogue,
                     const float* bias, const void* res, const void* aux, void* out, void* out2, int ldo,
                     float p_drop, uint64_t seed, uint32_t site, gsl_stream_t s);

/* The MUL form of gsl_gemm_nt_lora (FFN2-dX: out = (A W^T + t Q^T) * aux, bf16) with the two LoRA-gradient reductions that consume
 * its tiles fused into the epilogue instead of two gsl_lora_grad launches that re-read [M,N] tensors from HBM:
 *   G1[n*g1sn + j*g1sj] (+)= sum_m out[m,n] * U1[m,j]      (dB of the up-projection adapter: loralib autograd of vit_face.py:330)
 *   G2[n*g2sn + j*g2sj] (+)= sum_m Y2[m,n] * t[m,j]        (dA of the down-projection adapter; Y2 = the saved FFN hidden activation)
 * U1 [M, ldu1 >= 16] bf16 (columns r..15 zero or discarded), Y2 / aux / out [M,N] bf16 with row stride ldo, N % 8 == 0.
 * ws f32 >= gsl_gemm_mulgrad_ws_elems(M, N, r). Reductions are fixed-order (bit-reproducible).
 * aux_u8 != 0: aux is the 8-bit GELU' code tensor of GSL_EPI_BIAS_GELU_G8 (slab-major [N/64][M][64], N % 64 == 0) and p_drop the
 * dropout rate of that forward. dtype: GSL_BF16 or GSL_F16 (the operand format of every 16-bit tensor of the call).
 * gscale (nullable): device pointer to {S, 1/S} written by gsl_head_bwd — the reductions are multiplied by 1/S on the way out (the
 * operands carry loss-scaled gradients; a power of two, so the un-scaling is exact). */
GSL_API long gsl_gemm_mulgrad_ws_elems(int M, int N, int r);
GSL_API int gsl_gemm_nt_lora_mulgrad(const void* A, int lda, const void* W, int ldw, int K,
                             const void* P, int ldp, const void* Q, int ldq, float lora_scale, void* tout, int ldt,
                             int M, int N, const void* aux, void* out, int ldo,
                             const void* U1, int ldu1, float* G1, long g1sn, long g1sj,
                             const void* Y2, float* G2, long g2sn, long g2sj,
                             int r, int accumulate, float* ws, int aux_u8, float p_drop, int dtype, const float* gscale, gsl_stream_t s);

/* ---- K2 LayerNorm (nn.LayerNorm, vit_face.py:316-323, 498-500). x — the residual stream — is `x_dtype` (f32; bf16 when the bf16
 * speed mode carries the forward stream in bf16), rows of length D at stride x_row_stride (elements); y[dtype] [M,D]; mean/rstd f32 [M].
 * D in {64,128,256,512,768,1024}. y may be NULL: row statistics only (the input of GSL_EPI_STORE_LN, whose GEMM normalises in its epilogue). */
GSL_API int gsl_layernorm_fwd(const void* x, long x_row_stride, const float* gamma, const float* beta, float eps,
                      void* y, float* mean, float* rstd, int M, int D, int dtype, int x_dtype, gsl_stream_t s);
/* LayerNorm forward + the LoRA down-projection that reads its output, in one pass (bf16 mode): y = LN(x) [M,D] bf16 and
 * u = alpha * y P^T for the rank-r adapter of the layer that consumes y (FFN1's lora_A, vit_face.py:330 + loralib Linear.forward):
 * P [>= 16, D] bf16 at row stride ldp (rows j < r = lora_A[j,:], the rest zero), u [M,64] bf16 dense with columns >= 16 written as zero —
 * the LoRA K segment of gsl_gemm_nt. Replaces gsl_layernorm_fwd + a skinny gsl_gemm_nt that re-read y. x bf16 at x_row_stride; D in {512, 768}. */
GSL_API int gsl_layernorm_fwd_lora(const void* x, long x_row_stride, const float* gamma, const float* beta, float eps, void* y,
                           float* mean, float* rstd, int M, int D, const void* P, int ldp, float alpha, void* u, gsl_stream_t s);
/* dx = dres + LN'(dy) ; dxb[dtype] = dx * dropmask(site) (nullable). dy is `dtype` [M,D] (dense). dres / dx — the residual-GRADIENT
 * stream — are `stream_dtype`: f32, or bf16 when dtype is bf16 (speed mode: the stream is re-read and re-written by every LayerNorm
 * backward of the chain). x (the saved forward stream) is `x_dtype`.
 * dres/dx rows are io_row_stride elements apart (0 -> D; dres may alias dx: in-place update); the dropout counter of element (row, d) is
 * row*drop_row_stride + d (0 -> D). dxb is always dense [M,D].
 * dres_cls_T > 0: dres is COMPACT — it holds only the rows of the cls tokens ([M / dres_cls_T] rows, io_row_stride apart); row m
 * receives dres[m / dres_cls_T] when m % dres_cls_T == 0 and nothing otherwise, and dx is written dense [M,D]. (The stream gradient
 * leaving the cls-row-only backward of the last block is exactly zero off the cls rows: no zero-filled tensor is written or read.)
 * gmax (nullable; the overflow guard of the loss-scaled fp16 backward, round 6): device f32, raised (atomic max) to the largest |value| this call
 * read in dy or stored in dx — gscale + 2 of gsl_head_bwd. Every gradient of the chain passes a LayerNorm backward; a saturated 16-bit store
 * anywhere upstream (an operand of +-65504) or in the stream shows here as gmax >= 65504. A NaN read in dy or stored in dx (a NaN in x or
 * dres gets there) makes gmax a NaN, and stays one: the guard is then non-finite, which gsl_adamw_flat and gsl_head_bwd act on.
 * x_row_stride >= D; io_row_stride 0 (= D) or >= D. */
GSL_API int gsl_layernorm_bwd(const void* dy, const void* x, long x_row_stride, const float* gamma,
                      const float* mean, const float* rstd, const void* dres,
                      void* dx, long io_row_stride, void* dxb, int M, int D, int dtype, int stream_dtype, int x_dtype,
                      float p_drop, uint64_t seed, uint32_t site, long drop_row_stride, int dres_cls_T, float* gmax, gsl_stream_t s);

/* ---- K4 attention, head_dim 64, no mask, softmax(QK^T*scale)V (vit_face.py:358-376).
 * qkv_layout (the INPUT qkv): 0 = token-major qkv[dtype] [B*T, 3*H*64] (q|k|v, each 'b n (h d)', as the reference's to_qkv output),
 * 1 = head-major [B][H][3][T][64] (bf16 kernels only; written by gsl_gemm_nt's GSL_EPI_STORE_QKV_HM): every panel row is a full
 * 128-byte line next to its neighbours. Outputs are token-major in both cases: o[dtype] [B*T, H*64], lse f32 [B,H,T].
 * Token limit: 2 <= T <= GSL_ATTN_MAX_T (1025 = a 32 x 32 patch grid plus the cls token) for gsl_attention_fwd, gsl_attention_bwd and
 * gsl_attention_fwd_cls; a longer sequence fails with GSL_ERR_ARG. Up to 224 tokens (256 for the cls forward) an item's K / V sit in LDS
 * whole; above, they stream through LDS in 64-row panels with an online softmax (same output formats, same lse). gsl_attention_bwd_cls
 * takes any T. Which kernel a call launches is a function of the shape alone: gsl_attention_kernel_choice below. */
#define GSL_ATTN_MAX_T 1025
GSL_API int gsl_attention_fwd(const void* qkv, void* o, float* lse, int B, int T, int H, float scale, int dtype, int qkv_layout, gsl_stream_t s);
/* dqkv[dtype] [B*T,3*H*64] (token-major, always); delta_ws f32 [B,H,T] scratch. */
GSL_API int gsl_attention_bwd(const void* qkv, const void* o, const void* d_o, const float* lse, void* dqkv,
                      float* delta_ws, int B, int T, int H, float scale, int dtype, int qkv_layout, gsl_stream_t s);
/* The last transformer block when the head pools the cls token (vit_face.py:540): everything after its attention is token-wise, so
 * only the cls query's attention output is ever consumed. Forward of that one query row per (image, head) against the full K / V
 * panels: o_cls[dtype] [B, H*64], lse_cls f32 [B, H].
 * qkv_layout 0 / 1 as above (q = token 0 of the qkv tensor, q_cls ignored); 2: the block's projection computed Q for the cls rows only —
 * `qkv` is kv[dtype] token-major [B*T, 2*H*64] (k | v) and q_cls[dtype] [B, H*64] holds the queries. */
GSL_API int gsl_attention_fwd_cls(const void* qkv, const void* q_cls, void* o_cls, float* lse_cls, int B, int T, int H, float scale,
                                  int dtype, int qkv_layout, gsl_stream_t s);
/* Its backward: only the cls query carries an output gradient. d_o_cls[dtype] [B, H*64] is dO of the cls rows;
 * cls_compact != 0: o / lse are the [B, H*64] / [B, H] outputs of gsl_attention_fwd_cls, 0: the full tensors of gsl_attention_fwd
 * ([B*T, H*64] / [B, H, T]; the cls rows are read). qkv_layout 0 / 1: writes the full dqkv [B*T,3*H*64] (dQ rows of the other tokens
 * = 0; dq_cls unused); 2: writes dkv [B*T, 2*H*64] into `dqkv` and the query gradients into dq_cls [B, H*64]. */
GSL_API int gsl_attention_bwd_cls(const void* qkv, const void* q_cls, const void* o, const void* d_o_cls, const float* lse, void* dqkv,
                                  void* dq_cls, int B, int T, int H, float scale, int dtype, int qkv_layout, int cls_compact, gsl_stream_t s);

/* The kernel rule: the kernel(s) one of the four entry points above launches — a function of (B*H, T, dtype, direction) and the device's CU
 * count (256 when no device is present), the same one the launches call. direction: 0 gsl_attention_fwd, 1 gsl_attention_bwd,
 * 2 gsl_attention_fwd_cls, 3 gsl_attention_bwd_cls. The development build's GSL_ATTN_* knobs apply after it. Returns a gsl_attn_kernel, or
 * -1 for arguments the entry point refuses with GSL_ERR_ARG (sizes, T > GSL_ATTN_MAX_T, dtype, qkv_layout). "items" = B*H. */
enum gsl_attn_kernel {
  GSL_ATTN_FWD_LONG = 0,         /* 16-bit, T > 224: K / V panels streamed through LDS, online softmax                            */
  GSL_ATTN_FWD_T64 = 1,          /* 16-bit, T <= 64: one item per workgroup, four key tiles, 256 threads                          */
  GSL_ATTN_FWD_PERSISTENT = 2,   /* 16-bit, 64 < T <= 208, items >= 2 CUs: persistent wave-specialised, one workgroup of 1024 per CU */
  GSL_ATTN_FWD_1024 = 3,         /* 16-bit, 64 < T <= 224, items < CUs: one item per workgroup, sixteen waves                     */
  GSL_ATTN_FWD_512 = 4,          /* 16-bit, 64 < T <= 224 otherwise: one item per workgroup, eight waves                          */
  GSL_ATTN_FWD_F32_LONG = 5,     /* f32, T > 224                                                                                  */
  GSL_ATTN_FWD_F32 = 6,          /* f32, T <= 224: matrix-core kernel (64-row panel up to T = 64, else 224 rows)                  */
  GSL_ATTN_BWD_LONG = 7,         /* 16-bit, T > 224: dQ kernel, then dK / dV kernel, over streamed panels                         */
  GSL_ATTN_BWD_T64 = 8,          /* 16-bit, T <= 64: dQ kernel, then dK / dV kernel, 256 threads                                  */
  GSL_ATTN_BWD_MERGED = 9,       /* 16-bit, 192 < T <= 208, items >= 8 CUs: persistent, every score tile computed once            */
  GSL_ATTN_BWD_FUSED_1024 = 10,  /* 16-bit, 64 < T <= 224, items < CUs: both phases in one launch, sixteen waves                  */
  GSL_ATTN_BWD_FUSED_512 = 11,   /* 16-bit, 64 < T <= 224 otherwise: both phases in one launch, eight waves                       */
  GSL_ATTN_BWD_F32_LONG = 12,    /* f32, T > 224: dQ kernel, then dK / dV kernel                                                  */
  GSL_ATTN_BWD_F32 = 13,         /* f32, T <= 224: the matrix-core dQ and dK / dV kernels (panel as in the forward)               */
  GSL_ATTN_FWD_CLS = 14,         /* cls forward, T <= 256 (either dtype)                                                          */
  GSL_ATTN_FWD_CLS_LONG = 15,    /* cls forward, T > 256: 256-key chunks with an online max / sum                                 */
  GSL_ATTN_BWD_CLS = 16          /* cls backward, any T                                                                           */
};
GSL_API int gsl_attention_kernel_choice(int B, int T, int H, int dtype, int qkv_layout, int direction);

/* ---- K9 LoRA gradient (skinny, reduction over M rows): G[n*gsn + j*gsj] (+)= sum_m Y[m,n] * U[m,j]
 * Y[dtype] [M,N] with row stride ldy >= N elements (a column block of a wider tensor is allowed), U[dtype] [M,ldu] (first r columns
 * used, 1 <= r <= 64, ldu >= max(16, r), ldu % 8 == 0). Which columns of U are READ (U may itself be a column block of a wider tensor):
 *   r <= 16: columns 0..15 — columns r..15 must be readable zeros or belong to other adapters whose products are discarded;
 *   r > 16:  the form for 16-bit operands with 16-byte aligned U / Y and rows (N % 256 == 0, M >= 64, ldu >= 8 * ceil(r / 8)) reads
 *            the columns [0, 8 * ceil(r / 8)); every other form reads exactly the columns [0, r). Nothing else is read, and no result
 *            depends on a column outside [0, r). An aligned block at column offset c of a 64-wide tensor has c % 8 == 0, so
 *            c + r <= 64 gives c + 8 * ceil(r / 8) <= 64: the block may end at the row end.
 * The partial sums are laid out part[split][n][R] with the padded rank R in {8, 16, 32, 64}; the sums keep a fixed order (no atomics).
 * ws f32 >= gsl_lora_grad_ws_elems(): the largest need of any call with this (M, N, r), 0 where every call is refused (M, N <= 0, r outside
 * [1, 64], N % 4 != 0). gscale (nullable): device {S, 1/S} of a loss-scaled backward (see gsl_head_bwd): the sums are multiplied by 1/S
 * before they are stored / accumulated. */
GSL_API long gsl_lora_grad_ws_elems(int M, int N, int r);
GSL_API int gsl_lora_grad(const void* Y, long ldy, const void* U, int ldu, float* G, long gsn, long gsj,
                  int M, int N, int r, int dtype, int accumulate, float* ws, const float* gscale, gsl_stream_t s);
/* The same for n reductions in two launches per 24 descriptors (the launch-bound regime: a few-shot step runs 24 of them). 16-bit operands
 * only (dtype GSL_BF16 or GSL_F16, one format per call; gscale as above), N % 256 == 0, 16-byte aligned rows; any M >= 1. `descs` is a HOST array — the launches carry the descriptors by value, so a captured
 * HIP graph keeps them. The G of one call must not overlap. Entries of different ranks (1 <= r <= 64) may share a call; every entry runs
 * the aligned 16-bit form of gsl_lora_grad (the same bits as the single call), so U, ldu and the columns read follow its rule. ws: gsl_lora_grad_batch_ws_elems(descs, n) floats (-1: invalid descriptor). */
typedef struct gsl_lgrad_desc {
  const void* Y; long ldy; const void* U; int ldu; int M; int N; int r; int accumulate; int pad_; float* G; long gsn, gsj;
} gsl_lgrad_desc;
GSL_API long gsl_lora_grad_batch_ws_elems(const gsl_lgrad_desc* descs, int n);
GSL_API int gsl_lora_grad_batch(const gsl_lgrad_desc* descs, int n, float* ws, int dtype, const float* gscale, gsl_stream_t s);

/* The launch plan: how gsl_lora_grad runs a call — a function of the shape, the dtype, the row strides and the 16-byte alignment of Y and
 * U, the same one the launch calls. Takes the operand arguments of gsl_lora_grad with the same checks (GSL_ERR_ARG and the same message
 * where the launch refuses) and dereferences no pointer: it runs without a device, on made-up addresses. The development build's
 * GSL_LORA_GRAD_MFMA knob applies to it as to the launch.
 *   form    the partial kernel: the matrix-core form (16-bit operands, N % 256 == 0, M >= 64, 16-byte aligned U / Y and rows,
 *           ldu >= the columns it reads) or the VALU form (everything else)
 *   R       padded rank of the partial layout part[split][n][R]: 8, 16, 32 or 64
 *   bx      column blocks of the partial grid: N / 256 (MFMA), ceil(N / vector width / CG) (VALU)
 *   nsplit  row splits of the partial grid; split k owns the rows [k * rps, min(M, (k + 1) * rps))
 *   rps     rows per split (MFMA: a multiple of its 32-row slab)
 *   CG      VALU form: column groups of a workgroup, 64, 128 or 256 (its 256 threads walk 256 / CG interleaved row phases); MFMA: 0
 *   reduce  what sums the splits: one kernel over all of them (DIRECT, at most 32 splits), a first level over slabs of 32 consecutive
 *           splits and a second over the slabs (TWO_LEVEL), or the single launch whose four waves each own every fourth split (ONE_LAUNCH:
 *           MFMA form, at most 160 splits, N * R >= 8192) */
enum gsl_lgrad_form { GSL_LGRAD_MFMA = 0, GSL_LGRAD_VALU = 1 };
enum gsl_lgrad_reduce { GSL_LGRAD_REDUCE_DIRECT = 0, GSL_LGRAD_REDUCE_TWO_LEVEL = 1, GSL_LGRAD_REDUCE_ONE_LAUNCH = 2 };
typedef struct gsl_lgrad_plan { int form, R, bx, nsplit, rps, CG, reduce; } gsl_lgrad_plan;
GSL_API int gsl_lora_grad_plan(const void* Y, long ldy, const void* U, int ldu, int M, int N, int r, int dtype, gsl_lgrad_plan* out);
/* The same for gsl_lora_grad_batch(descs, n, ...): out[k] is the plan of entry k (always the aligned matrix-core body, summed by the batch
 * reducer in split order). The row splits of an entry depend on the other entries of its group of 24 descriptors. GSL_ERR_ARG, with the
 * message of the launch, for a descriptor the launch refuses. */
typedef struct gsl_lgrad_batch_plan { int R, bx, nsplit, rps; } gsl_lgrad_batch_plan;
GSL_API int gsl_lora_grad_batch_plan(const gsl_lgrad_desc* descs, int n, gsl_lgrad_batch_plan* out);


/* ---- K10 head: cls pool + LayerNorm + CosFace (vit_face.py:540-546, 171-208; s=64, m=0.35); ArcFace through the margin pair below.
 * linear_head != 0 selects the ViT-B/16 path instead (modified_VIT.py:32-38): logits = emb * W^T + head_bias, with Wn = W
 * un-normalised and cos_s = 1 on the backward side. */
GSL_API int gsl_cosface_prep(const float* W, float* Wn, int C, int D, gsl_stream_t s);   /* Wn = F.normalize(W) */
GSL_API int gsl_head_fwd(const void* x, int x_dtype, int T, const float* gamma, const float* beta, float eps,
                 const float* Wn, const int64_t* label, float* emb, float* mean, float* rstd,
                 float* logits, int B, int D, int C, float cos_s, float cos_m,
                 const float* head_bias, int linear_head, int pool_mean, gsl_stream_t s);
/* pool_mean = 0: the head pools token 0 (pool='cls'); 1: the mean over the T tokens (pool='mean', vit_face.py:540).
 * x is `x_dtype` (the residual stream, see gsl_layernorm_fwd).
 * dlogits [B,C] / demb [B,D] nullable. dx [B*T,D]: with pool='cls' the cls rows get the gradient and the others are zeroed,
 * with pool='mean' every token row gets d pooled / T. dxb[dtype] = dx * dropmask(site) (nullable). dx is `stream_dtype` (see
 * gsl_layernorm_bwd). compact != 0 (pool='cls' only): dx / dxb are [B,D], the cls rows alone — nothing is zero-filled; the dropout
 * counters stay those of the dense tensor.
 * gscale != NULL (fp16 operands): LOSS-SCALED backward. The kernel runs twice: pass 1 writes max|d loss / d stream| of every image to
 * amax_ws [B], pass 2 picks the power of two S with S * max in [2^10, 2^11), stores dx / dxb multiplied by S and publishes
 * gscale[0..1] = {S, 1/S} on the device (no host sync; HIP-graph safe). Every kernel downstream is linear in the gradient; the
 * LoRA-gradient reductions take gscale and divide S out.
 * The scale rule, exactly: max = m 2^ex with m in [0.5, 1) (frexp), S = 2^(E - ex), the exponent clamped to +-60 — a maximum that is a
 * power of two lands on 2^(E-1). max = 0 (every gradient zero): S = 1. gscale[1] is 1 / S, exact.
 * Non-finite gradients: an image whose gradient holds a NaN (a NaN or Inf row of dlogits: Inf - Inf in the sum over the classes) gets a
 * non-finite dx and its maximum is PASSED OVER (fmaxf): S is the rule's value for the largest finite image maximum, every other image is
 * S times its gradient, and gscale[0..1] stay finite powers of two. An image maximum of +Inf (no NaN in its row) gives S = 1. The
 * non-finite image reaches the overflow guard below through the LayerNorm backwards that read its dx.
 * Zero embeddings: F.normalize's clamp has derivative 0 below it, so an image with ||emb|| < 1e-12 (a constant row with beta = 0, or
 * any embedding under the clamp) gets d emb = d e-hat / 1e-12 without the projection term, as autograd gives the reference.
 * Overflow guard (round 6; GradScaler semantics without a host sync). gscale is f32 [4] that PERSISTS across steps (zero it once):
 *   [2] = the largest |scaled gradient| the LayerNorm backwards of this backward saw (gsl_layernorm_bwd's gmax; reset to 0 here),
 *   [3] = the exponent E in use: S * max lands in [2^(E-1), 2^E).
 * Pass 1 reads the PREVIOUS backward's [2]: >= 65504 (a 16-bit store saturated) or non-finite -> E drops by 2 (floor 4); below 2^9 with E
 * under target_exp -> E grows by 1; an E outside [4, 15] (the zeroed buffer) -> target_exp. target_exp: 0 = the default 11 (32x headroom at the head;
 * the largest gradient operand of a depth-6 chain measured 1.2x the head's). gsl_adamw_flat / _dev skip the update of a step whose [2] saturated.
 * Number of classes. Any C >= 1. C <= 1024: the per-image kernels; amax_ws is [B] floats and may be NULL without gscale, as above.
 * C > 1024: the class-tiled kernels (gsl_head_fwd*: the logits are a tiled f32 GEMM behind the per-image pool + LayerNorm; gsl_head_bwd*:
 * d e-hat = (s dlogits) . Wn is a tiled f32 GEMM that runs ONCE, also in the loss-scaled form). WORKSPACE CONTRACT for C > 1024: amax_ws is
 * REQUIRED in every mode, also with gscale == NULL, and holds B*(D+1) floats — [0, B) the per-image maxima as above, [B, B + B*D) d e-hat.
 * Supported range for C > 1024: B*C and C*D below 2^31 elements, Wn and emb 16-byte aligned; anything else is an argument error by name
 * before any launch (so is amax_ws == NULL). Results are bit-repeatable, and row b's do not depend on B. */
GSL_API int gsl_head_bwd(const float* dlogits, const float* demb, const void* x, int x_dtype, int T, const float* gamma,
                 const float* mean, const float* rstd, const float* emb, const float* Wn,
                 void* dx, void* dxb, int B, int D, int C, float cos_s, int dtype, int stream_dtype,
                 float p_drop, uint64_t seed, uint32_t site, int linear_head, int pool_mean, int compact,
                 float* gscale, float* amax_ws, int target_exp, gsl_stream_t s);
/* The margin pair: gsl_head_fwd / gsl_head_bwd with the head chosen by head_kind.
 *   head_kind 0 = CosFace: the kernels of gsl_head_fwd / gsl_head_bwd, bit for bit (cos_m is the margin; m, easy_margin, cos_y and
 *                 label are not read).
 *   head_kind 1 = ArcFace (vit_face.py:72-143; s=64, m=0.5, easy_margin=0): the label column of the logits is
 *                 s * phi(cos), phi = cos*cos(m) - sqrt(1 - cos^2)*sin(m) if cos > cos(pi - m) (easy_margin: cos > 0), else
 *                 cos - sin(pi - m)*m (easy_margin: cos); cos_m is not read, linear_head must be 0. The constants are computed
 *                 from the double m as the reference's math.* does, then rounded to float. The forward writes cos_y [B] = the
 *                 label column's cosine before the margin; the backward reads it (and label) to take the same branch and scales
 *                 dlogits[y] by d phi / d cos. A label outside [0, C) (-1, C, a value beyond 32 bits: the comparison is 64-bit)
 *                 names no class: no column takes the margin or the factor, and cos_y[b] is NOT written (nor read). logits = NULL:
 *                 cos_y is not written at all. The branch is a strict `>`: cos = th (easy margin: cos = +-0) takes cos - mm (cos)
 *                 in the forward and d phi = 1 in the backward. One departure: 1 - cos^2 is clamped at 0 and the derivative divides by
 *                 max(sine, 1e-6) (the reference gives NaN for |cos| > 1 and an infinite gradient at |cos| = 1).
 * Every other argument means what it means for gsl_head_fwd / gsl_head_bwd. */
GSL_API int gsl_head_fwd_margin(const void* x, int x_dtype, int T, const float* gamma, const float* beta, float eps,
                 const float* Wn, const int64_t* label, float* emb, float* mean, float* rstd,
                 float* logits, int B, int D, int C, float cos_s, float cos_m,
                 const float* head_bias, int linear_head, int pool_mean, int head_kind, double m, int easy_margin,
                 float* cos_y, gsl_stream_t s);
GSL_API int gsl_head_bwd_margin(const float* dlogits, const float* demb, const void* x, int x_dtype, int T, const float* gamma,
                 const float* mean, const float* rstd, const float* emb, const float* Wn,
                 void* dx, void* dxb, int B, int D, int C, float cos_s, int dtype, int stream_dtype,
                 float p_drop, uint64_t seed, uint32_t site, int linear_head, int pool_mean, int compact,
                 float* gscale, float* amax_ws, int target_exp, int head_kind, double m, int easy_margin,
                 const float* cos_y, const int64_t* label, gsl_stream_t s);

/* ---- K10w head weight gradient: d loss / d W of the classifier head from dlogits — the one trainable tensor of the linear-probe driver
 * (train/backbone_forget_main.py:596-600 freezes everything but the parameters named "loss", :657-670 retrains them with plain CE; the
 * baseline drivers' --ffn_open, train_own_forget_cl.py:426). What autograd gives the reference for vit_face.py:181-207 (CosFace),
 * :117-141 (ArcFace) and :47-50 (Softmax). All arithmetic f32.
 *   head_kind 0 = CosFace, 1 = ArcFace, 2 = linear (the Softmax head; cos_s, m, easy_margin, W, label and cos_y are not read).
 *   dlogits [B,C], emb [B,D] (the LayerNorm output gsl_head_fwd* writes, not normalised), W [C,D] the RAW weight, label [B] / cos_y [B]
 *   (ArcFace only: cos_y as written by gsl_head_fwd_margin).
 *   G[b,c] = cos_s * dlogits[b,c]; ArcFace multiplies the label column by d phi / d cos at cos_y[b] — the expression gsl_head_bwd_margin
 *   uses, a label outside [0, C) included (no column is scaled), so both take the same branch.
 *   d What_c = sum_b G[b,c] emb_b / max(||emb_b||, 1e-12);  dW_c = (d What_c - What_c (What_c . d What_c)) / ||W_c||, What_c = W_c / ||W_c||;
 *   ||W_c|| < 1e-12: dW_c = d What_c / 1e-12 (the derivative of F.normalize's clamp, as torch).
 *   linear: dW_c = sum_b dlogits[b,c] emb_b and, with dbias != NULL, dbias_c = sum_b dlogits[b,c]. dbias must be NULL for the cosine heads.
 * dW [C,D] and dbias [C] are plain stores of every element (no pre-zeroing, no accumulation), nothing else is written. No allocation, no
 * sync, no atomics, no workspace; two calls agree bit for bit; capturable in a HIP graph. Any B >= 1, any C >= 1 (no buffer is sized by B or
 * C; indices are size_t, B*C may exceed 2^31), D <= 1024.
 * Dispatch, on the call alone:
 *   C <= 1024  the per-class kernel (a workgroup of 16 waves per one or two classes): the sum over b runs per wave ascending, the 16 waves
 *              added in wave order — an order fixed by (B, C, D). The bits are what they always were.
 *   C > 1024   the class-tiled kernel, when its preconditions hold: D % 4 == 0 and emb 16-byte aligned (it loads emb as float4; dlogits,
 *              whose rows start at any dword, W and dW need no alignment). d What = G^T e-hat on v_mfma_f32_16x16x4_f32 (exact f32), a
 *              workgroup per 16 classes (C < 16384) or 64 classes, all D columns, ONE launch. Order of summation: every element of dW
 *              (and dbias) is one chain from 0 over ascending b, with zero-filled padding to the end of the last tile of 16 images (8 at
 *              D > 512) — no split of B over waves or workgroups. Row c of dW depends on neither C nor the tile c falls in; the linear
 *              kind equals gsl_gemm_nt(dlogits^T, emb^T) in f32 bit for bit. Row norms: a wave per row, an order fixed by D.
 *   C > 1024 and a precondition not met: the call falls back to the per-class kernel. It is never refused for its alignment or its D:
 *              the argument checks are the same at every C. */
GSL_API int gsl_head_wgrad(const float* dlogits, const float* emb, const float* W, const int64_t* label, const float* cos_y,
                 float* dW, float* dbias, int B, int C, int D, int head_kind, float cos_s, double m, int easy_margin,
                 gsl_stream_t s);

/* ---- K11 cross entropy (mean) + top-1 (engine_cl.py:65-78, util/utils.py:354-368).
 * out2 f32 [2] = { sum_i CE_i , #correct }; row_ws f32 [2*B] scratch (per-row loss / hit, summed in a fixed order).
 * Row loss = lse - x[y] with lse = max + log(sum exp(x - max)): its absolute error is half an ulp of |lse| (not of the loss), see
 * oracle/loss_probes.py for the bounds the tests hold every output to. A row counts as correct when its label is the FIRST index of the row
 * maximum (torch.argmax's rule on ties). Non-finite logits: -inf outside the label's place is an ordinary value (finite loss, gradient
 * exactly 0 there); -inf at the label gives +inf; +inf or NaN anywhere gives a NaN row loss, as torch does (the arg-max skips a NaN: the
 * row's hit is that of its other logits). A label outside [0, C): NaN
 * row loss (and sum), no hit, a NaN gradient row from gsl_ce_bwd; nothing outside the row is read or written. */
GSL_API int gsl_ce_fwd(const float* logits, const int64_t* labels, float* out2, float* row_ws, int B, int C, gsl_stream_t s);
/* dlogits (+)= coef[0] * scale * (softmax - onehot) ; coef is a DEVICE scalar (no host sync). accumulate = 1: every element is fl(old + g)
 * with g the value accumulate = 0 stores (two roundings, no fused multiply-add); the same holds for gsl_proto_kl_bwd / gsl_proto_l2_bwd. */
GSL_API int gsl_ce_bwd(const float* logits, const int64_t* labels, const float* coef, float scale,
               float* dlogits, int B, int C, int accumulate, gsl_stream_t s);

/* ---- K13 prototype KL (engine_cl.py:571-603): out1[0] = sum_i KL(softmax(proto[y_i]) || softmax(emb_i)). */
GSL_API int gsl_proto_kl_fwd(const float* emb, const int64_t* labels, const float* proto, float* out1, float* row_ws /*[B]*/,
                     int B, int D, int C, gsl_stream_t s);
GSL_API int gsl_proto_kl_bwd(const float* emb, const int64_t* labels, const float* proto, const float* coef,
                     float scale, float* demb, int B, int D, int C, int accumulate, gsl_stream_t s);

/* ---- K13b prototype l2 (engine_cl.py:593-594, engine.py:712-713: torch.mean((output - prototype_tensor) ** 2)), in the sum form of the
 * KL pair: out1[0] = sum_i (1/D) sum_d (emb[i,d] - proto[y_i,d])^2 — divided by the row count it is the reference's mean, and it takes the
 * place of the KL sums in gsl_loss_combine / gsl_loss_combine_pack. f32 accumulation, one wave per row, fixed-order row sum through
 * row_ws [B]. A label outside [0, C) or a NaN table row (a class without a prototype) gives a NaN sum. */
GSL_API int gsl_proto_l2_fwd(const float* emb, const int64_t* labels, const float* proto, float* out1, float* row_ws /*[B]*/,
                     int B, int D, int C, gsl_stream_t s);
/* demb (+)= coef[0] * scale * (2/D) * (emb - proto[y]) ; coef is a DEVICE scalar (no host sync). */
GSL_API int gsl_proto_l2_bwd(const float* emb, const int64_t* labels, const float* proto, const float* coef,
                     float scale, float* demb, int B, int D, int C, int accumulate, gsl_stream_t s);

/* ---- K11b precision@k for several k in one launch (util/utils.py:354-368): hits[j] = number of rows whose label is among the ks[j]
 * largest logits, counted as "fewer than ks[j] logits are strictly greater than the label's" (equal to output.topk(ks[j]) wherever the
 * ks[j]-th place is not tied). ks: HOST array of nk <= gsl_topk_max_k() positive ints (it travels in the kernel arguments);
 * hits: DEVICE int32 [nk], cleared by the call. An out-of-range label is never a hit. On a tie at the ks[j]-th place the rule counts every
 * row whose label's logit EQUALS the ks[j]-th largest as a hit (torch.topk picks one of the equals); k >= C counts every valid row. */
GSL_API int gsl_topk_max_k(void);
GSL_API int gsl_topk_hits(const float* logits, const int64_t* labels, int B, int C, const int* ks, int nk, int* hits, gsl_stream_t s);

/* ---- scalar tail of the step (engine_cl.py:65-125, single process): from the batch SUMS of the kernels above
 *   total = beta*relu(BND - ce_f_sum/n_f) + ce_r_sum/n_r + alpha*structure + w_f*relu(BND_pro - kl_f_sum/n_f) + w_r*kl_r_sum/n_r
 * meters8 = [beta*loss_forget, loss_remain, total, alpha*structure, top1_forget %, top1_remain %, proto_f, proto_r],
 * coefs5 = d total / d {ce_r_sum, ce_f_sum, kl_f_sum, kl_r_sum, structure} (relu'(0) = 0). kl_* / structure nullable (term absent).
 * Without the prototype term meters8[6] still logs w_f * relu(BND_pro), as the reference does; the total does not contain it.
 * Every operation is a single f32 rounding in the order of the reference's torch expression (bit-equal to oracle/loss_probes.py tail32).
 * relu keeps a NaN as torch's does: a NaN forget sum (a label out of range, a class without a prototype) gives a NaN total and NaN
 * meters8[0] / [2] / [6]; the coefficient of a NaN hinge is 0. n_r > 0 and n_f > 0 are required.
 * All inputs and outputs are device scalars / small device arrays: no host sync. */
GSL_API int gsl_loss_combine(const float* ce_r_sum, const float* ce_f_sum, const float* kl_f_sum, const float* kl_r_sum,
                     const float* structure, const float* hit_r, const float* hit_f, float n_r, float n_f,
                     float beta, float BND, float alpha, float w_f, float w_r, float BND_pro,
                     float* total, float* meters8, float* coefs5, gsl_stream_t s);

/* Data-parallel form of the scalar tail (SURVEY 8(e) collective C2; reference semantics train_own_forget_cl.py:494-497, engine_cl.py:78,99):
 * pack8 = the sum-all-reduced [ce_r_sum, ce_f_sum, hit_r, hit_f, n_r, n_f, kl_f_sum, kl_r_sum] — global batch sums and sizes, all on the
 * device. Same outputs as gsl_loss_combine; coefs5 are the derivatives with respect to THIS rank's local sums (= those of the global sums).
 * n_r and n_f are device values and are NOT checked. n_f = 0 (no forget row on any rank; then ce_f_sum = hit_f = kl_f_sum = 0) gives
 * what the reference's mean over an empty batch gives: 0 / 0 = NaN in the forget hinges, so total, meters8[0], [2], [4] and (with the
 * prototype term) [6] are NaN, coefs5[1] = coefs5[2] = 0, and the remain-side outputs (meters8[1], [5], [7], coefs5[0], [3], [4]) are
 * those of the remain rows alone. n_r = 0 likewise turns the remain side and the total NaN (coefs5[0] and [3] are +-inf). */
GSL_API int gsl_loss_combine_pack(const float* pack8, const float* structure, int has_proto, float beta, float BND, float alpha, float w_f,
                          float w_r, float BND_pro, float* total, float* meters8, float* coefs5, gsl_stream_t s);
/* The loss section of a single-process step in ONE launch (launch-bound batches): per-row CE / top-1 of logits [N,C] and prototype KL of
 * emb [N,D] against proto [Cp,D] (emb NULL: no prototype term), their sums over the remain rows [0,nr) and the forget rows [nr,N), the scalar
 * tail of gsl_loss_combine (out14 = total, meters8, coefs5) and the backward of all of it for an upstream gradient of 1: dlogits [N,C],
 * demb [N,D]. Coefficients and gradients bit-identical to (meters within an ulp of) gsl_ce_fwd + gsl_proto_kl_fwd + gsl_loss_combine + gsl_ce_bwd + gsl_proto_kl_bwd on the two row
 * ranges. 0 < nr < N <= gsl_loss_tail_max_rows(). structure (nullable): device scalar, the group-lasso value. */
GSL_API int gsl_loss_tail_max_rows(void);
GSL_API int gsl_loss_tail(const float* logits, const int64_t* labels, int N, int nr, int C, const float* emb, const float* proto, int D,
                  int Cp, const float* structure, float beta, float BND, float alpha, float w_f, float w_r, float BND_pro,
                  float* out14, float* dlogits, float* demb, gsl_stream_t s);
/* gsl_loss_tail with the l2 prototype distance (engine_cl.py:593-594) in place of the KL: emb, proto and demb are required. Coefficients
 * and gradients bit-identical to (meters within an ulp of) gsl_ce_fwd + gsl_proto_l2_fwd + gsl_loss_combine + gsl_ce_bwd + gsl_proto_l2_bwd
 * on the two row ranges. */
GSL_API int gsl_loss_tail_l2(const float* logits, const int64_t* labels, int N, int nr, int C, const float* emb, const float* proto, int D,
                  int Cp, const float* structure, float beta, float BND, float alpha, float w_f, float w_r, float BND_pro,
                  float* out14, float* dlogits, float* demb, gsl_stream_t s);



/* ---- K12 group-lasso norms over a flat LoRA buffer (engine_cl.py:349-432, util/cal_norm.py:4-146).
 * tensor t = flat[toff[t] .. +tnumel[t]) belongs to group tgroup[t] (tables on device, int64/int64/int32).
 * Outputs (f32 unless noted): tensor_sumsq[ntensors], group_norm[ngroups] = sqrt(sum sumsq),
 * cal_norm[ngroups] = sum sqrt(sumsq) (cal_norm.py 'L2'), loss[1] = sum_g group_norm,
 * mask u8[ngroups] = group_norm > tau.  partial_ws f32 [ntensors*GSL_NORM_SPLIT]. */
#define GSL_NORM_SPLIT 8
GSL_API int gsl_group_norms_fwd(const float* flat, const int64_t* toff, const int64_t* tnumel, const int32_t* tgroup,
                        int ntensors, int ngroups, float tau, float* partial_ws, float* tensor_sumsq,
                        float* group_norm, float* cal_norm, float* loss, uint8_t* mask, gsl_stream_t s);
/* gradflat[i] += coef[0]*scale * flat[i] / group_norm[g(i)]  (0 where group_norm == 0). */
GSL_API int gsl_group_norms_bwd(const float* flat, const int64_t* toff, const int64_t* tnumel, const int32_t* tgroup,
                        int ntensors, const float* group_norm, const float* coef, float scale,
                        float* gradflat, gsl_stream_t s);

/* ---- K14 fused AdamW over a flat buffer (torch.optim.AdamW as timm.create_optimizer builds it,
 * train_own_forget_cl.py:811-813): decoupled wd, bias correction, step >= 1. */
GSL_API int gsl_adamw_flat(float* p, const float* g, float* m, float* v, long n,
                   float lr, float beta1, float beta2, float eps, float wd, int step, const float* guard, gsl_stream_t s);
/* guard (nullable): device f32 — the overflow guard of a loss-scaled fp16 backward (gscale + 2 of gsl_head_bwd). The update is SKIPPED
 * (p, m, v untouched; torch.cuda.amp.GradScaler.step semantics) when *guard >= 65504 or is not finite: a gradient of this step was clipped. */
/* HIP-graph form of the same update: the step count t (>= 1, int64) and the learning rate (f32) are read from device memory,
 * so a captured graph of the whole forgetting step replays with fresh values (bias corrections 1 - beta^t in f64 in-kernel). */
GSL_API int gsl_adamw_flat_dev(float* p, const float* g, float* m, float* v, long n, const float* lr_dev, float beta1, float beta2,
                       float eps, float wd, const int64_t* step_dev, const float* guard, gsl_stream_t s);

/* ---- helpers: f32 -> dtype casts for the frozen-weight caches and padded LoRA operands. Round to nearest even; a FINITE value beyond the
 * largest finite value of the 16-bit type saturates to it — +-65504 in fp16 and, as measured on the MI355X (the kernels set the
 * saturation mode bit, which the bf16 convert honours too), +-3.3895e38 (0x7f7f) in bf16, where rounding alone would give Inf —; Inf and
 * NaN stay Inf and NaN (tests/test_hip_flat_edges.py). gsl_transpose_cast and gsl_pack_pad convert the same way. */
GSL_API int gsl_cast(const float* in, void* out, long n, int dtype, gsl_stream_t s);
/* out[dtype] [C,R] = in[R,C]^T */
GSL_API int gsl_transpose_cast(const float* in, void* out, int R, int C, int dtype, gsl_stream_t s);
/* out[dtype] [rows_out, ld_out] zero-padded copy: out[i, j] = scale * in[i*si + j*sj] for i<rows, j<cols. */
GSL_API int gsl_pack_pad(const float* in, long si, long sj, int rows, int cols, float scale,
                 void* out, int rows_out, int ld_out, int dtype, gsl_stream_t s);
/* The same for n packs in one launch. descs_dev: device array of n descriptors (all outputs share `dtype`); max_elems =
 * max over descriptors of rows_out * ld_out. The table is built once by the host and reused every step (HIP-graph friendly). */
typedef struct gsl_pack_desc {
  const float* in; long si, sj; int rows, cols; float scale; int pad_; void* out; int rows_out, ld_out;
} gsl_pack_desc;
GSL_API int gsl_pack_pad_batch(const gsl_pack_desc* descs_dev, int n, long max_elems, int dtype, gsl_stream_t s);

/* ---- face verification on pairs (util/utils.py:167-230 perform_val, util/verification.py evaluate / calculate_val); csrc/verif.hip.
 * V1, mode GSL_VERIF_FLIP_SUM: e0, e1 f32 [2P, D] (row stride ld elements) = the embeddings of the original and of the flipped images (rows
 * 2p, 2p + 1 = pair p), D <= 1024. Per row s = e0 + e1, n = s / ||s|| (a zero row stays zero, as sklearn.preprocessing.normalize);
 * dist[p] = sum (n[2p] - n[2p+1])^2; xnorm[0] = mean of the 4P row norms of e0 and e1. pair_norm_ws f32 [P] scratch; nemb (nullable) f32
 * [2P, D] receives n. Mode GSL_VERIF_PLAIN: e0, e1 [P, D], dist[p] = sum (e0[p] - e1[p])^2 (xnorm, pair_norm_ws, nemb unused) — on the nemb
 * of the other mode the same distances bit for bit. One wave64 per pair, fixed-order sums. */
enum { GSL_VERIF_FLIP_SUM = 0, GSL_VERIF_PLAIN = 1 };
GSL_API int gsl_verif_pair_dist(const float* e0, const float* e1, long ld, int P, int D, int mode, float* dist, float* xnorm,
                        float* pair_norm_ws, float* nemb, gsl_stream_t s);
/* V2: decision counts of the un-shuffled KFold(nrof_folds) TEST folds (contiguous, the first P % F one longer): counts int32 [F][Tn][2] =
 * { #(dist < thr & same), #(dist < thr & different) } with the compare (double)dist < thresholds[t], strict (np.less); fold_tot int32 [F][2] =
 * { same, different } pairs of the fold. The thresholds (f64, any order) are taken as given. The train counts of a fold are the totals minus it. */
GSL_API int gsl_verif_fold_counts(const float* dist, const uint8_t* issame, int P, const double* thresholds, int Tn, int nrof_folds,
                          int* counts, int* fold_tot, gsl_stream_t s);
/* V3: out f64 [2F + 2Tn + 1] = accuracy[F] (test accuracy at the fold's best threshold), best_threshold[F] (first arg-max of the train
 * accuracy, np.argmax's tie rule), tpr[Tn], fpr[Tn] (means over the folds in fold order, 0 where a fold has no same / different pair), and
 * (double)xnorm[0] if xnorm is given. Integer arithmetic up to the final IEEE f64 divisions. */
GSL_API int gsl_verif_select(const int* counts, const int* fold_tot, const double* thresholds, int Tn, int nrof_folds, const float* xnorm,
                     double* out, gsl_stream_t s);

/* ---- per-class evaluation (test/test_own.py:99-144 per-class accuracy, util/utils.py:527-547 class prototypes); csrc/classstat.hip.
 * All buffers are DEVICE buffers of the caller that persist across batches (clear them once, call per batch, finish once); no call
 * allocates, synchronises or uses a floating-point atomic, so every one of them can be captured in a HIP graph.
 * S1 (test_own.py:120-130): logits f32 [B, C] with row stride ld (elements), labels int64 [B]. Per row the prediction is the FIRST arg-max
 * of the row as torch.max(outputs, 1) returns it (a NaN ranks above every number); count[label] += 1, hit[label] += (prediction == label),
 * and, when confusion (int32 [C, C], nullable) is given, confusion[label][prediction] += 1 (a cell holds < 2^31 samples). count, hit: int64
 * [C]. A label outside [0, C) adds one to bad[0] (int64) and touches nothing else. Integer adds: independent of the order of the rows. */
GSL_API int gsl_class_stats(const float* logits, long ld, const int64_t* labels, int B, int C, int64_t* count, int64_t* hit, int64_t* bad,
                    int* confusion, gsl_stream_t s);
/* S2 (util/utils.py:540-542, `embeds_sum[label] += embed; embeds_count[label] += 1`): emb f32 [B, D] with row stride ld, sum f32 [C, D],
 * count int64 [C]. sum[c, :] += emb[i, :] for the rows with labels[i] == c in increasing i, one plain f32 add per row on top of the value
 * already in sum: over any split of a data set into batches the result is the reference's sequential sum bit for bit. count[c] += the
 * number of such rows; labels outside [0, C) are counted in bad[0] and skipped. D <= 2^20. */
GSL_API int gsl_class_embed_sum(const float* emb, long ld, const int64_t* labels, int B, int D, int C, float* sum, int64_t* count,
                        int64_t* bad, gsl_stream_t s);
/* S3: acc f64 [C] (nullable; needs hit) = 100 * hit / count, the f64 division of test_own.py:134 / :142; proto f32 [C, D] (nullable; needs
 * sum) = sum / count, the f32 division of util/utils.py:547. Classes with count == 0 hold NaN. */
GSL_API int gsl_class_finish(const int64_t* count, const int64_t* hit, const float* sum, int C, int D, double* acc, float* proto,
                     gsl_stream_t s);

/* dropout keep-mask as the kernels compute it (for tests): keep[i] = 1/0 for element index i. */
GSL_API int gsl_dropout_mask(uint8_t* keep, long n, float p_drop, uint64_t seed, uint32_t site, gsl_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* GSLORA_HIP_H */
