// head.hip — the two ends of the network and the scalar losses:
//   K1  patch gather (einops rearrange, vit_pytorch_face/vit_face.py:530); K1s its overlapping-window form (nn.Unfold, vits_face.py:446-450)
//   K10 cls-pool + LayerNorm + CosFace / ArcFace margin head (vit_face.py:540-546, 171-208, 72-143) fwd / bwd
//       ArcFace departs from the reference in one place: sine = sqrt(max(1 - cos^2, 0)) and its derivative divides by max(sine, 1e-6),
//       where the reference's sqrt returns NaN at |cos| > 1 (rounding) and an infinite gradient at |cos| = 1.
//   K11 mean cross-entropy + top-1 (engine_cl.py:65-78, util/utils.py:354-368) fwd / bwd
//   K13 prototype KL (engine_cl.py:571-603) fwd / bwd; K13b prototype l2 (engine_cl.py:593-594) fwd / bwd; K11b precision@k
// All are tiny next to the GEMMs; they exist so that a step needs no host sync and no [B,C]-sized
// PyTorch elementwise chain. Upstream gradient scalars arrive as DEVICE pointers (coef).
#include <cmath>

#include "gsl_common.h"

using namespace gsl;

// ------------------------------------------------------------------ K1 patchify
template <typename T>
__global__ void patchify_kernel(const float* __restrict__ img, T* __restrict__ out, int B, int C, int H, int W, int p) {
  fp16_sat_on();
  const int hp = H / p, wp = W / p, Tn = 1 + hp * wp, Kp = p * p * C;
  const long total = (long)B * Tn * p * p;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int p2 = (int)(idx % p);
    const int p1 = (int)((idx / p) % p);
    const int t = (int)((idx / (p * p)) % Tn);
    const int b = (int)(idx / ((long)p * p * Tn));
    T* o = out + ((size_t)b * Tn + t) * Kp + (size_t)(p1 * p + p2) * C;
    if (t == 0) {
      for (int c = 0; c < C; ++c) Elem<T>::st(o + c, 0.f);
    } else {
      const int h = (t - 1) / wp, w = (t - 1) % wp;
      const float* src = img + ((size_t)b * C * H + (size_t)(h * p + p1)) * W + (size_t)(w * p + p2);
      for (int c = 0; c < C; ++c) Elem<T>::st(o + c, src[(size_t)c * H * W]);
    }
  }
}

extern "C" int gsl_patchify(const float* img, void* out, int B, int C, int H, int W, int p, int dtype, gsl_stream_t s) {
  GSL_CHECK_ARG(img && out && B > 0 && C > 0 && p > 0 && H % p == 0 && W % p == 0, "shape");
  const long total = (long)B * (1 + (H / p) * (W / p)) * p * p;
  const int grid = (int)min((total + 255) / 256, (long)(256 * 16));
  if (dtype == GSL_BF16) hipLaunchKernelGGL(patchify_kernel<bf16_t>, dim3(grid), dim3(256), 0, as_stream(s), img, (bf16_t*)out, B, C, H, W, p);
  else if (dtype == GSL_F16) hipLaunchKernelGGL(patchify_kernel<f16_t>, dim3(grid), dim3(256), 0, as_stream(s), img, (f16_t*)out, B, C, H, W, p);
  else if (dtype == GSL_F32) hipLaunchKernelGGL(patchify_kernel<float>, dim3(grid), dim3(256), 0, as_stream(s), img, (float*)out, B, C, H, W, p);
  else return fail(GSL_ERR_ARG, "gsl_patchify: bad dtype%s %ld", "", dtype);
  return check_launch("gsl_patchify");
}

// ------------------------------------------------------------------ K1s overlapping unfold (ViTs_face, vits_face.py:446-450, 489-491)
// nn.Unfold(k, stride, pad) -> [B*T, ldo]: row b*T is the zero cls slot, row b*T + 1 + t window t (row-major over Lh x Lw), column
// j = c*k*k + kh*k + kw; out-of-image taps and the K padding j >= C*k*k are 0. Every element is written.
// The column decode is the same for every row: one LDS table per workgroup, {c*H*W + kh*W + kw, kh << 16 | kw}; padding columns carry an
// out-of-range kh, so they fail the bounds test like a padding tap. A workgroup takes UNF_ROWS consecutive rows (neighbouring windows of
// one image: the ~(k/stride)^2 re-reads of a pixel hit L2) and its lanes walk them as 8-column chunks, consecutive lanes on consecutive
// chunks of a row: one 16-byte store per lane for 16-bit outputs, two for f32. The cls row gets an out-of-range h0 and comes out 0.
constexpr int UNF_ROWS = 32;
constexpr int UNF_MAX_LDO = 4096;      // LDS table: 8 bytes per column

template <typename T>
__device__ __forceinline__ void unf_store8(T* p, const float v[8]);
template <>
__device__ __forceinline__ void unf_store8<float>(float* p, const float v[8]) {
  reinterpret_cast<float4*>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
  reinterpret_cast<float4*>(p)[1] = make_float4(v[4], v[5], v[6], v[7]);
}
template <>
__device__ __forceinline__ void unf_store8<bf16_t>(bf16_t* p, const float v[8]) {
  *reinterpret_cast<uint4*>(p) = make_uint4(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7]));
}
template <>
__device__ __forceinline__ void unf_store8<f16_t>(f16_t* p, const float v[8]) {
  *reinterpret_cast<uint4*>(p) = make_uint4(pack2h(v[0], v[1]), pack2h(v[2], v[3]), pack2h(v[4], v[5]), pack2h(v[6], v[7]));
}

// 8 consecutive columns of one row (tab = the table at the first of them); ok = false: no load, zeros
__device__ __forceinline__ void unf_gather8(const float* __restrict__ img, int H, int W, int h0, int w0, long base, const int2* tab, bool ok,
                                            float v[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int2 te = tab[e];
    const int h = h0 + (te.y >> 16), w = w0 + (te.y & 0xffff);
    v[e] = (ok && (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W) ? img[base + te.x] : 0.f;
  }
}

template <typename T>
__global__ void __launch_bounds__(256) unfold_patches_kernel(const float* __restrict__ img, T* __restrict__ out, int C, int H, int W, int k,
                                                             int stride, int pad, int Lw, int Tn, int ldo, int rows) {
  fp16_sat_on();
  extern __shared__ int2 unf_tab[];      // [ldo]
  __shared__ long r_base[UNF_ROWS];      // b*C*H*W + h0*W + w0 of the row's window
  __shared__ int r_h0[UNF_ROWS], r_w0[UNF_ROWS];
  const int kk = k * k, Kc = C * kk;
  for (int j = threadIdx.x; j < ldo; j += blockDim.x) {
    if (j < Kc) {
      const int c = j / kk, r = j - c * kk, kh = r / k, kw = r - kh * k;
      unf_tab[j] = make_int2(c * H * W + kh * W + kw, (kh << 16) | kw);
    } else {
      unf_tab[j] = make_int2(0, 0x7fff << 16);      // kh out of range: always 0
    }
  }
  const int nch = ldo >> 3, per = UNF_ROWS * nch;
  const int step_r = blockDim.x / nch, step_c = blockDim.x - step_r * nch;
  for (int blk = blockIdx.x; blk * UNF_ROWS < rows; blk += gridDim.x) {
    const int r0 = blk * UNF_ROWS;
    __syncthreads();      // (the table above / the previous block's row info is published and consumed)
    if (threadIdx.x < UNF_ROWS) {
      const int row = r0 + threadIdx.x;
      const int b = row / Tn, t = row - b * Tn;
      int h0 = -(1 << 24), w0 = 0;      // cls slot (or past the end): every tap out of range
      if (t > 0 && row < rows) {
        const int wh = (t - 1) / Lw, ww = (t - 1) - wh * Lw;
        h0 = wh * stride - pad;
        w0 = ww * stride - pad;
      }
      r_h0[threadIdx.x] = h0;
      r_w0[threadIdx.x] = w0;
      r_base[threadIdx.x] = (long)b * C * H * W + (long)h0 * W + w0;
    }
    __syncthreads();
    int rl = threadIdx.x / nch, ch = threadIdx.x - rl * nch;
    // two chunks per pass (i and i + blockDim): the gathers of both are in flight before either store waits on them
    for (int i = threadIdx.x; i < per; i += 2 * blockDim.x) {
      if (r0 + rl >= rows) break;
      int rl2 = rl + step_r, ch2 = ch + step_c;
      if (ch2 >= nch) { ch2 -= nch; ++rl2; }
      const bool in2 = i + (int)blockDim.x < per;      // (rl2 < UNF_ROWS)
      const bool ok2 = in2 && r0 + rl2 < rows;
      const int rb = in2 ? rl2 : rl;
      float va[8], vb[8];
      unf_gather8(img, H, W, r_h0[rl], r_w0[rl], r_base[rl], unf_tab + ch * 8, true, va);
      unf_gather8(img, H, W, r_h0[rb], r_w0[rb], r_base[rb], unf_tab + ch2 * 8, ok2, vb);
      unf_store8<T>(out + (size_t)(r0 + rl) * ldo + ch * 8, va);
      if (ok2) unf_store8<T>(out + (size_t)(r0 + rl2) * ldo + ch2 * 8, vb);
      rl = rl2 + step_r;
      ch = ch2 + step_c;
      if (ch >= nch) { ch -= nch; ++rl; }
    }
  }
}

extern "C" int gsl_unfold_patches(const float* img, void* out, int B, int C, int H, int W, int k, int stride, int pad, int ldo, int dtype,
                                  gsl_stream_t s) {
  GSL_CHECK_ARG(img && out && B > 0 && C > 0 && H > 0 && W > 0 && H < 32768 && W < 32768 && (long)C * H * W < (1L << 31), "shape");
  GSL_CHECK_ARG(k > 0 && stride > 0 && pad >= 0 && pad < k, "k > 0, stride > 0, 0 <= pad < k");
  GSL_CHECK_ARG(H + 2 * pad >= k && W + 2 * pad >= k, "Lh, Lw >= 1");
  const int Lh = (H + 2 * pad - k) / stride + 1, Lw = (W + 2 * pad - k) / stride + 1;
  GSL_CHECK_ARG((long)C * k * k <= ldo && ldo % 8 == 0 && ldo <= UNF_MAX_LDO, "C*k*k <= ldo <= 4096, ldo % 8 == 0");
  GSL_CHECK_ARG(((uintptr_t)out & 15) == 0, "out 16-byte aligned");
  const long Tn = 1 + (long)Lh * Lw, rows = (long)B * Tn;
  GSL_CHECK_ARG(rows < (1L << 30), "B*T < 2^30");
  const int nblk = (int)((rows + UNF_ROWS - 1) / UNF_ROWS);
  const int grid = nblk;      // one block of rows per workgroup (a capped grid left half the workgroups a second block: a 2x tail)
  const size_t lds = (size_t)ldo * sizeof(int2);
  if (dtype == GSL_BF16)
    hipLaunchKernelGGL(unfold_patches_kernel<bf16_t>, dim3(grid), dim3(256), lds, as_stream(s), img, (bf16_t*)out, C, H, W, k, stride, pad, Lw,
                       (int)Tn, ldo, (int)rows);
  else if (dtype == GSL_F16)
    hipLaunchKernelGGL(unfold_patches_kernel<f16_t>, dim3(grid), dim3(256), lds, as_stream(s), img, (f16_t*)out, C, H, W, k, stride, pad, Lw,
                       (int)Tn, ldo, (int)rows);
  else if (dtype == GSL_F32)
    hipLaunchKernelGGL(unfold_patches_kernel<float>, dim3(grid), dim3(256), lds, as_stream(s), img, (float*)out, C, H, W, k, stride, pad, Lw,
                       (int)Tn, ldo, (int)rows);
  else return fail(GSL_ERR_ARG, "gsl_unfold_patches: bad dtype%s %ld", "", dtype);
  return check_launch("gsl_unfold_patches");
}

// ------------------------------------------------------------------ K1 / K1s from uint8 images (ToTensor + Normalize fused into the gather)
// The source is the decoder's bytes, [B,C,H,W] (GSL_U8_NCHW) or [B,H,W,C] (GSL_U8_NHWC); the value of byte u in channel c is table[c*256 + u],
// a [C][256] f32 table the caller built with the host expression it wants to be bit-equal to (u/255 - mean[c]) / std[c]. The kernels look the
// value up (LDS copy of the table up to U8_LDS_MAX_C channels, global memory beyond) and store it through the float gathers' own helpers, so
// the operand equals the float gather of the normalised image bit for bit. Cls rows, padding taps and the K padding are 0, not table[c][0].
constexpr int U8_LDS_MAX_C = 16;      // 16 KB of LDS

__device__ __forceinline__ void u8_tab_stage(float* s_tab, const float* __restrict__ tab, int C) {
  if (C <= U8_LDS_MAX_C)
    for (int i = threadIdx.x; i < C * 256; i += blockDim.x) s_tab[i] = tab[i];
}
__device__ __forceinline__ float u8_map(const float* s_tab, const float* __restrict__ tab, bool in_lds, int c, uint32_t u) {
  const int i = (c << 8) | (int)u;
  return in_lds ? s_tab[i] : tab[i];
}
__device__ __forceinline__ uint32_t u8_byte(uint2 q, int j) { return ((j < 4 ? q.x : q.y) >> ((j & 3) * 8)) & 0xffu; }

// Wide form (p % 8 == 0, C = 1 or 3, img 8-byte and out 16-byte aligned): a lane takes 8 consecutive pixels of one patch row, all channels:
// C aligned 8-byte loads (NHWC: 8*C consecutive bytes; NCHW: 8 bytes of each channel plane), 8*C consecutive output elements, 16-byte stores.
// Consecutive lanes write consecutive segments of the operand.
template <typename T, int C>
__global__ void __launch_bounds__(256) patchify_u8_wide_kernel(const uint8_t* __restrict__ img, const float* __restrict__ tab, T* __restrict__ out,
                                                               int B, int H, int W, int p, int nhwc) {
  fp16_sat_on();
  __shared__ float s_tab[C * 256];
  for (int i = threadIdx.x; i < C * 256; i += blockDim.x) s_tab[i] = tab[i];
  __syncthreads();
  const int hp = H / p, wp = W / p, Tn = 1 + hp * wp, po = p >> 3, Kp = p * p * C;
  const long total = (long)B * Tn * p * po;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int o8 = (int)(idx % po);
    const int p1 = (int)((idx / po) % p);
    const int t = (int)((idx / ((long)po * p)) % Tn);
    const int b = (int)(idx / ((long)po * p * Tn));
    T* o = out + ((size_t)b * Tn + t) * Kp + (size_t)(p1 * p + o8 * 8) * C;
    float v[8 * C];
    if (t == 0) {
#pragma unroll
      for (int j = 0; j < 8 * C; ++j) v[j] = 0.f;
    } else {
      const int h = (t - 1) / wp, w = (t - 1) % wp;
      const size_t y = (size_t)(h * p + p1), x = (size_t)(w * p + o8 * 8);
      uint2 q[C];
      if (nhwc) {
        const uint2* src = reinterpret_cast<const uint2*>(img + (((size_t)b * H + y) * W + x) * C);
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = src[c];
#pragma unroll
        for (int j = 0; j < 8 * C; ++j) v[j] = s_tab[((j % C) << 8) | u8_byte(q[j >> 3], j & 7)];
      } else {
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = *reinterpret_cast<const uint2*>(img + (((size_t)b * C + c) * H + y) * W + x);
#pragma unroll
        for (int j = 0; j < 8 * C; ++j) v[j] = s_tab[((j % C) << 8) | u8_byte(q[j % C], j / C)];
      }
    }
#pragma unroll
    for (int g = 0; g < C; ++g) unf_store8<T>(o + g * 8, v + g * 8);
  }
}

// Any other geometry: the float gather's thread map (one (token, p1, p2) per thread, C elements), one byte per load.
template <typename T>
__global__ void patchify_u8_kernel(const uint8_t* __restrict__ img, const float* __restrict__ tab, T* __restrict__ out, int B, int C, int H, int W,
                                   int p, int nhwc) {
  fp16_sat_on();
  extern __shared__ float s_u8tab[];
  const bool in_lds = C <= U8_LDS_MAX_C;
  u8_tab_stage(s_u8tab, tab, C);
  __syncthreads();
  const int hp = H / p, wp = W / p, Tn = 1 + hp * wp, Kp = p * p * C;
  const long total = (long)B * Tn * p * p;
  const size_t sc = nhwc ? 1 : (size_t)H * W;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int p2 = (int)(idx % p);
    const int p1 = (int)((idx / p) % p);
    const int t = (int)((idx / (p * p)) % Tn);
    const int b = (int)(idx / ((long)p * p * Tn));
    T* o = out + ((size_t)b * Tn + t) * Kp + (size_t)(p1 * p + p2) * C;
    if (t == 0) {
      for (int c = 0; c < C; ++c) Elem<T>::st(o + c, 0.f);
    } else {
      const int h = (t - 1) / wp, w = (t - 1) % wp;
      const size_t y = (size_t)(h * p + p1), x = (size_t)(w * p + p2);
      const uint8_t* src = nhwc ? img + (((size_t)b * H + y) * W + x) * C : img + ((size_t)b * C * H + y) * W + x;
      for (int c = 0; c < C; ++c) Elem<T>::st(o + c, u8_map(s_u8tab, tab, in_lds, c, src[c * sc]));
    }
  }
}

template <typename T>
static void patchify_u8_launch(const uint8_t* img, int nhwc, const float* tab, T* out, int B, int C, int H, int W, int p, hipStream_t st) {
  const long Tn = 1 + (long)(H / p) * (W / p);
  const bool wide = p % 8 == 0 && (C == 1 || C == 3) && ((uintptr_t)img & 7) == 0 && ((uintptr_t)out & 15) == 0;
  const long total = wide ? (long)B * Tn * p * (p >> 3) : (long)B * Tn * p * p;
  const int grid = (int)min((total + 255) / 256, (long)(256 * 16));
  if (wide && C == 3) hipLaunchKernelGGL((patchify_u8_wide_kernel<T, 3>), dim3(grid), dim3(256), 0, st, img, tab, out, B, H, W, p, nhwc);
  else if (wide) hipLaunchKernelGGL((patchify_u8_wide_kernel<T, 1>), dim3(grid), dim3(256), 0, st, img, tab, out, B, H, W, p, nhwc);
  else
    hipLaunchKernelGGL(patchify_u8_kernel<T>, dim3(grid), dim3(256), C <= U8_LDS_MAX_C ? (size_t)C * 256 * sizeof(float) : 0, st, img, tab, out, B,
                       C, H, W, p, nhwc);
}

extern "C" int gsl_patchify_u8(const uint8_t* img, int layout, const float* table, void* out, int B, int C, int H, int W, int p, int dtype,
                               gsl_stream_t s) {
  GSL_CHECK_ARG(img && table && out && B > 0 && C > 0 && p > 0 && H > 0 && W > 0 && H % p == 0 && W % p == 0, "shape / null pointer");
  GSL_CHECK_ARG(layout == GSL_U8_NCHW || layout == GSL_U8_NHWC, "layout is GSL_U8_NCHW or GSL_U8_NHWC");
  GSL_CHECK_ARG(((uintptr_t)out & 15) == 0 && ((uintptr_t)table & 3) == 0, "out 16-byte aligned");
  if (dtype == GSL_BF16) patchify_u8_launch<bf16_t>(img, layout, table, (bf16_t*)out, B, C, H, W, p, as_stream(s));
  else if (dtype == GSL_F16) patchify_u8_launch<f16_t>(img, layout, table, (f16_t*)out, B, C, H, W, p, as_stream(s));
  else if (dtype == GSL_F32) patchify_u8_launch<float>(img, layout, table, (float*)out, B, C, H, W, p, as_stream(s));
  else return fail(GSL_ERR_ARG, "gsl_patchify_u8: bad dtype%s %ld", "", dtype);
  return check_launch("gsl_patchify_u8");
}

// The unfold from bytes: gsl_unfold_patches' row blocks, 8-column chunks and 16-byte stores. The column table holds the tap's BYTE offset in
// the source layout and {kh, kw << 8, c << 16} (-1: K padding). A lane keeps the aligned 8-byte word of the image it loaded last and takes
// the next tap from it when it lies inside: the kw run of a chunk costs one or two loads in NCHW (consecutive bytes), three or four in NHWC
// at C = 3 (every third byte), instead of eight. The last, partial word of the image is assembled from single bytes.
__device__ __forceinline__ uint2 u8_window(const uint8_t* __restrict__ img, long wi, long nbytes) {
  if (wi * 8 + 8 <= nbytes) return reinterpret_cast<const uint2*>(img)[wi];
  uint32_t lo = 0, hi = 0;
  for (int j = 0; j < 8; ++j) {
    const long a = wi * 8 + j;
    const uint32_t u = a < nbytes ? img[a] : 0u;
    if (j < 4) lo |= u << (j * 8);
    else hi |= u << ((j - 4) * 8);
  }
  return make_uint2(lo, hi);
}

__device__ __forceinline__ void unf_gather8_u8(const uint8_t* __restrict__ img, long nbytes, const float* s_val, const float* __restrict__ val,
                                               bool in_lds, int H, int W, int h0, int w0, long base, const int2* tab, bool ok, float v[8]) {
  uint2 win = make_uint2(0u, 0u);
  long widx = -1;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int2 te = tab[e];
    const int h = h0 + (te.y & 0xff), w = w0 + ((te.y >> 8) & 0xff);
    float r = 0.f;
    if (ok && te.y >= 0 && (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W) {
      const long a = base + te.x;
      if ((a >> 3) != widx) {
        widx = a >> 3;
        win = u8_window(img, widx, nbytes);
      }
      r = u8_map(s_val, val, in_lds, (te.y >> 16) & 0x7fff, u8_byte(win, (int)(a & 7)));
    }
    v[e] = r;
  }
}

template <typename T>
__global__ void __launch_bounds__(256) unfold_patches_u8_kernel(const uint8_t* __restrict__ img, long nbytes, const float* __restrict__ val,
                                                                T* __restrict__ out, int C, int H, int W, int k, int stride, int pad, int Lw, int Tn,
                                                                int ldo, int rows, int nhwc) {
  fp16_sat_on();
  extern __shared__ int2 unf_tab[];      // [ldo], then the value table [C][256] (C <= U8_LDS_MAX_C)
  __shared__ long r_base[UNF_ROWS];      // byte offset of the window's first tap
  __shared__ int r_h0[UNF_ROWS], r_w0[UNF_ROWS];
  float* s_val = reinterpret_cast<float*>(unf_tab + ldo);
  const bool in_lds = C <= U8_LDS_MAX_C;
  u8_tab_stage(s_val, val, C);
  const int kk = k * k, Kc = C * kk;
  for (int j = threadIdx.x; j < ldo; j += blockDim.x) {
    if (j < Kc) {
      const int c = j / kk, r = j - c * kk, kh = r / k, kw = r - kh * k;
      unf_tab[j] = make_int2(nhwc ? (kh * W + kw) * C + c : c * H * W + kh * W + kw, kh | (kw << 8) | (c << 16));
    } else {
      unf_tab[j] = make_int2(0, -1);      // K padding: always 0
    }
  }
  const int nch = ldo >> 3, per = UNF_ROWS * nch;
  const int step_r = blockDim.x / nch, step_c = blockDim.x - step_r * nch;
  for (int blk = blockIdx.x; blk * UNF_ROWS < rows; blk += gridDim.x) {
    const int r0 = blk * UNF_ROWS;
    __syncthreads();      // (the tables above / the previous block's row info are published and consumed)
    if (threadIdx.x < UNF_ROWS) {
      const int row = r0 + threadIdx.x;
      const int b = row / Tn, t = row - b * Tn;
      int h0 = -(1 << 24), w0 = 0;      // cls slot (or past the end): every tap out of range
      if (t > 0 && row < rows) {
        const int wh = (t - 1) / Lw, ww = (t - 1) - wh * Lw;
        h0 = wh * stride - pad;
        w0 = ww * stride - pad;
      }
      r_h0[threadIdx.x] = h0;
      r_w0[threadIdx.x] = w0;
      r_base[threadIdx.x] = nhwc ? (((long)b * H + h0) * W + w0) * C : (long)b * C * H * W + (long)h0 * W + w0;
    }
    __syncthreads();
    int rl = threadIdx.x / nch, ch = threadIdx.x - rl * nch;
    for (int i = threadIdx.x; i < per; i += 2 * blockDim.x) {      // two chunks per pass, as in the float form
      if (r0 + rl >= rows) break;
      int rl2 = rl + step_r, ch2 = ch + step_c;
      if (ch2 >= nch) { ch2 -= nch; ++rl2; }
      const bool in2 = i + (int)blockDim.x < per;
      const bool ok2 = in2 && r0 + rl2 < rows;
      const int rb = in2 ? rl2 : rl;
      float va[8], vb[8];
      unf_gather8_u8(img, nbytes, s_val, val, in_lds, H, W, r_h0[rl], r_w0[rl], r_base[rl], unf_tab + ch * 8, true, va);
      unf_gather8_u8(img, nbytes, s_val, val, in_lds, H, W, r_h0[rb], r_w0[rb], r_base[rb], unf_tab + ch2 * 8, ok2, vb);
      unf_store8<T>(out + (size_t)(r0 + rl) * ldo + ch * 8, va);
      if (ok2) unf_store8<T>(out + (size_t)(r0 + rl2) * ldo + ch2 * 8, vb);
      rl = rl2 + step_r;
      ch = ch2 + step_c;
      if (ch >= nch) { ch -= nch; ++rl; }
    }
  }
}

extern "C" int gsl_unfold_patches_u8(const uint8_t* img, int layout, const float* table, void* out, int B, int C, int H, int W, int k, int stride,
                                     int pad, int ldo, int dtype, gsl_stream_t s) {
  GSL_CHECK_ARG(img && table && out && B > 0 && C > 0 && H > 0 && W > 0 && H < 32768 && W < 32768 && (long)C * H * W < (1L << 31),
                "shape / null pointer");
  GSL_CHECK_ARG(layout == GSL_U8_NCHW || layout == GSL_U8_NHWC, "layout is GSL_U8_NCHW or GSL_U8_NHWC");
  GSL_CHECK_ARG(k > 0 && k < 256 && stride > 0 && pad >= 0 && pad < k, "0 < k < 256, stride > 0, 0 <= pad < k");
  GSL_CHECK_ARG(H + 2 * pad >= k && W + 2 * pad >= k, "Lh, Lw >= 1");
  const int Lh = (H + 2 * pad - k) / stride + 1, Lw = (W + 2 * pad - k) / stride + 1;
  GSL_CHECK_ARG((long)C * k * k <= ldo && ldo % 8 == 0 && ldo <= UNF_MAX_LDO, "C*k*k <= ldo <= 4096, ldo % 8 == 0");
  GSL_CHECK_ARG(((uintptr_t)out & 15) == 0 && ((uintptr_t)img & 7) == 0 && ((uintptr_t)table & 3) == 0, "out 16-byte, img 8-byte aligned");
  const long Tn = 1 + (long)Lh * Lw, rows = (long)B * Tn;
  GSL_CHECK_ARG(rows < (1L << 30), "B*T < 2^30");
  const int grid = (int)((rows + UNF_ROWS - 1) / UNF_ROWS);
  const size_t lds = (size_t)ldo * sizeof(int2) + (C <= U8_LDS_MAX_C ? (size_t)C * 256 * sizeof(float) : 0);
  const long nbytes = (long)B * C * H * W;
  const int nhwc = layout == GSL_U8_NHWC;
  if (dtype == GSL_BF16)
    hipLaunchKernelGGL(unfold_patches_u8_kernel<bf16_t>, dim3(grid), dim3(256), lds, as_stream(s), img, nbytes, table, (bf16_t*)out, C, H, W, k,
                       stride, pad, Lw, (int)Tn, ldo, (int)rows, nhwc);
  else if (dtype == GSL_F16)
    hipLaunchKernelGGL(unfold_patches_u8_kernel<f16_t>, dim3(grid), dim3(256), lds, as_stream(s), img, nbytes, table, (f16_t*)out, C, H, W, k,
                       stride, pad, Lw, (int)Tn, ldo, (int)rows, nhwc);
  else if (dtype == GSL_F32)
    hipLaunchKernelGGL(unfold_patches_u8_kernel<float>, dim3(grid), dim3(256), lds, as_stream(s), img, nbytes, table, (float*)out, C, H, W, k,
                       stride, pad, Lw, (int)Tn, ldo, (int)rows, nhwc);
  else return fail(GSL_ERR_ARG, "gsl_unfold_patches_u8: bad dtype%s %ld", "", dtype);
  return check_launch("gsl_unfold_patches_u8");
}

// ------------------------------------------------------------------ K10 head
__global__ void cosface_prep_kernel(const float* __restrict__ W, float* __restrict__ Wn, int C, int D) {
  fp16_sat_on();
  // one wave per class row: Wn = W / max(||W||, 1e-12)   (F.normalize, vit_face.py:181)
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (c >= C) return;
  float ss = 0.f;
  for (int d = lane; d < D; d += 64) { const float v = W[(size_t)c * D + d]; ss += v * v; }
  const float inv = 1.0f / fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
  for (int d = lane; d < D; d += 64) Wn[(size_t)c * D + d] = W[(size_t)c * D + d] * inv;
}
extern "C" int gsl_cosface_prep(const float* W, float* Wn, int C, int D, gsl_stream_t s) {
  GSL_CHECK_ARG(W && Wn && C > 0 && D > 0, "null/size");
  hipLaunchKernelGGL(cosface_prep_kernel, dim3((C + 3) / 4), dim3(256), 0, as_stream(s), W, Wn, C, D);
  return check_launch("gsl_cosface_prep");
}

constexpr int HEAD_MAXD = 1024;

// head kinds of the margin entry points, a template argument of both kernels: the margin code of a kind exists only in its own
// instantiations. HEAD_COSFACE also covers the plain linear head (runtime flag `linear`, as in gsl_head_fwd / gsl_head_bwd).
constexpr int HEAD_COSFACE = 0, HEAD_ARCFACE = 1;
// ArcFace constants (vit_face.py:98-101), computed on the host in double and passed as float
struct ArcMargin {
  float cos_m, sin_m, th, mm;
  int easy;
};
// phi(cos) of the label column (vit_face.py:127-132)
__device__ __forceinline__ float arc_phi(float c, const ArcMargin& a) {
  const float sine = sqrtf(fmaxf(1.0f - c * c, 0.0f));
  const float phi = c * a.cos_m - sine * a.sin_m;
  return a.easy ? (c > 0.0f ? phi : c) : (c > a.th ? phi : c - a.mm);
}
// d phi / d cos at the cosine the forward saw: the same comparison picks the branch
__device__ __forceinline__ float arc_dphi(float c, const ArcMargin& a) {
  if (!(a.easy ? c > 0.0f : c > a.th)) return 1.0f;
  const float sine = fmaxf(sqrtf(fmaxf(1.0f - c * c, 0.0f)), 1e-6f);
  return a.cos_m + a.sin_m * c / sine;
}

// X: element type of the residual stream x (f32, or bf16 in speed mode). KIND: HEAD_COSFACE / HEAD_ARCFACE; arc / cos_y are read
// by HEAD_ARCFACE only (cos_y [B]: the label column's cosine before the margin, for the backward)
template <typename X, int KIND>
__global__ __launch_bounds__(1024) void head_fwd_kernel(const X* __restrict__ x, int T, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float eps, const float* __restrict__ Wn,
                                                       const int64_t* __restrict__ label, float* __restrict__ emb,
                                                       float* __restrict__ mean, float* __restrict__ rstd,
                                                       float* __restrict__ logits, int D, int C, float cs, float cm,
                                                       const float* __restrict__ hbias, int linear, int pool_mean, ArcMargin arc,
                                                       float* __restrict__ cos_y) {
  fp16_sat_on();
  __shared__ float e[HEAD_MAXD];
  __shared__ float sm[16];
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, nwv = blockDim.x >> 6;      // 256 threads, or 1024 when few images share the chip
  const X* xr = x + (size_t)b * T * D;
  float s = 0.f;
  for (int d = tid; d < D; d += nt) {
    float pv = Elem<X>::ld(xr + d);                 // pool = 'cls': token 0 (vit_face.py:540)
    if (pool_mean) {                                // pool = 'mean': x.mean(dim=1) over all T tokens, summed in token order
      for (int t = 1; t < T; ++t) pv += Elem<X>::ld(xr + (size_t)t * D + d);
      pv = pv / (float)T;
    }
    e[d] = pv; s += pv;
  }
  const float mu = block_sum(s, sm) / D;
  float q = 0.f;
  for (int d = tid; d < D; d += nt) { const float c = e[d] - mu; q += c * c; }
  const float rs = rsqrtf(block_sum(q, sm) / D + eps);
  float nn = 0.f;
  for (int d = tid; d < D; d += nt) {
    const float v = (e[d] - mu) * rs * gamma[d] + beta[d];
    e[d] = v;
    emb[(size_t)b * D + d] = v;
    nn += v * v;
  }
  if (tid == 0) { mean[b] = mu; rstd[b] = rs; }
  const float inv = 1.0f / fmaxf(sqrtf(block_sum(nn, sm)), 1e-12f);   // block_sum syncs -> e[] complete
  if (!logits) return;
  const int lane = tid & 63, wave = tid >> 6;
  const long lab = label ? (long)label[b] : -1;
  // a wave owns classes wave, wave + 4, ...; five of them per round so that the loads of five W rows are in flight together (one
  // class per round made the kernel a chain of 25 dependent global-load latencies: 60 us for 100 classes at any batch size)
  constexpr int CB = 5;
  for (int c0 = wave; c0 < C; c0 += nwv * CB) {
    float dot[CB];
#pragma unroll
    for (int k = 0; k < CB; ++k) dot[k] = 0.f;
    for (int d = lane; d < D; d += 64) {
      const float ev = e[d];
#pragma unroll
      for (int k = 0; k < CB; ++k) {
        const int c = min(c0 + nwv * k, C - 1);
        dot[k] += ev * Wn[(size_t)c * D + d];
      }
    }
#pragma unroll
    for (int k = 0; k < CB; ++k) {
      const int c = c0 + nwv * k;
      float dk = wave_sum(dot[k]);
      if (lane == 0 && c < C) {
        if (linear) logits[(size_t)b * C + c] = dk + (hbias ? hbias[c] : 0.f);     // plain nn.Linear head (modified_VIT.py:34-36)
        else if constexpr (KIND == HEAD_ARCFACE) {
          dk *= inv;
          if (c == lab) { cos_y[b] = dk; dk = arc_phi(dk, arc); }
          logits[(size_t)b * C + c] = cs * dk;
        } else { dk *= inv; logits[(size_t)b * C + c] = cs * ((c == lab) ? (dk - cm) : dk); }
      }
    }
  }
}

template <int KIND>
static void head_fwd_launch(const void* x, int x_dtype, int T, const float* gamma, const float* beta, float eps, const float* Wn,
                            const int64_t* label, float* emb, float* mean, float* rstd, float* logits, int B, int D, int C, float cos_s,
                            float cos_m, const float* head_bias, int linear_head, int pool_mean, ArcMargin arc, float* cos_y, gsl_stream_t s) {
  const int nthr = B <= 128 ? 1024 : 256;      // one workgroup per image: with few images give each one 16 waves (100 class rows in two rounds)
  if (x_dtype == GSL_F16)
    hipLaunchKernelGGL((head_fwd_kernel<f16_t, KIND>), dim3(B), dim3(nthr), 0, as_stream(s), (const f16_t*)x, T, gamma, beta, eps, Wn, label,
                       emb, mean, rstd, logits, D, C, cos_s, cos_m, head_bias, linear_head, pool_mean, arc, cos_y);
  else if (x_dtype == GSL_BF16)
    hipLaunchKernelGGL((head_fwd_kernel<bf16_t, KIND>), dim3(B), dim3(nthr), 0, as_stream(s), (const bf16_t*)x, T, gamma, beta, eps, Wn, label,
                       emb, mean, rstd, logits, D, C, cos_s, cos_m, head_bias, linear_head, pool_mean, arc, cos_y);
  else
    hipLaunchKernelGGL((head_fwd_kernel<float, KIND>), dim3(B), dim3(nthr), 0, as_stream(s), (const float*)x, T, gamma, beta, eps, Wn, label,
                       emb, mean, rstd, logits, D, C, cos_s, cos_m, head_bias, linear_head, pool_mean, arc, cos_y);
}

extern "C" int gsl_head_fwd(const void* x, int x_dtype, int T, const float* gamma, const float* beta, float eps, const float* Wn,
                            const int64_t* label, float* emb, float* mean, float* rstd, float* logits, int B, int D, int C,
                            float cos_s, float cos_m, const float* head_bias, int linear_head, int pool_mean, gsl_stream_t s) {
  GSL_CHECK_ARG(x_dtype == GSL_F32 || x_dtype == GSL_BF16 || x_dtype == GSL_F16, "x dtype");
  GSL_CHECK_ARG(x && gamma && beta && emb && mean && rstd && B > 0 && T > 0, "null/size");
  GSL_CHECK_ARG(D > 0 && D <= HEAD_MAXD && (D % 4) == 0, "D <= 1024, D%4==0");
  GSL_CHECK_ARG(!logits || (Wn && C > 0), "Wn required for logits");
  head_fwd_launch<HEAD_COSFACE>(x, x_dtype, T, gamma, beta, eps, Wn, label, emb, mean, rstd, logits, B, D, C, cos_s, cos_m, head_bias,
                                linear_head, pool_mean, ArcMargin{}, nullptr, s);
  return check_launch("gsl_head_fwd");
}

// ArcFace constants of margin m (vit_face.py:98-101): math.cos / math.sin in double, as the reference computes them, then float
static ArcMargin arc_margin(double m, int easy_margin) {
  const double pi = 3.14159265358979323846;      // math.pi
  return ArcMargin{(float)std::cos(m), (float)std::sin(m), (float)std::cos(pi - m), (float)(std::sin(pi - m) * m), easy_margin ? 1 : 0};
}

extern "C" int gsl_head_fwd_margin(const void* x, int x_dtype, int T, const float* gamma, const float* beta, float eps, const float* Wn,
                                   const int64_t* label, float* emb, float* mean, float* rstd, float* logits, int B, int D, int C,
                                   float cos_s, float cos_m, const float* head_bias, int linear_head, int pool_mean, int head_kind,
                                   double m, int easy_margin, float* cos_y, gsl_stream_t s) {
  GSL_CHECK_ARG(head_kind == HEAD_COSFACE || head_kind == HEAD_ARCFACE, "head_kind: 0 (CosFace) or 1 (ArcFace)");
  GSL_CHECK_ARG(x_dtype == GSL_F32 || x_dtype == GSL_BF16 || x_dtype == GSL_F16, "x dtype");
  GSL_CHECK_ARG(x && gamma && beta && emb && mean && rstd && B > 0 && T > 0, "null/size");
  GSL_CHECK_ARG(D > 0 && D <= HEAD_MAXD && (D % 4) == 0, "D <= 1024, D%4==0");
  GSL_CHECK_ARG(!logits || (Wn && C > 0), "Wn required for logits");
  GSL_CHECK_ARG(head_kind != HEAD_ARCFACE || !linear_head, "ArcFace is a cosine head (linear_head = 0)");
  GSL_CHECK_ARG(head_kind != HEAD_ARCFACE || !logits || (label && cos_y), "ArcFace logits need label and cos_y [B]");
  if (head_kind == HEAD_ARCFACE)
    head_fwd_launch<HEAD_ARCFACE>(x, x_dtype, T, gamma, beta, eps, Wn, label, emb, mean, rstd, logits, B, D, C, cos_s, cos_m, head_bias,
                                  linear_head, pool_mean, arc_margin(m, easy_margin), cos_y, s);
  else
    head_fwd_launch<HEAD_COSFACE>(x, x_dtype, T, gamma, beta, eps, Wn, label, emb, mean, rstd, logits, B, D, C, cos_s, cos_m, head_bias,
                                  linear_head, pool_mean, ArcMargin{}, nullptr, s);
  return check_launch("gsl_head_fwd_margin");
}

// compact != 0 (pool = 'cls' only): dx / dxb are [B, D] — the gradient of the cls rows alone; the stream gradient of every other token is
// exactly zero and is neither written here nor read by the consumers (the cls-row-only backward of the last block, gsl_layernorm_bwd's
// dres_cls_T). The dropout counter of element (b, d) stays that of the dense tensor, (b*Tn)*D + d: same masks in both forms.
// KIND = HEAD_ARCFACE: the label column of dlogits is multiplied by d phi / d cos at cos_y [B] (written by the forward) before
// the sum over the classes; everything after that is the CosFace code.
template <typename T, typename S, typename X, int KIND>
__global__ __launch_bounds__(256) void head_bwd_kernel(const float* __restrict__ dlogits, const float* __restrict__ demb_in,
                                                       const X* __restrict__ x, int Tn, const float* __restrict__ gamma,
                                                       const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       const float* __restrict__ emb, const float* __restrict__ Wn,
                                                       S* __restrict__ dx, T* __restrict__ dxb, int D, int C, float cs,
                                                       DropCfg drop, int linear, int pool_mean, int compact,
                                                       float* __restrict__ amax_out, const float* __restrict__ amax_in, int n_amax,
                                                       float* __restrict__ gscale_out, int target_exp, ArcMargin arc,
                                                       const float* __restrict__ cos_y, const int64_t* __restrict__ label) {
  fp16_sat_on();
  resolve_drop(drop);
  // fp16 operands (round 5): the backward runs on gradients multiplied by a power of two S chosen from the largest stream gradient
  // this kernel produces, S * max|g| in [2^(target_exp-1), 2^target_exp). Pass 1 (amax_out) writes max|g| of every image and stores
  // nothing else; pass 2 (amax_in) reduces them — every block the same way — scales its stores and block 0 publishes {S, 1/S}
  // (gscale_out) for the LoRA-gradient reductions, which divide S out again. Power of two: exact in every format.
  float gs = 1.0f;
  if (amax_in) {
    float am = 0.f;
    for (int i = threadIdx.x; i < n_amax; i += 256) am = fmaxf(am, amax_in[i]);
    __shared__ float sma[16];
    am = block_max(am, sma);
    // the exponent in use: gscale[3], settled by pass 1 (overflow guard, see below); a caller without the guard's state passes target_exp alone
    const int tex = gscale_out ? (int)gscale_out[3] : target_exp;
    if (am > 0.f && am < 3.0e38f) {
      int ex;
      (void)frexpf(am, &ex);                 // am = m 2^ex, m in [0.5, 1)
      gs = ldexpf(1.0f, min(max(tex - ex, -60), 60));
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && gscale_out) { gscale_out[0] = gs; gscale_out[1] = 1.0f / gs; }
  }
  // Overflow guard (round 6): pass 1's block 0 settles the exponent E of THIS backward from what the PREVIOUS one saw — gscale[2] = the largest
  // |scaled gradient| its LayerNorm backwards read or stored: saturated (>= 65504) or non-finite -> E - 2 (floor 4); below 2^9 and E under the
  // target -> E + 1; E outside [4, 15] (a freshly zeroed buffer) -> the target — and clears gscale[2] for this backward. Pass 2 (a later launch)
  // reads E from gscale[3]. No host sync; replays of a captured graph carry the state in the buffer.
  if (amax_out && gscale_out && blockIdx.x == 0 && threadIdx.x == 0) {
    const float seen = gscale_out[2];
    int E = (int)gscale_out[3];
    if (!(gscale_out[3] >= 4.0f && gscale_out[3] <= 15.0f)) E = target_exp;
    else if (!(seen < 65504.0f)) E = max(E - 2, 4);
    else if (seen < 512.0f && seen > 0.f && E < target_exp) E = E + 1;
    gscale_out[3] = (float)E;
    gscale_out[2] = 0.0f;
  }
  __shared__ float de[HEAD_MAXD];   // d emb
  __shared__ float dl[1024];        // s * dlogits row (C <= 1024)
  __shared__ float xp[HEAD_MAXD];   // pooled row (pool = 'mean')
  __shared__ float sm[16];
  const int b = blockIdx.x, tid = threadIdx.x;
  // pool = 'cls': zero the non-cls token rows of this image (their stream gradient is exactly 0)
  if (!pool_mean && !compact && !amax_out) {
    const long n4 = (long)(Tn - 1) * D / 4;
    {
      S* z = dx + ((size_t)b * Tn + 1) * D;
      const float zero4[4] = {0.f, 0.f, 0.f, 0.f};
      for (long i = tid; i < n4; i += 256) Elem<S>::st4(z + i * 4, zero4);
    }
    if (dxb) {
      T* zb = dxb + ((size_t)b * Tn + 1) * D;
      const float zero[4] = {0.f, 0.f, 0.f, 0.f};
      for (long i = tid; i < n4; i += 256) Elem<T>::st4(zb + i * 4, zero);
    }
  }
  const float* er = emb + (size_t)b * D;
  float nn = 0.f;
  for (int d = tid; d < D; d += 256) nn += er[d] * er[d];
  const float nrm = fmaxf(sqrtf(block_sum(nn, sm)), 1e-12f);
  if (dlogits) {
    for (int c = tid; c < C; c += 256) dl[c] = cs * dlogits[(size_t)b * C + c];
    if constexpr (KIND == HEAD_ARCFACE) {      // the thread that stored dl[y] rescales it: no barrier needed in between
      const long y = (long)label[b];
      if (y >= 0 && y < C && tid == (int)(y & 255)) dl[y] *= arc_dphi(cos_y[b], arc);
    }
  }
  __syncthreads();
  float dotp = 0.f;
  for (int d = tid; d < D; d += 256) {
    float g = 0.f;
    if (dlogits) {
      for (int c = 0; c < C; ++c) g += dl[c] * Wn[(size_t)c * D + d];
    }
    de[d] = g;                       // d e-hat
    dotp += g * er[d];
  }
  const float proj = block_sum(dotp, sm) / (nrm * nrm);   // (e-hat . d e-hat) / ||e||
  const float mu = mean[b], rs = rstd[b];
  const X* xr = x + (size_t)b * Tn * D;
  for (int d = tid; d < D; d += 256) {          // the pooled row the forward normalised (same summation order)
    float pv = Elem<X>::ld(xr + d);
    if (pool_mean) {
      for (int t = 1; t < Tn; ++t) pv += Elem<X>::ld(xr + (size_t)t * D + d);
      pv = pv / (float)Tn;
    }
    xp[d] = pv;
  }
  float s1 = 0.f, s2 = 0.f;
  for (int d = tid; d < D; d += 256) {
    float g = linear ? de[d] : (de[d] - er[d] * proj) / nrm;   // d emb from the Linear / CosFace head
    if (demb_in) g += demb_in[(size_t)b * D + d];
    g *= gamma[d];
    de[d] = g;
    const float xh = (xp[d] - mu) * rs;
    s1 += g;
    s2 += g * xh;
  }
  const float c1 = block_sum(s1, sm) / D;
  const float c2 = block_sum(s2, sm) / D;
  if (amax_out) {      // pass 1 of the loss-scaled form: this image's largest |stream gradient|, nothing else
    float am = 0.f;
    for (int d = tid; d < D; d += 256) {
      const float xh = (xp[d] - mu) * rs;
      am = fmaxf(am, fabsf(rs * (de[d] - c1 - xh * c2)));
    }
    am = block_max(am, sm);
    if (tid == 0) amax_out[b] = pool_mean ? am / (float)Tn : am;
    return;
  }
  for (int d = tid; d < D; d += 256) {
    const float xh = (xp[d] - mu) * rs;
    const float g = gs * (rs * (de[d] - c1 - xh * c2));
    if (!pool_mean) {
      const size_t o = (size_t)b * Tn * D + d, oc = compact ? (size_t)b * D + d : o;
      Elem<S>::st(dx + oc, g);
      if (dxb) Elem<T>::st(dxb + oc, g * drop_mul(drop, (uint64_t)o));
    } else {                                     // every token receives d pooled / T
      const float gt = g / (float)Tn;
      for (int t = 0; t < Tn; ++t) {
        const size_t o = ((size_t)b * Tn + t) * D + d;
        Elem<S>::st(dx + o, gt);
        if (dxb) Elem<T>::st(dxb + o, gt * drop_mul(drop, (uint64_t)o));
      }
    }
  }
}

// Loss scale of the fp16 backward: S * max|stream gradient at the head| lands in [2^10, 2^11). Measured on the full ViT-P8S8 (CPU emulation,
// tools/emu_operand_precision.py): the largest gradient operand anywhere in the backward is 1.2x the head's, so the chain peaks near 2.5e3
// (26x below fp16's 65504; stores saturate, they never produce Inf), and the LoRA-gradient error is flat for S between 2^6 and 2^20.
constexpr int GSL_GRAD_TARGET_EXP = 11;
template <int KIND>
static void head_bwd_launch(const float* dlogits, const float* demb, const void* x, int x_dtype, int T, const float* gamma, const float* mean,
                            const float* rstd, const float* emb, const float* Wn, void* dx, void* dxb, int B, int D, int C, float cos_s, int dtype,
                            int stream_dtype, DropCfg drop, int linear_head, int pool_mean, int compact, float* gscale, float* amax_ws, int texp,
                            ArcMargin arc, const float* cos_y, const int64_t* label, gsl_stream_t s) {
#define GSL_HB(T_, S_, X_)                                                                                                          \
  do {                                                                                                                              \
    if (gscale)                                                                                                                     \
      hipLaunchKernelGGL((head_bwd_kernel<T_, S_, X_, KIND>), dim3(B), dim3(256), 0, as_stream(s), dlogits, demb, (const X_*)x, T, gamma, \
                         mean, rstd, emb, Wn, (S_*)dx, (T_*)dxb, D, C, cos_s, drop, linear_head, pool_mean, compact, amax_ws,        \
                         (const float*)nullptr, 0, gscale, texp, arc, cos_y, label);                                                 \
    hipLaunchKernelGGL((head_bwd_kernel<T_, S_, X_, KIND>), dim3(B), dim3(256), 0, as_stream(s), dlogits, demb, (const X_*)x, T, gamma,   \
                       mean, rstd, emb, Wn, (S_*)dx, (T_*)dxb, D, C, cos_s, drop, linear_head, pool_mean, compact, (float*)nullptr,   \
                       (const float*)(gscale ? amax_ws : nullptr), B, gscale, texp, arc, cos_y, label);                              \
  } while (0)
  if (dtype == GSL_F16 && stream_dtype == GSL_F16 && x_dtype == GSL_F16) GSL_HB(f16_t, f16_t, f16_t);
  else if (dtype == GSL_F16 && stream_dtype == GSL_F16) GSL_HB(f16_t, f16_t, float);
  else if (dtype == GSL_F16 && x_dtype == GSL_F16) GSL_HB(f16_t, float, f16_t);
  else if (dtype == GSL_F16) GSL_HB(f16_t, float, float);
  else if (dtype == GSL_BF16 && stream_dtype == GSL_BF16 && x_dtype == GSL_F16) GSL_HB(bf16_t, bf16_t, f16_t);
  else if (dtype == GSL_BF16 && x_dtype == GSL_F16) GSL_HB(bf16_t, float, f16_t);
  else if (dtype == GSL_BF16 && stream_dtype == GSL_BF16 && x_dtype == GSL_BF16) GSL_HB(bf16_t, bf16_t, bf16_t);
  else if (dtype == GSL_BF16 && stream_dtype == GSL_BF16) GSL_HB(bf16_t, bf16_t, float);
  else if (dtype == GSL_BF16 && x_dtype == GSL_BF16) GSL_HB(bf16_t, float, bf16_t);
  else if (dtype == GSL_BF16) GSL_HB(bf16_t, float, float);
  else GSL_HB(float, float, float);      // GSL_F32 (the callers reject any other dtype)
#undef GSL_HB
}

// the argument checks of both backward entry points (a macro: GSL_CHECK_ARG reports the caller's name)
#define GSL_HEAD_BWD_CHECKS()                                                                                                        \
  GSL_CHECK_ARG(x && gamma && mean && rstd && emb && dx && B > 0 && T >= 1, "null/size");                                          \
  GSL_CHECK_ARG(D > 0 && D <= HEAD_MAXD && (D % 4) == 0 && C <= 1024, "D <= 1024, D%4==0, C <= 1024");                               \
  GSL_CHECK_ARG(!dlogits || Wn, "Wn required with dlogits");                                                                         \
  GSL_CHECK_ARG(!(compact && pool_mean), "compact cls-row gradients need pool = 'cls'");                                            \
  GSL_CHECK_ARG(!gscale || amax_ws, "gscale (loss-scaled gradients) needs amax_ws [B]");                                            \
  GSL_CHECK_ARG(target_exp == 0 || (target_exp >= 4 && target_exp <= 15), "target_exp: 0 (default 11) or 4 .. 15");                \
  GSL_CHECK_ARG(stream_dtype == GSL_F32 || (stream_dtype == dtype && dtype != GSL_F32), "stream dtype (f32, or the operand format of a 16-bit mode)"); \
  GSL_CHECK_ARG(x_dtype == GSL_F32 || ((x_dtype == GSL_BF16 || x_dtype == GSL_F16) && dtype == GSL_BF16) || (x_dtype == GSL_F16 && dtype == GSL_F16), \
                "x dtype (a 16-bit stream only in a 16-bit mode; bf16 stream only with bf16 operands)")

extern "C" int gsl_head_bwd(const float* dlogits, const float* demb, const void* x, int x_dtype, int T, const float* gamma,
                            const float* mean, const float* rstd, const float* emb, const float* Wn, void* dx, void* dxb,
                            int B, int D, int C, float cos_s, int dtype, int stream_dtype, float p_drop, uint64_t seed, uint32_t site,
                            int linear_head, int pool_mean, int compact, float* gscale, float* amax_ws, int target_exp, gsl_stream_t s) {
  GSL_HEAD_BWD_CHECKS();
  if (dtype != GSL_F16 && dtype != GSL_BF16 && dtype != GSL_F32) return fail(GSL_ERR_ARG, "gsl_head_bwd: bad dtype%s %ld", "", dtype);
  head_bwd_launch<HEAD_COSFACE>(dlogits, demb, x, x_dtype, T, gamma, mean, rstd, emb, Wn, dx, dxb, B, D, C, cos_s, dtype, stream_dtype,
                                make_drop(p_drop, seed, site), linear_head, pool_mean, compact, gscale, amax_ws,
                                target_exp ? target_exp : GSL_GRAD_TARGET_EXP, ArcMargin{}, nullptr, nullptr, s);
  return check_launch("gsl_head_bwd");
}

extern "C" int gsl_head_bwd_margin(const float* dlogits, const float* demb, const void* x, int x_dtype, int T, const float* gamma,
                                   const float* mean, const float* rstd, const float* emb, const float* Wn, void* dx, void* dxb,
                                   int B, int D, int C, float cos_s, int dtype, int stream_dtype, float p_drop, uint64_t seed, uint32_t site,
                                   int linear_head, int pool_mean, int compact, float* gscale, float* amax_ws, int target_exp, int head_kind,
                                   double m, int easy_margin, const float* cos_y, const int64_t* label, gsl_stream_t s) {
  GSL_CHECK_ARG(head_kind == HEAD_COSFACE || head_kind == HEAD_ARCFACE, "head_kind: 0 (CosFace) or 1 (ArcFace)");
  GSL_HEAD_BWD_CHECKS();
  GSL_CHECK_ARG(head_kind != HEAD_ARCFACE || !linear_head, "ArcFace is a cosine head (linear_head = 0)");
  GSL_CHECK_ARG(head_kind != HEAD_ARCFACE || !dlogits || (label && cos_y), "ArcFace dlogits need label and cos_y [B]");
  if (dtype != GSL_F16 && dtype != GSL_BF16 && dtype != GSL_F32) return fail(GSL_ERR_ARG, "gsl_head_bwd_margin: bad dtype%s %ld", "", dtype);
  const int texp = target_exp ? target_exp : GSL_GRAD_TARGET_EXP;
  const DropCfg drop = make_drop(p_drop, seed, site);
  if (head_kind == HEAD_ARCFACE)
    head_bwd_launch<HEAD_ARCFACE>(dlogits, demb, x, x_dtype, T, gamma, mean, rstd, emb, Wn, dx, dxb, B, D, C, cos_s, dtype, stream_dtype, drop,
                                  linear_head, pool_mean, compact, gscale, amax_ws, texp, arc_margin(m, easy_margin), cos_y, label, s);
  else
    head_bwd_launch<HEAD_COSFACE>(dlogits, demb, x, x_dtype, T, gamma, mean, rstd, emb, Wn, dx, dxb, B, D, C, cos_s, dtype, stream_dtype, drop,
                                  linear_head, pool_mean, compact, gscale, amax_ws, texp, ArcMargin{}, nullptr, nullptr, s);
  return check_launch("gsl_head_bwd_margin");
}
#undef GSL_HEAD_BWD_CHECKS

// ------------------------------------------------------------------ K11 cross entropy
// wave-per-row log-softmax; one block so the batch sum is a fixed-order (deterministic) reduction.
__device__ __forceinline__ void row_softmax_stats(const float* row, int C, int lane, float& mx, float& lse, int& amax) {
  float m = -3.0e38f; int mi = 0x7fffffff;
  for (int c = lane; c < C; c += 64) { const float v = row[c]; if (v > m) { m = v; mi = c; } }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64); const int oi = __shfl_xor(mi, o, 64);
    if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
  }
  float se = 0.f;
  for (int c = lane; c < C; c += 64) se += expf(row[c] - m);
  se = wave_sum(se);
  mx = m; lse = m + logf(se); amax = mi;
}

__global__ __launch_bounds__(256) void ce_rows_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                      float* __restrict__ rows, int B, int C) {
  fp16_sat_on();
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B) return;
  float mx, lse; int am;
  row_softmax_stats(logits + (size_t)r * C, C, lane, mx, lse, am);
  // a label outside [0, C) (the reference's CrossEntropyLoss raises): NaN loss, no out-of-bounds read; the deferred meter read stops the run
  const long yl = (long)labels[r];
  const bool ok = yl >= 0 && yl < C;
  const int y = ok ? (int)yl : -1;
  if (lane == 0) { rows[2 * r] = ok ? lse - logits[(size_t)r * C + y] : __int_as_float(0x7fc00000); rows[2 * r + 1] = (am == y) ? 1.f : 0.f; }
}
// deterministic: lane-strided partial sums in a fixed order, fixed-order cross-wave combine
__global__ __launch_bounds__(256) void sum_rows_kernel(const float* __restrict__ rows, float* __restrict__ out, int B, int ncol) {
  fp16_sat_on();
  __shared__ float sm[16];
  for (int c = 0; c < ncol; ++c) {
    float a = 0.f;
    for (int r = threadIdx.x; r < B; r += blockDim.x) a += rows[(size_t)r * ncol + c];
    const float t = block_sum(a, sm);
    if (threadIdx.x == 0) out[c] = t;
  }
}
extern "C" int gsl_ce_fwd(const float* logits, const int64_t* labels, float* out2, float* row_ws, int B, int C, gsl_stream_t s) {
  GSL_CHECK_ARG(logits && labels && out2 && row_ws && B > 0 && C > 0, "null/size");
  hipLaunchKernelGGL(ce_rows_kernel, dim3((B + 3) / 4), dim3(256), 0, as_stream(s), logits, labels, row_ws, B, C);
  hipLaunchKernelGGL(sum_rows_kernel, dim3(1), dim3(256), 0, as_stream(s), row_ws, out2, B, 2);
  return check_launch("gsl_ce_fwd");
}

__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                     const float* __restrict__ coef, float scale, float* dlogits, int B, int C,
                                                     int accumulate) {
  fp16_sat_on();
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B) return;
  float mx, lse; int am;
  row_softmax_stats(logits + (size_t)r * C, C, lane, mx, lse, am);
  const float k = coef[0] * scale;
  const long yl = (long)labels[r];
  const bool ok = yl >= 0 && yl < C;      // out-of-range label: NaN gradient row (see ce_rows_kernel)
  const int y = ok ? (int)yl : -1;
  for (int c = lane; c < C; c += 64) {
    const float g = ok ? k * (expf(logits[(size_t)r * C + c] - lse) - (c == y ? 1.f : 0.f)) : __int_as_float(0x7fc00000);
    float* d = dlogits + (size_t)r * C + c;
    *d = accumulate ? (*d + g) : g;
  }
}
extern "C" int gsl_ce_bwd(const float* logits, const int64_t* labels, const float* coef, float scale, float* dlogits, int B,
                          int C, int accumulate, gsl_stream_t s) {
  GSL_CHECK_ARG(logits && labels && coef && dlogits && B > 0 && C > 0, "null/size");
  hipLaunchKernelGGL(ce_bwd_kernel, dim3((B + 3) / 4), dim3(256), 0, as_stream(s), logits, labels, coef, scale, dlogits, B, C, accumulate);
  return check_launch("gsl_ce_bwd");
}

// ------------------------------------------------------------------ K13 prototype KL
__device__ __forceinline__ float row_lse(const float* row, int D, int lane) {
  float m = -3.0e38f;
  for (int d = lane; d < D; d += 64) m = fmaxf(m, row[d]);
  m = wave_max(m);
  float se = 0.f;
  for (int d = lane; d < D; d += 64) se += expf(row[d] - m);
  return m + logf(wave_sum(se));
}

__global__ __launch_bounds__(256) void proto_kl_rows_kernel(const float* __restrict__ emb, const int64_t* __restrict__ labels,
                                                            const float* __restrict__ proto, float* __restrict__ rows, int B, int D, int C) {
  fp16_sat_on();
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B) return;
  const float* a = emb + (size_t)r * D;
  const long y = (long)labels[r];
  // a label outside the prototype table (the reference raises KeyError, engine_cl.py:587-589): no out-of-bounds read, the loss turns
  // NaN — a class missing INSIDE the table holds NaN rows (losses.prototype_table), with the same effect
  if (y < 0 || y >= C) { if (lane == 0) rows[r] = __int_as_float(0x7fc00000); return; }
  const float* t = proto + (size_t)y * D;
  const float la = row_lse(a, D, lane), lt = row_lse(t, D, lane);
  float acc = 0.f;
  for (int d = lane; d < D; d += 64) {
    const float ltd = t[d] - lt;
    acc += expf(ltd) * (ltd - (a[d] - la));
  }
  acc = wave_sum(acc);
  if (lane == 0) rows[r] = acc;
}
extern "C" int gsl_proto_kl_fwd(const float* emb, const int64_t* labels, const float* proto, float* out1, float* row_ws, int B,
                                int D, int C, gsl_stream_t s) {
  GSL_CHECK_ARG(emb && labels && proto && out1 && row_ws && B > 0 && D > 0 && C > 0, "null/size");
  hipLaunchKernelGGL(proto_kl_rows_kernel, dim3((B + 3) / 4), dim3(256), 0, as_stream(s), emb, labels, proto, row_ws, B, D, C);
  hipLaunchKernelGGL(sum_rows_kernel, dim3(1), dim3(256), 0, as_stream(s), row_ws, out1, B, 1);
  return check_launch("gsl_proto_kl_fwd");
}

__global__ __launch_bounds__(256) void proto_kl_bwd_kernel(const float* __restrict__ emb, const int64_t* __restrict__ labels,
                                                           const float* __restrict__ proto, const float* __restrict__ coef,
                                                           float scale, float* demb, int B, int D, int C, int accumulate) {
  fp16_sat_on();
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B) return;
  const float* a = emb + (size_t)r * D;
  const long y = (long)labels[r];
  if (y < 0 || y >= C) {       // see proto_kl_rows_kernel
    for (int d = lane; d < D; d += 64) demb[(size_t)r * D + d] = __int_as_float(0x7fc00000);
    return;
  }
  const float* t = proto + (size_t)y * D;
  const float la = row_lse(a, D, lane), lt = row_lse(t, D, lane);
  const float k = coef[0] * scale;
  for (int d = lane; d < D; d += 64) {
    const float g = k * (expf(a[d] - la) - expf(t[d] - lt));
    float* o = demb + (size_t)r * D + d;
    *o = accumulate ? (*o + g) : g;
  }
}
extern "C" int gsl_proto_kl_bwd(const float* emb, const int64_t* labels, const float* proto, const float* coef, float scale,
                                float* demb, int B, int D, int C, int accumulate, gsl_stream_t s) {
  GSL_CHECK_ARG(emb && labels && proto && coef && demb && B > 0 && D > 0 && C > 0, "null/size");
  hipLaunchKernelGGL(proto_kl_bwd_kernel, dim3((B + 3) / 4), dim3(256), 0, as_stream(s), emb, labels, proto, coef, scale, demb, B, D, C, accumulate);
  return check_launch("gsl_proto_kl_bwd");
}

// ------------------------------------------------------------------ K13b prototype l2 (engine_cl.py:593-594, engine.py:712-713)
// torch.mean((output - prototype_tensor) ** 2) in the SUM form of the KL pair above: row i holds (1/D) sum_d (emb - proto[y_i])^2, the
// entry point their sum; divided by the row count it is the reference's mean. One wave per row, lane-strided, explicit fmaf so that the
// one-launch loss tail (loss_tail_kernel<true>) repeats the row value bit for bit.
__device__ __forceinline__ float l2_grad_scale(int D) { return 2.0f / (float)D; }

__global__ __launch_bounds__(256) void proto_l2_rows_kernel(const float* __restrict__ emb, const int64_t* __restrict__ labels,
                                                            const float* __restrict__ proto, float* __restrict__ rows, int B, int D, int C) {
  fp16_sat_on();
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B) return;
  const float* a = emb + (size_t)r * D;
  const long y = (long)labels[r];
  if (y < 0 || y >= C) { if (lane == 0) rows[r] = __int_as_float(0x7fc00000); return; }      // see proto_kl_rows_kernel
  const float* t = proto + (size_t)y * D;
  float acc = 0.f;
  for (int d = lane; d < D; d += 64) {
    const float df = a[d] - t[d];
    acc = fmaf(df, df, acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) rows[r] = acc / (float)D;
}
extern "C" int gsl_proto_l2_fwd(const float* emb, const int64_t* labels, const float* proto, float* out1, float* row_ws, int B,
                                int D, int C, gsl_stream_t s) {
  GSL_CHECK_ARG(emb && labels && proto && out1 && row_ws && B > 0 && D > 0 && C > 0, "null/size");
  hipLaunchKernelGGL(proto_l2_rows_kernel, dim3((B + 3) / 4), dim3(256), 0, as_stream(s), emb, labels, proto, row_ws, B, D, C);
  hipLaunchKernelGGL(sum_rows_kernel, dim3(1), dim3(256), 0, as_stream(s), row_ws, out1, B, 1);
  return check_launch("gsl_proto_l2_fwd");
}

__global__ __launch_bounds__(256) void proto_l2_bwd_kernel(const float* __restrict__ emb, const int64_t* __restrict__ labels,
                                                           const float* __restrict__ proto, const float* __restrict__ coef,
                                                           float scale, float* demb, int B, int D, int C, int accumulate) {
  fp16_sat_on();
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B) return;
  const float* a = emb + (size_t)r * D;
  const long y = (long)labels[r];
  if (y < 0 || y >= C) {       // see proto_kl_rows_kernel
    for (int d = lane; d < D; d += 64) demb[(size_t)r * D + d] = __int_as_float(0x7fc00000);
    return;
  }
  const float* t = proto + (size_t)y * D;
  const float k = coef[0] * scale;
  const float s2 = l2_grad_scale(D);
  for (int d = lane; d < D; d += 64) {
    const float g = k * (s2 * (a[d] - t[d]));
    float* o = demb + (size_t)r * D + d;
    *o = accumulate ? (*o + g) : g;
  }
}
extern "C" int gsl_proto_l2_bwd(const float* emb, const int64_t* labels, const float* proto, const float* coef, float scale,
                                float* demb, int B, int D, int C, int accumulate, gsl_stream_t s) {
  GSL_CHECK_ARG(emb && labels && proto && coef && demb && B > 0 && D > 0 && C > 0, "null/size");
  hipLaunchKernelGGL(proto_l2_bwd_kernel, dim3((B + 3) / 4), dim3(256), 0, as_stream(s), emb, labels, proto, coef, scale, demb, B, D, C, accumulate);
  return check_launch("gsl_proto_l2_bwd");
}

// ------------------------------------------------------------------ K11b precision@k for several k (util/utils.py:354-368)
// One launch: a wave per row counts the logits strictly greater than the label's logit; the row is a top-k hit when that count is below
// k (= the label is among output.topk(k) wherever the k-th place is not tied). Hits are integers: per-block LDS counters, then one
// integer atomic per k and block, so the result does not depend on the order of the blocks.
constexpr int TOPK_MAX_K = 16;
struct TopkKs { int k[TOPK_MAX_K]; };
__global__ __launch_bounds__(256) void topk_hits_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, int B, int C,
                                                        TopkKs ks, int nk, int* __restrict__ hits) {
  __shared__ int h_s[TOPK_MAX_K];
  if (threadIdx.x < TOPK_MAX_K) h_s[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r < B) {
    const long yl = (long)labels[r];
    if (yl >= 0 && yl < C) {      // an out-of-range label is never a hit (no out-of-bounds read), as in ce_rows_kernel
      const float* row = logits + (size_t)r * C;
      const float yv = row[yl];
      int cnt = 0;
      for (int c = lane; c < C; c += 64) cnt += row[c] > yv ? 1 : 0;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
      if (lane < nk && cnt < ks.k[lane]) atomicAdd(&h_s[lane], 1);
    }
  }
  __syncthreads();
  if (threadIdx.x < nk && h_s[threadIdx.x] > 0) atomicAdd(hits + threadIdx.x, h_s[threadIdx.x]);
}
extern "C" int gsl_topk_max_k(void) { return TOPK_MAX_K; }
extern "C" int gsl_topk_hits(const float* logits, const int64_t* labels, int B, int C, const int* ks_host, int nk, int* hits, gsl_stream_t s) {
  GSL_CHECK_ARG(logits && labels && ks_host && hits && B > 0 && C > 0 && nk > 0 && nk <= TOPK_MAX_K, "null/size (1 <= nk <= 16 values of k)");
  TopkKs ks = {};
  for (int i = 0; i < nk; ++i) {
    GSL_CHECK_ARG(ks_host[i] > 0, "k > 0");
    ks.k[i] = ks_host[i];
  }
  if (hipMemsetAsync(hits, 0, sizeof(int) * (size_t)nk, as_stream(s)) != hipSuccess) return check_launch("gsl_topk_hits (clearing the counters)");
  hipLaunchKernelGGL(topk_hits_kernel, dim3((B + 3) / 4), dim3(256), 0, as_stream(s), logits, labels, B, C, ks, nk, hits);
  return check_launch("gsl_topk_hits");
}

// =====================================================================================
// The scalar tail of the step (engine_cl.py:65-125): total = beta*relu(BND - CE_f) + CE_r + alpha*L_s + w_f*relu(BND_pro - KL_f)
// + w_r*KL_r from the SUMS produced by the kernels above, the 8 meter values, and the 5 partial derivatives the backward hands
// to those kernels as upstream gradients. One thread: it replaces ~35 one-element torch kernels per step (3.5 % of the step at the
// reference's batch 48, where every launch counts). Same f32 operations in the same order as the torch expression it replaces.
// =====================================================================================
__global__ void loss_combine_kernel(const float* ce_r_sum, const float* ce_f_sum, const float* kl_f_sum, const float* kl_r_sum,
                                    const float* structure, const float* hit_r, const float* hit_f, float n_r, float n_f, float beta,
                                    float BND, float alpha, float w_f, float w_r, float BND_pro, float* total, float* meters,
                                    float* coefs) {
  fp16_sat_on();
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float loss_remain = ce_r_sum[0] / n_r;
  const float hinge_f = BND - ce_f_sum[0] / n_f;
  const float loss_forget = fmaxf(hinge_f, 0.f);
  const float st = structure ? structure[0] : 0.f;
  float pro_f = 0.f, pro_r = 0.f, hinge_p = 0.f;
  if (kl_f_sum) { hinge_p = BND_pro - kl_f_sum[0] / n_f; pro_f = w_f * fmaxf(hinge_p, 0.f); }
  if (kl_r_sum) pro_r = w_r * (kl_r_sum[0] / n_r);
  const float tot = loss_forget * beta + loss_remain + st * alpha + (pro_f + pro_r);
  total[0] = tot;
  meters[0] = beta * loss_forget; meters[1] = loss_remain; meters[2] = tot; meters[3] = alpha * st;
  meters[4] = hit_f[0] * (100.0f / n_f); meters[5] = hit_r[0] * (100.0f / n_r); meters[7] = pro_r;
  // without the prototype term the reference still LOGS w_f * relu(BND_pro - 0) in losses_prototype_forget (engine_cl.py:103-110,
  // engine.py:118-125: prototype_loss_forget is the constant 0 there); the total does not contain it
  meters[6] = kl_f_sum ? pro_f : w_f * fmaxf(BND_pro, 0.f);
  coefs[0] = 1.0f / n_r;                                     // d total / d ce_r_sum
  coefs[1] = hinge_f > 0.f ? -beta / n_f : 0.f;              // d total / d ce_f_sum   (relu'(0) = 0 as in torch)
  coefs[2] = (kl_f_sum && hinge_p > 0.f) ? -w_f / n_f : 0.f; // d total / d kl_f_sum
  coefs[3] = kl_r_sum ? w_r / n_r : 0.f;                     // d total / d kl_r_sum
  coefs[4] = alpha;                                          // d total / d structure
}
// Data-parallel form: the eight batch sums arrive as ONE all-reduced device array (gslora_hip/step.py packs and sum-all-reduces them
// before the hinges so that relu(BND - mean CE_f) / relu(BND_pro - mean KL_f) see the GLOBAL batch means, the reference's single-GPU /
// nn.DataParallel semantics, train_own_forget_cl.py:494-497): pack8 = [ce_r, ce_f, hit_r, hit_f, n_r, n_f, kl_f, kl_r]. The batch sizes
// are read from the pack, so no host value depends on the other ranks.
__global__ void loss_combine_pack_kernel(const float* pack, const float* structure, int has_proto, float beta, float BND, float alpha,
                                         float w_f, float w_r, float BND_pro, float* total, float* meters, float* coefs) {
  fp16_sat_on();
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float n_r = pack[4], n_f = pack[5];
  const float loss_remain = pack[0] / n_r;
  const float hinge_f = BND - pack[1] / n_f;
  const float loss_forget = fmaxf(hinge_f, 0.f);
  const float st = structure ? structure[0] : 0.f;
  float pro_f = 0.f, pro_r = 0.f, hinge_p = 0.f;
  if (has_proto) { hinge_p = BND_pro - pack[6] / n_f; pro_f = w_f * fmaxf(hinge_p, 0.f); pro_r = w_r * (pack[7] / n_r); }
  const float tot = loss_forget * beta + loss_remain + st * alpha + (pro_f + pro_r);
  total[0] = tot;
  meters[0] = beta * loss_forget; meters[1] = loss_remain; meters[2] = tot; meters[3] = alpha * st;
  meters[4] = pack[3] * (100.0f / n_f); meters[5] = pack[2] * (100.0f / n_r); meters[7] = pro_r;
  meters[6] = has_proto ? pro_f : w_f * fmaxf(BND_pro, 0.f);
  coefs[0] = 1.0f / n_r;
  coefs[1] = hinge_f > 0.f ? -beta / n_f : 0.f;
  coefs[2] = (has_proto && hinge_p > 0.f) ? -w_f / n_f : 0.f;
  coefs[3] = has_proto ? w_r / n_r : 0.f;
  coefs[4] = alpha;
}
extern "C" int gsl_loss_combine_pack(const float* pack8, const float* structure, int has_proto, float beta, float BND, float alpha,
                                     float w_f, float w_r, float BND_pro, float* total, float* meters8, float* coefs5, gsl_stream_t s) {
  GSL_CHECK_ARG(pack8 && total && meters8 && coefs5, "null");
  hipLaunchKernelGGL(loss_combine_pack_kernel, dim3(1), dim3(64), 0, as_stream(s), pack8, structure, has_proto, beta, BND, alpha, w_f, w_r,
                     BND_pro, total, meters8, coefs5);
  return check_launch("gsl_loss_combine_pack");
}
extern "C" int gsl_loss_combine(const float* ce_r_sum, const float* ce_f_sum, const float* kl_f_sum, const float* kl_r_sum,
                                const float* structure, const float* hit_r, const float* hit_f, float n_r, float n_f, float beta,
                                float BND, float alpha, float w_f, float w_r, float BND_pro, float* total, float* meters8,
                                float* coefs5, gsl_stream_t s) {
  GSL_CHECK_ARG(ce_r_sum && ce_f_sum && hit_r && hit_f && total && meters8 && coefs5 && n_r > 0.f && n_f > 0.f, "null/size");
  hipLaunchKernelGGL(loss_combine_kernel, dim3(1), dim3(64), 0, as_stream(s), ce_r_sum, ce_f_sum, kl_f_sum, kl_r_sum, structure, hit_r,
                     hit_f, n_r, n_f, beta, BND, alpha, w_f, w_r, BND_pro, total, meters8, coefs5);
  return check_launch("gsl_loss_combine");
}

// =====================================================================================
// The whole loss section of a single-process step in ONE launch (the launch-bound regime: few-shot batches replay ~20 one-block kernels
// here — CE rows + sums for the remain and forget rows, prototype KL rows + sums, the scalar tail, and the four backward kernels that
// turn its five coefficients into dlogits / demb). One workgroup of 16 waves: a wave owns every 16th row; row statistics stay in LDS
// between the forward and the backward half. Same device functions, same fixed summation orders as the separate kernels
// (sum_rows_kernel's 256-lane partition included): coefficients and gradients bit-identical to the multi-launch path.
// rows [0, nr) are the remain batch, [nr, N) the forget batch (engine_cl.py:59-125); N <= GSL_LOSS_TAIL_MAX_ROWS.
// =====================================================================================
constexpr int LT_MAX = 256, LT_V = 16;      // rows per launch; values per lane of a row held in registers (C, D <= 64 * LT_V)
// a row in registers: element lane + 64 i in v[i] (the lane-strided order of row_softmax_stats / row_lse); every pass over the row then
// runs from registers — the workgroup is alone on its CU, each global pass would be an exposed L2 round trip
__device__ __forceinline__ void lt_load(const float* row, int n, int lane, float v[LT_V]) {
#pragma unroll
  for (int i = 0; i < LT_V; ++i) { const int c = lane + 64 * i; v[i] = c < n ? row[c] : 0.f; }
}
__device__ __forceinline__ float lt_lse(const float v[LT_V], int n, int lane) {      // = row_lse
  float m = -3.0e38f;
#pragma unroll
  for (int i = 0; i < LT_V; ++i) if (lane + 64 * i < n) m = fmaxf(m, v[i]);
  m = wave_max(m);
  float se = 0.f;
#pragma unroll
  for (int i = 0; i < LT_V; ++i) if (lane + 64 * i < n) se += expf(v[i] - m);
  return m + logf(wave_sum(se));
}
// L2: the prototype term is the l2 distance (proto_l2_rows_kernel / proto_l2_bwd_kernel) instead of the KL (gsl_loss_tail_l2); the
// instantiation with L2 = false is the kernel gsl_loss_tail has always launched
template <bool L2>
__global__ __launch_bounds__(1024) void loss_tail_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, int N, int nr,
                                                         int C, const float* __restrict__ emb, const float* __restrict__ proto, int D,
                                                         int Cp, const float* structure, float beta, float BND, float alpha, float w_f,
                                                         float w_r, float BND_pro, float* out14, float* __restrict__ dlogits,
                                                         float* __restrict__ demb) {
  fp16_sat_on();
  __shared__ float ce_s[LT_MAX], hit_s[LT_MAX], kl_s[LT_MAX], lse_s[LT_MAX], la_s[LT_MAX], lt_s[LT_MAX];
  __shared__ float sm[16], coef_s[5];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nf = N - nr;
  for (int r = wave; r < N; r += 16) {
    float lg[LT_V];
    lt_load(logits + (size_t)r * C, C, lane, lg);
    // row_softmax_stats on the registers: max with the first-index tie-break, then the log-sum-exp
    float m = -3.0e38f; int mi = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < LT_V; ++i) { const int c = lane + 64 * i; if (c < C && lg[i] > m) { m = lg[i]; mi = c; } }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float om = __shfl_xor(m, o, 64); const int oi = __shfl_xor(mi, o, 64);
      if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
    }
    float se = 0.f;
#pragma unroll
    for (int i = 0; i < LT_V; ++i) if (lane + 64 * i < C) se += expf(lg[i] - m);
    se = wave_sum(se);
    const float lse = m + logf(se);
    const long yl = (long)labels[r];
    const bool y_ok = yl >= 0 && yl < C;      // out-of-range label: NaN loss / gradient row, no out-of-bounds read (see ce_rows_kernel)
    const int y = y_ok ? (int)yl : -1;
    if (lane == 0) { ce_s[r] = y_ok ? lse - logits[(size_t)r * C + y] : __int_as_float(0x7fc00000); hit_s[r] = (mi == y) ? 1.f : 0.f; lse_s[r] = lse; }
    if (emb) {
      if (yl < 0 || yl >= Cp) { if (lane == 0) kl_s[r] = __int_as_float(0x7fc00000); continue; }
      float a[LT_V], t[LT_V];
      lt_load(emb + (size_t)r * D, D, lane, a);
      lt_load(proto + (size_t)yl * D, D, lane, t);
      if constexpr (L2) {
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < LT_V; ++i) if (lane + 64 * i < D) {
          const float df = a[i] - t[i];
          acc = fmaf(df, df, acc);
        }
        acc = wave_sum(acc);
        if (lane == 0) kl_s[r] = acc / (float)D;
        continue;
      }
      const float la = lt_lse(a, D, lane), lt = lt_lse(t, D, lane);
      float acc = 0.f;
#pragma unroll
      for (int i = 0; i < LT_V; ++i) if (lane + 64 * i < D) {
        const float ltd = t[i] - lt;
        acc += expf(ltd) * (ltd - (a[i] - la));
      }
      acc = wave_sum(acc);
      if (lane == 0) { kl_s[r] = acc; la_s[r] = la; lt_s[r] = lt; }
    }
  }
  __syncthreads();
  // the six batch sums, in sum_rows_kernel's order (256 lanes stride the rows, fixed-order combine; the other waves add exact zeros)
  auto range_sum = [&](const float* v, int base, int n) {
    float a = 0.f;
    if (threadIdx.x < 256) for (int r = threadIdx.x; r < n; r += 256) a += v[base + r];
    return block_sum(a, sm);
  };
  const float ce_r = range_sum(ce_s, 0, nr), hit_r = range_sum(hit_s, 0, nr);
  const float ce_f = range_sum(ce_s, nr, nf), hit_f = range_sum(hit_s, nr, nf);
  float kl_f = 0.f, kl_r = 0.f;
  if (emb) { kl_f = range_sum(kl_s, nr, nf); kl_r = range_sum(kl_s, 0, nr); }
  if (threadIdx.x == 0) {      // gsl_loss_combine, operation for operation
    const float n_r = (float)nr, n_f = (float)nf;
    const float loss_remain = ce_r / n_r;
    const float hinge_f = BND - ce_f / n_f;
    const float loss_forget = fmaxf(hinge_f, 0.f);
    const float st = structure ? structure[0] : 0.f;
    float pro_f = 0.f, pro_r = 0.f, hinge_p = 0.f;
    if (emb) { hinge_p = BND_pro - kl_f / n_f; pro_f = w_f * fmaxf(hinge_p, 0.f); pro_r = w_r * (kl_r / n_r); }
    const float tot = loss_forget * beta + loss_remain + st * alpha + (pro_f + pro_r);
    float* meters = out14 + 1;
    float* coefs = out14 + 9;
    out14[0] = tot;
    meters[0] = beta * loss_forget; meters[1] = loss_remain; meters[2] = tot; meters[3] = alpha * st;
    meters[4] = hit_f * (100.0f / n_f); meters[5] = hit_r * (100.0f / n_r); meters[7] = pro_r;
    meters[6] = emb ? pro_f : w_f * fmaxf(BND_pro, 0.f);
    coef_s[0] = coefs[0] = 1.0f / n_r;
    coef_s[1] = coefs[1] = hinge_f > 0.f ? -beta / n_f : 0.f;
    coef_s[2] = coefs[2] = (emb && hinge_p > 0.f) ? -w_f / n_f : 0.f;
    coef_s[3] = coefs[3] = emb ? w_r / n_r : 0.f;
    coef_s[4] = coefs[4] = alpha;
  }
  __syncthreads();
  for (int r = wave; r < N; r += 16) {      // gsl_ce_bwd / gsl_proto_kl_bwd with the coefficients above (upstream gradient 1)
    const float k = coef_s[r < nr ? 0 : 1] * 1.0f;
    const long yl = (long)labels[r];
    const bool y_ok = yl >= 0 && yl < C;
    const int y = y_ok ? (int)yl : -1;
    const float lse = lse_s[r];
    float lg[LT_V];
    lt_load(logits + (size_t)r * C, C, lane, lg);
#pragma unroll
    for (int i = 0; i < LT_V; ++i) { const int c = lane + 64 * i; if (c < C) dlogits[(size_t)r * C + c] = y_ok ? k * (expf(lg[i] - lse) - (c == y ? 1.f : 0.f)) : __int_as_float(0x7fc00000); }
    if (emb) {
      if (yl < 0 || yl >= Cp) {
        for (int d = lane; d < D; d += 64) demb[(size_t)r * D + d] = __int_as_float(0x7fc00000);
        continue;
      }
      float a[LT_V], t[LT_V];
      lt_load(emb + (size_t)r * D, D, lane, a);
      lt_load(proto + (size_t)yl * D, D, lane, t);
      const float kk = coef_s[r < nr ? 3 : 2] * 1.0f;
      if constexpr (L2) {
        const float s2 = l2_grad_scale(D);
#pragma unroll
        for (int i = 0; i < LT_V; ++i) { const int d = lane + 64 * i; if (d < D) demb[(size_t)r * D + d] = kk * (s2 * (a[i] - t[i])); }
        continue;
      }
      const float la = la_s[r], lt = lt_s[r];
#pragma unroll
      for (int i = 0; i < LT_V; ++i) { const int d = lane + 64 * i; if (d < D) demb[(size_t)r * D + d] = kk * (expf(a[i] - la) - expf(t[i] - lt)); }
    }
  }
}
extern "C" int gsl_loss_tail_max_rows(void) { return LT_MAX; }
extern "C" int gsl_loss_tail(const float* logits, const int64_t* labels, int N, int nr, int C, const float* emb, const float* proto, int D,
                             int Cp, const float* structure, float beta, float BND, float alpha, float w_f, float w_r, float BND_pro,
                             float* out14, float* dlogits, float* demb, gsl_stream_t s) {
  GSL_CHECK_ARG(logits && labels && out14 && dlogits && N > 0 && N <= LT_MAX && nr > 0 && nr < N && C > 0 && C <= 64 * LT_V && D <= 64 * LT_V,
                "null/size (0 < nr < N <= 256 rows, C and D <= 1024)");
  GSL_CHECK_ARG(!emb || (proto && demb && D > 0 && Cp > 0), "prototype term: emb, proto and demb together");
  hipLaunchKernelGGL(loss_tail_kernel<false>, dim3(1), dim3(1024), 0, as_stream(s), logits, labels, N, nr, C, emb, proto, D, Cp, structure, beta, BND,
                     alpha, w_f, w_r, BND_pro, out14, dlogits, demb);
  return check_launch("gsl_loss_tail");
}
// gsl_loss_tail with the l2 prototype distance (engine_cl.py:593-594); the prototype term is required here (without one, gsl_loss_tail)
extern "C" int gsl_loss_tail_l2(const float* logits, const int64_t* labels, int N, int nr, int C, const float* emb, const float* proto, int D,
                                int Cp, const float* structure, float beta, float BND, float alpha, float w_f, float w_r, float BND_pro,
                                float* out14, float* dlogits, float* demb, gsl_stream_t s) {
  GSL_CHECK_ARG(logits && labels && out14 && dlogits && N > 0 && N <= LT_MAX && nr > 0 && nr < N && C > 0 && C <= 64 * LT_V && D <= 64 * LT_V,
                "null/size (0 < nr < N <= 256 rows, C and D <= 1024)");
  GSL_CHECK_ARG(emb && proto && demb && D > 0 && Cp > 0, "prototype term: emb, proto and demb are required");
  hipLaunchKernelGGL(loss_tail_kernel<true>, dim3(1), dim3(1024), 0, as_stream(s), logits, labels, N, nr, C, emb, proto, D, Cp, structure, beta, BND,
                     alpha, w_f, w_r, BND_pro, out14, dlogits, demb);
  return check_launch("gsl_loss_tail_l2");
}
