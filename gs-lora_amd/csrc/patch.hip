// patch.hip — the input end of the network, image -> patch operand of the embedding GEMM:
//   K1  patch gather (einops rearrange, vit_pytorch_face/vit_face.py:530); K1s its overlapping-window form (nn.Unfold, vits_face.py:446-450)
//   and both from uint8 images (ToTensor + Normalize fused into the gather).

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
// out-of-range kw (65535: beyond every W the entry accepts, independent of H), so they fail the bounds test like a padding tap. A workgroup takes UNF_ROWS consecutive rows (neighbouring windows of
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
      // kw = 0xffff: w = w0 + 65535 >= 65535 - pad > W for every accepted W < 32768 (pad < k <= 64), whatever H and h0 are. (kh = 0x7fff alone
      // was in range again at H + pad >= 32768: row -pad of the image, read in front of it.) Always 0.
      unf_tab[j] = make_int2(0, (0x7fff << 16) | 0xffff);
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
