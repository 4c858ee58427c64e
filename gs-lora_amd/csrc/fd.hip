// fd.hip — libgslora_fd.so: the function-distance term of the DER / DER++ and FDR baselines (include/gslora_fd.h).
//   gsf_rowdist_*   the distance between a student's and a frozen teacher's [B, W] rows (embeddings: DER; logits: FDR) and its gradient
// A fifth product library: its own error string; nothing shared with libgslora_hip.so but the headers (gsl_common.h and the public ones),
// and with the other side libraries gsl_chunks.h: the alignment predicate and the one-workgroup sum of the reduce kernel.
#include "gsl_chunks.h"

#include "../../include/gslora_fd.h"

using namespace gsl;

namespace gsl { thread_local char g_err[512] = {0}; }
extern "C" const char* gsf_last_error(void) { return gsl::g_err; }

constexpr int FD_WAVE_MAX_W = 1024;      // the plan's threshold: up to it a wave serves a row (at most four groups per lane)

// every row of a [B, .] tensor with row stride ld starts on a 16-byte boundary
static inline bool rows_aligned16(const void* p, long ld, int B) { return aligned16(p) && (B == 1 || (ld & 3) == 0); }

// The sum of squared differences over the groups first, first + stride, .. of one row pair: this thread's elements in ascending order.
template <bool VEC>
__device__ __forceinline__ float fd_partial(const float* __restrict__ a, const float* __restrict__ t, int W, int first, int stride) {
#pragma clang fp contract(off)
  float acc = 0.f;
  const int ng = (W + 3) >> 2;
  for (int g = first; g < ng; g += stride) {
    const int c = g << 2;
    if (VEC && c + 4 <= W) {
      const float4 x = *reinterpret_cast<const float4*>(a + c);
      const float4 y = *reinterpret_cast<const float4*>(t + c);
      const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
      acc += d0 * d0;
      acc += d1 * d1;
      acc += d2 * d2;
      acc += d3 * d3;
    } else {
      const int e = min(W, c + 4);
      for (int i = c; i < e; ++i) {
        const float d = a[i] - t[i];
        acc += d * d;
      }
    }
  }
  return acc;
}

template <bool VEC>
__global__ __launch_bounds__(256) void fd_rows_wave_kernel(const float* __restrict__ a, long ld_a, const float* __restrict__ t, long ld_t, int B,
                                                           int W, float* __restrict__ ws) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B) return;      // (no workgroup barrier in this kernel)
  const float s = wave_sum(fd_partial<VEC>(a + (size_t)r * ld_a, t + (size_t)r * ld_t, W, lane, 64));
  if (lane == 0) ws[r] = s;
}

template <bool VEC>
__global__ __launch_bounds__(256) void fd_rows_block_kernel(const float* __restrict__ a, long ld_a, const float* __restrict__ t, long ld_t, int B,
                                                            int W, float* __restrict__ ws) {
  __shared__ float sm[16];
  const int r = blockIdx.x;
  const float s = block_sum(fd_partial<VEC>(a + (size_t)r * ld_a, t + (size_t)r * ld_t, W, threadIdx.x, 256), sm);
  if (threadIdx.x == 0) ws[r] = s;
}

// the batch sum (256 threads stride the rows, fixed-order combine) and the result
__global__ __launch_bounds__(256) void fd_reduce_kernel(const float* __restrict__ ws, int B, int mode, float* __restrict__ out1) {
#pragma clang fp contract(off)
  __shared__ float sm[16];
  const float tot = strided_sum(ws, B, sm, [&](float s) { return mode == GSF_ROWNORM ? sqrtf(s) : s; });
  if (threadIdx.x == 0) {
    if (mode == GSF_ROWNORM) {
      out1[0] = tot / (float)B;
    } else {
      const float n = sqrtf(tot);
      out1[0] = n * n;
    }
  }
}

__device__ __forceinline__ float fd_grad(float x, float y, float k, bool zero, float old, int accumulate) {
#pragma clang fp contract(off)
  const float v = zero ? 0.f : (x - y) * k;
  return accumulate ? old + v : v;
}

template <bool WAVE, bool VEC>
__global__ __launch_bounds__(256) void fd_bwd_kernel(const float* __restrict__ a, long ld_a, const float* __restrict__ t, long ld_t,
                                                     const float* __restrict__ ws, const float* __restrict__ gout, int B, int W, int mode,
                                                     float coef, float* d, long ld_d, int accumulate) {
#pragma clang fp contract(off)
  const int r = WAVE ? blockIdx.x * 4 + (threadIdx.x >> 6) : blockIdx.x;
  if (r >= B) return;
  const int first = WAVE ? (threadIdx.x & 63) : threadIdx.x, stride = WAVE ? 64 : 256;
  const float* __restrict__ arow = a + (size_t)r * ld_a;
  const float* __restrict__ trow = t + (size_t)r * ld_t;
  float* drow = d + (size_t)r * ld_d;
  const float gc = gout[0] * coef;
  float k;
  bool zero = false;
  if (mode == GSF_ROWNORM) {
    const float s = ws[r];
    zero = s == 0.f;
    k = (gc / (float)B) / sqrtf(s);
  } else {
    k = 2.f * gc;
  }
  const int ng = (W + 3) >> 2;
  for (int g = first; g < ng; g += stride) {
    const int c = g << 2;
    if (VEC && c + 4 <= W) {
      const float4 x = *reinterpret_cast<const float4*>(arow + c);
      const float4 y = *reinterpret_cast<const float4*>(trow + c);
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
      if (accumulate) o = *reinterpret_cast<const float4*>(drow + c);
      o.x = fd_grad(x.x, y.x, k, zero, o.x, accumulate);
      o.y = fd_grad(x.y, y.y, k, zero, o.y, accumulate);
      o.z = fd_grad(x.z, y.z, k, zero, o.z, accumulate);
      o.w = fd_grad(x.w, y.w, k, zero, o.w, accumulate);
      *reinterpret_cast<float4*>(drow + c) = o;
    } else {
      const int e = min(W, c + 4);
      for (int i = c; i < e; ++i) drow[i] = fd_grad(arow[i], trow[i], k, zero, accumulate ? drow[i] : 0.f, accumulate);
    }
  }
}

static int fd_check(const char* who, int B, int W) {
  GSL_CHECK_ARG_AS(who, B >= 1 && W >= 1, "B >= 1, W >= 1");
  GSL_CHECK_ARG_AS(who, W <= GSF_MAX_W, "W <= 2^30");
  return GSL_OK;
}

extern "C" int gsf_rowdist_plan(int B, int W, int* kernel, int* grid, long* ws_elems) {
  GSL_TRY(fd_check(__func__, B, W));
  GSL_CHECK_ARG(kernel && grid && ws_elems, "null result");
  const bool wave = W <= FD_WAVE_MAX_W;
  *kernel = wave ? GSF_WAVE : GSF_BLOCK;
  *grid = wave ? (int)(((long)B + 3) / 4) : B;
  *ws_elems = (long)B;
  return GSL_OK;
}

extern "C" long gsf_rowdist_ws_elems(int B, int W) { return fd_check(__func__, B, W) == GSL_OK ? (long)B : -1; }

static int fd_args(const char* who, const float* a, long ld_a, const float* t, long ld_t, int B, int W, int mode) {
  GSL_TRY(fd_check(who, B, W));
  GSL_CHECK_ARG_AS(who, a && t, "null a or t");
  GSL_CHECK_ARG_AS(who, ld_a >= W && ld_t >= W, "ld_a >= W, ld_t >= W");
  GSL_CHECK_ARG_AS(who, mode == GSF_SQ || mode == GSF_ROWNORM, "mode is GSF_SQ or GSF_ROWNORM");
  return GSL_OK;
}

extern "C" int gsf_rowdist_fwd(const float* a, long ld_a, const float* t, long ld_t, int B, int W, int mode, float* out1, float* ws,
                               gsl_stream_t s) {
  GSL_TRY(fd_args(__func__, a, ld_a, t, ld_t, B, W, mode));
  GSL_CHECK_ARG(out1, "null out");
  GSL_CHECK_ARG(ws, "null ws");
  int kernel, grid; long elems;
  GSL_TRY(gsf_rowdist_plan(B, W, &kernel, &grid, &elems));
  const bool vec = rows_aligned16(a, ld_a, B) && rows_aligned16(t, ld_t, B);
  auto rows = kernel == GSF_WAVE ? (vec ? fd_rows_wave_kernel<true> : fd_rows_wave_kernel<false>)
                                 : (vec ? fd_rows_block_kernel<true> : fd_rows_block_kernel<false>);
  hipLaunchKernelGGL(rows, dim3(grid), dim3(256), 0, as_stream(s), a, ld_a, t, ld_t, B, W, ws);
  GSL_TRY(check_launch("gsf_rowdist_fwd(rows)"));
  hipLaunchKernelGGL(fd_reduce_kernel, dim3(1), dim3(256), 0, as_stream(s), ws, B, mode, out1);
  return check_launch("gsf_rowdist_fwd(reduce)");
}

extern "C" int gsf_rowdist_bwd(const float* a, long ld_a, const float* t, long ld_t, const float* ws, const float* gout, int B, int W, int mode,
                               float coef, float* d, long ld_d, int accumulate, gsl_stream_t s) {
  GSL_TRY(fd_args(__func__, a, ld_a, t, ld_t, B, W, mode));
  GSL_CHECK_ARG(ws && gout && d, "null ws, gout or d");
  GSL_CHECK_ARG(ld_d >= W, "ld_d >= W");
  int kernel, grid; long elems;
  GSL_TRY(gsf_rowdist_plan(B, W, &kernel, &grid, &elems));
  const bool vec = rows_aligned16(a, ld_a, B) && rows_aligned16(t, ld_t, B) && rows_aligned16(d, ld_d, B);
  auto bwd = kernel == GSF_WAVE ? (vec ? fd_bwd_kernel<true, true> : fd_bwd_kernel<true, false>)
                                : (vec ? fd_bwd_kernel<false, true> : fd_bwd_kernel<false, false>);
  hipLaunchKernelGGL(bwd, dim3(grid), dim3(256), 0, as_stream(s), a, ld_a, t, ld_t, ws, gout, B, W, mode, coef, d, ld_d, accumulate);
  return check_launch(__func__);
}
