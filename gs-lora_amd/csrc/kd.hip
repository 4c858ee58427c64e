// kd.hip — libgslora_kd.so: the loss side of the SCRUB baseline (include/gslora_kd.h).
//   gsk_kd_ce_*       DistillKL (reference util/sgda_utils.py) fused with the student's mean cross-entropy, and the gradient of both in one
//                     pass over the two logit matrices
//   gsk_param_dist_*  param_dist (util/sgda_utils.py) over every parameter at once: two launches forward, one backward
// A fourth product library: its own error string; nothing shared with libgslora_hip.so but the headers (gsl_common.h and the public ones),
// and with the other side libraries gsl_chunks.h: gsk_param_dist_* are its chunked sum, owner search and chunk walk.
#include "gsl_chunks.h"

#include "../../include/gslora_kd.h"

using namespace gsl;

namespace gsl { thread_local char g_err[512] = {0}; }
extern "C" const char* gsk_last_error(void) { return gsl::g_err; }

#define GSK_NAN __int_as_float(0x7fc00000)

// =====================================================================================
// gsk_kd_ce_*. The row walk is that of loss.hip (element c of a row belongs to thread c mod STRIDE, a thread visits its elements in
// ascending order); the row functions are written once over the two forms that hold a row pair.
// =====================================================================================
constexpr int KD_V = 16;                     // values per lane of a row held in registers
constexpr int KD_WAVE_MAX_C = 64 * KD_V;     // the plan's threshold: above it a wave cannot hold both rows
constexpr int KD_MAX_C = 1 << 30;            // column counters are ints that step by 256

// wave per row: both rows in registers, loaded once
struct WaveRows {
  float s[KD_V], t[KD_V];
  int n, lane;
  __device__ __forceinline__ WaveRows(const float* ys, const float* yt, int n_, int lane_) : n(n_), lane(lane_) {
#pragma unroll
    for (int i = 0; i < KD_V; ++i) {
      const int c = lane + 64 * i;
      s[i] = c < n ? ys[c] : 0.f;
      t[i] = c < n ? yt[c] : 0.f;
    }
  }
  template <typename F> __device__ __forceinline__ void each(F&& f) const {      // f(c, ys[c], yt[c]) for this lane's elements
#pragma unroll
    for (int i = 0; i < KD_V; ++i) { const int c = lane + 64 * i; if (c < n) f(c, s[i], t[i]); }
  }
  __device__ __forceinline__ float sum(float v) const { return wave_sum(v); }
  __device__ __forceinline__ float max(float v) const { return wave_max(v); }
};
// workgroup per row: every pass reads memory (the row pair of a wide head stays in L2 between the passes)
struct BlockRows {
  const float* ys;
  const float* yt;
  int n;
  float* sm;
  template <typename F> __device__ __forceinline__ void each(F&& f) const {
    for (int c = threadIdx.x; c < n; c += 256) f(c, ys[c], yt[c]);
  }
  __device__ __forceinline__ float sum(float v) const { return block_sum(v, sm); }
  __device__ __forceinline__ float max(float v) const { return block_max(v, sm); }
};

struct KdRow { float la, lt, ls, kd, ce; };

// One row pair. The maximum of a = ys / T is fl(max(ys) / T): a correctly rounded division by T > 0 is monotone, so one maximum of ys
// serves lse(a) and lse(ys). ys_row: the student's row in memory, for the label's logit.
template <typename R>
__device__ __forceinline__ KdRow kd_ce_row(const R& r, const float* ys_row, float T, bool with_ce, long label) {
  float ms = -3.0e38f, mt = -3.0e38f;
  r.each([&](int, float s, float t) { ms = fmaxf(ms, s); mt = fmaxf(mt, t); });
  ms = r.max(ms);
  mt = r.max(mt);
  const float ma = ms / T, mtt = mt / T;
  float sa = 0.f, st = 0.f, ss = 0.f;
  r.each([&](int, float s, float t) { sa += expf(s / T - ma); st += expf(t / T - mtt); });
  KdRow o;
  o.la = ma + logf(r.sum(sa));
  o.lt = mtt + logf(r.sum(st));
  float acc = 0.f;
  r.each([&](int, float s, float t) {
    const float ltd = t / T - o.lt;
    acc += expf(ltd) * (ltd - (s / T - o.la));      // exp(lt) (lt - la) on the shifted logs: an underflowed class adds 0 * finite
  });
  o.kd = r.sum(acc);
  o.ls = 0.f;
  o.ce = 0.f;
  if (with_ce) {
    r.each([&](int, float s, float) { ss += expf(s - ms); });
    o.ls = ms + logf(r.sum(ss));
    const bool ok = label >= 0 && label < r.n;
    o.ce = ok ? o.ls - ys_row[ok ? label : 0] : GSK_NAN;
  }
  return o;
}

__device__ __forceinline__ void kd_row_store(float* __restrict__ ws, int B, int r, const KdRow& o) {
  ws[r] = o.la;
  ws[(size_t)B + r] = o.lt;
  ws[2 * (size_t)B + r] = o.ls;
  ws[3 * (size_t)B + r] = o.kd;
  ws[4 * (size_t)B + r] = o.ce;
}

__global__ __launch_bounds__(256) void kd_rows_wave_kernel(const float* __restrict__ ys, long ld_s, const float* __restrict__ yt, long ld_t,
                                                           const int64_t* __restrict__ labels, int B, int C, float T, int with_ce,
                                                           float* __restrict__ ws) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B) return;      // (no workgroup barrier in this kernel)
  const float* srow = ys + (size_t)r * ld_s;
  const WaveRows rows(srow, yt + (size_t)r * ld_t, C, lane);
  const KdRow o = kd_ce_row(rows, srow, T, with_ce != 0, with_ce ? (long)labels[r] : 0L);
  if (lane == 0) kd_row_store(ws, B, r, o);
}

__global__ __launch_bounds__(256) void kd_rows_block_kernel(const float* __restrict__ ys, long ld_s, const float* __restrict__ yt, long ld_t,
                                                            const int64_t* __restrict__ labels, int B, int C, float T, int with_ce,
                                                            float* __restrict__ ws) {
  __shared__ float sm[16];
  const int r = blockIdx.x;
  const float* srow = ys + (size_t)r * ld_s;
  const BlockRows rows{srow, yt + (size_t)r * ld_t, C, sm};
  const KdRow o = kd_ce_row(rows, srow, T, with_ce != 0, with_ce ? (long)labels[r] : 0L);
  if (threadIdx.x == 0) kd_row_store(ws, B, r, o);
}

// the batch sums (sum_rows_kernel's order: 256 threads stride the rows, fixed-order combine) and the three results
__global__ __launch_bounds__(256) void kd_ce_reduce_kernel(const float* __restrict__ ws, int B, float T2, float c_kd, float c_ce,
                                                           float* __restrict__ out3) {
#pragma clang fp contract(off)
  __shared__ float sm[16];
  // (not two strided_sum calls: one loop keeps both loads of a trip in flight — two loops cost 3.8 us of 13.5 at B = 4096,
  //  profiles/side_kernels_dedupe.md)
  float a = 0.f, b = 0.f;
  for (int r = threadIdx.x; r < B; r += 256) { a += ws[3 * (size_t)B + r]; b += ws[4 * (size_t)B + r]; }
  const float kd = block_sum(a, sm), ce = block_sum(b, sm);
  if (threadIdx.x == 0) {
    const float n = (float)B;
    const float o0 = (kd * T2) / n;
    const float o1 = c_ce != 0.f ? ce / n : 0.f;
    const float w0 = c_kd * o0, w1 = c_ce * o1;
    out3[0] = o0;
    out3[1] = o1;
    out3[2] = w0 + w1;
  }
}

// one element of the gradient: every operation rounded on its own
__device__ __forceinline__ float kd_ce_grad(float s, float t, float T, float la, float lt, float ls, float k1, float k2, bool with_ce, bool hot) {
#pragma clang fp contract(off)
  const float a = s / T, u = t / T;
  const float dp = expf(a - la) - expf(u - lt);
  float v = k1 * dp;
  if (with_ce) {
    const float dq = expf(s - ls) - (hot ? 1.f : 0.f);
    const float w = k2 * dq;
    v = v + w;
  }
  return v;
}
__device__ __forceinline__ void kd_grad_store(float* o, float g, int accumulate) {
#pragma clang fp contract(off)
  *o = accumulate ? (*o + g) : g;
}

template <bool WAVE>
__global__ __launch_bounds__(256) void kd_ce_bwd_kernel(const float* __restrict__ ys, long ld_s, const float* __restrict__ yt, long ld_t,
                                                        const int64_t* __restrict__ labels, const float* __restrict__ ws,
                                                        const float* __restrict__ gout, int B, int C, float T, float k_kd, float k_ce,
                                                        int with_ce, float* d, long ld_d, int accumulate) {
#pragma clang fp contract(off)
  const int r = WAVE ? blockIdx.x * 4 + (threadIdx.x >> 6) : blockIdx.x;
  if (r >= B) return;
  const int first = WAVE ? (threadIdx.x & 63) : threadIdx.x, step = WAVE ? 64 : 256;
  const float* __restrict__ srow = ys + (size_t)r * ld_s;
  const float* __restrict__ trow = yt + (size_t)r * ld_t;
  float* drow = d + (size_t)r * ld_d;
  long y = 0;
  if (with_ce) {
    y = (long)labels[r];
    if (!(y >= 0 && y < C)) {
      for (int c = first; c < C; c += step) drow[c] = GSK_NAN;
      return;
    }
  }
  const float g = gout[0];
  const float k1 = g * k_kd, k2 = g * k_ce;
  const float la = ws[r], lt = ws[(size_t)B + r], ls = ws[2 * (size_t)B + r];
  for (int c = first; c < C; c += step)
    kd_grad_store(drow + c, kd_ce_grad(srow[c], trow[c], T, la, lt, ls, k1, k2, with_ce != 0, c == (int)y), accumulate);
}

static int kd_check(const char* who, int B, int C) {
  GSL_CHECK_ARG_AS(who, B >= 1 && C >= 1, "B >= 1, C >= 1");
  GSL_CHECK_ARG_AS(who, C <= KD_MAX_C, "C <= 2^30");
  return GSL_OK;
}

extern "C" int gsk_kd_plan(int B, int C, int* kernel, int* grid, long* ws_elems) {
  GSL_TRY(kd_check(__func__, B, C));
  GSL_CHECK_ARG(kernel && grid && ws_elems, "null result");
  const bool wave = C <= KD_WAVE_MAX_C;
  *kernel = wave ? GSK_KD_WAVE : GSK_KD_BLOCK;
  *grid = wave ? (B + 3) / 4 : B;
  *ws_elems = 5L * B;
  return GSL_OK;
}

extern "C" long gsk_kd_ws_elems(int B, int C) { return kd_check(__func__, B, C) == GSL_OK ? 5L * B : -1; }

static int kd_args(const char* who, const float* ys, long ld_s, const float* yt, long ld_t, const int64_t* labels, int B, int C, float T,
                   float c_ce) {
  GSL_TRY(kd_check(who, B, C));
  GSL_CHECK_ARG_AS(who, ys && yt, "null logits");
  GSL_CHECK_ARG_AS(who, ld_s >= C && ld_t >= C, "ld_s >= C, ld_t >= C");
  GSL_CHECK_ARG_AS(who, T > 0.f, "T > 0");
  GSL_CHECK_ARG_AS(who, labels || c_ce == 0.f, "labels == NULL needs c_ce == 0");
  return GSL_OK;
}

extern "C" int gsk_kd_ce_fwd(const float* ys, long ld_s, const float* yt, long ld_t, const int64_t* labels, int B, int C, float T, float c_kd,
                             float c_ce, float* out3, float* ws, gsl_stream_t s) {
  GSL_TRY(kd_args(__func__, ys, ld_s, yt, ld_t, labels, B, C, T, c_ce));
  GSL_CHECK_ARG(out3, "null out");
  GSL_CHECK_ARG(ws, "null ws");
  int kernel, grid; long elems;
  GSL_TRY(gsk_kd_plan(B, C, &kernel, &grid, &elems));
  const int with_ce = c_ce != 0.f;
  if (kernel == GSK_KD_WAVE)
    hipLaunchKernelGGL(kd_rows_wave_kernel, dim3(grid), dim3(256), 0, as_stream(s), ys, ld_s, yt, ld_t, labels, B, C, T, with_ce, ws);
  else
    hipLaunchKernelGGL(kd_rows_block_kernel, dim3(grid), dim3(256), 0, as_stream(s), ys, ld_s, yt, ld_t, labels, B, C, T, with_ce, ws);
  GSL_TRY(check_launch("gsk_kd_ce_fwd(rows)"));
  const float T2 = (float)((double)T * (double)T);
  hipLaunchKernelGGL(kd_ce_reduce_kernel, dim3(1), dim3(256), 0, as_stream(s), ws, B, T2, c_kd, c_ce, out3);
  return check_launch("gsk_kd_ce_fwd(reduce)");
}

extern "C" int gsk_kd_ce_bwd(const float* ys, long ld_s, const float* yt, long ld_t, const int64_t* labels, const float* ws, const float* gout,
                             int B, int C, float T, float c_kd, float c_ce, float* d, long ld_d, int accumulate, gsl_stream_t s) {
  GSL_TRY(kd_args(__func__, ys, ld_s, yt, ld_t, labels, B, C, T, c_ce));
  GSL_CHECK_ARG(ws && gout && d, "null ws, gout or d");
  GSL_CHECK_ARG(ld_d >= C, "ld_d >= C");
  int kernel, grid; long elems;
  GSL_TRY(gsk_kd_plan(B, C, &kernel, &grid, &elems));
  const float n = (float)B;
  const float k_kd = c_kd * (T / n), k_ce = c_ce / n;
  const int with_ce = c_ce != 0.f;      // the forward's rule
  hipLaunchKernelGGL(kernel == GSK_KD_WAVE ? kd_ce_bwd_kernel<true> : kd_ce_bwd_kernel<false>, dim3(grid), dim3(256), 0, as_stream(s), ys, ld_s,
                     yt, ld_t, labels, ws, gout, B, C, T, k_kd, k_ce, with_ce, d, ld_d, accumulate);
  return check_launch(__func__);
}

// =====================================================================================
// gsk_param_dist_*: the table is built on the host (gsk_param_dist_layout), the kernels look their entry up by workgroup index.
// =====================================================================================
extern "C" int gsk_param_dist_layout(const void* const* p, const void* const* q, const long* n, const int* trainable, int n_entries,
                                     gsk_dist_entry* table, long* total_blocks, long* bwd_blocks, long* g_elems) {
  GSL_CHECK_ARG(p && q && n && trainable && table, "null host array");
  GSL_CHECK_ARG(total_blocks && bwd_blocks && g_elems, "null result");
  GSL_CHECK_ARG(n_entries >= 1 && n_entries < (1 << 20), "1 <= n_entries < 2^20");
  long blk = 0, bblk = 0, goff = 0;
  for (int e = 0; e < n_entries; ++e) {
    GSL_CHECK_ARG(p[e] && q[e], "null tensor in an entry");
    GSL_CHECK_ARG(n[e] >= 1 && n[e] < (1L << 31), "1 <= n < 2^31 in every entry");
    GSL_CHECK_ARG(aligned4(p[e]) && aligned4(q[e]), "tensors are 4-byte aligned");
    gsk_dist_entry& o = table[e];
    o.p = static_cast<const float*>(p[e]);
    o.q = static_cast<const float*>(q[e]);
    o.n = n[e];
    o.nblk = chunk_blocks(n[e]);
    o.chunk = chunk_len(n[e], o.nblk);
    o.blk0 = (int)blk;
    o.bblk0 = (int)bblk;
    o.pad_ = 0;
    blk += o.nblk;
    if (trainable[e]) {
      o.goff = goff;
      goff += (n[e] + 3) / 4 * 4;
      bblk += o.nblk;
    } else {
      o.goff = -1;
    }
    GSL_CHECK_ARG(blk < (1L << 31), "fewer than 2^31 workgroups");
  }
  *total_blocks = blk;
  *bwd_blocks = bblk;
  *g_elems = goff;
  return GSL_OK;
}

// The forward's owner is the last entry whose blk0 <= b. The backward's is the last one whose bblk0 <= b: a frozen entry shares its bblk0
// with the trainable entry behind it, which is the later of the two; frozen entries at the end hold bwd_blocks, beyond every b — always a
// trainable one for b < bwd_blocks.
__global__ __launch_bounds__(256) void param_dist_partial_kernel(const gsk_dist_entry* __restrict__ tab, int n_entries, float* __restrict__ ws) {
  __shared__ float sm[16];
  const gsk_dist_entry e = tab[chunk_owner(tab, n_entries, blockIdx.x, &gsk_dist_entry::blk0)];
  const float* __restrict__ p = e.p;
  const float* __restrict__ q = e.q;
  const long i0 = (long)(blockIdx.x - e.blk0) * e.chunk, i1 = min(e.n, i0 + e.chunk);
  const float s = chunk_partial(i0, i1, sm, [&](long i) { return quad_term(p, q, nullptr, i); });
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void param_dist_reduce_kernel(const gsk_dist_entry* __restrict__ tab, int n_entries, const float* __restrict__ ws,
                                                                float p, float* __restrict__ norms, float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ float sm[16];
  float total = 0.f;
  for (int e = 0; e < n_entries; ++e) {
    const float s = strided_sum(ws + tab[e].blk0, tab[e].nblk, sm);      // every thread holds the result
    const float nrm = sqrtf(s);
    if (threadIdx.x == 0) norms[e] = nrm;
    total = total + nrm;
  }
  if (threadIdx.x == 0) out[0] = p * total;
}

__global__ __launch_bounds__(256) void param_dist_bwd_kernel(const gsk_dist_entry* __restrict__ tab, int n_entries, float p,
                                                             const float* __restrict__ gout, const float* __restrict__ norms,
                                                             float* __restrict__ gbase) {
#pragma clang fp contract(off)
  const int k = chunk_owner(tab, n_entries, blockIdx.x, &gsk_dist_entry::bblk0);
  const gsk_dist_entry e = tab[k];
  if (e.goff < 0) return;      // (not reached for a table gsk_param_dist_layout made)
  const float* __restrict__ a = e.p;
  const float* __restrict__ b = e.q;
  float* __restrict__ g = gbase + e.goff;
  const long i0 = (long)(blockIdx.x - e.bblk0) * e.chunk, i1 = min(e.n, i0 + e.chunk);
  if (i0 >= i1) return;
  const float nrm = norms[k];
  const bool zero = nrm == 0.f;
  const float coef = zero ? 0.f : (gout[0] * p) / nrm;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(g);
  chunk_walk(i0, i1, (bits & 15) == 0, [&](long i) {
    const float4 x = *reinterpret_cast<const float4*>(a + i);
    const float4 y = *reinterpret_cast<const float4*>(b + i);
    float4 o;
    o.x = zero ? 0.f : (x.x - y.x) * coef;
    o.y = zero ? 0.f : (x.y - y.y) * coef;
    o.z = zero ? 0.f : (x.z - y.z) * coef;
    o.w = zero ? 0.f : (x.w - y.w) * coef;
    *reinterpret_cast<float4*>(g + i) = o;
  }, [&](long i) { g[i] = zero ? 0.f : (a[i] - b[i]) * coef; });
}

extern "C" int gsk_param_dist_fwd(const gsk_dist_entry* table_dev, int n_entries, long total_blocks, float p, float* out, float* norms, float* ws,
                                  gsl_stream_t s) {
  GSL_CHECK_ARG(table_dev && out && norms, "null table, out or norms");
  GSL_CHECK_ARG(ws, "null ws");
  GSL_CHECK_ARG(n_entries >= 1 && total_blocks >= n_entries && total_blocks < (1L << 31), "n_entries >= 1, n_entries <= total_blocks < 2^31");
  hipLaunchKernelGGL(param_dist_partial_kernel, dim3((unsigned)total_blocks), dim3(256), 0, as_stream(s), table_dev, n_entries, ws);
  GSL_TRY(check_launch("gsk_param_dist_fwd(partial)"));
  hipLaunchKernelGGL(param_dist_reduce_kernel, dim3(1), dim3(256), 0, as_stream(s), table_dev, n_entries, ws, p, norms, out);
  return check_launch("gsk_param_dist_fwd(reduce)");
}

extern "C" int gsk_param_dist_bwd(const gsk_dist_entry* table_dev, int n_entries, long bwd_blocks, float p, const float* gout, const float* norms,
                                  float* g, gsl_stream_t s) {
  GSL_CHECK_ARG(table_dev && gout && norms && g, "null table, gout, norms or g");
  GSL_CHECK_ARG(aligned4(g), "g is 4-byte aligned");
  GSL_CHECK_ARG(n_entries >= 1 && bwd_blocks >= 1 && bwd_blocks < (1L << 31), "n_entries >= 1, 1 <= bwd_blocks < 2^31");
  hipLaunchKernelGGL(param_dist_bwd_kernel, dim3((unsigned)bwd_blocks), dim3(256), 0, as_stream(s), table_dev, n_entries, p, gout, norms, g);
  return check_launch(__func__);
}
