// at.hip — libgslora_at.so: the attention-transfer term of the LIRF baseline (include/gslora_at.h).
//   gsa_at_fwd   at_loss of a student's and a teacher's [B, T, D] mid stream, with the table G that carries its gradient
//   gsa_at_bwd   the gradient added in place to the stream gradient at the boundary between the two half networks
// A sixth product library: its own error string; nothing shared with libgslora_hip.so but the headers (gsl_common.h and the public ones),
// and with the other side libraries gsl_chunks.h: the alignment predicate and the one-workgroup sum of stage 3.
#include "gsl_chunks.h"

#include "../../include/gslora_at.h"

using namespace gsl;

namespace gsl { thread_local char g_err[512] = {0}; }
extern "C" const char* gsa_last_error(void) { return gsl::g_err; }

constexpr int AT_ROWS_PER_SPLIT = 16;      // the plan: a workgroup of stage 1 sums at least this many tokens (but the last of an image)
constexpr int AT_TARGET_GROUPS = 512;      // .. and the token axis is split until about this many workgroups exist
constexpr int AT_MAX_SPLIT = 64;
constexpr float AT_EPS = 1e-12f;           // F.normalize's eps
constexpr float AT_THRESHOLD = 0.005f;

// N consecutive elements as floats: one 16-byte access (N * sizeof(E) == 16) or one 8-byte access (N == 4 of a 16-bit type)
template <typename E, int N> struct Vec;
template <typename E> struct Vec<E, 4> {
  static __device__ __forceinline__ void ld(const E* p, float v[4]) { Elem<E>::ld4(p, v); }
  static __device__ __forceinline__ void st(E* p, const float v[4]) { Elem<E>::st4(p, v); }
};
template <> struct Vec<f16_t, 8> {
  static __device__ __forceinline__ void ld(const f16_t* p, float v[8]) {
    const uint4 t = *reinterpret_cast<const uint4*>(p);
    unpack2h(t.x, v[0], v[1]); unpack2h(t.y, v[2], v[3]); unpack2h(t.z, v[4], v[5]); unpack2h(t.w, v[6], v[7]);
  }
  static __device__ __forceinline__ void st(f16_t* p, const float v[8]) {
    *reinterpret_cast<uint4*>(p) = make_uint4(pack2h(v[0], v[1]), pack2h(v[2], v[3]), pack2h(v[4], v[5]), pack2h(v[6], v[7]));
  }
};
template <> struct Vec<bf16_t, 8> {
  static __device__ __forceinline__ void ld(const bf16_t* p, float v[8]) {
    const uint4 t = *reinterpret_cast<const uint4*>(p);
    unpack2s(t.x, 0, v[0], v[1]); unpack2s(t.y, 0, v[2], v[3]); unpack2s(t.z, 0, v[4], v[5]); unpack2s(t.w, 0, v[6], v[7]);
  }
  static __device__ __forceinline__ void st(bf16_t* p, const float v[8]) {
    *reinterpret_cast<uint4*>(p) = make_uint4(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7]));
  }
};

// ---- stage 1: per (image, channel) the sum of squares over a range of tokens, of the student's and the teacher's stream.
// grid (B, nsplit). A thread owns one 16-byte group of channels (cg) and the tokens r0 + rl, r0 + rl + nrl, .. of its split (rl = tid / ncg,
// nrl = 256 / ncg whole row lanes; the threads behind them idle), summed in ascending order; the row lanes of a channel are then added in
// ascending order through LDS. part: [B, nsplit, 2, D] (student, teacher).
template <typename E>
__global__ __launch_bounds__(256) void at_sumsq_kernel(const E* __restrict__ xs, long ld_s, const E* __restrict__ xt, long ld_t, int T, int D,
                                                       int chunk, float* __restrict__ part) {
  constexpr int V = 16 / (int)sizeof(E);
  __shared__ float sm[2 * 256 * V];
  const int b = blockIdx.x, sp = blockIdx.y, nsplit = gridDim.y;
  const int ncg = D / V, nrl = 256 / ncg;
  const int rl = threadIdx.x / ncg, cg = threadIdx.x - rl * ncg;
  const int r0 = sp * chunk, r1 = min(T, r0 + chunk);
  float as[V], at[V];
#pragma unroll
  for (int j = 0; j < V; ++j) as[j] = at[j] = 0.f;
  if (rl < nrl) {
    const E* ps = xs + ((size_t)b * T) * ld_s + (size_t)cg * V;
    const E* pt = xt + ((size_t)b * T) * ld_t + (size_t)cg * V;
#pragma unroll 2
    for (int t = r0 + rl; t < r1; t += nrl) {
      float vs[V], vt[V];
      Vec<E, V>::ld(ps + (size_t)t * ld_s, vs);
      Vec<E, V>::ld(pt + (size_t)t * ld_t, vt);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        as[j] += vs[j] * vs[j];
        at[j] += vt[j] * vt[j];
      }
    }
    // (neighbouring threads are V floats apart: a V-way bank conflict, once per workgroup behind its whole stream of global loads)
#pragma unroll
    for (int j = 0; j < V; ++j) {
      sm[rl * D + cg * V + j] = as[j];
      sm[256 * V + rl * D + cg * V + j] = at[j];
    }
  }
  __syncthreads();
  float* out = part + ((size_t)b * nsplit + sp) * 2 * D;
  for (int d = threadIdx.x; d < D; d += 256) {
    float s = 0.f, t = 0.f;
    for (int r = 0; r < nrl; ++r) {
      s += sm[r * D + d];
      t += sm[256 * V + r * D + d];
    }
    out[d] = s;
    out[D + d] = t;
  }
}

// ---- stage 2: a workgroup per image. Thread i owns channels i, i + 256, .. (at most four).
__global__ __launch_bounds__(256) void at_image_kernel(const float* __restrict__ part, int nsplit, int B, int T, int D, float* __restrict__ lossp,
                                                       float* __restrict__ G, float* __restrict__ As, float* __restrict__ At) {
#pragma clang fp contract(off)
  __shared__ float sm[16];
  const int b = blockIdx.x;
  float qs[4], qt[4];
  float ss = 0.f, st = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int d = threadIdx.x + 256 * k;
    float s = 0.f, t = 0.f;
    if (d < D) {
      for (int sp = 0; sp < nsplit; ++sp) {      // the splits of the token axis in ascending order
        const float* p = part + ((size_t)b * nsplit + sp) * 2 * D;
        s += p[d];
        t += p[D + d];
      }
    }
    qs[k] = s / (float)T;
    qt[k] = t / (float)T;
    ss += qs[k] * qs[k];
    st += qt[k] * qt[k];
  }
  const float ns = sqrtf(block_sum(ss, sm)), nt = sqrtf(block_sum(st, sm));
  const float den_s = fmaxf(ns, AT_EPS), den_t = fmaxf(nt, AT_EPS);
  const float gscale = 2.f / ((float)B * (float)D);
  float a[4], ga[4];
  float lp = 0.f, dot = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int d = threadIdx.x + 256 * k;
    a[k] = qs[k] / den_s;
    const float y = qt[k] / den_t;
    const bool zs = a[k] < AT_THRESHOLD, zt = y < AT_THRESHOLD;
    const float ms = zs ? 0.f : a[k], mt = zt ? 0.f : y;
    const float diff = ms - mt;
    lp += diff * diff;
    ga[k] = zs ? 0.f : diff * gscale;      // d loss / d at_s before the threshold: zero where the student's entry was zeroed
    dot += ga[k] * a[k];
    if (d < D) {
      if (As) As[(size_t)b * D + d] = ms;
      if (At) At[(size_t)b * D + d] = mt;
    }
  }
  lp = block_sum(lp, sm);
  dot = block_sum(dot, sm);
  if (threadIdx.x == 0) lossp[b] = lp;
  // F.normalize's backward: q / max(n, eps) with n = |q|; below eps the denominator is the constant
  const float k2 = 2.f / (float)T;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int d = threadIdx.x + 256 * k;
    const float dq = ns >= AT_EPS ? (ga[k] - a[k] * dot) / ns : ga[k] / AT_EPS;
    if (d < D) G[(size_t)b * D + d] = dq * k2;
  }
}

// ---- stage 3: the images' partial sums in a fixed order (256 threads stride them), and the mean
__global__ __launch_bounds__(256) void at_value_kernel(const float* __restrict__ lossp, int B, int D, float* __restrict__ loss) {
#pragma clang fp contract(off)
  __shared__ float sm[16];
  const float tot = strided_sum(lossp, B, sm);
  if (threadIdx.x == 0) loss[0] = tot / ((float)B * (float)D);
}

// ---- backward: dmid[b, t, d] = fl(dmid + (coef * S * G[b, d]) * xs[b, t, d]); a thread per group of V channels of one token
template <typename X, typename S, int V>
__global__ __launch_bounds__(256) void at_bwd_kernel(const X* __restrict__ xs, long ld_s, const float* __restrict__ G, const float* __restrict__ coef,
                                                     const float* __restrict__ scale, long ngroups, int T, int D, S* dmid, long ld_d) {
#pragma clang fp contract(off)
  fp16_sat_on();
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= ngroups) return;      // (no workgroup barrier in this kernel)
  const int ncg = D / V;
  const long row = g / ncg;
  const int c = (int)(g - row * ncg) * V;
  const long b = row / T;
  const float k = coef[0] * scale[0];
  float x[V], o[V], gv[V];
  Vec<X, V>::ld(xs + (size_t)row * ld_s + c, x);
  S* dp = dmid + (size_t)row * ld_d + c;
  Vec<S, V>::ld(dp, o);
#pragma unroll
  for (int j = 0; j < V; j += 4) Vec<float, 4>::ld(G + (size_t)b * D + c + j, gv + j);
#pragma unroll
  for (int j = 0; j < V; ++j) o[j] = o[j] + (k * gv[j]) * x[j];
  Vec<S, V>::st(dp, o);
}

static int at_check(const char* who, int B, int T, int D) {
  GSL_CHECK_ARG_AS(who, B >= 1 && T >= 1, "B >= 1, T >= 1");
  GSL_CHECK_ARG_AS(who, T <= GSA_MAX_T, "T <= 1025");
  GSL_CHECK_ARG_AS(who, D >= 64 && D <= GSA_MAX_D && D % 64 == 0, "D a multiple of 64, 64 <= D <= 1024");
  GSL_CHECK_ARG_AS(who, (long)B * T <= GSA_MAX_ROWS, "B * T <= 2^24");
  return GSL_OK;
}

extern "C" int gsa_at_plan(int B, int T, int D, int* nsplit, int* chunk, long* ws_elems) {
  GSL_TRY(at_check(__func__, B, T, D));
  GSL_CHECK_ARG(nsplit && chunk && ws_elems, "null result");
  int ns = (AT_TARGET_GROUPS + B - 1) / B;
  ns = min(ns, T / AT_ROWS_PER_SPLIT);      // (a piece holds at least AT_ROWS_PER_SPLIT tokens)
  ns = max(1, min(ns, AT_MAX_SPLIT));
  const int ch = (T + ns - 1) / ns;
  ns = (T + ch - 1) / ch;      // no empty split
  *nsplit = ns;
  *chunk = ch;
  *ws_elems = (long)B * ns * 2 * D + B;
  return GSL_OK;
}

extern "C" long gsa_at_ws_elems(int B, int T, int D) {
  int ns, ch; long n;
  return gsa_at_plan(B, T, D, &ns, &ch, &n) == GSL_OK ? n : -1;
}

static int at_stream_arg(const char* who, const void* p, long ld, int dtype, int D) {
  GSL_CHECK_ARG_AS(who, dtype == GSL_F32 || dtype == GSL_BF16 || dtype == GSL_F16, "dtype is GSL_F32, GSL_BF16 or GSL_F16");
  GSL_CHECK_ARG_AS(who, ld >= D, "leading dimension >= D");
  GSL_CHECK_ARG_AS(who, aligned16(p) && (ld * (dtype == GSL_F32 ? 4 : 2)) % 16 == 0, "16-byte aligned rows (base pointer and leading dimension)");
  return GSL_OK;
}

extern "C" int gsa_at_fwd(const void* xs, long ld_s, const void* xt, long ld_t, int dtype, int B, int T, int D, float* loss, float* G,
                          float* at_s, float* at_t, float* ws, gsl_stream_t s) {
  GSL_TRY(at_check(__func__, B, T, D));
  GSL_CHECK_ARG(xs && xt, "null xs or xt");
  GSL_CHECK_ARG(loss && G && ws, "null loss, G or ws");
  GSL_TRY(at_stream_arg(__func__, xs, ld_s, dtype, D));
  GSL_TRY(at_stream_arg(__func__, xt, ld_t, dtype, D));
  GSL_CHECK_ARG(aligned16(G), "G 16-byte aligned");
  int nsplit, chunk; long elems;
  GSL_TRY(gsa_at_plan(B, T, D, &nsplit, &chunk, &elems));
  float* lossp = ws + (size_t)B * nsplit * 2 * D;
  dispatch_elem_type(dtype, [&](auto e) {
    using E = typename decltype(e)::type;
    hipLaunchKernelGGL(at_sumsq_kernel<E>, dim3(B, nsplit), dim3(256), 0, as_stream(s), static_cast<const E*>(xs), ld_s,
                       static_cast<const E*>(xt), ld_t, T, D, chunk, ws);
  });
  GSL_TRY(check_launch("gsa_at_fwd(sums)"));
  hipLaunchKernelGGL(at_image_kernel, dim3(B), dim3(256), 0, as_stream(s), ws, nsplit, B, T, D, lossp, G, at_s, at_t);
  GSL_TRY(check_launch("gsa_at_fwd(images)"));
  hipLaunchKernelGGL(at_value_kernel, dim3(1), dim3(256), 0, as_stream(s), lossp, B, D, loss);
  return check_launch("gsa_at_fwd(value)");
}

template <typename X, typename S>
static void at_bwd_launch(const void* xs, long ld_s, const float* G, const float* coef, const float* scale, int B, int T, int D, void* dmid,
                          long ld_d, gsl_stream_t s) {
  constexpr int V = (sizeof(X) == 2 && sizeof(S) == 2) ? 8 : 4;
  const long ngroups = (long)B * T * (D / V);
  hipLaunchKernelGGL((at_bwd_kernel<X, S, V>), dim3((unsigned)((ngroups + 255) / 256)), dim3(256), 0, as_stream(s), static_cast<const X*>(xs), ld_s,
                     G, coef, scale, ngroups, T, D, static_cast<S*>(dmid), ld_d);
}

extern "C" int gsa_at_bwd(const void* xs, long ld_s, int x_dtype, const float* G, const float* coef, const float* scale, int B, int T, int D,
                          void* dmid, long ld_d, int d_dtype, gsl_stream_t s) {
  GSL_TRY(at_check(__func__, B, T, D));
  GSL_CHECK_ARG(xs && G && coef && scale && dmid, "null xs, G, coef, scale or dmid");
  GSL_TRY(at_stream_arg(__func__, xs, ld_s, x_dtype, D));
  GSL_TRY(at_stream_arg(__func__, dmid, ld_d, d_dtype, D));
  GSL_CHECK_ARG(aligned16(G), "G 16-byte aligned");
  dispatch_elem_type(x_dtype, [&](auto x) {
    using X = typename decltype(x)::type;
    dispatch_elem_type(d_dtype, [&](auto d) {
      using S = typename decltype(d)::type;
      at_bwd_launch<X, S>(xs, ld_s, G, coef, scale, B, T, D, dmid, ld_d, s);
    });
  });
  return check_launch(__func__);
}
