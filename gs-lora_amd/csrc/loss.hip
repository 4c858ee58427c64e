// loss.hip — the losses of the step, from the head's logits / embeddings to the scalar total and back:
//   K11 mean cross-entropy + top-1 (engine_cl.py:65-78, util/utils.py:354-368) fwd / bwd; K11b precision@k
//   K13 prototype KL (engine_cl.py:571-603) fwd / bwd; K13b prototype l2 (engine_cl.py:593-594, engine.py:712-713) fwd / bwd
//   the scalar tail (hinges, total, meters, coefficients: engine_cl.py:65-125) and the whole section as one launch (gsl_loss_tail)
// All are tiny next to the GEMMs; they exist so that a step needs no host sync and no [B,C]-sized PyTorch elementwise chain.
// Upstream gradient scalars arrive as DEVICE pointers (coef).
// Every formula is written ONCE: the row functions are templated on where the row lives (global memory for the stand-alone kernels,
// registers for the one-launch tail), the scalar tail is one function that three kernels call — the forms agree bit for bit by construction.
#include "gsl_common.h"

using namespace gsl;

#define GSL_NAN __int_as_float(0x7fc00000)
// GSL_CHECK_ARG for a launcher that several entry points share: the error text names the entry point
#define GSL_CHECK_ARG_OF(who, cond, msg)                                                                       \
  do {                                                                                                         \
    if (!(cond)) return fail(GSL_ERR_ARG, "%s: argument check failed: " msg " (%ld,%ld)", who, 0, 0);         \
  } while (0)

// ------------------------------------------------------------------ rows
// A wave owns a row; lane l visits elements l, l + 64, ... in that order, whichever form holds them. get(i, c): element c = lane + 64 i.
constexpr int LT_MAX = 256, LT_V = 16;      // the one-launch tail: rows per launch; values per lane of a row held in registers (n <= 64 * LT_V)
struct GlobalRow {      // any n; every pass reads memory
  static constexpr bool IN_REGS = false;
  const float* p;
  __device__ __forceinline__ GlobalRow(const float* row, int, int) : p(row) {}
  __device__ __forceinline__ float get(int, int c) const { return p[c]; }
};
struct RegRow {      // n <= 64 * LT_V, loaded once: the tail's workgroup is alone on its CU, each global pass would be an exposed L2 round trip
  static constexpr bool IN_REGS = true;
  const float* p;
  float v[LT_V];
  __device__ __forceinline__ RegRow(const float* row, int n, int lane) : p(row) {
#pragma unroll
    for (int i = 0; i < LT_V; ++i) { const int c = lane + 64 * i; v[i] = c < n ? row[c] : 0.f; }
  }
  __device__ __forceinline__ float get(int i, int) const { return v[i]; }
};
template <typename Row, typename F>
__device__ __forceinline__ void row_each(int n, int lane, F&& f) {      // f(i, c) for this lane's elements
  if constexpr (Row::IN_REGS) {
#pragma unroll
    for (int i = 0; i < LT_V; ++i) { const int c = lane + 64 * i; if (c < n) f(i, c); }
  } else {
    for (int i = 0, c = lane; c < n; ++i, c += 64) f(i, c);
  }
}

// log-sum-exp of a row and the index of its maximum (the first one among equals)
template <typename Row>
__device__ __forceinline__ void row_softmax_stats(const Row& x, int n, int lane, float& lse, int& amax) {
  float m = -3.0e38f; int mi = 0x7fffffff;
  row_each<Row>(n, lane, [&](int i, int c) { const float v = x.get(i, c); if (v > m) { m = v; mi = c; } });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64); const int oi = __shfl_xor(mi, o, 64);
    if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
  }
  float se = 0.f;
  row_each<Row>(n, lane, [&](int i, int c) { se += expf(x.get(i, c) - m); });
  lse = m + logf(wave_sum(se));
  amax = mi;
}
template <typename Row>
__device__ __forceinline__ float row_lse(const Row& x, int n, int lane) {
  float m = -3.0e38f;
  row_each<Row>(n, lane, [&](int i, int c) { m = fmaxf(m, x.get(i, c)); });
  m = wave_max(m);
  float se = 0.f;
  row_each<Row>(n, lane, [&](int i, int c) { se += expf(x.get(i, c) - m); });
  return m + logf(wave_sum(se));
}

// A label outside [0, n) (the reference's CrossEntropyLoss raises; its prototype look-up raises KeyError, engine_cl.py:587-589): NaN loss and
// NaN gradient row, no out-of-bounds read; the deferred meter read stops the run. A class missing INSIDE the prototype table holds NaN rows
// (losses.prototype_table), with the same effect.
__device__ __forceinline__ bool label_ok(long y, int n) { return y >= 0 && y < n; }
__device__ __forceinline__ void nan_row(float* row, int n, int lane) {
  for (int c = lane; c < n; c += 64) row[c] = GSL_NAN;
}
// accumulate: fl(old + g) with g the value accumulate = 0 stores. Contraction is off here: fused into the product that forms g, the add
// rounded once where the unrolled loop paired two elements and twice on the odd one behind them
__device__ __forceinline__ void grad_store(float* o, float g, int accumulate) {
#pragma clang fp contract(off)
  *o = accumulate ? (*o + g) : g;
}

// ---- cross entropy of one row: loss, top-1 hit, and the log-sum-exp its gradient needs
template <typename Row>
__device__ __forceinline__ void ce_row(const Row& x, int C, long yl, int lane, float& loss, float& hit, float& lse) {
  int am;
  row_softmax_stats(x, C, lane, lse, am);
  const bool ok = label_ok(yl, C);
  loss = ok ? lse - x.p[ok ? yl : 0] : GSL_NAN;
  hit = (ok && am == (int)yl) ? 1.f : 0.f;
}
// dlogits[c] = k (softmax - onehot)
template <typename Row>
__device__ __forceinline__ void ce_row_bwd(const Row& x, int C, long yl, float lse, float k, float* d, int accumulate, int lane) {
  if (!label_ok(yl, C)) { nan_row(d, C, lane); return; }
  const int y = (int)yl;
  row_each<Row>(C, lane, [&](int i, int c) { grad_store(d + c, k * (expf(x.get(i, c) - lse) - (c == y ? 1.f : 0.f)), accumulate); });
}

// ---- prototype distance of one row a against its prototype t. KL: sum_d softmax(t) (log softmax(t) - log softmax(a)), with the two
// log-sum-exps as its statistics. l2 (the SUM form of torch.mean((output - prototype_tensor) ** 2)): (1/D) sum_d (a - t)^2, no statistics;
// divided by the row count the batch sum is the reference's mean.
struct ProtoStats { float la, lt; };
__device__ __forceinline__ float l2_grad_scale(int D) { return 2.0f / (float)D; }
template <bool L2, typename Row>
__device__ __forceinline__ ProtoStats proto_stats(const Row& a, const Row& t, int D, int lane) {
  if constexpr (L2) return ProtoStats{0.f, 0.f};
  else return ProtoStats{row_lse(a, D, lane), row_lse(t, D, lane)};
}
template <bool L2, typename Row>
__device__ __forceinline__ float proto_row(const Row& a, const Row& t, int D, int lane, ProtoStats st) {
  float acc = 0.f;
  if constexpr (L2) {
    row_each<Row>(D, lane, [&](int i, int d) { const float df = a.get(i, d) - t.get(i, d); acc = fmaf(df, df, acc); });
    return wave_sum(acc) / (float)D;
  } else {
    row_each<Row>(D, lane, [&](int i, int d) { const float ltd = t.get(i, d) - st.lt; acc += expf(ltd) * (ltd - (a.get(i, d) - st.la)); });
    return wave_sum(acc);
  }
}
template <bool L2, typename Row>
__device__ __forceinline__ void proto_row_bwd(const Row& a, const Row& t, int D, ProtoStats st, float k, float* o, int accumulate, int lane) {
  const float s2 = l2_grad_scale(D);
  row_each<Row>(D, lane, [&](int i, int d) {
    const float av = a.get(i, d), tv = t.get(i, d);
    grad_store(o + d, L2 ? k * (s2 * (av - tv)) : k * (expf(av - st.la) - expf(tv - st.lt)), accumulate);
  });
}

// ------------------------------------------------------------------ K11 / K13 / K13b as stand-alone kernels
// wave-per-row; the batch sum is one block's fixed-order (deterministic) reduction of the per-row values.
__global__ __launch_bounds__(256) void ce_rows_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                      float* __restrict__ rows, int B, int C) {
  fp16_sat_on();
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B) return;
  float loss, hit, lse;
  ce_row(GlobalRow(logits + (size_t)r * C, C, lane), C, (long)labels[r], lane, loss, hit, lse);
  if (lane == 0) { rows[2 * r] = loss; rows[2 * r + 1] = hit; }
}
__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                     const float* __restrict__ coef, float scale, float* dlogits, int B, int C,
                                                     int accumulate) {
  fp16_sat_on();
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B) return;
  const GlobalRow x(logits + (size_t)r * C, C, lane);
  float lse; int am;
  row_softmax_stats(x, C, lane, lse, am);
  ce_row_bwd(x, C, (long)labels[r], lse, coef[0] * scale, dlogits + (size_t)r * C, accumulate, lane);
}
template <bool L2>
__global__ __launch_bounds__(256) void proto_rows_kernel(const float* __restrict__ emb, const int64_t* __restrict__ labels,
                                                         const float* __restrict__ proto, float* __restrict__ rows, int B, int D, int C) {
  fp16_sat_on();
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B) return;
  const long y = (long)labels[r];
  if (!label_ok(y, C)) { if (lane == 0) rows[r] = GSL_NAN; return; }
  const GlobalRow a(emb + (size_t)r * D, D, lane), t(proto + (size_t)y * D, D, lane);
  const float v = proto_row<L2>(a, t, D, lane, proto_stats<L2>(a, t, D, lane));
  if (lane == 0) rows[r] = v;
}
template <bool L2>
__global__ __launch_bounds__(256) void proto_bwd_kernel(const float* __restrict__ emb, const int64_t* __restrict__ labels,
                                                        const float* __restrict__ proto, const float* __restrict__ coef, float scale,
                                                        float* demb, int B, int D, int C, int accumulate) {
  fp16_sat_on();
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B) return;
  const long y = (long)labels[r];
  if (!label_ok(y, C)) { nan_row(demb + (size_t)r * D, D, lane); return; }
  const GlobalRow a(emb + (size_t)r * D, D, lane), t(proto + (size_t)y * D, D, lane);
  proto_row_bwd<L2>(a, t, D, proto_stats<L2>(a, t, D, lane), coef[0] * scale, demb + (size_t)r * D, accumulate, lane);
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
extern "C" int gsl_ce_bwd(const float* logits, const int64_t* labels, const float* coef, float scale, float* dlogits, int B,
                          int C, int accumulate, gsl_stream_t s) {
  GSL_CHECK_ARG(logits && labels && coef && dlogits && B > 0 && C > 0, "null/size");
  hipLaunchKernelGGL(ce_bwd_kernel, dim3((B + 3) / 4), dim3(256), 0, as_stream(s), logits, labels, coef, scale, dlogits, B, C, accumulate);
  return check_launch("gsl_ce_bwd");
}

static int proto_fwd(const char* who, bool l2, const float* emb, const int64_t* labels, const float* proto, float* out1, float* row_ws, int B,
                     int D, int C, gsl_stream_t s) {
  GSL_CHECK_ARG_OF(who, emb && labels && proto && out1 && row_ws && B > 0 && D > 0 && C > 0, "null/size");
  hipLaunchKernelGGL(l2 ? proto_rows_kernel<true> : proto_rows_kernel<false>, dim3((B + 3) / 4), dim3(256), 0, as_stream(s), emb, labels, proto,
                     row_ws, B, D, C);
  hipLaunchKernelGGL(sum_rows_kernel, dim3(1), dim3(256), 0, as_stream(s), row_ws, out1, B, 1);
  return check_launch(who);
}
static int proto_bwd(const char* who, bool l2, const float* emb, const int64_t* labels, const float* proto, const float* coef, float scale,
                     float* demb, int B, int D, int C, int accumulate, gsl_stream_t s) {
  GSL_CHECK_ARG_OF(who, emb && labels && proto && coef && demb && B > 0 && D > 0 && C > 0, "null/size");
  hipLaunchKernelGGL(l2 ? proto_bwd_kernel<true> : proto_bwd_kernel<false>, dim3((B + 3) / 4), dim3(256), 0, as_stream(s), emb, labels, proto,
                     coef, scale, demb, B, D, C, accumulate);
  return check_launch(who);
}
extern "C" int gsl_proto_kl_fwd(const float* emb, const int64_t* labels, const float* proto, float* out1, float* row_ws, int B,
                                int D, int C, gsl_stream_t s) {
  return proto_fwd(__func__, false, emb, labels, proto, out1, row_ws, B, D, C, s);
}
extern "C" int gsl_proto_l2_fwd(const float* emb, const int64_t* labels, const float* proto, float* out1, float* row_ws, int B,
                                int D, int C, gsl_stream_t s) {
  return proto_fwd(__func__, true, emb, labels, proto, out1, row_ws, B, D, C, s);
}
extern "C" int gsl_proto_kl_bwd(const float* emb, const int64_t* labels, const float* proto, const float* coef, float scale,
                                float* demb, int B, int D, int C, int accumulate, gsl_stream_t s) {
  return proto_bwd(__func__, false, emb, labels, proto, coef, scale, demb, B, D, C, accumulate, s);
}
extern "C" int gsl_proto_l2_bwd(const float* emb, const int64_t* labels, const float* proto, const float* coef, float scale,
                                float* demb, int B, int D, int C, int accumulate, gsl_stream_t s) {
  return proto_bwd(__func__, true, emb, labels, proto, coef, scale, demb, B, D, C, accumulate, s);
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
    if (label_ok(yl, C)) {      // an out-of-range label is never a hit (no out-of-bounds read)
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
// + w_r*KL_r from the batch SUMS of the kernels above, the 8 meter values, and the 5 partial derivatives the backward hands to those
// kernels as upstream gradients. One thread: it replaces ~35 one-element torch kernels per step (3.5 % of the step at the reference's
// batch 48, where every launch counts). The f32 operations of the torch expression in its order, each rounded on its own: contraction is
// off in this function, so its three callers — gsl_loss_combine, gsl_loss_combine_pack, gsl_loss_tail[_l2] — give the same bits.
// has_proto false: the prototype term is absent (kl_f / kl_r are not used).
// =====================================================================================
struct LossHyper { float beta, BND, alpha, w_f, w_r, BND_pro; };
// torch's relu: a NaN stays a NaN (fmaxf(NaN, 0) is 0 — a NaN forget sum, from a label out of range or a class without a prototype, or
// n_f = 0 in the pack, would leave a finite total and finite meters, and the deferred meter read would not stop the run)
__device__ __forceinline__ float relu_nan(float v) { return v > 0.f ? v : (v != v ? v : 0.f); }
__device__ __forceinline__ void loss_scalar_tail(float ce_r, float ce_f, float kl_f, float kl_r, float hit_r, float hit_f, float n_r, float n_f,
                                                 const float* structure, bool has_proto, LossHyper h, float* total, float* meters,
                                                 float* coefs) {
#pragma clang fp contract(off)
  const float loss_remain = ce_r / n_r;
  const float hinge_f = h.BND - ce_f / n_f;
  const float loss_forget = relu_nan(hinge_f);
  const float st = structure ? structure[0] : 0.f;
  float pro_f = 0.f, pro_r = 0.f, hinge_p = 0.f;
  if (has_proto) { hinge_p = h.BND_pro - kl_f / n_f; pro_f = h.w_f * relu_nan(hinge_p); pro_r = h.w_r * (kl_r / n_r); }
  const float tot = loss_forget * h.beta + loss_remain + st * h.alpha + (pro_f + pro_r);
  total[0] = tot;
  meters[0] = h.beta * loss_forget; meters[1] = loss_remain; meters[2] = tot; meters[3] = h.alpha * st;
  meters[4] = hit_f * (100.0f / n_f); meters[5] = hit_r * (100.0f / n_r); meters[7] = pro_r;
  // without the prototype term the reference still LOGS w_f * relu(BND_pro - 0) in losses_prototype_forget (engine_cl.py:103-110,
  // engine.py:118-125: prototype_loss_forget is the constant 0 there); the total does not contain it
  meters[6] = has_proto ? pro_f : h.w_f * relu_nan(h.BND_pro);
  coefs[0] = 1.0f / n_r;                                          // d total / d ce_r_sum
  coefs[1] = hinge_f > 0.f ? -h.beta / n_f : 0.f;                 // d total / d ce_f_sum   (relu'(0) = 0 as in torch)
  coefs[2] = (has_proto && hinge_p > 0.f) ? -h.w_f / n_f : 0.f;   // d total / d kl_f_sum
  coefs[3] = has_proto ? h.w_r / n_r : 0.f;                       // d total / d kl_r_sum
  coefs[4] = h.alpha;                                             // d total / d structure
}

__global__ void loss_combine_kernel(const float* ce_r_sum, const float* ce_f_sum, const float* kl_f_sum, const float* kl_r_sum,
                                    const float* structure, const float* hit_r, const float* hit_f, float n_r, float n_f, LossHyper h,
                                    float* total, float* meters, float* coefs) {
  fp16_sat_on();
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const bool has_proto = kl_f_sum != nullptr;
  loss_scalar_tail(ce_r_sum[0], ce_f_sum[0], has_proto ? kl_f_sum[0] : 0.f, has_proto ? kl_r_sum[0] : 0.f, hit_r[0], hit_f[0], n_r, n_f,
                   structure, has_proto, h, total, meters, coefs);
}
// Data-parallel form: the eight batch sums arrive as ONE all-reduced device array (gslora_hip/step.py packs and sum-all-reduces them
// before the hinges so that relu(BND - mean CE_f) / relu(BND_pro - mean KL_f) see the GLOBAL batch means, the reference's single-GPU /
// nn.DataParallel semantics, train_own_forget_cl.py:494-497): pack8 = [ce_r, ce_f, hit_r, hit_f, n_r, n_f, kl_f, kl_r]. The batch sizes
// are read from the pack, so no host value depends on the other ranks.
__global__ void loss_combine_pack_kernel(const float* pack, const float* structure, int has_proto, LossHyper h, float* total, float* meters,
                                         float* coefs) {
  fp16_sat_on();
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  loss_scalar_tail(pack[0], pack[1], pack[6], pack[7], pack[2], pack[3], pack[4], pack[5], structure, has_proto != 0, h, total, meters, coefs);
}
extern "C" int gsl_loss_combine_pack(const float* pack8, const float* structure, int has_proto, float beta, float BND, float alpha,
                                     float w_f, float w_r, float BND_pro, float* total, float* meters8, float* coefs5, gsl_stream_t s) {
  GSL_CHECK_ARG(pack8 && total && meters8 && coefs5, "null");
  hipLaunchKernelGGL(loss_combine_pack_kernel, dim3(1), dim3(64), 0, as_stream(s), pack8, structure, has_proto,
                     LossHyper{beta, BND, alpha, w_f, w_r, BND_pro}, total, meters8, coefs5);
  return check_launch("gsl_loss_combine_pack");
}
extern "C" int gsl_loss_combine(const float* ce_r_sum, const float* ce_f_sum, const float* kl_f_sum, const float* kl_r_sum,
                                const float* structure, const float* hit_r, const float* hit_f, float n_r, float n_f, float beta,
                                float BND, float alpha, float w_f, float w_r, float BND_pro, float* total, float* meters8,
                                float* coefs5, gsl_stream_t s) {
  GSL_CHECK_ARG(ce_r_sum && ce_f_sum && hit_r && hit_f && total && meters8 && coefs5 && n_r > 0.f && n_f > 0.f, "null/size");
  GSL_CHECK_ARG(!kl_f_sum == !kl_r_sum, "prototype term: kl_f_sum and kl_r_sum together");
  hipLaunchKernelGGL(loss_combine_kernel, dim3(1), dim3(64), 0, as_stream(s), ce_r_sum, ce_f_sum, kl_f_sum, kl_r_sum, structure, hit_r,
                     hit_f, n_r, n_f, LossHyper{beta, BND, alpha, w_f, w_r, BND_pro}, total, meters8, coefs5);
  return check_launch("gsl_loss_combine");
}

// =====================================================================================
// The whole loss section of a single-process step in ONE launch (the launch-bound regime: few-shot batches replay ~20 one-block kernels
// here — CE rows + sums for the remain and forget rows, prototype rows + sums, the scalar tail, and the four backward kernels that
// turn its five coefficients into dlogits / demb). One workgroup of 16 waves: a wave owns every 16th row and holds it in registers
// (RegRow); row statistics stay in LDS between the forward and the backward half. The row functions and the scalar tail of the kernels
// above, the same fixed summation orders (sum_rows_kernel's 256-lane partition included): every output bit-identical to the
// multi-launch path. rows [0, nr) are the remain batch, [nr, N) the forget batch (engine_cl.py:59-125); N <= LT_MAX.
// L2: the prototype term is the l2 distance instead of the KL (gsl_loss_tail_l2).
// =====================================================================================
template <bool L2>
__global__ __launch_bounds__(1024) void loss_tail_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, int N, int nr,
                                                         int C, const float* __restrict__ emb, const float* __restrict__ proto, int D,
                                                         int Cp, const float* structure, LossHyper h, float* out14,
                                                         float* __restrict__ dlogits, float* __restrict__ demb) {
  fp16_sat_on();
  __shared__ float ce_s[LT_MAX], hit_s[LT_MAX], kl_s[LT_MAX], lse_s[LT_MAX], la_s[LT_MAX], lt_s[LT_MAX];
  __shared__ float sm[16], coef_s[5];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nf = N - nr;
  for (int r = wave; r < N; r += 16) {
    const long yl = (long)labels[r];
    float loss, hit, lse;
    ce_row(RegRow(logits + (size_t)r * C, C, lane), C, yl, lane, loss, hit, lse);
    if (lane == 0) { ce_s[r] = loss; hit_s[r] = hit; lse_s[r] = lse; }
    if (emb) {
      if (!label_ok(yl, Cp)) { if (lane == 0) kl_s[r] = GSL_NAN; continue; }
      const RegRow a(emb + (size_t)r * D, D, lane), t(proto + (size_t)yl * D, D, lane);
      const ProtoStats st = proto_stats<L2>(a, t, D, lane);
      const float v = proto_row<L2>(a, t, D, lane, st);
      if (lane == 0) { kl_s[r] = v; la_s[r] = st.la; lt_s[r] = st.lt; }
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
  if (threadIdx.x == 0) {
    float c5[5];
    loss_scalar_tail(ce_r, ce_f, kl_f, kl_r, hit_r, hit_f, (float)nr, (float)nf, structure, emb != nullptr, h, out14, out14 + 1, c5);
#pragma unroll
    for (int j = 0; j < 5; ++j) coef_s[j] = out14[9 + j] = c5[j];
  }
  __syncthreads();
  for (int r = wave; r < N; r += 16) {      // gsl_ce_bwd / gsl_proto_*_bwd with the coefficients above (upstream gradient 1)
    const long yl = (long)labels[r];
    ce_row_bwd(RegRow(logits + (size_t)r * C, C, lane), C, yl, lse_s[r], coef_s[r < nr ? 0 : 1] * 1.0f, dlogits + (size_t)r * C, 0, lane);
    if (emb) {
      if (!label_ok(yl, Cp)) { nan_row(demb + (size_t)r * D, D, lane); continue; }
      const RegRow a(emb + (size_t)r * D, D, lane), t(proto + (size_t)yl * D, D, lane);
      proto_row_bwd<L2>(a, t, D, ProtoStats{la_s[r], lt_s[r]}, coef_s[r < nr ? 3 : 2] * 1.0f, demb + (size_t)r * D, 0, lane);
    }
  }
}
extern "C" int gsl_loss_tail_max_rows(void) { return LT_MAX; }
// l2: the prototype term is required (without one, gsl_loss_tail)
static int loss_tail(const char* who, bool l2, const float* logits, const int64_t* labels, int N, int nr, int C, const float* emb,
                     const float* proto, int D, int Cp, const float* structure, LossHyper h, float* out14, float* dlogits, float* demb,
                     gsl_stream_t s) {
  GSL_CHECK_ARG_OF(who, logits && labels && out14 && dlogits && N > 0 && N <= LT_MAX && nr > 0 && nr < N && C > 0 && C <= 64 * LT_V && D <= 64 * LT_V,
                   "null/size (0 < nr < N <= 256 rows, C and D <= 1024)");
  if (l2) GSL_CHECK_ARG_OF(who, emb && proto && demb && D > 0 && Cp > 0, "prototype term: emb, proto and demb are required");
  else GSL_CHECK_ARG_OF(who, !emb || (proto && demb && D > 0 && Cp > 0), "prototype term: emb, proto and demb together");
  hipLaunchKernelGGL(l2 ? loss_tail_kernel<true> : loss_tail_kernel<false>, dim3(1), dim3(1024), 0, as_stream(s), logits, labels, N, nr, C, emb,
                     proto, D, Cp, structure, h, out14, dlogits, demb);
  return check_launch(who);
}
extern "C" int gsl_loss_tail(const float* logits, const int64_t* labels, int N, int nr, int C, const float* emb, const float* proto, int D,
                             int Cp, const float* structure, float beta, float BND, float alpha, float w_f, float w_r, float BND_pro,
                             float* out14, float* dlogits, float* demb, gsl_stream_t s) {
  return loss_tail(__func__, false, logits, labels, N, nr, C, emb, proto, D, Cp, structure, LossHyper{beta, BND, alpha, w_f, w_r, BND_pro}, out14,
                   dlogits, demb, s);
}
extern "C" int gsl_loss_tail_l2(const float* logits, const int64_t* labels, int N, int nr, int C, const float* emb, const float* proto, int D,
                                int Cp, const float* structure, float beta, float BND, float alpha, float w_f, float w_r, float BND_pro,
                                float* out14, float* dlogits, float* demb, gsl_stream_t s) {
  return loss_tail(__func__, true, logits, labels, N, nr, C, emb, proto, D, Cp, structure, LossHyper{beta, BND, alpha, w_f, w_r, BND_pro}, out14,
                   dlogits, demb, s);
}
