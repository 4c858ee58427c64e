// classstat.hip — per-class evaluation on the device (test/test_own.py:99-144 per-class accuracy, util/utils.py:527-547 class prototypes):
//   S1  class statistics of one batch of logits: count[label] += 1, hit[label] += (first arg-max == label), confusion[label][arg-max] += 1
//   S2  class embedding sums of one batch: sum[c, :] += emb[i, :] for the rows with label[i] == c, in increasing i, and count[c] += 1
//   S3  finish: acc[c] = 100 hit / count (f64, the reference's Python floats), proto[c, :] = sum[c, :] / count[c] (f32 true division)
// The buffers belong to the caller and persist across batches. S1's counters are integers, so their value does not depend on the order of
// the adds; S2 gives every (class, column) ONE owner lane that adds the matching rows one by one with plain f32 adds on top of the value
// already in `sum` — across batches that is the reference's sequential `embeds_sum[label] += embed`, bit for bit. No kernel allocates,
// synchronises or uses a floating-point atomic.
#include "gsl_common.h"

using namespace gsl;

// ------------------------------------------------------------------ S1 class statistics
// torch.max(outputs, 1): the FIRST index of the maximum, a NaN ranking above every number (the first NaN wins). +0 and -0 are equal.
__device__ __forceinline__ bool argmax_before(float a, int ia, float b, int ib) {
  const bool na = a != a, nb = b != b;
  if (na || nb) return na && (!nb || ia < ib);
  return a == b ? ia < ib : a > b;
}

// One wave64 per row, 4 rows per workgroup; ld = row stride of the logits in elements. A label outside [0, C) counts in bad[0] alone.
__global__ void __launch_bounds__(256) class_stats_kernel(const float* __restrict__ logits, long ld, const int64_t* __restrict__ labels, int B,
                                                          int C, unsigned long long* __restrict__ count, unsigned long long* __restrict__ hit,
                                                          unsigned long long* __restrict__ bad, int* __restrict__ confusion) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B) return;      // (wave-uniform; no barrier below)
  const float* row = logits + (size_t)r * ld;
  float m = -INFINITY;
  int mi = 0x7fffffff;      // a lane without a column never wins: every real column has a lower index
  for (int c = lane; c < C; c += 64) {
    const float v = row[c];
    if (argmax_before(v, c, m, mi)) { m = v; mi = c; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oi = __shfl_xor(mi, o, 64);
    if (argmax_before(om, oi, m, mi)) { m = om; mi = oi; }
  }
  if (lane != 0) return;
  const long yl = (long)labels[r];
  if (yl < 0 || yl >= C) {
    atomicAdd(bad, 1ull);
    return;
  }
  atomicAdd(count + yl, 1ull);
  if (mi == (int)yl) atomicAdd(hit + yl, 1ull);
  if (confusion) atomicAdd(confusion + (size_t)yl * C + mi, 1);
}

extern "C" int gsl_class_stats(const float* logits, long ld, const int64_t* labels, int B, int C, int64_t* count, int64_t* hit, int64_t* bad,
                               int* confusion, gsl_stream_t s) {
  GSL_CHECK_ARG(logits && labels && count && hit && bad, "null pointer");
  GSL_CHECK_ARG(B > 0 && C > 0 && ld >= C, "B > 0, C > 0, ld >= C");
  hipLaunchKernelGGL(class_stats_kernel, dim3((B + 3) / 4), dim3(256), 0, as_stream(s), logits, ld, labels, B, C,
                     reinterpret_cast<unsigned long long*>(count), reinterpret_cast<unsigned long long*>(hit),
                     reinterpret_cast<unsigned long long*>(bad), confusion);
  return check_launch("gsl_class_stats");
}

// ------------------------------------------------------------------ S2 class embedding sums
constexpr int CSUM_CHUNK = 1024;      // labels of the batch staged in LDS at a time (as int, -1 = out of range) + the rows that match

// Workgroup (c, x): class c, columns x*256 .. x*256 + 255. Per chunk of the batch: the labels go to LDS, wave 0 compacts the indices of
// the rows of class c IN ORDER (ballot + prefix count), then every lane adds those rows to its own column. Workgroup (c, 0) owns count[c];
// workgroup (0, 0) also counts the labels outside [0, C) into bad[0]. One owner per address: plain loads and stores, no atomics.
__global__ void __launch_bounds__(256) class_embed_sum_kernel(const float* __restrict__ emb, long ld, const int64_t* __restrict__ labels, int B,
                                                              int D, int C, float* __restrict__ sum, long long* __restrict__ count,
                                                              long long* __restrict__ bad) {
  __shared__ int lab[CSUM_CHUNK];
  __shared__ int rows[CSUM_CHUNK];
  __shared__ int n_rows, n_bad;
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int d = blockIdx.y * 256 + tid;
  float acc = d < D ? sum[(size_t)c * D + d] : 0.f;
  long long n_c = 0, n_b = 0;
  for (int c0 = 0; c0 < B; c0 += CSUM_CHUNK) {
    const int n = min(CSUM_CHUNK, B - c0);
    __syncthreads();      // (the previous chunk is consumed)
    for (int i = tid; i < n; i += 256) {
      const long yl = (long)labels[c0 + i];
      lab[i] = (yl >= 0 && yl < C) ? (int)yl : -1;
    }
    __syncthreads();
    if (tid < 64) {
      int cnt = 0, nb = 0;
      for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const int y = i < n ? lab[i] : -2;
        const unsigned long long match = __ballot(y == c), out = __ballot(y == -1);
        if (y == c) rows[cnt + __popcll(match & ((1ull << lane) - 1ull))] = c0 + i;
        cnt += __popcll(match);
        nb += __popcll(out);
      }
      if (lane == 0) { n_rows = cnt; n_bad = nb; }
    }
    __syncthreads();
    const int nr = n_rows;
    n_c += nr;
    n_b += n_bad;
    if (d < D) {
#pragma unroll 4
      for (int j = 0; j < nr; ++j) acc += emb[(size_t)rows[j] * ld + d];      // one row at a time, in row order: the reference's +=
    }
  }
  if (d < D) sum[(size_t)c * D + d] = acc;
  if (blockIdx.y == 0 && tid == 0) {
    if (n_c) count[c] += n_c;
    if (c == 0 && n_b) bad[0] += n_b;
  }
}

extern "C" int gsl_class_embed_sum(const float* emb, long ld, const int64_t* labels, int B, int D, int C, float* sum, int64_t* count,
                                   int64_t* bad, gsl_stream_t s) {
  GSL_CHECK_ARG(emb && labels && sum && count && bad, "null pointer");
  GSL_CHECK_ARG(B > 0 && C > 0 && D > 0 && D <= (1 << 20) && ld >= D, "B > 0, C > 0, 0 < D <= 2^20, ld >= D");
  hipLaunchKernelGGL(class_embed_sum_kernel, dim3(C, (D + 255) / 256), dim3(256), 0, as_stream(s), emb, ld, labels, B, D, C, sum,
                     reinterpret_cast<long long*>(count), reinterpret_cast<long long*>(bad));
  return check_launch("gsl_class_embed_sum");
}

// ------------------------------------------------------------------ S3 finish
// Workgroup c: acc[c] = (double)(100 hit[c]) / (double)count[c] — the IEEE f64 division Python makes of `100 * class_correct / class_total`
// (test_own.py:134, :142) — and proto[c, :] = sum[c, :] / (float)count[c] (util/utils.py:547). A class without a sample gets NaN in both.
__global__ void __launch_bounds__(256) class_finish_kernel(const long long* __restrict__ count, const long long* __restrict__ hit,
                                                           const float* __restrict__ sum, int D, double* __restrict__ acc,
                                                           float* __restrict__ proto) {
  const int c = blockIdx.x;
  const long long n = count[c];
  if (acc && threadIdx.x == 0) acc[c] = n ? (double)(100 * hit[c]) / (double)n : __longlong_as_double(0x7ff8000000000000ll);
  if (proto) {
    const float fn = (float)n;
    for (int d = threadIdx.x; d < D; d += 256) proto[(size_t)c * D + d] = n ? sum[(size_t)c * D + d] / fn : __int_as_float(0x7fc00000);
  }
}

extern "C" int gsl_class_finish(const int64_t* count, const int64_t* hit, const float* sum, int C, int D, double* acc, float* proto,
                                gsl_stream_t s) {
  GSL_CHECK_ARG(count && (acc || proto) && (!acc || hit) && (!proto || (sum && D > 0)), "null pointer (acc needs hit; proto needs sum and D > 0)");
  GSL_CHECK_ARG(C > 0, "C > 0");
  hipLaunchKernelGGL(class_finish_kernel, dim3(C), dim3(256), 0, as_stream(s), reinterpret_cast<const long long*>(count),
                     reinterpret_cast<const long long*>(hit), sum, D, acc, proto);
  return check_launch("gsl_class_finish");
}
