// gsl_chunks.h — what the side libraries (train.hip, reg.hip, kd.hip, fd.hip, at.hip) share beyond gsl_common.h: the chunked f64 sum of a
// flat tensor, the one-workgroup sum over a workspace, the owner search of a table kernel and the vector / scalar walk of a chunk.
// Header only; every library keeps its own error string, prefix, export map and public header. No source of libgslora_hip.so includes it.
#pragma once
#include "gsl_common.h"

namespace gsl {

static inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ------------------------------------------------------------------ the partition rule (ABI: restated in gslora_train.h, _reg.h, _kd.h)
// A tensor of n elements is summed in chunk_blocks(n) chunks of chunk_len(n, nblk) elements, one workgroup and one f32 partial each;
// chunk b is [b * len, min(n, (b + 1) * len)).
constexpr int CHUNK_MAX_BLOCKS = 1024;
constexpr long CHUNK_MIN_ELEMS = 1024;
static inline int chunk_blocks(long n) { return (int)min((long)CHUNK_MAX_BLOCKS, (n + CHUNK_MIN_ELEMS - 1) / CHUNK_MIN_ELEMS); }
static inline long chunk_len(long n, int nblk) { return (n + nblk - 1) / nblk; }

// The partial of chunk [i0, i1) by a workgroup of 256: thread t adds term(i) (a double) for i = i0 + t, i0 + t + 256, .. in f64 — the
// difference of two f32 values and its square are exact there — and rounds to f32 once: a tensor of one element comes out correctly
// rounded, and the f32 sums behind it add at most one rounding per level. Every thread holds the result. No fp-contract pragma: the f64
// terms may fuse, as they always have.
template <typename Term>
__device__ __forceinline__ float chunk_partial(long i0, long i1, float* sm, Term&& term) {
  double acc = 0.0;
  for (long i = i0 + threadIdx.x; i < i1; i += 256) acc += term(i);
  return block_sum((float)acc, sm);
}
// omega_i (p_i - p0_i)^2, omega == nullptr: the identity. The term of gst_reg_quad_fwd and gsr_reg_multi_fwd (whose bits must agree) and
// of gsk_param_dist_fwd.
__device__ __forceinline__ double quad_term(const float* __restrict__ p, const float* __restrict__ p0, const float* __restrict__ omega, long i) {
  const double d = (double)p[i] - (double)p0[i];
  return omega ? (double)omega[i] * (d * d) : d * d;
}

// sum_i map(ws[i]) over n floats by ONE workgroup of 256: thread t adds elements t, t + 256, .. in ascending order, block_sum combines in
// a fixed order. Every thread holds the result. Additions only: a caller's fp-contract pragma has nothing to reach here; arithmetic
// inside `map` is the caller's.
template <typename Map>
__device__ __forceinline__ float strided_sum(const float* __restrict__ ws, int n, float* sm, Map&& map) {
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += map(ws[i]);
  return block_sum(s, sm);
}
__device__ __forceinline__ float strided_sum(const float* __restrict__ ws, int n, float* sm) {
  return strided_sum(ws, n, sm, [](float v) { return v; });
}

// The entry (of the first `count`) that owns workgroup b: the last one whose `first` member (blk0, bblk0) is <= b.
template <typename E>
__device__ __forceinline__ int chunk_owner(const E* __restrict__ tab, int count, int b, int E::*first) {
  int lo = 0, hi = count - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].*first <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Chunk [i0, i1) by a workgroup of 256 as a vector body and scalar edges. vec (every pointer the bodies touch is 16-byte aligned): the
// body starts at the first multiple of 4 at or behind i0, thread t takes its groups t, t + 256, .. through body4(i); the elements in
// front of and behind it — all of them without vec — go through body1(i), thread t taking the t-th, (t + 256)-th, .. of them in ascending
// order. Integer arithmetic only: rounding rules are those of the caller's lambdas.
template <typename Body4, typename Body1>
__device__ __forceinline__ void chunk_walk(long i0, long i1, bool vec, Body4&& body4, Body1&& body1) {
  long v0 = i1, nvec = 0;      // the vector body [v0, v0 + 4 nvec)
  if (vec) {
    v0 = min(i1, (i0 + 3) & ~3L);
    nvec = (i1 - v0) / 4;
  }
  for (long v = threadIdx.x; v < nvec; v += 256) body4(v0 + 4 * v);
  const long body_end = v0 + 4 * nvec, head = v0 - i0, nscalar = (i1 - i0) - 4 * nvec;      // [i0, v0) and [body_end, i1)
  for (long j = threadIdx.x; j < nscalar; j += 256) body1(j < head ? i0 + j : body_end + (j - head));
}

}  // namespace gsl
