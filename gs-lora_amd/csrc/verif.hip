// verif.hip — face verification on pairs (util/utils.py:167-230 perform_val, util/verification.py evaluate / calculate_roc / calculate_val):
//   V1  pair distances: s = e0 + e1 (original + flipped image), n = s / ||s|| (sklearn.preprocessing.normalize: a zero row stays zero),
//       dist[p] = sum (n[2p] - n[2p+1])^2, and xnorm = the mean row norm of e0 and e1 (utils.py:205-213)
//   V2  per-fold decision counts: for every un-shuffled KFold test fold and every threshold, #(dist < thr & same) and #(dist < thr & different)
//   V3  per-fold threshold selection (first arg-max of the TRAIN accuracy), test accuracy there, and the fold-averaged tpr / fpr
// Everything between V1's distances and V3's final divisions is integer arithmetic: the counts do not depend on a summation order, the
// train counts of a fold are the totals minus the fold's, and the divisions are IEEE f64 on the same integers the reference divides
// (float(tp + tn) / dist.size) — the outputs are the reference's bit for bit whenever the decisions dist < thr are the same.
// No kernel allocates, synchronises or uses a floating-point atomic; all sums run in a fixed order.
#include "gsl_common.h"

using namespace gsl;

// ------------------------------------------------------------------ V1 pair distances
constexpr int VERIF_MAXD = 1024;                 // a row lives in registers: VERIF_MAXD / 64 values per lane
constexpr int VERIF_NV = VERIF_MAXD / 64;

// One wave64 per pair; 4 pairs per workgroup. Lane l holds columns l, l + 64, ... of the pair's two rows. ld = row stride in elements.
// PLAIN = false (perform_val): rows 2p, 2p + 1 of e0 / e1 [2P, D]; the rows are summed and normalised first.
//   pair_norm [P]: the pair's four row norms (e0 and e1 of rows 2p, 2p + 1), summed in a fixed order, for the xnorm reduction below.
// PLAIN = true (calculate_roc / calculate_val on embeddings that are normalised already): row p of e0 against row p of e1 [P, D].
// Both forms take the squared differences in the same lanes and add them in the same order: the plain form on the normalised
// embeddings the other form wrote gives the same distances bit for bit.
template <bool PLAIN>
__global__ void __launch_bounds__(256) verif_pair_dist_kernel(const float* __restrict__ e0, const float* __restrict__ e1, long ld, int P, int D,
                                                              float* __restrict__ dist, float* __restrict__ pair_norm,
                                                              float* __restrict__ nemb) {
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= P) return;      // (wave-uniform; no barrier below)
  float s[2][VERIF_NV];
  float nrm[2] = {1.f, 1.f}, nsum = 0.f;
  if constexpr (PLAIN) {
#pragma unroll
    for (int v = 0; v < VERIF_NV; ++v) {
      const int d = lane + v * 64;
      s[0][v] = d < D ? e0[(size_t)p * ld + d] : 0.f;
      s[1][v] = d < D ? e1[(size_t)p * ld + d] : 0.f;
    }
  } else {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const size_t row = ((size_t)2 * p + r) * ld;
      float qa = 0.f, qb = 0.f, qs = 0.f;
#pragma unroll
      for (int v = 0; v < VERIF_NV; ++v) {
        const int d = lane + v * 64;
        const float a = d < D ? e0[row + d] : 0.f, b = d < D ? e1[row + d] : 0.f;
        const float t = a + b;
        s[r][v] = t;
        qa += a * a;
        qb += b * b;
        qs += t * t;
      }
      const float na = sqrtf(wave_sum(qa)), nb = sqrtf(wave_sum(qb));
      nsum += na;
      nsum += nb;
      const float ns = sqrtf(wave_sum(qs));
      nrm[r] = ns == 0.f ? 1.f : ns;      // sklearn's _handle_zeros_in_scale: a zero row is divided by 1
    }
  }
  float q = 0.f;
#pragma unroll
  for (int v = 0; v < VERIF_NV; ++v) {
    const int d = lane + v * 64;
    float n0 = s[0][v], n1 = s[1][v];
    if constexpr (!PLAIN) {
      n0 = n0 / nrm[0];
      n1 = n1 / nrm[1];
      if (nemb && d < D) {
        nemb[((size_t)2 * p) * D + d] = n0;
        nemb[((size_t)2 * p + 1) * D + d] = n1;
      }
    }
    const float df = n0 - n1;
    q += df * df;      // (columns >= D hold 0 - 0)
  }
  q = wave_sum(q);
  if (lane == 0) {
    dist[p] = q;
    if constexpr (!PLAIN) pair_norm[p] = nsum;
  }
}

// xnorm[0] = sum(pair_norm) / (4 P): one workgroup, strided f64 partial sums, fixed-order combine
__global__ void __launch_bounds__(256) verif_xnorm_kernel(const float* __restrict__ pair_norm, int P, float* __restrict__ xnorm) {
  __shared__ double part[256];
  double a = 0.0;
  for (int i = threadIdx.x; i < P; i += 256) a += (double)pair_norm[i];
  part[threadIdx.x] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < 256; ++i) t += part[i];
    xnorm[0] = (float)(t / (4.0 * (double)P));
  }
}

extern "C" int gsl_verif_pair_dist(const float* e0, const float* e1, long ld, int P, int D, int mode, float* dist, float* xnorm,
                                   float* pair_norm_ws, float* nemb, gsl_stream_t s) {
  GSL_CHECK_ARG(mode == GSL_VERIF_FLIP_SUM || mode == GSL_VERIF_PLAIN, "mode is GSL_VERIF_FLIP_SUM or GSL_VERIF_PLAIN");
  GSL_CHECK_ARG(e0 && e1 && dist && (mode == GSL_VERIF_PLAIN || (xnorm && pair_norm_ws)), "null pointer");
  GSL_CHECK_ARG(P > 0 && P < (1 << 29) && D > 0 && D <= VERIF_MAXD && ld >= D, "0 < P < 2^29, 0 < D <= 1024, ld >= D");
  if (mode == GSL_VERIF_PLAIN) {
    hipLaunchKernelGGL(verif_pair_dist_kernel<true>, dim3((P + 3) / 4), dim3(256), 0, as_stream(s), e0, e1, ld, P, D, dist, nullptr, nullptr);
  } else {
    hipLaunchKernelGGL(verif_pair_dist_kernel<false>, dim3((P + 3) / 4), dim3(256), 0, as_stream(s), e0, e1, ld, P, D, dist, pair_norm_ws, nemb);
    hipLaunchKernelGGL(verif_xnorm_kernel, dim3(1), dim3(256), 0, as_stream(s), pair_norm_ws, P, xnorm);
  }
  return check_launch("gsl_verif_pair_dist");
}

// ------------------------------------------------------------------ V2 fold counts
// sklearn KFold(n_splits = F, shuffle = False): contiguous test folds, the first P % F of them one pair longer
__device__ __forceinline__ void verif_fold_range(int P, int F, int f, int& start, int& len) {
  const int base = P / F, rem = P % F;
  start = f * base + min(f, rem);
  len = base + (f < rem ? 1 : 0);
}

constexpr int VERIF_CHUNK = 4096;      // pairs of a fold staged in LDS at a time: 16 KB of distances + 4 KB of flags

// Workgroup (x, f): thresholds x*256 .. x*256 + 255 against test fold f. The fold's distances pass through LDS in chunks; every lane walks
// a chunk in the same order (LDS broadcast reads) and counts its own threshold: integers, no reduction across lanes. The compare is
// np.less on the reference's operands: (double)dist < thr, strict; a NaN distance is never accepted. The thresholds need no order.
__global__ void __launch_bounds__(256) verif_fold_counts_kernel(const float* __restrict__ dist, const uint8_t* __restrict__ issame, int P,
                                                                const double* __restrict__ thr, int Tn, int F, int* __restrict__ counts,
                                                                int* __restrict__ fold_tot) {
  __shared__ float sd[VERIF_CHUNK];
  __shared__ uint8_t ss[VERIF_CHUNK];
  const int f = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  int start, len;
  verif_fold_range(P, F, f, start, len);
  const double th = t < Tn ? thr[t] : 0.0;
  int ta = 0, fa = 0, nsame = 0;
  for (int c0 = 0; c0 < len; c0 += VERIF_CHUNK) {
    const int n = min(VERIF_CHUNK, len - c0);
    __syncthreads();      // (the previous chunk is consumed)
    for (int i = threadIdx.x; i < n; i += 256) {
      sd[i] = dist[start + c0 + i];
      ss[i] = issame[start + c0 + i] != 0 ? 1 : 0;
    }
    __syncthreads();
    for (int i = 0; i < n; ++i) {
      const int same = ss[i];
      const int acc = (double)sd[i] < th ? 1 : 0;
      ta += acc & same;
      fa += acc & (same ^ 1);
      nsame += same;
    }
  }
  if (t < Tn) {
    counts[((size_t)f * Tn + t) * 2] = ta;
    counts[((size_t)f * Tn + t) * 2 + 1] = fa;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    fold_tot[f * 2] = nsame;
    fold_tot[f * 2 + 1] = len - nsame;
  }
}

extern "C" int gsl_verif_fold_counts(const float* dist, const uint8_t* issame, int P, const double* thresholds, int Tn, int nrof_folds,
                                     int* counts, int* fold_tot, gsl_stream_t s) {
  GSL_CHECK_ARG(dist && issame && thresholds && counts && fold_tot, "null pointer");
  GSL_CHECK_ARG(nrof_folds >= 1 && nrof_folds <= 65535 && P >= nrof_folds && P < (1 << 30), "1 <= nrof_folds <= P < 2^30, nrof_folds <= 65535");
  GSL_CHECK_ARG(Tn > 0 && Tn <= (1 << 20), "0 < Tn <= 2^20");
  hipLaunchKernelGGL(verif_fold_counts_kernel, dim3((Tn + 255) / 256, nrof_folds), dim3(256), 0, as_stream(s), dist, issame, P, thresholds, Tn,
                     nrof_folds, counts, fold_tot);
  return check_launch("gsl_verif_fold_counts");
}

// ------------------------------------------------------------------ V3 threshold selection and the ROC
// Workgroup f < F: fold f. TRAIN counts of threshold t = (sum over all folds) - (fold f's); train accuracy = (ta + ndiff - fa) / n_train, one
// denominator for the whole fold, so its first arg-max (np.argmax) is the first arg-max of the integer numerator. out[f] = the test accuracy
// at that threshold, float(tp + tn) / n_test; out[F + f] = the threshold.
// Workgroup F: tpr[t], fpr[t] = mean over the folds, in fold order (np.mean over axis 0 adds the rows in order), of
// ta / nsame (0 if the fold holds no same pair) and fa / ndiff (0 if it holds no different pair); out[2F + t], out[2F + Tn + t].
// out[2F + 2Tn] = (double)xnorm[0] when xnorm is given: the host reads one buffer.
__global__ void __launch_bounds__(256) verif_select_kernel(const int* __restrict__ counts, const int* __restrict__ fold_tot,
                                                           const double* __restrict__ thr, int Tn, int F, const float* __restrict__ xnorm,
                                                           double* __restrict__ out) {
  const int f = blockIdx.x, tid = threadIdx.x;
  if (f == F) {
    for (int t = tid; t < Tn; t += 256) {
      double st = 0.0, sf = 0.0;
      for (int g = 0; g < F; ++g) {
        const int ta = counts[((size_t)g * Tn + t) * 2], fa = counts[((size_t)g * Tn + t) * 2 + 1];
        const int ns = fold_tot[g * 2], nd = fold_tot[g * 2 + 1];
        st += ns == 0 ? 0.0 : (double)ta / (double)ns;
        sf += nd == 0 ? 0.0 : (double)fa / (double)nd;
      }
      out[2 * F + t] = st / (double)F;
      out[2 * F + Tn + t] = sf / (double)F;
    }
    if (tid == 0 && xnorm) out[2 * F + 2 * Tn] = (double)xnorm[0];
    return;
  }
  __shared__ long long s_num[256];
  __shared__ int s_idx[256];
  long long tot_d = 0;
  for (int g = 0; g < F; ++g) tot_d += fold_tot[g * 2 + 1];
  const long long nd_tr = tot_d - fold_tot[f * 2 + 1];
  long long best = -1;
  int bi = 0x7fffffff;
  for (int t = tid; t < Tn; t += 256) {      // ascending t: a strict > keeps the first maximum
    long long ta = 0, fa = 0;
    for (int g = 0; g < F; ++g) {
      ta += counts[((size_t)g * Tn + t) * 2];
      fa += counts[((size_t)g * Tn + t) * 2 + 1];
    }
    ta -= counts[((size_t)f * Tn + t) * 2];
    fa -= counts[((size_t)f * Tn + t) * 2 + 1];
    const long long num = ta + nd_tr - fa;      // tp + tn of the train folds
    if (num > best) { best = num; bi = t; }
  }
  s_num[tid] = best;
  s_idx[tid] = bi;
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < 256; ++i)
      if (s_num[i] > best || (s_num[i] == best && s_idx[i] < bi)) { best = s_num[i]; bi = s_idx[i]; }
    const int ns = fold_tot[f * 2], nd = fold_tot[f * 2 + 1];
    const int ta = counts[((size_t)f * Tn + bi) * 2], fa = counts[((size_t)f * Tn + bi) * 2 + 1];
    out[f] = (double)(ta + (nd - fa)) / (double)(ns + nd);
    out[F + f] = thr[bi];
  }
}

extern "C" int gsl_verif_select(const int* counts, const int* fold_tot, const double* thresholds, int Tn, int nrof_folds, const float* xnorm,
                                double* out, gsl_stream_t s) {
  GSL_CHECK_ARG(counts && fold_tot && thresholds && out, "null pointer");
  GSL_CHECK_ARG(nrof_folds >= 2 && nrof_folds <= 65535 && Tn > 0 && Tn <= (1 << 20), "2 <= nrof_folds <= 65535, 0 < Tn <= 2^20");
  hipLaunchKernelGGL(verif_select_kernel, dim3(nrof_folds + 1), dim3(256), 0, as_stream(s), counts, fold_tot, thresholds, Tn, nrof_folds, xnorm,
                     out);
  return check_launch("gsl_verif_select");
}
