// head.hip — the output end of the network:
//   K10 cls-pool + LayerNorm + CosFace / ArcFace margin head (vit_face.py:540-546, 171-208, 72-143) fwd / bwd
//       ArcFace departs from the reference in one place: sine = sqrt(max(1 - cos^2, 0)) and its derivative divides by max(sine, 1e-6),
//       where the reference's sqrt returns NaN at |cos| > 1 (rounding) and an infinite gradient at |cos| = 1.
// The losses behind it are in loss.hip, the patch gathers in front of the network in patch.hip.
#include <cmath>

#include "gsl_common.h"

using namespace gsl;

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

// ------------------------------------------------------------------ K10w head weight gradient (the linear-probe step)
// d loss / d W of the head from the upstream dlogits: what autograd gives for F.linear(F.normalize(emb), F.normalize(W)) * s with the
// margin on the label column (vit_face.py:181-207, 117-141), or for the plain nn.Linear of the Softmax head (:47-50). The reference
// trains this tensor alone in train/backbone_forget_main.py:596-600, 657-670.
//   G[b,c] = cos_s * dlogits[b,c], the ArcFace label column times arc_dphi(cos_y[b]) — the expression and the label rule of head_bwd_kernel
//   d What_c = sum_b G[b,c] * emb_b / max(||emb_b||, 1e-12);  dW_c = (d What_c - What_c (What_c . d What_c)) / ||W_c||
//   ||W_c|| < 1e-12: F.normalize's clamp has derivative 0 there, dW_c = d What_c / 1e-12
//   linear: dW_c = sum_b dlogits[b,c] * emb_b, dbias_c = sum_b dlogits[b,c]
// One workgroup of 16 waves per tile of CT classes, all D columns: wave w owns the images w, w + 16, ... in ascending order (a lane holds
// the columns lane, lane + 64, ... of the image's row, so the row norm is one wave reduction and the row is read once for the CT classes),
// then the 16 partial sums are added in wave order through LDS. The order of every sum is fixed by (B, C, D): no atomics, bit-repeatable.
// Nothing in LDS is sized by C; every element of dW (and dbias) is stored.
constexpr int HEAD_LINEAR = 2;      // head_kind of gsl_head_wgrad only: the plain classifier (no normalisation, no margin)
constexpr int HW_WAVES = 16;

// KM: the columns a lane holds of one row (D <= 64 * KM), so that D = 512 pays for 8 and not for HEAD_MAXD / 64 = 16.
template <int KIND, int CT, int KM>
__global__ __launch_bounds__(1024) void head_wgrad_kernel(const float* __restrict__ dlogits, const float* __restrict__ emb,
                                                         const float* __restrict__ W, const int64_t* __restrict__ label,
                                                         const float* __restrict__ cos_y, float* __restrict__ dW,
                                                         float* __restrict__ dbias, int B, int C, int D, float cs, ArcMargin arc) {
  constexpr int U = KM > 8 ? 2 : 4;         // images per round: up to 32 row loads of a lane in flight (eight images spill at CT = 2)
  constexpr int NQ = (KM + 3) / 4;          // 256-column chunks
  __shared__ float red[HW_WAVES][256];      // one 256-column chunk of every wave's partial sums
  __shared__ float fin[CT][64 * KM];        // d What (cosine heads) / dW (linear) of the tile's classes
  __shared__ float sb[HW_WAVES][CT];        // the waves' dbias partial sums
  __shared__ float sm[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = blockIdx.x * CT;
  float acc[CT][KM];
  float gsum[CT];
#pragma unroll
  for (int j = 0; j < CT; ++j) {
    gsum[j] = 0.f;
#pragma unroll
    for (int k = 0; k < KM; ++k) acc[j][k] = 0.f;
  }
  // U images per round (b, b + 16, ...: the wave's ascending order). Every load of the round — the rows, their dlogits, label and cos_y —
  // is issued before the first use, so a round costs one trip to memory; the work is latency-bound (B / (16 U) rounds per wave).
  for (int b0 = wave; b0 < B; b0 += U * HW_WAVES) {
    float e[U][KM], g[U][CT], cy[U];
    int y[U];      // the label where it lies in [0, C) (head_bwd_kernel's rule), else -1
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int b = b0 + u * HW_WAVES;
      const bool live = b < B;      // (a dead row adds 0 * 0 to every sum)
      const float* er = emb + (size_t)(live ? b : b0) * D;
#pragma unroll
      for (int k = 0; k < KM; ++k) {
        const int d = k * 64 + lane;
        e[u][k] = (live && d < D) ? er[d] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < CT; ++j) g[u][j] = (live && c0 + j < C) ? dlogits[(size_t)b * C + c0 + j] : 0.f;
      y[u] = -1;
      cy[u] = 0.f;
      if constexpr (KIND == HEAD_ARCFACE) {
        if (live) {
          const int64_t yl = label[b];
          y[u] = (yl >= 0 && yl < C) ? (int)yl : -1;
          cy[u] = cos_y[b];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float inv = 1.0f;
      if constexpr (KIND != HEAD_LINEAR) {
        float ss = 0.f;
#pragma unroll
        for (int k = 0; k < KM; ++k) ss += e[u][k] * e[u][k];
        inv = 1.0f / fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
      }
      float dphi = 1.0f;
      if constexpr (KIND == HEAD_ARCFACE) {
        if (y[u] >= c0 && y[u] < c0 + CT) dphi = arc_dphi(cy[u], arc);      // (other tiles never use it)
      }
#pragma unroll
      for (int j = 0; j < CT; ++j) {
        float gv = g[u][j];
        if constexpr (KIND == HEAD_LINEAR) gsum[j] += gv;
        if constexpr (KIND != HEAD_LINEAR) gv *= cs;
        if constexpr (KIND == HEAD_ARCFACE) { if (c0 + j == y[u]) gv *= dphi; }
        const float gi = gv * inv;
#pragma unroll
        for (int k = 0; k < KM; ++k) acc[j][k] += gi * e[u][k];
      }
    }
  }
  // the 16 waves' partial sums, added in wave order: 256 columns at a time through red[][]
#pragma unroll
  for (int j = 0; j < CT; ++j) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (q * 256 < D) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (4 * q + i < KM) red[wave][i * 64 + lane] = acc[j][4 * q + i];
        wg_barrier_lds();
        if (tid < 256 && q * 256 + tid < 64 * KM) {
          float s = 0.f;
#pragma unroll
          for (int w = 0; w < HW_WAVES; ++w) s += red[w][tid];
          fin[j][q * 256 + tid] = s;
        }
        wg_barrier_lds();
      }
    }
  }
  if constexpr (KIND == HEAD_LINEAR) {
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < CT; ++j) sb[wave][j] = gsum[j];
    }
    wg_barrier_lds();
    if (dbias && tid < CT && c0 + tid < C) {
      float s = 0.f;
      for (int w = 0; w < HW_WAVES; ++w) s += sb[w][tid];
      dbias[c0 + tid] = s;
    }
  }
  for (int j = 0; j < CT; ++j) {
    const int c = c0 + j;
    if (c >= C) break;      // (uniform over the workgroup)
    const bool in = tid < D;      // D <= 64 * KM <= the workgroup size: a thread finishes one column
    const float f = in ? fin[j][tid] : 0.f;
    if constexpr (KIND == HEAD_LINEAR) {
      if (in) dW[(size_t)c * D + tid] = f;
    } else {
      const float w = in ? W[(size_t)c * D + tid] : 0.f;
      const float raw = sqrtf(block_sum(w * w, sm));
      const float dot = block_sum(w * f, sm);
      const float nrm = fmaxf(raw, 1e-12f);
      if (in) dW[(size_t)c * D + tid] = (raw >= 1e-12f) ? (f - (w / nrm) * (dot / nrm)) / nrm : f / nrm;
    }
  }
}

template <int KIND, int CT>
static void head_wgrad_launch_ct(const float* dlogits, const float* emb, const float* W, const int64_t* label, const float* cos_y, float* dW,
                                 float* dbias, int B, int C, int D, float cs, ArcMargin arc, gsl_stream_t s) {
  const dim3 grid((C + CT - 1) / CT), block(HW_WAVES * 64);
  if (D <= 256)
    hipLaunchKernelGGL((head_wgrad_kernel<KIND, CT, 4>), grid, block, 0, as_stream(s), dlogits, emb, W, label, cos_y, dW, dbias, B, C, D, cs, arc);
  else if (D <= 512)
    hipLaunchKernelGGL((head_wgrad_kernel<KIND, CT, 8>), grid, block, 0, as_stream(s), dlogits, emb, W, label, cos_y, dW, dbias, B, C, D, cs, arc);
  else
    hipLaunchKernelGGL((head_wgrad_kernel<KIND, CT, 16>), grid, block, 0, as_stream(s), dlogits, emb, W, label, cos_y, dW, dbias, B, C, D, cs, arc);
}

template <int KIND>
static void head_wgrad_launch(const float* dlogits, const float* emb, const float* W, const int64_t* label, const float* cos_y, float* dW,
                              float* dbias, int B, int C, int D, float cs, ArcMargin arc, gsl_stream_t s) {
  // A workgroup per class up to 256 classes. The cosine heads need every row's norm, so a workgroup reads all of emb whatever part of
  // dW it owns: splitting the columns over more workgroups would shorten no wave's chain of rounds and multiply the L2 traffic, and
  // splitting the batch would need a second pass or float atomics. Many classes: two per workgroup, which read every row once for both.
  if (C <= 256)
    head_wgrad_launch_ct<KIND, 1>(dlogits, emb, W, label, cos_y, dW, dbias, B, C, D, cs, arc, s);
  else
    head_wgrad_launch_ct<KIND, 2>(dlogits, emb, W, label, cos_y, dW, dbias, B, C, D, cs, arc, s);
}

extern "C" int gsl_head_wgrad(const float* dlogits, const float* emb, const float* W, const int64_t* label, const float* cos_y, float* dW,
                              float* dbias, int B, int C, int D, int head_kind, float cos_s, double m, int easy_margin, gsl_stream_t s) {
  GSL_CHECK_ARG(head_kind == HEAD_COSFACE || head_kind == HEAD_ARCFACE || head_kind == HEAD_LINEAR, "head_kind: 0 (CosFace), 1 (ArcFace) or 2 (linear)");
  GSL_CHECK_ARG(dlogits && emb && dW && B > 0 && C > 0, "null/size");
  GSL_CHECK_ARG(head_kind == HEAD_LINEAR || W, "the cosine heads read W");
  GSL_CHECK_ARG(D > 0 && D <= HEAD_MAXD, "D <= 1024");
  GSL_CHECK_ARG(head_kind != HEAD_ARCFACE || (label && cos_y), "ArcFace needs label and cos_y [B]");
  GSL_CHECK_ARG(head_kind == HEAD_LINEAR || !dbias, "dbias belongs to the linear head");
  if (head_kind == HEAD_ARCFACE)
    head_wgrad_launch<HEAD_ARCFACE>(dlogits, emb, W, label, cos_y, dW, nullptr, B, C, D, cos_s, arc_margin(m, easy_margin), s);
  else if (head_kind == HEAD_LINEAR)
    head_wgrad_launch<HEAD_LINEAR>(dlogits, emb, W, nullptr, nullptr, dW, dbias, B, C, D, 1.0f, ArcMargin{}, s);
  else
    head_wgrad_launch<HEAD_COSFACE>(dlogits, emb, W, nullptr, nullptr, dW, nullptr, B, C, D, cos_s, ArcMargin{}, s);
  return check_launch("gsl_head_wgrad");
}
