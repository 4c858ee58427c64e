// head.hip — the output end of the network:
//   K10 cls-pool + LayerNorm + CosFace / ArcFace margin head (vit_face.py:540-546, 171-208, 72-143) fwd / bwd
//       ArcFace departs from the reference in one place: sine = sqrt(max(1 - cos^2, 0)) and its derivative divides by max(sine, 1e-6),
//       where the reference's sqrt returns NaN at |cos| > 1 (rounding) and an infinite gradient at |cos| = 1.
//       F.normalize's clamp max(||v||, 1e-12) has derivative 0 below it: the backward (an embedding under the clamp) and the weight
//       gradient (a row of W under it) then give d v = d v-hat / 1e-12 without the projection term, as autograd gives the reference.
// The losses behind it are in loss.hip, the patch gathers in front of the network in patch.hip.
#include <cmath>
#include <type_traits>

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
constexpr int HEAD_LINEAR = 2;      // head_kind of gsl_head_wgrad only: the plain classifier (no normalisation, no margin)
template <int V> using HeadInt = std::integral_constant<int, V>;      // a tile or kind constant on its way into a template argument
// The one place a head_kind becomes the KIND template value: f(HeadInt<KIND>). WGRAD: the caller is the weight gradient, whose kernels
// exist for HEAD_LINEAR too (the forward and backward kernels do not: their linear head is the run-time flag).
template <bool WGRAD = false, typename F>
static void head_for_kind(int kind, F&& f) {
  if (kind == HEAD_ARCFACE) return f(HeadInt<HEAD_ARCFACE>{});
  if constexpr (WGRAD) {
    if (kind == HEAD_LINEAR) return f(HeadInt<HEAD_LINEAR>{});
  }
  f(HeadInt<HEAD_COSFACE>{});
}
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

// ------------------------------------------------------------------ K10t class-tiled head, C > HEAD_TILED_C
// The per-image kernels above and below read all of Wn once per image and (the backward) keep an image's dlogits row in LDS: fine at
// C = 100, refused or ruinous at the 10 572 / 85 742 / 93 431 identities face transformers train on. Above HEAD_TILED_C classes the four
// entry points run the head's two products as tiled f32 GEMMs on v_mfma_f32_16x16x4_f32 (exact f32, a k-ordered fmaf chain per output —
// the instruction of gemm_f32_mfma_kernel), so Wn is read once per image TILE:
//   forward   head_fwd_kernel(logits = NULL) writes emb / mean / rstd, then head_logits_tiled_kernel: logits tile = emb tile . Wn tile^T
//   backward  head_de_tiled_kernel: d e-hat [B, D] = (s dlogits, the ArcFace label column times d phi) . Wn into the workspace, ONCE, then
//             head_bwd_kernel<.., WS = true>, which takes d e-hat from there (twice in the loss-scaled form, as ever: it is cheap)
// Every output element is one chain over ascending k that starts at 0 and runs over zero-filled padding to the K tile's end: the value of
// row b depends on neither B nor the tile b falls in. Rows / columns past B, C, D are never read (clamped row, or a zero in its place)
// and never written. No LDS array is sized by C. Index arithmetic on [B, C] / [C, D] is size_t; the entry points hold B C and C D below 2^31.
constexpr int HEAD_TILED_C = 1024;      // C <= this: the per-image kernels, bit for bit what they always computed
typedef __attribute__((ext_vector_type(4))) float head_f32x4_t;
constexpr int HT_BK = 32;               // K tile of the logits kernel: 32 columns of D
constexpr int HT_LDA = HT_BK + 4;       // row stride of a [row][k] panel: 36 r + fc covers the 64 banks once over a fragment read
constexpr int HL_BM = 64, HL_BN = 128;  // logits tile: images x classes; 4 waves of 32 x 64 (2 x 4 fragments)

__device__ __forceinline__ float4 keep4(bool keep, float4 v) {      // v, or zeros for a chunk outside the tensor
  return make_float4(keep ? v.x : 0.f, keep ? v.y : 0.f, keep ? v.z : 0.f, keep ? v.w : 0.f);
}

template <int KIND>
__global__ __launch_bounds__(256) void head_logits_tiled_kernel(const float* __restrict__ emb, const float* __restrict__ Wn,
                                                                const int64_t* __restrict__ label, float* __restrict__ logits, int B,
                                                                int D, int C, float cs, float cm, const float* __restrict__ hbias,
                                                                int linear, ArcMargin arc, float* __restrict__ cos_y) {
  fp16_sat_on();
  __shared__ __attribute__((aligned(16))) float As[HL_BM * HT_LDA];
  __shared__ __attribute__((aligned(16))) float Ws[HL_BN * HT_LDA];
  __shared__ float invs[HL_BM];
  __shared__ int labs[HL_BM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // image tiles fastest: the workgroups in flight together share a few class tiles of Wn (21.6 MB at C = 10 572, D = 512) in L2
  const int nbm = (B + HL_BM - 1) / HL_BM;
  const int m0 = (blockIdx.x % nbm) * HL_BM, n0 = (blockIdx.x / nbm) * HL_BN;
  // 1 / max(||emb_b||, 1e-12) of the tile's images: a wave per row, lanes over d, one wave reduction — the order is fixed by D alone
  for (int r = wave; r < HL_BM; r += 4) {
    const int b = m0 + r;
    float inv = 1.0f;
    int lab = -1;
    if (b < B) {
      if (!linear) {
        float ss = 0.f;
        for (int d = lane; d < D; d += 64) { const float v = emb[(size_t)b * D + d]; ss += v * v; }
        inv = 1.0f / fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
      }
      if (label) { const int64_t y = label[b]; lab = (y >= 0 && y < C) ? (int)y : -1; }
    }
    if (lane == 0) { invs[r] = inv; labs[r] = lab; }
  }
  const int lrow = tid >> 3, lch = (tid & 7) * 4;      // staging: 32 rows x 8 float4 per pass
  float4 ra[HL_BM / 32], rw[HL_BN / 32];
  // Every load is unconditional on a clamped (in-bounds) address and what lies outside the tensor is replaced by zero afterwards: a
  // load under a condition compiles to a branch with its own s_waitcnt vmcnt(0), i.e. one memory round trip per load instead of per tile.
  auto fetch = [&](int k0) {
    const bool kin = k0 + lch < D;      // (D % 4 == 0: a float4 lies inside the row or outside it)
    const int kc = min(k0 + lch, D - 4);
#pragma unroll
    for (int i = 0; i < HL_BM / 32; ++i) {
      const int gm = min(m0 + lrow + 32 * i, B - 1);
      ra[i] = *reinterpret_cast<const float4*>(emb + (size_t)gm * D + kc);
    }
#pragma unroll
    for (int i = 0; i < HL_BN / 32; ++i) {
      const int gn = min(n0 + lrow + 32 * i, C - 1);
      rw[i] = *reinterpret_cast<const float4*>(Wn + (size_t)gn * D + kc);
    }
#pragma unroll
    for (int i = 0; i < HL_BM / 32; ++i) ra[i] = keep4(kin, ra[i]);
#pragma unroll
    for (int i = 0; i < HL_BN / 32; ++i) rw[i] = keep4(kin, rw[i]);
  };
  head_f32x4_t acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = head_f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int fr = lane & 15, fc = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const int nk = (D + HT_BK - 1) / HT_BK;
  fetch(0);
  for (int kt = 0; kt < nk; ++kt) {
#pragma unroll
    for (int i = 0; i < HL_BM / 32; ++i) *reinterpret_cast<float4*>(&As[(lrow + 32 * i) * HT_LDA + lch]) = ra[i];
#pragma unroll
    for (int i = 0; i < HL_BN / 32; ++i) *reinterpret_cast<float4*>(&Ws[(lrow + 32 * i) * HT_LDA + lch]) = rw[i];
    wg_barrier_lds();
    if (kt + 1 < nk) fetch((kt + 1) * HT_BK);      // the next tile's loads fly under this tile's MFMAs
#pragma unroll
    for (int ks = 0; ks < HT_BK / 4; ++ks) {
      float af[2], wf[4];
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i] = As[(wm * 32 + i * 16 + fr) * HT_LDA + ks * 4 + fc];
#pragma unroll
      for (int j = 0; j < 4; ++j) wf[j] = Ws[(wn * 64 + j * 16 + fr) * HT_LDA + ks * 4 + fc];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], wf[j], acc[i][j], 0, 0, 0);
    }
    wg_barrier_lds();      // every wave has read the panels before the next tile overwrites them
  }
  // a lane holds images 4 fc + r, class fr of every fragment: a store instruction writes 16 consecutive classes of 4 images
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = wm * 32 + i * 16 + 4 * fc + r, b = m0 + row;
      if (b >= B) continue;
      const float inv = invs[row];
      const int lab = labs[row];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = n0 + wn * 64 + j * 16 + fr;
        if (c >= C) continue;
        float dk = acc[i][j][r];
        float* out = logits + (size_t)b * C + c;
        if (linear) *out = dk + (hbias ? hbias[c] : 0.f);
        else if constexpr (KIND == HEAD_ARCFACE) {
          dk *= inv;
          if (c == lab) { cos_y[b] = dk; dk = arc_phi(dk, arc); }
          *out = cs * dk;
        } else { dk *= inv; *out = cs * ((c == lab) ? (dk - cm) : dk); }
      }
    }
}

// ------------------------------------------------------------------ host side of the forward and the backward
// One head call as the host side passes it around: an entry point fills one by name, then checks it and launches from it.
struct HeadCall {
  const char* who;                                            // the entry point: the name in front of a refusal or a launch error
  const void* x; int x_dtype, T; const float *gamma, *beta; float eps;      // the stream [B, T, D] and the head's LayerNorm
  const float *Wn, *hbias; const int64_t* label;
  float *emb, *mean, *rstd, *cos_y;                           // written by the forward, read by the backward (cos_y: ArcFace only)
  float* logits;
  const float *dlogits, *demb; void *dx, *dxb;                // backward
  int B, D, C; float cos_s, cos_m;
  int dtype, stream_dtype;                                    // backward: T and S of the kernels (check_row_dtypes; X is x_dtype)
  DropCfg drop; int linear, pool_mean, compact;
  float *gscale, *amax_ws; int target_exp;                    // loss-scaled backward (fp16 operands); amax_ws also holds d e-hat above 1024 classes
  int kind; ArcMargin arc;
  const float* W; float *dW, *dbias;                          // weight gradient
  hipStream_t st;
};

// ArcFace constants of margin m (vit_face.py:98-101): math.cos / math.sin in double, as the reference computes them, then float
static ArcMargin arc_margin(double m, int easy_margin) {
  const double pi = 3.14159265358979323846;      // math.pi
  return ArcMargin{(float)std::cos(m), (float)std::sin(m), (float)std::cos(pi - m), (float)(std::sin(pi - m) * m), easy_margin ? 1 : 0};
}
static void head_set_kind(HeadCall& c, int head_kind, double m, int easy_margin) {
  c.kind = head_kind;
  c.arc = head_kind == HEAD_ARCFACE ? arc_margin(m, easy_margin) : ArcMargin{};
}

// what the class-tiled kernels ask for; `used`: the call touches the [B, C] / [C, D] tensors at all (logits / dlogits given)
static int head_check_tiled(const HeadCall& c, bool used) {
  GSL_CHECK_ARG_AS(c.who, !used || c.C <= HEAD_TILED_C || ((long long)c.B * c.C < (1ll << 31) && (long long)c.C * c.D < (1ll << 31)),
                   "C out of range: above 1024 classes B*C and C*D must stay below 2^31 elements");
  GSL_CHECK_ARG_AS(c.who, !used || c.C <= HEAD_TILED_C || ((((uintptr_t)c.Wn) | ((uintptr_t)c.emb)) & 15) == 0,
                   "above 1024 classes Wn and emb must be 16-byte aligned (the tiled kernels load float4)");
  return GSL_OK;
}

static int head_fwd_check(const HeadCall& c) {
  GSL_CHECK_ARG_AS(c.who, c.kind == HEAD_COSFACE || c.kind == HEAD_ARCFACE, "head_kind: 0 (CosFace) or 1 (ArcFace)");
  GSL_CHECK_ARG_AS(c.who, c.x_dtype == GSL_F32 || c.x_dtype == GSL_BF16 || c.x_dtype == GSL_F16, "x dtype");
  GSL_CHECK_ARG_AS(c.who, c.x && c.gamma && c.beta && c.emb && c.mean && c.rstd && c.B > 0 && c.T > 0, "null/size");
  GSL_CHECK_ARG_AS(c.who, c.D > 0 && c.D <= HEAD_MAXD && (c.D % 4) == 0, "D <= 1024, D%4==0");
  GSL_CHECK_ARG_AS(c.who, !c.logits || (c.Wn && c.C > 0), "Wn required for logits");
  GSL_TRY(head_check_tiled(c, c.logits != nullptr));
  GSL_CHECK_ARG_AS(c.who, c.kind != HEAD_ARCFACE || !c.linear, "ArcFace is a cosine head (linear_head = 0)");
  GSL_CHECK_ARG_AS(c.who, c.kind != HEAD_ARCFACE || !c.logits || (c.label && c.cos_y), "ArcFace logits need label and cos_y [B]");
  return GSL_OK;
}

static int head_fwd_launch(const HeadCall& c) {
  // class-tiled: the per-image kernel stops behind emb / mean / rstd (no logits), the logits are a GEMM of their own
  const bool tiled = c.logits && c.C > HEAD_TILED_C;
  float* const own_logits = tiled ? nullptr : c.logits;
  const int nthr = c.B <= 128 ? 1024 : 256;      // one workgroup per image: with few images give each one 16 waves (100 class rows in two rounds)
  head_for_kind(c.kind, [&](auto kind) {
    constexpr int KIND = decltype(kind)::value;
    dispatch_elem_type(c.x_dtype, [&](auto x) {
      using X = typename decltype(x)::type;
      hipLaunchKernelGGL((head_fwd_kernel<X, KIND>), dim3(c.B), dim3(nthr), 0, c.st, (const X*)c.x, c.T, c.gamma, c.beta, c.eps, c.Wn, c.label, c.emb,
                         c.mean, c.rstd, own_logits, c.D, c.C, c.cos_s, c.cos_m, c.hbias, c.linear, c.pool_mean, c.arc, c.cos_y);
    });
    if (tiled) {
      const int nblk = ((c.B + HL_BM - 1) / HL_BM) * ((c.C + HL_BN - 1) / HL_BN);
      hipLaunchKernelGGL((head_logits_tiled_kernel<KIND>), dim3(nblk), dim3(256), 0, c.st, (const float*)c.emb, c.Wn, c.label, c.logits, c.B, c.D, c.C,
                         c.cos_s, c.cos_m, c.hbias, c.linear, c.arc, c.cos_y);
    }
  });
  return check_launch(c.who);
}

extern "C" int gsl_head_fwd(const void* x, int x_dtype, int T, const float* gamma, const float* beta, float eps, const float* Wn,
                            const int64_t* label, float* emb, float* mean, float* rstd, float* logits, int B, int D, int C,
                            float cos_s, float cos_m, const float* head_bias, int linear_head, int pool_mean, gsl_stream_t s) {
  HeadCall c{};      // the margin form with the CosFace kind and no cos_y
  c.who = __func__; c.x = x; c.x_dtype = x_dtype; c.T = T; c.gamma = gamma; c.beta = beta; c.eps = eps; c.Wn = Wn; c.label = label; c.emb = emb;
  c.mean = mean; c.rstd = rstd; c.logits = logits; c.B = B; c.D = D; c.C = C; c.cos_s = cos_s; c.cos_m = cos_m; c.hbias = head_bias;
  c.linear = linear_head; c.pool_mean = pool_mean; c.st = as_stream(s);
  head_set_kind(c, HEAD_COSFACE, 0.0, 0);
  GSL_TRY(head_fwd_check(c));
  return head_fwd_launch(c);
}

extern "C" int gsl_head_fwd_margin(const void* x, int x_dtype, int T, const float* gamma, const float* beta, float eps, const float* Wn,
                                   const int64_t* label, float* emb, float* mean, float* rstd, float* logits, int B, int D, int C,
                                   float cos_s, float cos_m, const float* head_bias, int linear_head, int pool_mean, int head_kind,
                                   double m, int easy_margin, float* cos_y, gsl_stream_t s) {
  HeadCall c{};
  c.who = __func__; c.x = x; c.x_dtype = x_dtype; c.T = T; c.gamma = gamma; c.beta = beta; c.eps = eps; c.Wn = Wn; c.label = label; c.emb = emb;
  c.mean = mean; c.rstd = rstd; c.logits = logits; c.B = B; c.D = D; c.C = C; c.cos_s = cos_s; c.cos_m = cos_m; c.hbias = head_bias;
  c.linear = linear_head; c.pool_mean = pool_mean; c.cos_y = cos_y; c.st = as_stream(s);
  head_set_kind(c, head_kind, m, easy_margin);
  GSL_TRY(head_fwd_check(c));
  return head_fwd_launch(c);
}

// Stage 1 of the class-tiled backward: ws [B, D] = G . Wn with G[b, c] = cs * dlogits[b, c], the ArcFace label column times
// d phi / d cos at cos_y[b] — head_bwd_kernel's expressions, in its order. One workgroup per (32 images x 64 columns) tile runs the whole
// class loop, classes ascending in K tiles of 128: a fixed partition, no atomics. Type-independent (f32 in, f32 out).
// The workgroup is alone on its CU at the flagship shape (B = 1024, D = 512: 256 tiles), so a K tile is a round trip to memory that only
// its own MFMAs can hide: 128 classes per tile put 48 KB of loads in flight per CU, with a quarter of the barriers of a 32-class tile.
constexpr int HD_BM = 32, HD_BN = 64;   // d e-hat tile: images x columns; 4 waves of 16 x 32 (1 x 2 fragments)
constexpr int HD_BK = 128;              // classes per K tile
constexpr int HD_LDA = HD_BK + 4;       // row stride of the [image][class] panel: 132 fr + fc covers the 64 banks once
constexpr int HD_LDW = HD_BN + 16;      // row stride of the [class][column] panel of Wn: 80 fc + fr covers the 64 banks once

template <int KIND>
__global__ __launch_bounds__(256) void head_de_tiled_kernel(const float* __restrict__ dlogits, const float* __restrict__ Wn,
                                                            const int64_t* __restrict__ label, const float* __restrict__ cos_y,
                                                            float* __restrict__ ws, int B, int D, int C, float cs, ArcMargin arc) {
  fp16_sat_on();
  __shared__ __attribute__((aligned(16))) float As[HD_BM * HD_LDA];      // G tile [image][class]
  __shared__ __attribute__((aligned(16))) float Ws[HD_BK * HD_LDW];      // Wn tile [class][column]
  __shared__ float dph[HD_BM];
  __shared__ int labs[HD_BM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // image tiles fastest: workgroup i runs on XCD i % 8, so an XCD holds every column tile of its image tiles — together they read whole
  // rows of Wn (all L2 channels; one 256-byte slice per 2 KB row from every workgroup of an XCD camps on two of them) and share dlogits
  const int nbm = (B + HD_BM - 1) / HD_BM;
  const int m0 = (blockIdx.x % nbm) * HD_BM, d0 = (blockIdx.x / nbm) * HD_BN;
  if (tid < HD_BM) {
    int lab = -1;
    float dp = 1.0f;
    if constexpr (KIND == HEAD_ARCFACE) {
      if (m0 + tid < B) {
        const int64_t y = label[m0 + tid];
        if (y >= 0 && y < C) { lab = (int)y; dp = arc_dphi(cos_y[m0 + tid], arc); }
      }
    }
    labs[tid] = lab; dph[tid] = dp;
  }
  wg_barrier_lds();
  const int ak = tid & (HD_BK - 1), ar = tid / HD_BK;   // G staging: 2 rows x 128 classes per pass (rows of dlogits start at any dword)
  const int wr = tid >> 4, wch = (tid & 15) * 4;        // Wn staging: 16 classes x 16 float4 per pass
  float ra[HD_BM / 2];
  float4 rw[HD_BK / 16];
  // unconditional loads on clamped (in-bounds) addresses, zero selected afterwards for what lies outside (see head_logits_tiled_kernel)
  const int dc = min(d0 + wch, D - 4);
  const bool din = d0 + wch < D;
  auto fetch = [&](int k0) {
    const int c = k0 + ak, cc = min(c, C - 1);
#pragma unroll
    for (int i = 0; i < HD_BM / 2; ++i) ra[i] = dlogits[(size_t)min(m0 + ar + 2 * i, B - 1) * C + cc];
#pragma unroll
    for (int i = 0; i < HD_BK / 16; ++i) rw[i] = *reinterpret_cast<const float4*>(Wn + (size_t)min(k0 + wr + 16 * i, C - 1) * D + dc);
#pragma unroll
    for (int i = 0; i < HD_BM / 2; ++i) {
      const int r = ar + 2 * i;
      float v = (m0 + r < B && c < C) ? cs * ra[i] : 0.f;
      if constexpr (KIND == HEAD_ARCFACE) { if (c == labs[r]) v *= dph[r]; }
      ra[i] = v;
    }
#pragma unroll
    for (int i = 0; i < HD_BK / 16; ++i) rw[i] = keep4(din && k0 + wr + 16 * i < C, rw[i]);
  };
  head_f32x4_t acc[2];
  acc[0] = acc[1] = head_f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int fr = lane & 15, fc = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const int nk = (C + HD_BK - 1) / HD_BK;
  fetch(0);
  for (int kt = 0; kt < nk; ++kt) {
#pragma unroll
    for (int i = 0; i < HD_BM / 2; ++i) As[(ar + 2 * i) * HD_LDA + ak] = ra[i];
#pragma unroll
    for (int i = 0; i < HD_BK / 16; ++i) *reinterpret_cast<float4*>(&Ws[(wr + 16 * i) * HD_LDW + wch]) = rw[i];
    wg_barrier_lds();
    if (kt + 1 < nk) fetch((kt + 1) * HD_BK);
#pragma unroll
    for (int ks = 0; ks < HD_BK / 4; ++ks) {
      const float af = As[(wm * 16 + fr) * HD_LDA + ks * 4 + fc];
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, Ws[(ks * 4 + fc) * HD_LDW + wn * 32 + j * 16 + fr], acc[j], 0, 0, 0);
    }
    wg_barrier_lds();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = m0 + wm * 16 + 4 * fc + r;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int d = d0 + wn * 32 + j * 16 + fr;
      if (b < B && d < D) ws[(size_t)b * D + d] = acc[j][r];
    }
  }
}

// compact != 0 (pool = 'cls' only): dx / dxb are [B, D] — the gradient of the cls rows alone; the stream gradient of every other token is
// exactly zero and is neither written here nor read by the consumers (the cls-row-only backward of the last block, gsl_layernorm_bwd's
// dres_cls_T). The dropout counter of element (b, d) stays that of the dense tensor, (b*Tn)*D + d: same masks in both forms.
// KIND = HEAD_ARCFACE: the label column of dlogits is multiplied by d phi / d cos at cos_y [B] (written by the forward) before
// the sum over the classes; everything after that is the CosFace code.
// WS = true (stage 2 of the class-tiled backward, C > HEAD_TILED_C): d e-hat [B, D] was left in the workspace by head_de_tiled_kernel and
// arrives through the Wn argument; the class loop and dl[] do not exist in these instantiations, everything else is the code below.
template <typename T, typename S, typename X, int KIND, bool WS = false>
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
  const float raw = sqrtf(block_sum(nn, sm));
  const float nrm = fmaxf(raw, 1e-12f);
  if constexpr (!WS) {
    if (dlogits) {
      for (int c = tid; c < C; c += 256) dl[c] = cs * dlogits[(size_t)b * C + c];
      if constexpr (KIND == HEAD_ARCFACE) {      // the thread that stored dl[y] rescales it: no barrier needed in between
        const long y = (long)label[b];
        if (y >= 0 && y < C && tid == (int)(y & 255)) dl[y] *= arc_dphi(cos_y[b], arc);
      }
    }
  }
  __syncthreads();
  float dotp = 0.f;
  for (int d = tid; d < D; d += 256) {
    float g = 0.f;
    if constexpr (WS) {
      if (dlogits) g = Wn[(size_t)b * D + d];
    } else if (dlogits) {
      for (int c = 0; c < C; ++c) g += dl[c] * Wn[(size_t)c * D + d];
    }
    de[d] = g;                       // d e-hat
    dotp += g * er[d];
  }
  // (e-hat . d e-hat) / ||e||; ||e|| < 1e-12: F.normalize's clamp has derivative 0 there, d e = d e-hat / 1e-12 (the rule of head_wgrad_kernel)
  const float projn = block_sum(dotp, sm) / (nrm * nrm);
  const float proj = (raw < 1e-12f) ? 0.0f : projn;      // (a NaN norm keeps the NaN projection)
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

static int head_bwd_check(const HeadCall& c) {
  GSL_CHECK_ARG_AS(c.who, c.kind == HEAD_COSFACE || c.kind == HEAD_ARCFACE, "head_kind: 0 (CosFace) or 1 (ArcFace)");
  GSL_CHECK_ARG_AS(c.who, c.x && c.gamma && c.mean && c.rstd && c.emb && c.dx && c.B > 0 && c.T >= 1, "null/size");
  GSL_CHECK_ARG_AS(c.who, c.D > 0 && c.D <= HEAD_MAXD && (c.D % 4) == 0, "D <= 1024, D%4==0");
  GSL_CHECK_ARG_AS(c.who, c.C <= HEAD_TILED_C || c.amax_ws,
                   "C > 1024 needs the workspace amax_ws [B*(D+1)] (d e-hat of the class-tiled backward), also without gscale");
  GSL_TRY(head_check_tiled(c, c.dlogits != nullptr));
  GSL_CHECK_ARG_AS(c.who, !c.dlogits || c.Wn, "Wn required with dlogits");
  GSL_CHECK_ARG_AS(c.who, !(c.compact && c.pool_mean), "compact cls-row gradients need pool = 'cls'");
  GSL_CHECK_ARG_AS(c.who, !c.gscale || c.amax_ws, "gscale (loss-scaled gradients) needs amax_ws [B]");
  GSL_CHECK_ARG_AS(c.who, c.target_exp == 0 || (c.target_exp >= 4 && c.target_exp <= 15), "target_exp: 0 (default 11) or 4 .. 15");
  GSL_TRY(check_row_dtypes(c.who, c.dtype, c.stream_dtype, c.x_dtype));
  GSL_CHECK_ARG_AS(c.who, c.kind != HEAD_ARCFACE || !c.linear, "ArcFace is a cosine head (linear_head = 0)");
  GSL_CHECK_ARG_AS(c.who, c.kind != HEAD_ARCFACE || !c.dlogits || (c.label && c.cos_y), "ArcFace dlogits need label and cos_y [B]");
  if (c.dtype != GSL_F16 && c.dtype != GSL_BF16 && c.dtype != GSL_F32) return fail(GSL_ERR_ARG, "%s: bad dtype %ld", c.who, c.dtype);
  return GSL_OK;
}

// The per-image kernel. WS = false: `src` is Wn and the kernel runs the class loop; WS = true: `src` is d e-hat [B, D], left in the
// workspace by head_de_tiled_kernel. Loss-scaled (gscale): two launches, the second reads what the first wrote.
template <int KIND, bool WS>
static void head_bwd_rows(const HeadCall& c, const float* src) {
  const int texp = c.target_exp ? c.target_exp : GSL_GRAD_TARGET_EXP;
  dispatch_row_types(c.dtype, c.stream_dtype, c.x_dtype, [&](auto t, auto s, auto x) {
    using T = typename decltype(t)::type;
    using S = typename decltype(s)::type;
    using X = typename decltype(x)::type;
    auto pass = [&](float* amax_out, const float* amax_in, int n_amax) {
      hipLaunchKernelGGL((head_bwd_kernel<T, S, X, KIND, WS>), dim3(c.B), dim3(256), 0, c.st, c.dlogits, c.demb, (const X*)c.x, c.T, c.gamma, c.mean,
                         c.rstd, c.emb, src, (S*)c.dx, (T*)c.dxb, c.D, c.C, c.cos_s, c.drop, c.linear, c.pool_mean, c.compact, amax_out, amax_in,
                         n_amax, c.gscale, texp, c.arc, c.cos_y, c.label);
    };
    if (c.gscale) pass(c.amax_ws, nullptr, 0);                    // the amax pass: every image's largest |stream gradient| into amax_ws [B]
    pass(nullptr, c.gscale ? c.amax_ws : nullptr, c.B);           // the main pass: the stores, times the power of two those maxima select
  });
}

static int head_bwd_launch(const HeadCall& c) {
  head_for_kind(c.kind, [&](auto kind) {
    constexpr int KIND = decltype(kind)::value;
    if (c.C <= HEAD_TILED_C) {
      head_bwd_rows<KIND, false>(c, c.Wn);
      return;
    }
    // class-tiled: d e-hat once into amax_ws [B, B + B D), then the per-image kernel without its class loop
    float* de = c.amax_ws + c.B;
    if (c.dlogits) {
      const int nblk = ((c.B + HD_BM - 1) / HD_BM) * ((c.D + HD_BN - 1) / HD_BN);
      hipLaunchKernelGGL((head_de_tiled_kernel<KIND>), dim3(nblk), dim3(256), 0, c.st, c.dlogits, c.Wn, c.label, (const float*)c.cos_y, de, c.B, c.D,
                         c.C, c.cos_s, c.arc);
    }
    head_bwd_rows<KIND, true>(c, de);
  });
  return check_launch(c.who);
}

extern "C" int gsl_head_bwd(const float* dlogits, const float* demb, const void* x, int x_dtype, int T, const float* gamma,
                            const float* mean, const float* rstd, const float* emb, const float* Wn, void* dx, void* dxb,
                            int B, int D, int C, float cos_s, int dtype, int stream_dtype, float p_drop, uint64_t seed, uint32_t site,
                            int linear_head, int pool_mean, int compact, float* gscale, float* amax_ws, int target_exp, gsl_stream_t s) {
  HeadCall c{};      // the margin form with the CosFace kind, no cos_y and no label
  c.who = __func__; c.dlogits = dlogits; c.demb = demb; c.x = x; c.x_dtype = x_dtype; c.T = T; c.gamma = gamma; c.mean = const_cast<float*>(mean);
  c.rstd = const_cast<float*>(rstd); c.emb = const_cast<float*>(emb); c.Wn = Wn; c.dx = dx; c.dxb = dxb; c.B = B; c.D = D; c.C = C; c.cos_s = cos_s;
  c.dtype = dtype; c.stream_dtype = stream_dtype; c.drop = make_drop(p_drop, seed, site); c.linear = linear_head; c.pool_mean = pool_mean;
  c.compact = compact; c.gscale = gscale; c.amax_ws = amax_ws; c.target_exp = target_exp; c.st = as_stream(s);
  head_set_kind(c, HEAD_COSFACE, 0.0, 0);
  GSL_TRY(head_bwd_check(c));
  return head_bwd_launch(c);
}

extern "C" int gsl_head_bwd_margin(const float* dlogits, const float* demb, const void* x, int x_dtype, int T, const float* gamma,
                                   const float* mean, const float* rstd, const float* emb, const float* Wn, void* dx, void* dxb,
                                   int B, int D, int C, float cos_s, int dtype, int stream_dtype, float p_drop, uint64_t seed, uint32_t site,
                                   int linear_head, int pool_mean, int compact, float* gscale, float* amax_ws, int target_exp, int head_kind,
                                   double m, int easy_margin, const float* cos_y, const int64_t* label, gsl_stream_t s) {
  HeadCall c{};
  c.who = __func__; c.dlogits = dlogits; c.demb = demb; c.x = x; c.x_dtype = x_dtype; c.T = T; c.gamma = gamma; c.mean = const_cast<float*>(mean);
  c.rstd = const_cast<float*>(rstd); c.emb = const_cast<float*>(emb); c.Wn = Wn; c.dx = dx; c.dxb = dxb; c.B = B; c.D = D; c.C = C; c.cos_s = cos_s;
  c.dtype = dtype; c.stream_dtype = stream_dtype; c.drop = make_drop(p_drop, seed, site); c.linear = linear_head; c.pool_mean = pool_mean;
  c.compact = compact; c.gscale = gscale; c.amax_ws = amax_ws; c.target_exp = target_exp; c.cos_y = const_cast<float*>(cos_y); c.label = label;
  c.st = as_stream(s);
  head_set_kind(c, head_kind, m, easy_margin);
  GSL_TRY(head_bwd_check(c));
  return head_bwd_launch(c);
}

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

// The class-tiled form, C > HEAD_TILED_C: d What [C, D] = G^T . e-hat on v_mfma_f32_16x16x4_f32, the instruction and
// the summation rule of head_logits_tiled_kernel / head_de_tiled_kernel. A workgroup owns a tile of CT = 16 NI classes and ALL D columns
// (NW waves of 16 NJ columns each), so the row-wise epilogue of the cosine heads runs on the accumulators and the call stays one launch
// without a workspace. It walks the batch in K tiles of BK images, ascending: every element of dW is ONE chain from 0 over ascending b
// with zero-filled padding to the K tile's end — no split of B over waves or workgroups, no atomics; row c depends on neither C nor CT.
// The per-class kernel read all of emb per TWO classes; this one reads it per 16 or 64, and dlogits (the large operand) exactly once:
// workgroup i owns the columns [CT i, CT i + CT) of every dlogits row.
//   staging  wave w loads the rows w, w + NW, ... of the K tile, a lane the float4 chunks 4 lane + 256 q of a row: the row's squared norm is
//            a sum over the lane's chunks (q ascending) and one wave reduction, an order fixed by D alone, taken from the registers the row
//            is staged through (emb is read once). e-hat = emb / max(||emb||, 1e-12) is what goes to LDS; the linear kind stores emb as is.
//   G        cs * dlogits, the ArcFace label column times arc_dphi(cos_y[b]): head_de_tiled_kernel's expressions. Rows of dlogits start at
//            any dword (C is arbitrary): scalar loads, 16 NI consecutive classes per image.
//   loads    unconditional on clamped in-bounds addresses, zeros selected when the registers are staged (see head_logits_tiled_kernel);
//            the next K tile's loads are issued before this tile's MFMAs.
//   dbias    (linear) the threads of the first CT columns add the tile's G column in image order: the same ascending chain.
//   epilogue head_wgrad_kernel's expression, a wave per class row (through the e-hat panel): ||W_c||^2 and W_c . d What_c are a lane's
//            columns lane, lane + 64, ... in ascending order and one wave reduction, an order fixed by D alone.
// Preconditions, checked by the caller: D % 4 == 0 and emb 16-byte aligned (the float4 loads of emb). W, dlogits and dW are scalar accesses.
// No LDS array is sized by B or C.
template <int KIND, int NW, int NI, int NJ>
__global__ __launch_bounds__(NW * 64) void head_wgrad_tiled_kernel(const float* __restrict__ dlogits, const float* __restrict__ emb,
                                                                  const float* __restrict__ W, const int64_t* __restrict__ label,
                                                                  const float* __restrict__ cos_y, float* __restrict__ dW,
                                                                  float* __restrict__ dbias, int B, int C, int D, float cs, ArcMargin arc) {
  constexpr int NT = NW * 64, CT = 16 * NI, DW = NW * 16 * NJ;      // threads, classes and columns of the workgroup (DW >= D)
  constexpr int BK = DW > 512 ? 8 : 16;                             // images per K tile (the e-hat panel stays at 33 KB)
  constexpr int LDE = DW + 16;                                      // row stride of the [image][column] panel: 16 fc + fr covers the 64 banks once
  constexpr int LDG = CT == 16 ? 16 : CT + 16;                      // ... and of the [image][class] panel
  constexpr int RPW = BK / NW, NQ = (DW + 255) / 256;               // staging of e-hat: rows per wave, float4 chunks per lane and row
  constexpr int NG = (BK * CT + NT - 1) / NT;                       // staging of G: elements per thread
  constexpr bool GFULL = NG * NT == BK * CT;
  constexpr int PR = DW > 512 ? 8 : 16, LDP = DW + 4, NC = DW / 64;  // epilogue: class rows per pass through the panel, their stride (16 fc + fr
  static_assert(PR * LDP <= BK * LDE, "the epilogue reuses Es");     // over a fragment store), 64-column chunks of a row
  __shared__ __attribute__((aligned(16))) float Es[BK * LDE];
  __shared__ float Gs[BK * LDG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t c0 = (size_t)blockIdx.x * CT;
  auto lastc = [&](size_t c) { return c < (size_t)C ? c : (size_t)C - 1; };      // the class, or the last one: a clamped row
  struct Regs {      // a K tile on its way from memory to LDS
    float4 re[RPW][NQ];
    float rg[NG], rcy[NG];
    int64_t ry[NG];
  };
  auto fetch = [&](Regs& R, int k0) {
    auto& re = R.re; auto& rg = R.rg; auto& rcy = R.rcy; auto& ry = R.ry;
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const float* er = emb + (size_t)min(k0 + wave + NW * i, B - 1) * D;
#pragma unroll
      for (int q = 0; q < NQ; ++q) re[i][q] = *reinterpret_cast<const float4*>(er + min(4 * lane + 256 * q, D - 4));
    }
#pragma unroll
    for (int i = 0; i < NG; ++i) {
      const int idx = tid + NT * i, b = min(k0 + min(idx / CT, BK - 1), B - 1);
      rg[i] = dlogits[(size_t)b * C + lastc(c0 + idx % CT)];
      if constexpr (KIND == HEAD_ARCFACE) { ry[i] = label[b]; rcy[i] = cos_y[b]; }
    }
  };
  // registers -> LDS: zeros for what lies outside the tensors, the row norms, the margin's derivative
  auto stage = [&](Regs& R, int k0) {
    auto& re = R.re; auto& rg = R.rg; auto& rcy = R.rcy; auto& ry = R.ry;
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const int r = wave + NW * i;
      const bool live = k0 + r < B;
      float ss = 0.f;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {      // (D % 4 == 0: a float4 lies inside the row or outside it)
        const float4 v = keep4(live && 4 * lane + 256 * q < D, re[i][q]);
        re[i][q] = v;
        ss += v.x * v.x; ss += v.y * v.y; ss += v.z * v.z; ss += v.w * v.w;
      }
      if constexpr (KIND != HEAD_LINEAR) {
        const float inv = 1.0f / fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
#pragma unroll
        for (int q = 0; q < NQ; ++q) re[i][q] = make_float4(re[i][q].x * inv, re[i][q].y * inv, re[i][q].z * inv, re[i][q].w * inv);
      }
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        if (4 * lane + 256 * q < DW) *reinterpret_cast<float4*>(&Es[r * LDE + 4 * lane + 256 * q]) = re[i][q];
    }
#pragma unroll
    for (int i = 0; i < NG; ++i) {
      const int idx = tid + NT * i, r = idx / CT, cl = idx % CT;
      if (GFULL || idx < BK * CT) {
        const size_t c = c0 + cl;
        const bool live = k0 + r < B && c < (size_t)C;
        float v = live ? rg[i] : 0.f;
        if constexpr (KIND != HEAD_LINEAR) v *= cs;
        if constexpr (KIND == HEAD_ARCFACE) { if (live && ry[i] == (int64_t)c) v *= arc_dphi(rcy[i], arc); }
        Gs[r * LDG + cl] = v;
      }
    }
  };
  head_f32x4_t acc[NI][NJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = head_f32x4_t{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  const int fr = lane & 15, fc = lane >> 4;
  const int wcol = wave * 16 * NJ;
  const int nk = (B + BK - 1) / BK;
  auto tile = [&](Regs& R, int kt) {
    stage(R, kt * BK);
    wg_barrier_lds();
    if (kt + 1 < nk) fetch(R, (kt + 1) * BK);      // the next tile's loads fly under this tile's MFMAs
#pragma unroll
    for (int ks = 0; ks < BK / 4; ++ks) {
      float gf[NI], ef[NJ];
#pragma unroll
      for (int i = 0; i < NI; ++i) gf[i] = Gs[(ks * 4 + fc) * LDG + i * 16 + fr];
#pragma unroll
      for (int j = 0; j < NJ; ++j) ef[j] = Es[(ks * 4 + fc) * LDE + wcol + j * 16 + fr];
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(gf[i], ef[j], acc[i][j], 0, 0, 0);
    }
    if constexpr (KIND == HEAD_LINEAR) {
      if (dbias && tid < CT) {
#pragma unroll
        for (int k = 0; k < BK; ++k) bsum += Gs[k * LDG + tid];
      }
    }
    wg_barrier_lds();      // every wave has read the panels before the next tile overwrites them
  };
  Regs r0;
  fetch(r0, 0);
  for (int kt = 0; kt < nk; ++kt) tile(r0, kt);
  if constexpr (KIND == HEAD_LINEAR) {
    if (dbias && tid < CT && c0 + tid < (size_t)C) dbias[c0 + tid] = bsum;
  }
  // Epilogue. A lane holds the classes 4 fc + r, column fr of every fragment; the rows go through the (now free) e-hat panel, PR classes at
  // a time, so that a WAVE finishes a class row with its lanes over the columns: the row's two sums are a lane's columns (ascending) and
  // one wave reduction, W is read once, and W loads / dW stores are whole 256-byte runs of a row. (Finishing the rows on the accumulators
  // — 64-byte runs, two passes over W, the sums across waves through LDS — spilled 60 - 150 registers at 64 classes x 512 / 1024 columns.)
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int h = 0; h < 16 / PR; ++h) {
      if (PR == 16 || (fc >> 1) == h) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int j = 0; j < NJ; ++j) Es[((4 * fc + r) & (PR - 1)) * LDP + wcol + j * 16 + fr] = acc[i][j][r];
      }
      wg_barrier_lds();
      for (int rr = wave; rr < PR; rr += NW) {
        const size_t c = c0 + i * 16 + h * PR + rr;
        if (c >= (size_t)C) break;      // (uniform over the wave; the barriers are outside this loop)
        float f[NC], w[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) {
          f[q] = Es[rr * LDP + lane + 64 * q];
          if constexpr (KIND != HEAD_LINEAR) w[q] = W[c * D + min(lane + 64 * q, D - 1)];
        }
        if constexpr (KIND == HEAD_LINEAR) {
#pragma unroll
          for (int q = 0; q < NC; ++q)
            if (lane + 64 * q < D) dW[c * D + lane + 64 * q] = f[q];
        } else {
          float ss = 0.f, dot = 0.f;
#pragma unroll
          for (int q = 0; q < NC; ++q) {
            w[q] = lane + 64 * q < D ? w[q] : 0.f;
            ss += w[q] * w[q];
            dot += w[q] * f[q];
          }
          const float raw = sqrtf(wave_sum(ss));
          dot = wave_sum(dot);
          const float nrm = fmaxf(raw, 1e-12f);
#pragma unroll
          for (int q = 0; q < NC; ++q)
            if (lane + 64 * q < D) dW[c * D + lane + 64 * q] = (raw >= 1e-12f) ? (f[q] - (w[q] / nrm) * (dot / nrm)) / nrm : f[q] / nrm;
        }
      }
      wg_barrier_lds();      // the panel is read before the next PR rows overwrite it
    }
}

// Which tile (B = 1024, D = 512, CosFace, microseconds, profiles/head_large_c.md): 16 classes on 8 waves 167 / 221 / 224 / 296 / 435 at
// C = 8192 / 10 572 / 12 288 / 16 384 / 24 576; 64 classes on 4 waves 262 up to 16 384 (at most one workgroup per CU: the time of one
// workgroup), then 394, and 1196 at 93 431, where the 16-class tile (then still on 4 waves) took 1616: 11.7 GB of emb reads from L2.
constexpr int HWT_WIDE_C = 16384;      // classes from which a workgroup takes 64 and not 16

// The rule of gsl_head_wgrad: (C, D, alignment of emb) -> the form and its tile constants, as template arguments:
//   tiled(NW, NI, NJ)   head_wgrad_tiled_kernel: NW waves, 16 NI classes a workgroup, 16 NJ columns a wave (NW 16 NJ >= D)
//   per_class(CT, KM)   head_wgrad_kernel: CT classes a workgroup, KM columns a lane (64 KM >= D)
template <typename FT, typename FC>
static void head_wgrad_rule(int C, int D, const float* emb, FT&& tiled, FC&& per_class) {
  // Above HEAD_TILED_C classes the class-tiled kernel, where its loads are legal: D % 4 == 0 and emb 16-byte aligned. A call that does not
  // meet them is not refused (the entry point always took any C and any D <= 1024): it runs the per-class kernel below, as it always did.
  if (C > HEAD_TILED_C && (D % 4) == 0 && (((uintptr_t)emb) & 15) == 0) {
    if (C >= HWT_WIDE_C) {      // 64 classes a workgroup
      if (D <= 128) tiled(HeadInt<4>{}, HeadInt<4>{}, HeadInt<2>{});
      else if (D <= 256) tiled(HeadInt<4>{}, HeadInt<4>{}, HeadInt<4>{});
      else if (D <= 512) tiled(HeadInt<4>{}, HeadInt<4>{}, HeadInt<8>{});
      else tiled(HeadInt<8>{}, HeadInt<4>{}, HeadInt<8>{});
    } else {      // 16 classes a workgroup on 8 waves: few workgroups (65 at C = 1025), so each brings two waves per SIMD of its own to cover
                  // the LDS and barrier latencies of a K tile (4 waves: 150 us at C = 1025 and 2048; 8 waves: 107 / 109 us)
      if (D <= 128) tiled(HeadInt<8>{}, HeadInt<1>{}, HeadInt<1>{});
      else if (D <= 256) tiled(HeadInt<8>{}, HeadInt<1>{}, HeadInt<2>{});
      else if (D <= 512) tiled(HeadInt<8>{}, HeadInt<1>{}, HeadInt<4>{});
      else tiled(HeadInt<8>{}, HeadInt<1>{}, HeadInt<8>{});
    }
    return;
  }
  // A workgroup per class up to 256 classes. The cosine heads need every row's norm, so a workgroup reads all of emb whatever part of
  // dW it owns: splitting the columns over more workgroups would shorten no wave's chain of rounds and multiply the L2 traffic, and
  // splitting the batch would need a second pass or float atomics. Many classes: two per workgroup, which read every row once for both.
  if (C <= 256) {
    if (D <= 256) per_class(HeadInt<1>{}, HeadInt<4>{});
    else if (D <= 512) per_class(HeadInt<1>{}, HeadInt<8>{});
    else per_class(HeadInt<1>{}, HeadInt<16>{});
  } else {
    if (D <= 256) per_class(HeadInt<2>{}, HeadInt<4>{});
    else if (D <= 512) per_class(HeadInt<2>{}, HeadInt<8>{});
    else per_class(HeadInt<2>{}, HeadInt<16>{});
  }
}

static int head_wgrad_launch(const HeadCall& c) {
  head_for_kind<true>(c.kind, [&](auto kind) {
    constexpr int KIND = decltype(kind)::value;
    head_wgrad_rule(
        c.C, c.D, c.emb,
        [&](auto nw, auto ni, auto nj) {
          constexpr int NW = decltype(nw)::value, NI = decltype(ni)::value, NJ = decltype(nj)::value;
          hipLaunchKernelGGL((head_wgrad_tiled_kernel<KIND, NW, NI, NJ>), dim3((c.C - 1) / (16 * NI) + 1), dim3(64 * NW), 0, c.st, c.dlogits,
                             (const float*)c.emb, c.W, c.label, (const float*)c.cos_y, c.dW, c.dbias, c.B, c.C, c.D, c.cos_s, c.arc);
        },
        [&](auto ct, auto km) {
          constexpr int CT = decltype(ct)::value, KM = decltype(km)::value;
          hipLaunchKernelGGL((head_wgrad_kernel<KIND, CT, KM>), dim3((c.C + CT - 1) / CT), dim3(HW_WAVES * 64), 0, c.st, c.dlogits,
                             (const float*)c.emb, c.W, c.label, (const float*)c.cos_y, c.dW, c.dbias, c.B, c.C, c.D, c.cos_s, c.arc);
        });
  });
  return check_launch(c.who);
}

extern "C" int gsl_head_wgrad(const float* dlogits, const float* emb, const float* W, const int64_t* label, const float* cos_y, float* dW,
                              float* dbias, int B, int C, int D, int head_kind, float cos_s, double m, int easy_margin, gsl_stream_t s) {
  GSL_CHECK_ARG(head_kind == HEAD_COSFACE || head_kind == HEAD_ARCFACE || head_kind == HEAD_LINEAR, "head_kind: 0 (CosFace), 1 (ArcFace) or 2 (linear)");
  GSL_CHECK_ARG(dlogits && emb && dW && B > 0 && C > 0, "null/size");
  GSL_CHECK_ARG(head_kind == HEAD_LINEAR || W, "the cosine heads read W");
  GSL_CHECK_ARG(D > 0 && D <= HEAD_MAXD, "D <= 1024");
  GSL_CHECK_ARG(head_kind != HEAD_ARCFACE || (label && cos_y), "ArcFace needs label and cos_y [B]");
  GSL_CHECK_ARG(head_kind == HEAD_LINEAR || !dbias, "dbias belongs to the linear head");
  HeadCall c{};
  c.who = __func__; c.dlogits = dlogits; c.emb = const_cast<float*>(emb); c.W = W; c.label = label; c.cos_y = const_cast<float*>(cos_y); c.dW = dW;
  c.dbias = dbias; c.B = B; c.C = C; c.D = D; c.cos_s = head_kind == HEAD_LINEAR ? 1.0f : cos_s; c.st = as_stream(s);
  head_set_kind(c, head_kind, m, easy_margin);
  return head_wgrad_launch(c);
}
