// train.hip — libgslora_train.so: the kernels that train weights of the backbone (include/gslora_train.h).
//   gst_wgrad       dW[n,k] (+)= c * sum_m Y[m,n] X[m,k], db[n] (+)= c * sum_m Y[m,n]: the weight / bias gradient of an nn.Linear whose input X
//                   and output gradient Y are both wide (the FFN linears, reference vit_pytorch_face/vit_face.py:330-333, trained by
//                   train/train_own_forget_cl.py:432-439 --only_ffn)
//   gst_reg_quad_*  sum(importance * (p - task_param) ** 2) and its gradient (reference engine_cl.py:455-457, get_reg_loss)
// A second product library: its own error string; nothing shared with libgslora_hip.so but the headers (gsl_common.h and the public ones),
// and with the other side libraries gsl_chunks.h: the chunked sum gst_reg_quad_fwd is written over.
#include "gsl_chunks.h"

#include "../../include/gslora_train.h"

using namespace gsl;

namespace gsl { thread_local char g_err[512] = {0}; }
extern "C" const char* gst_last_error(void) { return gsl::g_err; }

// =====================================================================================
// gst_wgrad. The contraction runs over m, the slow index of both row-major operands: slabs of WgFmt::KS rows of Y and X go through LDS as
// full coalesced rows, and the MFMA fragments are gathered from there — 16-bit formats with gfx950's LDS transpose read (the
// two-dimensional generalisation of lgm_block in lora.hip: there U has at most 64 columns, here both operands are tiles of 128), f32 with
// plain reads (v_mfma_f32_16x16x4_f32 takes one element per lane: 16 consecutive columns of one slab row are 16 consecutive lanes).
// One workgroup = 4 waves = one 128 x 128 output tile of one row split, a wave owns 64 x 64 of it (4 x 4 fragments, 64 accumulator
// registers). The row-slab loop is double-buffered in LDS and the global loads run two slabs ahead of the MFMAs.
// =====================================================================================
constexpr int WG_TILE = 128;          // output tile edge (n and k)
constexpr int WG_SLAB = 32;           // granularity of a row split
constexpr int WG_MIN_SLABS = 4;       // a split holds at least 128 rows (unless M has fewer): each split costs one [N, K] f32 slab of partials
constexpr int WG_TARGET = 1024;       // workgroups wanted: 256 CUs four times over

typedef short wg_v4s_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) wg_v4s_t* wg_lds_v4s_p;
typedef __attribute__((ext_vector_type(8))) __bf16 wg_bf16x8_t;
typedef __attribute__((ext_vector_type(8))) _Float16 wg_f16x8_t;
typedef __attribute__((ext_vector_type(4))) float wg_f32x4_t;

// FMT = the gsl_dtype value: 0 f32, 1 bf16, 2 fp16
template <int FMT> struct WgFmt {
  static constexpr int ES = FMT == GSL_F32 ? 4 : 2;       // bytes per element
  static constexpr int KS = FMT == GSL_F32 ? 16 : 32;     // rows of a slab
  static constexpr int CH = 16 / ES;                      // elements of a 16-byte chunk
  static constexpr int CPR = WG_TILE / CH;                // chunks per slab row
  // LDS row length in elements. 16-bit: 136 = 68 dwords, the sixteen rows of a transpose read start at sixteen different multiples of 4 dwords
  // (mod 64) and each spans 8: every bank is touched exactly twice by the 64 x 8 bytes of the read, its two-pass minimum (lgm_uld in lora.hip).
  // f32: 144 dwords, the four slab rows of a fragment read start 16 banks apart: conflict-free. Rows stay 16-byte aligned.
  static constexpr int LD = FMT == GSL_F32 ? WG_TILE + 16 : WG_TILE + 8;
  static constexpr int BUF = KS * LD * ES;                // bytes of one buffer of one operand
};

template <int FMT>
__device__ __forceinline__ float wg_elem(const unsigned char* p) {
  if constexpr (FMT == GSL_F32) return *reinterpret_cast<const float*>(p);
  else if constexpr (FMT == GSL_BF16) return bf2f(*reinterpret_cast<const bf16_t*>(p));
  else return (float)*reinterpret_cast<const _Float16*>(p);
}

// part [nsplit][N][K], dbpart [nsplit][N] (written by the k-tile-0 workgroups from the Y slabs they have staged; nullptr: no bias gradient)
template <int FMT>
__global__ __launch_bounds__(256) void wgrad_partial_kernel(const unsigned char* __restrict__ Y, long ldy, const unsigned char* __restrict__ X, long ldx,
                                                            float* __restrict__ part, float* __restrict__ dbpart, int M, int N, int K,
                                                            int tiles_k, int tiles, int nsplit, int rps) {
  using F = WgFmt<FMT>;
  constexpr int ES = F::ES, KS = F::KS, CH = F::CH, CPR = F::CPR, LD = F::LD, BUF = F::BUF;
  __shared__ __attribute__((aligned(16))) unsigned char ys[2 * BUF];
  __shared__ __attribute__((aligned(16))) unsigned char xs[2 * BUF];
  // XCD-aware order: hardware deals workgroup ids round-robin to the 8 XCDs; the logical ids an XCD receives are made consecutive, and
  // consecutive logical ids are the tiles of ONE row split — they read the same rows of Y and X, which then cross HBM once per XCD and are
  // shared through its L2.
  const int total = tiles * nsplit, chunk = (total + 7) / 8;
  const int logical = ((int)blockIdx.x % 8) * chunk + (int)blockIdx.x / 8;
  if (logical >= total) return;      // (the whole workgroup: before any barrier)
  const int split = logical / tiles, tile = logical - split * tiles;
  const int n0 = (tile / tiles_k) * WG_TILE, k0 = (tile % tiles_k) * WG_TILE;
  const int r0 = split * rps, r1 = min(M, r0 + rps);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = (wave >> 1) * 64, wk = (wave & 1) * 64;      // this wave's 64 x 64 piece of the tile
  const bool active = n0 + wn < N && k0 + wk < K;             // N, K are multiples of 64: a wave's piece is inside or outside as a whole
  const bool do_db = dbpart != nullptr && k0 == 0 && tid < WG_TILE && n0 + tid < N;

  // this thread's two 16-byte chunks of a slab of each operand: chunk c = tid + 256 i sits in slab row c / CPR at column (c % CPR) * CH
  const int row_a = tid / CPR, row_b = (tid + 256) / CPR, col = (tid % CPR) * CH;      // (256 % CPR == 0: both chunks share the column)
  const bool ycol = n0 + col < N, xcol = k0 + col < K;
  const unsigned char* yp = Y + ((size_t)n0 + col) * ES;
  const unsigned char* xp = X + ((size_t)k0 + col) * ES;
  // Two register sets: the loads of slab i + 2 are issued before the MFMAs of slab i, while slab i + 1 waits in the other set for its turn
  // in LDS — two slabs of global loads in flight per workgroup (one slab of MFMAs covers a fraction of the memory latency under load).
  struct Slab { uint4 ya, yb, xa, xb; };
  Slab R0, R1;
  auto gload = [&](Slab& R, int rb) {      // (a slab past the split: no load is issued, the registers are zeros)
    R.ya = R.yb = R.xa = R.xb = make_uint4(0, 0, 0, 0);
    const int ma = rb + row_a, mb = rb + row_b;
    if (ma < r1 && ycol) R.ya = *reinterpret_cast<const uint4*>(yp + (size_t)ma * ldy * ES);
    if (mb < r1 && ycol) R.yb = *reinterpret_cast<const uint4*>(yp + (size_t)mb * ldy * ES);
    if (ma < r1 && xcol) R.xa = *reinterpret_cast<const uint4*>(xp + (size_t)ma * ldx * ES);
    if (mb < r1 && xcol) R.xb = *reinterpret_cast<const uint4*>(xp + (size_t)mb * ldx * ES);
  };
  auto lstore = [&](int buf, const Slab& R) {
    *reinterpret_cast<uint4*>(&ys[buf * BUF + (row_a * LD + col) * ES]) = R.ya;
    *reinterpret_cast<uint4*>(&ys[buf * BUF + (row_b * LD + col) * ES]) = R.yb;
    *reinterpret_cast<uint4*>(&xs[buf * BUF + (row_a * LD + col) * ES]) = R.xa;
    *reinterpret_cast<uint4*>(&xs[buf * BUF + (row_b * LD + col) * ES]) = R.xb;
  };
  wg_f32x4_t acc[4][4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[t][b] = wg_f32x4_t{0.f, 0.f, 0.f, 0.f};
  float dbs = 0.f;
  const int g = lane >> 4, i16 = lane & 15;
  const int trow = 4 * g + (i16 >> 2), tcol = (i16 & 3) * 4;       // this lane's piece of a 4 x 16 block (transpose-read address)

  // the MFMAs (and the bias column sums) of the slab in LDS buffer `buf`
  auto compute = [&](int buf) {
    const unsigned char* yb = ys + buf * BUF;
    const unsigned char* xb = xs + buf * BUF;
    if (active) {
      if constexpr (FMT == GSL_F32) {
#pragma unroll
        for (int s = 0; s < KS / 4; ++s) {
          const int row = 4 * s + g;
          float bv[4];
#pragma unroll
          for (int b = 0; b < 4; ++b) bv[b] = *reinterpret_cast<const float*>(xb + (row * LD + wk + b * 16 + i16) * 4);
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const float av = *reinterpret_cast<const float*>(yb + (row * LD + wn + t * 16 + i16) * 4);
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[t][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[b], acc[t][b], 0, 0, 0);
          }
        }
      } else {
        union Frag { wg_v4s_t h[2]; wg_bf16x8_t v; wg_f16x8_t w; };
        Frag bf[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const unsigned char* p = xb + (trow * LD + wk + b * 16 + tcol) * 2;
          bf[b].h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wg_lds_v4s_p)(p));
          bf[b].h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wg_lds_v4s_p)(p + 16 * LD * 2));
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          Frag af;
          const unsigned char* p = yb + (trow * LD + wn + t * 16 + tcol) * 2;
          af.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wg_lds_v4s_p)(p));
          af.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wg_lds_v4s_p)(p + 16 * LD * 2));
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            if constexpr (FMT == GSL_F16) acc[t][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af.w, bf[b].w, acc[t][b], 0, 0, 0);
            else acc[t][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af.v, bf[b].v, acc[t][b], 0, 0, 0);
          }
        }
      }
    }
    if (do_db) {      // column tid of the staged Y slab, rows ascending (rows past the split are zeros)
#pragma unroll 8
      for (int rr = 0; rr < KS; ++rr) dbs += wg_elem<FMT>(yb + (rr * LD + tid) * ES);
    }
  };
  gload(R0, r0);
  gload(R1, r0 + KS);
  lstore(0, R0);
  wg_barrier_lds();
  for (int rb = r0;;) {      // two slabs per trip: the roles of the register sets and of the LDS buffers swap
    gload(R0, rb + 2 * KS);
    compute(0);
    if (rb + KS < r1) lstore(1, R1);
    wg_barrier_lds();
    rb += KS;
    if (rb >= r1) break;
    gload(R1, rb + 2 * KS);
    compute(1);
    if (rb + KS < r1) lstore(0, R0);
    wg_barrier_lds();
    rb += KS;
    if (rb >= r1) break;
  }
  // acc[t][b][r] = sum_m Y[m, n0 + wn + 16 t + 4 g + r] * X[m, k0 + wk + 16 b + (lane & 15)]
  if (active) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + wn + t * 16 + 4 * g + r;
        float* p = part + ((size_t)split * N + n) * K + k0 + wk + i16;
#pragma unroll
        for (int b = 0; b < 4; ++b) p[b * 16] = acc[t][b][r];
      }
  }
  if (do_db) dbpart[(size_t)split * N + n0 + tid] = dbs;
}

// splits in ascending order; c applied; store or accumulate. Elements [0, N*K) are dW, [N*K, N*K + N) are db (when asked for).
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, const float* __restrict__ dbpart, float* dW, long ldw,
                                                           float* db, int N, int K, int nsplit, int accumulate, const float* __restrict__ gscale) {
  const int NK = N * K;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= NK + (db ? N : 0)) return;
  const float* p;
  size_t stride;
  float* out;
  if (idx < NK) {
    const int n = idx / K, k = idx - n * K;
    p = part + idx; stride = (size_t)NK; out = dW + (size_t)n * ldw + k;
  } else {
    p = dbpart + (idx - NK); stride = (size_t)N; out = db + (idx - NK);
  }
  float s = 0.f;
  for (int sp = 0; sp < nsplit; ++sp) s += p[(size_t)sp * stride];
  if (gscale) s *= gscale[1];      // loss-scaled backward (fp16 operands): divide the power-of-two scale out, exactly
  *out = accumulate ? (*out + s) : s;
}

// ------------------------------------------------------------------ host side of gst_wgrad
struct WgPlan { int tile_n, tile_k, tiles_n, tiles_k, nsplit, rps; };
static WgPlan wg_plan(int M, int N, int K) {
  WgPlan p{};
  p.tile_n = p.tile_k = WG_TILE;
  p.tiles_n = (N + WG_TILE - 1) / WG_TILE;
  p.tiles_k = (K + WG_TILE - 1) / WG_TILE;
  const int tiles = p.tiles_n * p.tiles_k;
  const int slabs = (M + WG_SLAB - 1) / WG_SLAB;
  const int want = max(1, min(max(1, WG_TARGET / tiles), (slabs + WG_MIN_SLABS - 1) / WG_MIN_SLABS));
  p.rps = ((slabs + want - 1) / want) * WG_SLAB;
  p.nsplit = (M + p.rps - 1) / p.rps;
  return p;
}
static int wg_check_shape(const char* who, int M, int N, int K, int dtype) {
  GSL_CHECK_ARG_AS(who, dtype == GSL_F32 || dtype == GSL_BF16 || dtype == GSL_F16, "dtype (GSL_F32, GSL_BF16 or GSL_F16)");
  GSL_CHECK_ARG_AS(who, M >= 1, "M >= 1");
  GSL_CHECK_ARG_AS(who, N >= 64 && (N % 64) == 0, "N % 64 == 0");
  GSL_CHECK_ARG_AS(who, K >= 64 && (K % 64) == 0, "K % 64 == 0");
  GSL_CHECK_ARG_AS(who, (long)N * K + N < (1L << 31), "N * K + N < 2^31");
  return GSL_OK;
}

extern "C" long gst_wgrad_ws_elems(int M, int N, int K, int dtype) {
  if (wg_check_shape(__func__, M, N, K, dtype) != GSL_OK) return -1;
  return (long)wg_plan(M, N, K).nsplit * ((long)N * K + N);
}

extern "C" int gst_wgrad_plan(int M, int N, int K, int dtype, int* tile_n, int* tile_k, int* nsplit, int* rows_per_split) {
  GSL_TRY(wg_check_shape(__func__, M, N, K, dtype));
  GSL_CHECK_ARG(tile_n && tile_k && nsplit && rows_per_split, "null output pointer");
  const WgPlan p = wg_plan(M, N, K);
  *tile_n = p.tile_n; *tile_k = p.tile_k; *nsplit = p.nsplit; *rows_per_split = p.rps;
  return GSL_OK;
}

extern "C" int gst_wgrad(const void* Y, long ldy, const void* X, long ldx, float* dW, long ldw, float* db, int M, int N, int K, int dtype,
                         int accumulate, float* ws, const float* gscale, gsl_stream_t s) {
  GSL_TRY(wg_check_shape(__func__, M, N, K, dtype));
  GSL_CHECK_ARG(Y && X && dW, "null operand or output");
  GSL_CHECK_ARG(ws, "null ws");
  GSL_CHECK_ARG(ldy >= N, "ldy >= N");
  GSL_CHECK_ARG(ldx >= K, "ldx >= K");
  GSL_CHECK_ARG(ldw >= K, "ldw >= K");
  const long es = dtype == GSL_F32 ? 4 : 2;
  GSL_CHECK_ARG((reinterpret_cast<uintptr_t>(Y) % 16) == 0 && (ldy * es) % 16 == 0, "rows of Y 16-byte aligned");
  GSL_CHECK_ARG((reinterpret_cast<uintptr_t>(X) % 16) == 0 && (ldx * es) % 16 == 0, "rows of X 16-byte aligned");
  GSL_CHECK_ARG((reinterpret_cast<uintptr_t>(dW) % 4) == 0 && (reinterpret_cast<uintptr_t>(ws) % 4) == 0, "f32 pointers 4-byte aligned");
  const WgPlan p = wg_plan(M, N, K);
  const int tiles = p.tiles_n * p.tiles_k, total = tiles * p.nsplit;
  const int grid = ((total + 7) / 8) * 8;
  float* dbpart = db ? ws + (size_t)p.nsplit * N * K : nullptr;
  hipStream_t st = as_stream(s);
  const unsigned char* Yb = static_cast<const unsigned char*>(Y);
  const unsigned char* Xb = static_cast<const unsigned char*>(X);
  if (dtype == GSL_F32)
    hipLaunchKernelGGL(wgrad_partial_kernel<GSL_F32>, dim3(grid), dim3(256), 0, st, Yb, ldy, Xb, ldx, ws, dbpart, M, N, K, p.tiles_k, tiles, p.nsplit, p.rps);
  else if (dtype == GSL_BF16)
    hipLaunchKernelGGL(wgrad_partial_kernel<GSL_BF16>, dim3(grid), dim3(256), 0, st, Yb, ldy, Xb, ldx, ws, dbpart, M, N, K, p.tiles_k, tiles, p.nsplit, p.rps);
  else
    hipLaunchKernelGGL(wgrad_partial_kernel<GSL_F16>, dim3(grid), dim3(256), 0, st, Yb, ldy, Xb, ldx, ws, dbpart, M, N, K, p.tiles_k, tiles, p.nsplit, p.rps);
  GSL_TRY(check_launch("gst_wgrad(partial)"));
  const int outs = N * K + (db ? N : 0);
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((outs + 255) / 256), dim3(256), 0, st, ws, dbpart, dW, ldw, db, N, K, p.nsplit, accumulate, gscale);
  return check_launch("gst_wgrad(reduce)");
}

// =====================================================================================
// gst_reg_quad_*: sum_i omega_i (p_i - p0_i)^2 and its gradient. Forward: the fixed partition of gsl_chunks.h, one partial per chunk in
// ws, one reduce launch in ascending chunk order.
// =====================================================================================
__global__ __launch_bounds__(256) void reg_quad_partial_kernel(const float* __restrict__ p, const float* __restrict__ p0, const float* __restrict__ omega,
                                                               long n, long chunk, float* __restrict__ ws) {
  __shared__ float sm[16];
  const long i0 = (long)blockIdx.x * chunk, i1 = min(n, i0 + chunk);
  const float s = chunk_partial(i0, i1, sm, [&](long i) { return quad_term(p, p0, omega, i); });
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void reg_quad_reduce_kernel(const float* __restrict__ ws, int nblk, float* out, int accumulate) {
  __shared__ float sm[16];
  const float s = strided_sum(ws, nblk, sm);
  if (threadIdx.x == 0) out[0] = accumulate ? out[0] + s : s;
}
// g += ((coef * 2) * omega) * (p - p0), every operation rounded on its own
__global__ __launch_bounds__(256) void reg_quad_bwd_kernel(const float* __restrict__ p, const float* __restrict__ p0, const float* __restrict__ omega,
                                                           long n, const float* __restrict__ coef, float* __restrict__ g) {
#pragma clang fp contract(off)      // (HIP's __fmul_rn / __fadd_rn are plain operators: the compiler would fuse them into v_fma)
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float c = coef[0] * 2.0f;
  if (omega) c = c * omega[i];
  const float d = p[i] - p0[i];
  const float t = c * d;
  g[i] = g[i] + t;
}

extern "C" long gst_reg_quad_ws_elems(long n) { return n >= 1 ? chunk_blocks(n) : -1; }

extern "C" int gst_reg_quad_fwd(const float* p, const float* p0, const float* omega, long n, float* out, int accumulate, float* ws,
                                gsl_stream_t s) {
  GSL_CHECK_ARG(p && p0 && out, "null tensor");
  GSL_CHECK_ARG(ws, "null ws");
  GSL_CHECK_ARG(n >= 1, "n >= 1");
  const int nblk = chunk_blocks(n);
  const long chunk = chunk_len(n, nblk);
  hipLaunchKernelGGL(reg_quad_partial_kernel, dim3(nblk), dim3(256), 0, as_stream(s), p, p0, omega, n, chunk, ws);
  GSL_TRY(check_launch("gst_reg_quad_fwd(partial)"));
  hipLaunchKernelGGL(reg_quad_reduce_kernel, dim3(1), dim3(256), 0, as_stream(s), ws, nblk, out, accumulate);
  return check_launch("gst_reg_quad_fwd(reduce)");
}

extern "C" int gst_reg_quad_bwd(const float* p, const float* p0, const float* omega, long n, const float* coef, float* g, gsl_stream_t s) {
  GSL_CHECK_ARG(p && p0 && g && coef, "null tensor");
  GSL_CHECK_ARG(n >= 1 && (n + 255) / 256 < (1L << 31), "n >= 1");
  hipLaunchKernelGGL(reg_quad_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(s), p, p0, omega, n, coef, g);
  return check_launch(__func__);
}
