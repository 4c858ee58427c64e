// reg.hip — libgslora_reg.so: what the L2 / EWC / MAS baselines need around the FFN-training step (include/gslora_reg.h).
//   gsr_importance_acc  omega += grad^2 * len(batch) / len(loader) (EWC) or |grad| / len(loader) (MAS): reference
//                       train/train_own_forget_cl.py:1501-1509 and :1554-1558
//   gsr_sq_mean_*       mean(logits^2) and its gradient, the objective MAS differentiates (train/train_own_forget_cl.py:1548-1549)
//   gsr_reg_multi_*     get_reg_loss (engine_cl.py:449-459) over every term and tensor at once, bit for bit the sequence of gst_reg_quad_*
//                       calls of libgslora_train.so
// A third product library: its own error string; nothing shared with libgslora_hip.so but the headers (gsl_common.h and the public ones),
// and with the other side libraries gsl_chunks.h: gsr_reg_multi_fwd and gst_reg_quad_fwd are the same partition rule, chunk sum and term.
#include "gsl_chunks.h"

#include "../../include/gslora_reg.h"

using namespace gsl;

namespace gsl { thread_local char g_err[512] = {0}; }
extern "C" const char* gsr_last_error(void) { return gsl::g_err; }

// =====================================================================================
// gsr_importance_acc. Memory-bound: 8 bytes read and 4 written per element. The vector body starts at the first element where omega is
// 16-byte aligned (g is aligned there too, or there is no vector body); the elements in front of and behind it go one by one. (Not
// chunk_walk: the split is made on the host from the pointers' residue — the pointers themselves need not be aligned — and the loops are
// grid-stride.)
// =====================================================================================
constexpr int IA_MAX_BLOCKS = 2048;      // 256 CUs eight times over; the loops are grid-stride

__device__ __forceinline__ float ia_term(float g, int kind, float a, float b) {
#pragma clang fp contract(off)
  if (kind == GSR_EWC) {
    const float sq = g * g;
    const float w = sq * a;
    return w / b;
  }
  return fabsf(g) / b;
}

__global__ __launch_bounds__(256) void importance_acc_kernel(float* __restrict__ omega, const float* __restrict__ g, long n, long head,
                                                             long nvec, int kind, float a, float b, const float* __restrict__ guard,
                                                             int* __restrict__ skipped) {
#pragma clang fp contract(off)
  if (guard && !(*guard < 65504.0f)) {      // a saturated (or non-finite) fp16 backward is not squared into the Fisher
    if (skipped && blockIdx.x == 0 && threadIdx.x == 0) skipped[0] = skipped[0] + 1;
    return;
  }
  const long tid = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
  float4* __restrict__ ov = reinterpret_cast<float4*>(omega + head);
  const float4* __restrict__ gv = reinterpret_cast<const float4*>(g + head);
  for (long v = tid; v < nvec; v += stride) {
    float4 o = ov[v];
    const float4 x = gv[v];
    o.x = o.x + ia_term(x.x, kind, a, b);
    o.y = o.y + ia_term(x.y, kind, a, b);
    o.z = o.z + ia_term(x.z, kind, a, b);
    o.w = o.w + ia_term(x.w, kind, a, b);
    ov[v] = o;
  }
  const long body_end = head + 4 * nvec, nscalar = n - 4 * nvec;      // the scalar elements: [0, head) and [body_end, n)
  for (long j = tid; j < nscalar; j += stride) {
    const long i = j < head ? j : body_end + (j - head);
    omega[i] = omega[i] + ia_term(g[i], kind, a, b);
  }
}

extern "C" int gsr_importance_acc(float* omega, const float* g, long n, int kind, float a, float b, const float* guard, int* skipped,
                                  gsl_stream_t s) {
  GSL_CHECK_ARG(omega && g, "null tensor");
  GSL_CHECK_ARG(aligned4(omega) && aligned4(g), "omega and g are 4-byte aligned");
  GSL_CHECK_ARG(n >= 1 && n < (1L << 31), "1 <= n < 2^31");
  GSL_CHECK_ARG(kind == GSR_EWC || kind == GSR_MAS, "kind is GSR_EWC or GSR_MAS");
  GSL_CHECK_ARG(b != 0.0f, "b != 0");
  const uintptr_t mo = reinterpret_cast<uintptr_t>(omega) & 15, mg = reinterpret_cast<uintptr_t>(g) & 15;
  long head = n, nvec = 0;
  if (mo == mg) {
    head = min(n, (long)(((16 - mo) & 15) / 4));
    nvec = (n - head) / 4;
  }
  const long work = max(nvec, n - 4 * nvec);
  const int grid = (int)min((long)IA_MAX_BLOCKS, (work + 255) / 256);
  hipLaunchKernelGGL(importance_acc_kernel, dim3(grid), dim3(256), 0, as_stream(s), omega, g, n, head, nvec, kind, a, b, guard, skipped);
  return check_launch(__func__);
}

// =====================================================================================
// gsr_sq_mean_*. The forward is the chunked sum of gsl_chunks.h: fixed chunks, f64 per thread, one ascending reduce.
// =====================================================================================
__global__ __launch_bounds__(256) void sq_mean_partial_kernel(const float* __restrict__ x, long ldx, int C, long n, long chunk,
                                                              float* __restrict__ ws) {
  __shared__ float sm[16];
  const long i0 = (long)blockIdx.x * chunk, i1 = min(n, i0 + chunk);
  const float s = chunk_partial(i0, i1, sm, [&](long i) {
    const long r = i / C;
    const double v = (double)x[r * ldx + (i - r * C)];
    return v * v;      // exact in f64
  });
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void sq_mean_reduce_kernel(const float* __restrict__ ws, int nblk, float count, float* __restrict__ out) {
  __shared__ float sm[16];
  const float s = strided_sum(ws, nblk, sm);
  if (threadIdx.x == 0) out[0] = s / count;
}
__global__ __launch_bounds__(256) void sq_mean_bwd_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ gout,
                                                          float* __restrict__ dx, long lddx, int C, long n, float count) {
#pragma clang fp contract(off)
  const float q = gout[0] / count;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const long r = i / C, c = i - r * C;
    const float twice = 2.0f * x[r * ldx + c];
    dx[r * lddx + c] = q * twice;
  }
}

static int sq_mean_check(const char* who, int B, int C) {
  GSL_CHECK_ARG_AS(who, B >= 1 && C >= 1, "B >= 1, C >= 1");
  GSL_CHECK_ARG_AS(who, (long)B * C < (1L << 31), "B * C < 2^31");
  return GSL_OK;
}

extern "C" long gsr_sq_mean_ws_elems(int B, int C) { return sq_mean_check(__func__, B, C) == GSL_OK ? chunk_blocks((long)B * C) : -1; }

extern "C" int gsr_sq_mean_fwd(const float* x, long ldx, int B, int C, float* out, float* ws, gsl_stream_t s) {
  GSL_TRY(sq_mean_check(__func__, B, C));
  GSL_CHECK_ARG(x && out, "null tensor");
  GSL_CHECK_ARG(ws, "null ws");
  GSL_CHECK_ARG(ldx >= C, "ldx >= C");
  const long n = (long)B * C;
  const int nblk = chunk_blocks(n);
  const long chunk = chunk_len(n, nblk);
  hipLaunchKernelGGL(sq_mean_partial_kernel, dim3(nblk), dim3(256), 0, as_stream(s), x, ldx, C, n, chunk, ws);
  GSL_TRY(check_launch("gsr_sq_mean_fwd(partial)"));
  hipLaunchKernelGGL(sq_mean_reduce_kernel, dim3(1), dim3(256), 0, as_stream(s), ws, nblk, (float)n, out);
  return check_launch("gsr_sq_mean_fwd(reduce)");
}

extern "C" int gsr_sq_mean_bwd(const float* x, long ldx, const float* gout, float* dx, long lddx, int B, int C, gsl_stream_t s) {
  GSL_TRY(sq_mean_check(__func__, B, C));
  GSL_CHECK_ARG(x && gout && dx, "null tensor");
  GSL_CHECK_ARG(ldx >= C && lddx >= C, "ldx >= C, lddx >= C");
  const long n = (long)B * C;
  const int grid = (int)min((long)IA_MAX_BLOCKS, (n + 255) / 256);
  hipLaunchKernelGGL(sq_mean_bwd_kernel, dim3(grid), dim3(256), 0, as_stream(s), x, ldx, gout, dx, lddx, C, n, (float)n);
  return check_launch(__func__);
}

// =====================================================================================
// gsr_reg_multi_*: the table is built on the host (gsr_reg_multi_layout), the kernels look their entry up by workgroup index.
// =====================================================================================
extern "C" int gsr_reg_multi_layout(const void* const* p, const void* const* p0, const void* const* omega, const long* n, int n_terms,
                                    int n_tensors, gsr_reg_entry* table, long* total_blocks, long* bwd_blocks, long* g_elems) {
  GSL_CHECK_ARG(p && p0 && omega && n && table, "null host array");
  GSL_CHECK_ARG(total_blocks && bwd_blocks && g_elems, "null result");
  GSL_CHECK_ARG(n_terms >= 1 && n_tensors >= 1 && (long)n_terms * n_tensors < (1L << 20), "n_terms >= 1, n_tensors >= 1, fewer than 2^20 entries");
  long blk = 0, goff = 0;
  for (int k = 0; k < n_terms; ++k) {
    for (int t = 0; t < n_tensors; ++t) {
      const int e = k * n_tensors + t;
      GSL_CHECK_ARG(p[e] && p0[e], "null tensor in an entry");
      GSL_CHECK_ARG(n[e] >= 1 && n[e] < (1L << 31), "1 <= n < 2^31 in every entry");
      GSL_CHECK_ARG(aligned4(p[e]) && aligned4(p0[e]) && aligned4(omega[e]), "tensors are 4-byte aligned");
      GSL_CHECK_ARG(k == 0 || (p[e] == p[t] && n[e] == n[t]), "every term of a tensor has the same p and n");
      gsr_reg_entry& o = table[e];
      o.p = static_cast<const float*>(p[e]);
      o.p0 = static_cast<const float*>(p0[e]);
      o.omega = static_cast<const float*>(omega[e]);
      o.n = n[e];
      o.nblk = chunk_blocks(n[e]);
      o.chunk = chunk_len(n[e], o.nblk);
      o.blk0 = (int)blk;
      if (k == 0) {
        o.goff = goff;
        goff += (n[e] + 3) / 4 * 4;
      } else {
        o.goff = table[t].goff;
      }
      blk += o.nblk;
      GSL_CHECK_ARG(blk < (1L << 31), "fewer than 2^31 workgroups");
    }
    if (k == 0) *bwd_blocks = blk;
  }
  *total_blocks = blk;
  *g_elems = goff;
  return GSL_OK;
}

__global__ __launch_bounds__(256) void reg_multi_partial_kernel(const gsr_reg_entry* __restrict__ tab, int n_entries, float* __restrict__ ws) {
  __shared__ float sm[16];
  const gsr_reg_entry e = tab[chunk_owner(tab, n_entries, blockIdx.x, &gsr_reg_entry::blk0)];
  const float* __restrict__ p = e.p;
  const float* __restrict__ p0 = e.p0;
  const float* __restrict__ omega = e.omega;
  const long i0 = (long)(blockIdx.x - e.blk0) * e.chunk, i1 = min(e.n, i0 + e.chunk);
  // reg_quad_partial_kernel's sum (csrc/train.hip): the same helper over the same term
  const float s = chunk_partial(i0, i1, sm, [&](long i) { return quad_term(p, p0, omega, i); });
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void reg_multi_reduce_kernel(const gsr_reg_entry* __restrict__ tab, int n_entries, const float* __restrict__ ws,
                                                               float* __restrict__ out) {
  __shared__ float sm[16];
  float total = 0.f;
  for (int e = 0; e < n_entries; ++e) {
    const float s = strided_sum(ws + tab[e].blk0, tab[e].nblk, sm);      // reg_quad_reduce_kernel's sum (every thread holds the result)
    total = e ? total + s : s;                                           // accumulate = e > 0
  }
  if (threadIdx.x == 0) out[0] = total;
}

// one element of tensor t through the terms in order: g + ((c2 * omega_k) * (p - p0_k)), every operation rounded on its own
__device__ __forceinline__ float rm_elem(float g, float p, const gsr_reg_entry* __restrict__ tab, int t, int n_terms, int n_tensors, long i, float c2) {
#pragma clang fp contract(off)
  for (int k = 0; k < n_terms; ++k) {
    const gsr_reg_entry* e = tab + (long)k * n_tensors + t;
    float c = c2;
    if (e->omega) c = c * e->omega[i];
    const float d = p - e->p0[i];
    const float w = c * d;
    g = g + w;
  }
  return g;
}

__global__ __launch_bounds__(256) void reg_multi_bwd_kernel(const gsr_reg_entry* __restrict__ tab, int n_terms, int n_tensors,
                                                            const float* __restrict__ coef, float* __restrict__ gbase) {
#pragma clang fp contract(off)
  const int t = chunk_owner(tab, n_tensors, blockIdx.x, &gsr_reg_entry::blk0);
  const gsr_reg_entry e0 = tab[t];
  const float* __restrict__ p = e0.p;
  float* __restrict__ g = gbase + e0.goff;
  const long i0 = (long)(blockIdx.x - e0.blk0) * e0.chunk, i1 = min(e0.n, i0 + e0.chunk);
  const float c2 = coef[0] * 2.0f;
  uintptr_t bits = reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g);
  for (int k = 0; k < n_terms; ++k) {
    const gsr_reg_entry* e = tab + (long)k * n_tensors + t;
    bits |= reinterpret_cast<uintptr_t>(e->p0) | reinterpret_cast<uintptr_t>(e->omega);
  }
  chunk_walk(i0, i1, (bits & 15) == 0, [&](long i) {
    float4 gg = *reinterpret_cast<const float4*>(g + i);
    const float4 pp = *reinterpret_cast<const float4*>(p + i);
    for (int k = 0; k < n_terms; ++k) {
      const gsr_reg_entry* e = tab + (long)k * n_tensors + t;
      const float4 q = *reinterpret_cast<const float4*>(e->p0 + i);
      float4 c = make_float4(c2, c2, c2, c2);
      if (e->omega) {
        const float4 om = *reinterpret_cast<const float4*>(e->omega + i);
        c.x = c.x * om.x; c.y = c.y * om.y; c.z = c.z * om.z; c.w = c.w * om.w;
      }
      const float dx = pp.x - q.x, dy = pp.y - q.y, dz = pp.z - q.z, dw = pp.w - q.w;
      const float wx = c.x * dx, wy = c.y * dy, wz = c.z * dz, ww = c.w * dw;
      gg.x = gg.x + wx; gg.y = gg.y + wy; gg.z = gg.z + wz; gg.w = gg.w + ww;
    }
    *reinterpret_cast<float4*>(g + i) = gg;
  }, [&](long i) { g[i] = rm_elem(g[i], p[i], tab, t, n_terms, n_tensors, i, c2); });
}

extern "C" int gsr_reg_multi_fwd(const gsr_reg_entry* table_dev, int n_entries, long total_blocks, float* out, float* ws, gsl_stream_t s) {
  GSL_CHECK_ARG(table_dev && out, "null table or out");
  GSL_CHECK_ARG(ws, "null ws");
  GSL_CHECK_ARG(n_entries >= 1 && total_blocks >= n_entries && total_blocks < (1L << 31), "n_entries >= 1, n_entries <= total_blocks < 2^31");
  hipLaunchKernelGGL(reg_multi_partial_kernel, dim3((unsigned)total_blocks), dim3(256), 0, as_stream(s), table_dev, n_entries, ws);
  GSL_TRY(check_launch("gsr_reg_multi_fwd(partial)"));
  hipLaunchKernelGGL(reg_multi_reduce_kernel, dim3(1), dim3(256), 0, as_stream(s), table_dev, n_entries, ws, out);
  return check_launch("gsr_reg_multi_fwd(reduce)");
}

extern "C" int gsr_reg_multi_bwd(const gsr_reg_entry* table_dev, int n_terms, int n_tensors, long bwd_blocks, const float* coef, float* g,
                                 gsl_stream_t s) {
  GSL_CHECK_ARG(table_dev && coef && g, "null table, coef or g");
  GSL_CHECK_ARG(aligned4(g), "g is 4-byte aligned");
  GSL_CHECK_ARG(n_terms >= 1 && n_tensors >= 1 && bwd_blocks >= n_tensors && bwd_blocks < (1L << 31), "n_terms >= 1, n_tensors <= bwd_blocks < 2^31");
  hipLaunchKernelGGL(reg_multi_bwd_kernel, dim3((unsigned)bwd_blocks), dim3(256), 0, as_stream(s), table_dev, n_terms, n_tensors, coef, g);
  return check_launch(__func__);
}
