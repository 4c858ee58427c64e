/* gslora_reg.h — C ABI of libgslora_reg.so: what the regularisation baselines (L2 / EWC / MAS) need around the FFN-training step of
 * libgslora_train.so — the accumulation of an importance matrix, the objective MAS differentiates, and the quadratic regulariser of ALL
 * terms and tensors in two launches forward and one backward. A third product library: a process that trains LoRA only, or the head only,
 * never opens it.
 *
 * Conventions are those of gslora_hip.h, whose enums this header uses (gsl_status, gsl_stream_t):
 *  - every pointer is a DEVICE pointer unless stated otherwise; sizes are elements; the stream is explicit;
 *  - every function returns an int status (GSL_OK = 0); gsr_last_error() holds the text of this thread's last refusal;
 *  - no allocation inside, no getenv(), no global state; argument errors are refused by name before any launch;
 *  - results are deterministic: fixed-order sums, no atomics, the same bits on every call.
 */
#ifndef GSLORA_REG_H
#define GSLORA_REG_H

#include "gslora_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

GSL_API const char* gsr_last_error(void);

/* ---- importance accumulation (reference train/train_own_forget_cl.py:1501-1509, EWC: p += grad ** 2 * len(samples) / len(loader);
 * :1554-1558, MAS: p += grad.abs() / len(loader))
 *
 *   kind GSR_EWC   omega[i] = omega[i] + ((g[i] * g[i]) * a) / b
 *   kind GSR_MAS   omega[i] = omega[i] + fabsf(g[i]) / b                     (a is not read)
 *
 * omega, g: flat f32 of any length 1 <= n < 2^31, 4-byte aligned. Every operation is rounded on its own (no fused multiply-add) and the
 * division is the correctly rounded one: the bits of the torch expressions above on f32 tensors. guard (nullable): the device float of a
 * loss-scaled fp16 backward (the largest scaled gradient it stored); when !(*guard < 65504) — a 16-bit store saturated, or the value is not
 * finite — omega is left untouched (the rule of gsl_adamw_flat: no host sync) and skipped[0] (nullable, a device int) is incremented once.
 * One launch, grid-stride; 16-byte loads and stores over the part where omega and g are 16-byte aligned together, scalar accesses for the
 * elements in front of and behind it (and for everything when the two pointers are misaligned differently). */
enum { GSR_EWC = 0, GSR_MAS = 1 };
GSL_API int gsr_importance_acc(float* omega, const float* g, long n, int kind, float a, float b, const float* guard, int* skipped,
                               gsl_stream_t s);

/* ---- mean of squares (reference train/train_own_forget_cl.py:1548-1549, MAS: outputs.pow_(2); loss = outputs.mean())
 *
 *   forward   out[0] = sum_{r,c} x[r*ldx + c]^2 / (float)(B*C)
 *   backward  dx[r*lddx + c] = (gout[0] / (float)(B*C)) * (2 * x[r*ldx + c])          gout: a DEVICE float
 *
 * x [B, C] f32 with row stride ldx >= C, dx [B, C] with row stride lddx >= C (pad columns are not written); B >= 1, C >= 1, B*C < 2^31.
 * Forward: the B*C elements in row-major order are cut into min(1024, ceil(B*C / 1024)) chunks; a thread forms and sums its squares in
 * f64 and rounds once, a workgroup sums its threads in f32 into ws (gsr_sq_mean_ws_elems(B, C) floats), one reduce launch sums the chunks
 * in ascending order and divides. No atomics. Backward: the quotient is rounded once and the product once (2 * x is exact) — the bits of
 * torch autograd for x.pow(2).mean(). */
GSL_API long gsr_sq_mean_ws_elems(int B, int C);
GSL_API int gsr_sq_mean_fwd(const float* x, long ldx, int B, int C, float* out, float* ws, gsl_stream_t s);
GSL_API int gsr_sq_mean_bwd(const float* x, long ldx, const float* gout, float* dx, long lddx, int B, int C, gsl_stream_t s);

/* ---- batched quadratic regulariser (reference engine_cl.py:449-459, get_reg_loss: every term and every trainable tensor)
 *
 *   forward   out[0] = sum over entries e in order of  S_e,  S_e = sum_i omega_i (p_i - p0_i)^2 of entry e    (omega == NULL: 1)
 *   backward  g_t[i] = g_t[i] + ((coef[0] * 2) * omega_k[i]) * (p[i] - p0_k[i])   for the terms k = 0, 1, .. in order, per tensor t
 *
 * An ENTRY is one (term, tensor) pair; entries are term-major: e = k * n_tensors + t. The partition of an entry is that of
 * gst_reg_quad_fwd (gslora_train.h): nblk = min(1024, ceil(n / 1024)) workgroups, each over chunk = ceil(n / nblk) consecutive elements,
 * a thread summing the elements chunk_start + lane, + 256, .. in f64 and rounding once. S_e is formed exactly as gst_reg_quad_fwd forms it
 * and the running total is out = S_0, then out = out + S_e: the forward is bit-identical to the sequence of gst_reg_quad_fwd(accumulate =
 * e > 0) calls, the backward to the sequence of gst_reg_quad_bwd calls (every operation rounded on its own).
 *
 * gsr_reg_multi_layout is a HOST function that launches nothing: from HOST arrays p, p0, omega (omega[e] may be NULL) and n of n_terms *
 * n_tensors entries it fills the caller's HOST table, assigns every tensor its place goff in one flat gradient buffer (places are
 * multiples of 4 elements, so that an aligned buffer keeps every tensor 16-byte aligned) and returns total_blocks (the forward's grid and
 * the floats of ws), bwd_blocks (the backward's grid: the workgroups of one term) and g_elems (the floats of the gradient buffer).
 * Within a tensor every term has the same p and n. The caller copies the table to the device as it is.
 * gsr_reg_multi_fwd: total_blocks partial workgroups that look their entry up in the table, then one reduce workgroup over the entries.
 * gsr_reg_multi_bwd: one launch; a workgroup owns a chunk of one tensor and walks the terms, g read and written once per element:
 * 16-byte accesses where p, g and every p0_k / omega_k of the tensor are 16-byte aligned (then only the chunk's edges are scalar), scalar
 * accesses otherwise. The forward's loads stay 4 bytes per lane: a thread's elements and their order are part of the result. */
typedef struct gsr_reg_entry {
  const float* p;
  const float* p0;
  const float* omega; /* NULL: 1 */
  long n;
  long chunk; /* elements per workgroup: ceil(n / nblk) */
  long goff;  /* first element of this tensor in the flat gradient buffer */
  int blk0;   /* first workgroup (and ws slot) of this entry */
  int nblk;   /* min(1024, ceil(n / 1024)) */
} gsr_reg_entry;

GSL_API int gsr_reg_multi_layout(const void* const* p, const void* const* p0, const void* const* omega, const long* n, int n_terms,
                                 int n_tensors, gsr_reg_entry* table, long* total_blocks, long* bwd_blocks, long* g_elems);
GSL_API int gsr_reg_multi_fwd(const gsr_reg_entry* table_dev, int n_entries, long total_blocks, float* out, float* ws, gsl_stream_t s);
GSL_API int gsr_reg_multi_bwd(const gsr_reg_entry* table_dev, int n_terms, int n_tensors, long bwd_blocks, const float* coef, float* g,
                              gsl_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
