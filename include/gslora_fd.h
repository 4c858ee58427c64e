/* gslora_fd.h — C ABI of libgslora_fd.so: the function-distance term of the DER / DER++ and FDR baselines (reference
 * baselines/DERtrain.py, DER_regularzaion_loss; baselines/FDRtrain.py, regularization_loss) — the distance between a student's and a frozen
 * teacher's [B, W] outputs (embeddings or logits) and its gradient to the student's rows.
 * A fifth product library: a process that takes no DER or FDR step never opens it.
 *
 * Conventions are those of gslora_hip.h, whose enums this header uses (gsl_status, gsl_stream_t):
 *  - every pointer is a DEVICE pointer unless stated otherwise; sizes are elements; the stream is explicit;
 *  - every function returns an int status (GSL_OK = 0); gsf_last_error() holds the text of this thread's last refusal;
 *  - no allocation inside, no getenv(), no global state; argument errors are refused by name before any launch;
 *  - results are deterministic: fixed-order sums, no atomics, the same bits on every call.
 */
#ifndef GSLORA_FD_H
#define GSLORA_FD_H

#include "gslora_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

GSL_API const char* gsf_last_error(void);

/* ---- row distance of two [B, W] matrices
 *
 * a (student), t (teacher): f32 [B, W] with unit column stride and row strides ld_a, ld_t >= W. Per row b
 *
 *   S_b = sum_c fl(fl(a[b, c] - t[b, c])^2)        f32, every operation rounded on its own (no fused multiply-add), in the fixed order below
 *
 * and the forward's result is, by mode,
 *
 *   GSF_SQ       n = sqrtf(sum_b S_b),  out[0] = n * n            torch.norm(a - t, p=2) squared, as DER_regularzaion_loss forms it
 *   GSF_ROWNORM  out[0] = (sum_b sqrtf(S_b)) / B                  torch.norm(a - t, 2, 1).mean(), FDR's regularization_loss
 *
 * ws: gsf_rowdist_ws_elems(B, W) = B floats; the forward leaves S_b there and the backward (GSF_ROWNORM) reads it: no reduction is
 * recomputed. The backward is one launch:
 *
 *   GSF_SQ       d[b, c] = fl(a - t) * (2 * (g * coef))
 *   GSF_ROWNORM  d[b, c] = fl(a - t) * (((g * coef) / B) / sqrtf(S_b)),   exactly 0 in a row with S_b == 0 (torch.norm's subgradient at 0)
 *
 * g = gout[0] (a DEVICE float), coef a host float (the method's lambda); every operation rounded on its own. accumulate: d = fl(d_old +
 * value), the value formed first (the rule of gsl_ce_bwd). d: [B, W] with row stride ld_d >= W; pad columns (c >= W) of a, t and d are
 * neither read nor written. A NaN in row b makes S_b, the forward's value and (GSF_ROWNORM) the whole of row b of d NaN, and touches no
 * other row of d.
 *
 * Element ownership, the same in both kernels and on both load paths: a row is cut into groups of four consecutive elements (the last may
 * be partial); a thread owns groups first, first + STRIDE, .. and sums its elements in ascending order. A group is one 16-byte access when
 * every row of every tensor of the call starts on a 16-byte boundary (base pointers 16-byte aligned, row strides multiples of 4, or
 * B == 1) and the group is whole; otherwise its elements are 4-byte accesses. The choice does not change a bit of the result.
 *
 * Two kernels serve the rows, and gsf_rowdist_plan — a HOST function that launches nothing, the rule both launches call — says which:
 *   GSF_WAVE   W <= 1024: a wave per row, four rows per workgroup, lane l owns groups l, l + 64, ..; S_b is the butterfly sum of the
 *              lanes. grid = ceil(B / 4).
 *   GSF_BLOCK  W > 1024: a workgroup per row, thread i owns groups i, i + 256, ..; waves summed by butterfly, then the four wave sums in
 *              order. grid = B.
 * The forward is that launch plus ONE reduce workgroup (256 threads stride the rows, fixed-order combine).
 * Refused by name: B < 1, W < 1, W > GSF_MAX_W, a null pointer, a row stride below W, an unknown mode. */
enum { GSF_WAVE = 0, GSF_BLOCK = 1 };
enum { GSF_SQ = 0, GSF_ROWNORM = 1 };
#define GSF_MAX_W (1 << 30)
GSL_API int gsf_rowdist_plan(int B, int W, int* kernel, int* grid, long* ws_elems); /* HOST pointers */
GSL_API long gsf_rowdist_ws_elems(int B, int W);                                    /* -1: refused */
GSL_API int gsf_rowdist_fwd(const float* a, long ld_a, const float* t, long ld_t, int B, int W, int mode, float* out1, float* ws,
                            gsl_stream_t s);
GSL_API int gsf_rowdist_bwd(const float* a, long ld_a, const float* t, long ld_t, const float* ws, const float* gout, int B, int W, int mode,
                            float coef, float* d, long ld_d, int accumulate, gsl_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
