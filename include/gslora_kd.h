/* gslora_kd.h — C ABI of libgslora_kd.so: the loss side of the SCRUB baseline (reference baselines/SCRUBtrain.py, util/sgda_utils.py) — the
 * temperature-softened KL between student and teacher logits fused with the cross-entropy of the student (DistillKL + criterion_cls of
 * SCRUBtrain.py) and the parameter distance to a running average (param_dist) over every tensor in two launches forward and one backward.
 * A fourth product library: a process that runs no SCRUB step never opens it.
 *
 * Conventions are those of gslora_hip.h, whose enums this header uses (gsl_status, gsl_stream_t):
 *  - every pointer is a DEVICE pointer unless stated otherwise; sizes are elements; the stream is explicit;
 *  - every function returns an int status (GSL_OK = 0); gsk_last_error() holds the text of this thread's last refusal;
 *  - no allocation inside, no getenv(), no global state; argument errors are refused by name before any launch;
 *  - results are deterministic: fixed-order sums, no atomics, the same bits on every call.
 */
#ifndef GSLORA_KD_H
#define GSLORA_KD_H

#include "gslora_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

GSL_API const char* gsk_last_error(void);

/* ---- distillation + cross-entropy of [B, C] logits (reference util/sgda_utils.py, DistillKL.forward: F.kl_div(F.log_softmax(y_s / T),
 * F.softmax(y_t / T), reduction="sum") * T**2 / B; baselines/SCRUBtrain.py: loss = gamma * criterion_cls + alpha * criterion_div, and the
 * max steps' loss = -criterion_div)
 *
 * ys (student), yt (teacher): f32 [B, C] with unit column stride and row strides ld_s, ld_t >= C; labels: int64 [B], NULL only with
 * c_ce == 0. Per row b, with a = ys / T and t = yt / T (correctly rounded f32 divisions):
 *
 *   KD_b = sum_c exp(lt_c) * (lt_c - la_c),   lt_c = t_c - lse(t),  la_c = a_c - lse(a)        (a class whose exp underflows adds 0)
 *   CE_b = lse(ys) - ys[label_b]
 *
 *   out[0] = ((sum_b KD_b) * fl(T * T)) / B
 *   out[1] = (sum_b CE_b) / B                    0 when c_ce == 0: the cross-entropy is then not computed and labels are not read
 *   out[2] = c_kd * out[0] + c_ce * out[1]
 *
 * The three lines of out[] and every element of d are formed with each operation rounded on its own (no fused multiply-add). Inside a
 * row (the log-sum-exps, KD_b, CE_b) the compiler may fuse a multiply into the add behind it: fixed code, so the same bits on every call.
 *
 *   d[b, c] = (g * k_kd) * (exp(la_c) - exp(lt_c)) + (g * k_ce) * (exp(ys_c - lse(ys)) - [c == label_b])
 *             k_kd = c_kd * (T / B), k_ce = c_ce / B (host floats), g = gout[0] (a DEVICE float); the second product and the add are
 *             left out when c_ce == 0 (the forward's rule: c_ce itself is tested, not k_ce). accumulate: d = fl(d_old + value), the value formed first (the rule of gsl_ce_bwd).
 *
 * A label outside [0, C) (with c_ce != 0): CE_b is NaN, so out[1] and out[2] are, and row b of d is NaN; nothing out of bounds is read.
 * ws: gsk_kd_ws_elems(B, C) = 5 B floats — planes la, lt, lse(ys), KD_b, CE_b of B floats each (the last three planes hold 0 / KD_b / 0
 * when c_ce == 0); the forward writes all of it, the backward reads the first three planes and recomputes no reduction: one pass over ys
 * and yt. d: [B, C] with row stride ld_d >= C; pad columns are neither read nor written.
 *
 * Two kernels serve the rows, and gsk_kd_plan — a HOST function that launches nothing, the rule both launches call — says which:
 *   GSK_KD_WAVE   C <= 1024: a wave per row, four rows per workgroup, lane l holds elements l, l + 64, .. of both rows in registers; the
 *                 forward reads ys and yt from memory once. grid = ceil(B / 4).
 *   GSK_KD_BLOCK  C > 1024: a workgroup per row, thread i visits i, i + 256, ..; block reductions in fixed order. grid = B.
 * The forward is that launch plus one reduce workgroup (the batch sums: 256 threads stride the rows, fixed-order combine). */
enum { GSK_KD_WAVE = 0, GSK_KD_BLOCK = 1 };
GSL_API int gsk_kd_plan(int B, int C, int* kernel, int* grid, long* ws_elems); /* HOST pointers */
GSL_API long gsk_kd_ws_elems(int B, int C);                                     /* -1: refused */
GSL_API int gsk_kd_ce_fwd(const float* ys, long ld_s, const float* yt, long ld_t, const int64_t* labels, int B, int C, float T, float c_kd,
                          float c_ce, float* out3, float* ws, gsl_stream_t s);
GSL_API int gsk_kd_ce_bwd(const float* ys, long ld_s, const float* yt, long ld_t, const int64_t* labels, const float* ws, const float* gout,
                          int B, int C, float T, float c_kd, float c_ce, float* d, long ld_d, int accumulate, gsl_stream_t s);

/* ---- batched parameter distance (reference util/sgda_utils.py, param_dist: p * sum over ALL of model.parameters(), the frozen ones
 * included, of torch.norm(p_k - q_k))
 *
 *   forward   norm_k = sqrt(S_k),  S_k = sum_i (p_k[i] - q_k[i])^2;   out[0] = p * (norm_0 + norm_1 + ..)   (running f32 total, in order)
 *   backward  g_k[i] = (p_k[i] - q_k[i]) * ((gout[0] * p) / norm_k)   for the entries that have a place in the gradient buffer;
 *             exactly 0 where norm_k == 0 (torch.norm's subgradient at 0)
 *
 * gsk_param_dist_layout is a HOST function that launches nothing: from HOST arrays of the entries' two pointers, sizes and
 * trainable flags it fills the caller's HOST table. The partition of an entry is that of gsr_reg_multi_layout: nblk = min(1024,
 * ceil(n / 1024)) workgroups over chunk = ceil(n / nblk) consecutive elements. A trainable entry gets goff, its place in one flat gradient
 * buffer (places are multiples of 4 elements, disjoint, in entry order), and its backward workgroups [bblk0, bblk0 + nblk); a frozen entry
 * gets goff = -1 and no backward workgroup (its bblk0 is that of the next trainable entry). Returns total_blocks (the forward's grid, the
 * floats of ws), bwd_blocks (the backward's grid, 0 when nothing trains) and g_elems. The caller copies the table to the device as it is.
 * gsk_param_dist_fwd: total_blocks partial workgroups (a thread sums its squares of differences in f64 and rounds once; the workgroup sums
 * its threads in f32 into ws), then ONE reduce workgroup that walks the entries in order: the fixed-order sum of the entry's partials, its
 * square root into norms[k] (n_entries floats, kept for the backward), the running total, out[0] = p * total.
 * gsk_param_dist_bwd: one launch over bwd_blocks workgroups, every element of a trainable view written once (the padding between views
 * is not touched: the caller zero-initialises the buffer); 16-byte accesses where p_k, q_k and the view are 16-byte aligned (then only
 * a chunk's edges are scalar), scalar accesses otherwise. */
typedef struct gsk_dist_entry {
  const float* p;
  const float* q;
  long n;
  long chunk; /* elements per workgroup: ceil(n / nblk) */
  long goff;  /* first element of this tensor in the flat gradient buffer, or -1 for a frozen tensor */
  int blk0;   /* first forward workgroup (and ws slot) of this entry */
  int nblk;   /* min(1024, ceil(n / 1024)) */
  int bblk0;  /* first backward workgroup of this entry (frozen: that of the next trainable entry) */
  int pad_;
} gsk_dist_entry;

GSL_API int gsk_param_dist_layout(const void* const* p, const void* const* q, const long* n, const int* trainable, int n_entries,
                                  gsk_dist_entry* table, long* total_blocks, long* bwd_blocks, long* g_elems);
GSL_API int gsk_param_dist_fwd(const gsk_dist_entry* table_dev, int n_entries, long total_blocks, float p, float* out, float* norms, float* ws,
                               gsl_stream_t s);
GSL_API int gsk_param_dist_bwd(const gsk_dist_entry* table_dev, int n_entries, long bwd_blocks, float p, const float* gout, const float* norms,
                               float* g, gsl_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
