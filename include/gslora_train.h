/* gslora_train.h — C ABI of libgslora_train.so: the kernels that train WEIGHTS of the backbone (the FFN linears of the reference's
 * --only_ffn mode) and the quadratic regulariser of its L2 / EWC / MAS baselines. A second product library beside libgslora_hip.so:
 * a process that trains LoRA only never opens it.
 *
 * Conventions are those of gslora_hip.h, whose enums this header uses (gsl_dtype, gsl_status, gsl_stream_t):
 *  - every pointer is a DEVICE pointer unless stated otherwise; sizes are elements; the stream is explicit;
 *  - every function returns an int status (GSL_OK = 0); gst_last_error() holds the text of this thread's last refusal;
 *  - no allocation inside, no getenv(), no global state; argument errors are refused by name before any launch;
 *  - results are deterministic: fixed-order sums, no atomics, the same bits on every call and under HIP-graph replay.
 */
#ifndef GSLORA_TRAIN_H
#define GSLORA_TRAIN_H

#include "gslora_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

GSL_API const char* gst_last_error(void);

/* ---- weight-gradient GEMM (autograd of nn.Linear for `weight` and `bias`: the two FFN linears of reference
 * vit_pytorch_face/vit_face.py:330-333 under train/train_own_forget_cl.py:432-439, --only_ffn)
 *
 *   dW[n*ldw + k] (+)= c * sum_m Y[m,n] * X[m,k]        db[n] (+)= c * sum_m Y[m,n]        c = gscale ? gscale[1] : 1
 *
 * Y [M,N] (ldy) and X [M,K] (ldx) row-major in `dtype` (GSL_F32, GSL_BF16 or GSL_F16); dW [N,K] (ldw) and db [N] (nullable) f32.
 * Any M >= 1; N % 64 == 0 and K % 64 == 0; rows of Y and X 16-byte aligned (base pointer and ld * element size); ldy >= N, ldx >= K,
 * ldw >= K. gscale (nullable): device floats {S, 1/S, ..} of a loss-scaled fp16 backward — the sums are multiplied by 1/S on the way out.
 * Two launches: f32 partial sums per (row split, output tile) on the matrix cores into ws ([split][N][K], then [split][N] for db),
 * then their reduction in ascending split order, which applies c and stores (accumulate = 0) or adds (accumulate = 1).
 * Every output element is one fixed-order sum: m ascending within a split, splits ascending. ws: gst_wgrad_ws_elems(M, N, K, dtype)
 * floats. gst_wgrad_plan answers what the launch itself uses: the output tile (tile_n x tile_k), the number of row splits and the rows
 * of each (the last split holds the remainder). */
GSL_API long gst_wgrad_ws_elems(int M, int N, int K, int dtype);
GSL_API int gst_wgrad_plan(int M, int N, int K, int dtype, int* tile_n, int* tile_k, int* nsplit, int* rows_per_split);
GSL_API int gst_wgrad(const void* Y, long ldy, const void* X, long ldx, float* dW, long ldw, float* db, int M, int N, int K, int dtype,
                      int accumulate, float* ws, const float* gscale, gsl_stream_t s);

/* ---- quadratic regulariser (reference engine_cl.py:455-457, get_reg_loss: sum(importance * (p - task_param) ** 2) of one tensor)
 *
 *   forward   out[0] (+)= sum_i omega_i * (p_i - p0_i)^2           omega == NULL: omega_i = 1 (the L2 baseline)
 *   backward  g_i += ((coef[0] * 2) * omega_i) * (p_i - p0_i)      coef: a DEVICE float (upstream gradient times lambda)
 *
 * p, p0, omega, g: flat f32 of any length n >= 1. The forward sums fixed chunks of the tensor into ws (gst_reg_quad_ws_elems(n) floats)
 * and reduces them in a second launch in ascending order; accumulate = 1 adds to out[0]. The backward evaluates the expression above in
 * f32 with every product and the sum rounded separately (no fused multiply-add). */
GSL_API long gst_reg_quad_ws_elems(long n);
GSL_API int gst_reg_quad_fwd(const float* p, const float* p0, const float* omega, long n, float* out, int accumulate, float* ws,
                             gsl_stream_t s);
GSL_API int gst_reg_quad_bwd(const float* p, const float* p0, const float* omega, long n, const float* coef, float* g, gsl_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
