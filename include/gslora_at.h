/* gslora_at.h — C ABI of libgslora_at.so: the attention-transfer term of the LIRF baseline (reference baselines/LIRFtrain.py, at and
 * at_loss) on the [B, T, D] stream between the lower and the upper half of the network, and its gradient to the student's stream.
 * A sixth product library: a process that takes no LIRF step never opens it.
 *
 * Conventions are those of gslora_hip.h, whose enums this header uses (gsl_status, gsl_dtype, gsl_stream_t):
 *  - every pointer is a DEVICE pointer unless stated otherwise; sizes are elements; the stream is explicit;
 *  - every function returns an int status (GSL_OK = 0); gsa_last_error() holds the text of this thread's last refusal;
 *  - no allocation inside, no getenv(), no global state; argument errors are refused by name before any launch;
 *  - results are deterministic: fixed-order sums, no atomics, the same bits on every call.
 */
#ifndef GSLORA_AT_H
#define GSLORA_AT_H

#include "gslora_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

GSL_API const char* gsa_last_error(void);

/* ---- at_loss(xs, xt) of two streams
 *
 * xs (student), xt (teacher): rows of D elements of one type `dtype` (GSL_F32, GSL_F16 or GSL_BF16) with unit column stride and row strides
 * ld_s, ld_t >= D; token t of image b is row b * T + t. Images 0 .. B-1 are read: xs may have more rows behind them (the remain batch of a
 * fused forward), which are not touched. Every row starts on a 16-byte boundary (base pointer and ld * sizeof(element) multiples of 16):
 * all accesses are 16-byte ones. 64 <= D <= 1024, D % 64 == 0, T <= 1025, B * T <= 2^24.
 *
 *   q[b, d]  = (sum_t x[b, t, d]^2) / T                     f32 sums of the elements converted to f32
 *   n[b]     = sqrtf(sum_d q[b, d]^2)
 *   a[b, d]  = q[b, d] / max(n[b], 1e-12)                   F.normalize
 *   at[b, d] = a[b, d] < 0.005 ? 0 : a[b, d]
 *   loss[0]  = (sum_b sum_d (at_s - at_t)^2) / (B * D)
 *   G[b, d]  = d loss / d xs[b, t, d] / xs[b, t, d] = (2 / T) * d loss / d q_s[b, d]     [B, D] f32, 16-byte aligned
 *
 * G carries, in order, the squared difference, the threshold (no gradient ARRIVES at an entry of the student that it zeroed),
 * F.normalize's backward (for n < 1e-12 the denominator is the constant) and the mean of squares. G itself is not zero at a zeroed
 * entry: the entry still feeds the norm n, which leaves -a * <g, a> / n there (tiny, as a < 0.005; autograd on the reference gives the
 * same). An all-zero image has at = 0 and G = 0; equal streams give loss = 0 and G = 0 exactly. at_s, at_t: optional [B, D] f32 outputs
 * of the two tables at (either may be null).
 *
 * Three launches. Stage 1, grid (B, nsplit): a workgroup sums the squares of `chunk` consecutive tokens of one image, of both streams;
 * a thread owns one 16-byte group of channels and every (256 / groups-per-row)-th token of the chunk in ascending order, the threads of one
 * channel are then added in ascending order through LDS. Stage 2, a workgroup per image: the splits in ascending order, then everything above
 * up to the image's part of the loss. Stage 3, one workgroup: the images' parts in a fixed order. gsa_at_plan — a HOST function that launches
 * nothing, the rule the forward calls — gives nsplit and chunk: the token axis is cut until about 512 workgroups exist, into chunks of at
 * least 16 tokens and at most 64 pieces. ws: gsa_at_ws_elems(B, T, D) = B * nsplit * 2 * D + B floats, 16-byte aligned.
 * Refused by name: B < 1, T < 1, T > 1025, D not a multiple of 64 in [64, 1024], B * T > 2^24, a null pointer, an unknown dtype, a row
 * stride below D, a row that is not 16-byte aligned. */
#define GSA_MAX_T 1025
#define GSA_MAX_D 1024
#define GSA_MAX_ROWS (1 << 24)
GSL_API int gsa_at_plan(int B, int T, int D, int* nsplit, int* chunk, long* ws_elems); /* HOST pointers */
GSL_API long gsa_at_ws_elems(int B, int T, int D);                                     /* -1: refused */
GSL_API int gsa_at_fwd(const void* xs, long ld_s, const void* xt, long ld_t, int dtype, int B, int T, int D, float* loss, float* G,
                       float* at_s, float* at_t, float* ws, gsl_stream_t s);

/* ---- the gradient, added in place at the boundary
 *
 *   dmid[b, t, d] = fl(dmid[b, t, d] + (fl(coef[0] * scale[0]) * G[b, d]) * xs[b, t, d])        b < B
 *
 * every operation rounded to f32 on its own, then once to dmid's element type d_dtype (GSL_F32, or the 16-bit operand format of the pass:
 * fp16 saturates at +-65504). coef: a DEVICE float, the upstream gradient times the term's weight; scale: a DEVICE float, the loss scale of
 * the pass (a power of two in fp16 mode, else 1). xs: as above, of type x_dtype; dmid: rows of D elements, row stride ld_d >= D, 16-byte
 * aligned rows. Rows b * T + t with b >= B and the pad columns are neither read nor written. One launch: a thread per group of 4 channels
 * (8 when both tensors are 16-bit) of one token; one read of xs, one read and one write of dmid. */
GSL_API int gsa_at_bwd(const void* xs, long ld_s, int x_dtype, const float* G, const float* coef, const float* scale, int B, int T, int D,
                       void* dmid, long ld_d, int d_dtype, gsl_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
