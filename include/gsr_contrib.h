/*
 * gsr_contrib.h -- C ABI of the per-Gaussian blend-weight statistics of one or many renders
 * (part of libgsr_hip.so; kernels and entry points in csrc/contrib_stats.hip).
 *
 * For every Gaussian, over the (pixel, entry) pairs the colour pass BLENDED: the sum of the blend weights w = alpha * T, the largest
 * of them, and how many there were.  These are what pruning by contribution asks for (LightGaussian's significance score, RadSplat's
 * "max ray contribution", Mini-Splatting's importance), and the library's only other route to the sum is a whole gsr_backward.
 *
 * gsr_contrib_accumulate runs AFTER the gsr_forward that filled the three workspaces (geometry, binning, image) and re-reads what it
 * left on the device, as gsr_depth.h's calls do: the per-tile lists, the records, the reachability bytes, and per pixel the last
 * contributor.  No per-Gaussian stage and no list build runs again, and the colour path does not know of this header.
 *
 * Per entry the decisions are the colour pass's, from the same expression (csrc/gsr_device.h), as gsr_depth.h states them:
 *   - skipped on power > 0 and on alpha < 1/255;  alpha = min(0.99, opacity * G);
 *   - the walk ends at the pixel's recorded last contributor, so the stop test (T < 1e-4) is not evaluated again;
 *   - w = alpha * T with T the running transmittance, continued as T - alpha * T: the bits of gsr_depth_forward's weight.
 *
 * One row of 16 bytes per Gaussian:
 *   sum_q32  += floor(w * 2^32) per blended pair.  w < 1, so a term fits in 32 bits; the scaling is exact in float32 and the
 *               conversion truncates, so the sum is exact integer arithmetic on a wrapping unsigned 64-bit word.  It depends neither on
 *               the order of addition, nor on the wave geometry, nor on the route by which the forward pass built its lists, nor on
 *               the order in which views are added.
 *   max_bits  = max(max_bits, bit pattern of w).  w >= 0: unsigned order on the bits is float order.
 *   count    += 1 per blended pair.
 * An all-zero row is the empty statistic: the caller clears `rows` (16 P bytes) with a memset before the first view.  The call
 * always ACCUMULATES into `rows`, with integer atomics, so many views -- on one stream or several -- add into the same rows.
 *
 * Capacity: `count` wraps once a Gaussian has been blended into more than 2^32 - 1 pixels, and the integer part of sum_q32 (its
 * upper 32 bits) cannot wrap sooner.  2^32 - 1 pixels are about 500 full 4K views (3840 x 2160).  The C call does NOT saturate
 * and does not count views: a caller that may come near keeps the total of W * H over the views it adds below 2^32 (the Python
 * collector refuses before that point).
 *
 *   - works for renders made with raw_params = 1 (the fused-step extension) as for any other: only the records are read, never the
 *     caller's parameters.
 *   - NOT refused while the option "deterministic_bwd" is on -- in contrast to gsr_depth_backward, which sums floats: integer
 *     atomics are order-independent, so the rows are the same bytes from run to run in any mode.
 *   - no workspace, no host wait, no second stream.
 *   - P == 0 or R == 0 (R = the pair count gsr_forward reported): success, nothing is read or written.
 *   - refused, in this order and with texts that begin with the call's name: bad sizes or an image too large
 *     (GSR_ERR_INVALID_ARGUMENT); a geometry, image or binning workspace smaller than gsr_forward's (GSR_ERR_WORKSPACE); `rows` or a
 *     workspace pointer missing (GSR_ERR_INVALID_ARGUMENT).  A refused call writes nothing.
 *
 * gsr_contrib_read: one streaming pass over the rows into up to three dense vectors,
 *     weight_sum[g]  = (float)((double)sum_q32 * 2^-32)     (one rounding: the double product is exact up to 2^53)
 *     weight_max[g]  = max_bits reinterpreted as float32
 *     pixel_count[g] = count                                (the same 32 bits, as int32)
 * Any output may be NULL; all three NULL is refused, as is a missing `rows` (P > 0).  P == 0: nothing to do.  The rows are not
 * changed.
 *
 * Same conventions as gsr.h: device pointers, caller-owned buffers, work enqueued on `stream`, 0 = ok or a GSR_ERR_* code with its
 * text in gsr_last_error(), never aborts.
 */
#ifndef GSR_CONTRIB_H
#define GSR_CONTRIB_H
#include <stddef.h>
#include <stdint.h>
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
typedef struct { uint64_t sum_q32; uint32_t max_bits; uint32_t count; } gsr_contrib_row_t;
int32_t gsr_contrib_accumulate(gsr_stream_t stream, int32_t P, int32_t W, int32_t H, int64_t R,
                               const void *geom_ws, size_t geom_bytes, const void *binning_ws, size_t binning_bytes,
                               const void *img_ws, size_t img_bytes, gsr_contrib_row_t *rows /*[P]*/);
int32_t gsr_contrib_read(gsr_stream_t stream, int32_t P, const gsr_contrib_row_t *rows /*[P]*/,
                         float *weight_sum /*[P] or NULL*/, float *weight_max /*[P] or NULL*/, int32_t *pixel_count /*[P] or NULL*/);
#ifdef __cplusplus
}
#endif
#endif
