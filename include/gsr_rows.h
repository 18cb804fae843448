/*
 * gsr_rows.h -- C ABI of the row glue of the Gaussian transformer: from the network's flat Gaussian rows to the six dense
 * parameter buffers gsr_forward takes, and from the per-camera gradient arenas gsr_backward fills back to ONE packed row gradient
 * (part of libgsr_hip.so; kernels and entry points in csrc/rows.hip).
 *
 * Every network-side call site of the reference renders `unflattenGaussians(rows)` (model/box_sort.py:17-27;
 * train_stacked_transformer.py:200-212, train_transformer.py:185-186, train_autoencoder.py:155,166-168): six strided views of
 * the row tensor, made dense once per camera before the rasterizer, and six gradients per camera pushed back through slice and
 * reshape nodes, each of which allocates and zero-fills a [P, D] tensor.  The two functions here replace that with one launch
 * per direction.
 *
 * Row layout (the one flattenGaussians writes): D = 3 K + 14 float32 columns for K SH coefficients, 1 <= K <= GSR_ROWS_MAX_K, so
 * 17 <= D <= 62:
 *     0 .. 3K-1       features [K, 3] row-major: DC is columns 0..2, the rest 3..3K-1
 *     3K .. 3K+3      rotation (un-normalised quaternion)
 *     3K+4            opacity logit
 *     3K+5 .. 3K+7    xyz
 *     3K+8 .. 3K+10   log-scale
 *     3K+11 .. 3K+13  flags (start / pad / end markers of the token stream; no rasterizer input)
 *
 * gsr_rows_unpack: rows [P, D] contiguous -> six separate dense buffers of exactly the shapes gsr_forward(..., shs_rest,
 *   raw_params = 1) takes: xyz [P,3], f_dc [P,1,3], f_rest [P,K-1,3], opacity [P,1], scaling [P,3], rotation [P,4].
 *   f_rest is NULL if and only if K = 1.  rotation must be 16-byte aligned (gsr_forward reads a quaternion as one 16-byte load):
 *   a misaligned pointer is refused.  A pure bit copy: NaN payloads, infinities and -0.0 arrive unchanged; the flag columns are
 *   not read.  One launch; P = 0 is legal and launches nothing.  An output whose range intersects that of rows is refused.
 *
 * gsr_rows_grad_pack: B gradient arenas -> grad_rows [P, D], overwritten.
 *   arenas is a HOST array of B device pointers, read before the call returns (they travel to the kernel by value);
 *   1 <= B <= GSR_ROWS_MAX_B (callers chunk larger sets and add the chunk results in order).
 *   An arena holds one camera's parameter gradients as gsr_backward writes them for the fused form when they are carved from a
 *   gradient arena (rasterizer.HipBackend._gradient_outputs), consecutively and without padding:
 *       dL/dxyz [P,3], dL/df_dc [P,3], dL/df_rest [P,3(K-1)], dL/dopacity [P], dL/dscaling [P,3], dL/drotation [P,4]
 *   = P (3 K + 11) floats.  An arena needs 4-byte alignment only.
 *   Column c of row p of grad_rows is ((a_0 + a_1) + a_2) + ... over the cameras in index order, in float32, each term the
 *   entry of that column's block; the sum starts from a_0 itself, not from 0 + a_0, so B = 1 is a bit copy and keeps -0.0.  The
 *   three flag columns are exactly +0.0.  No atomics: the result is bitwise identical from run to run.
 *   One launch; P = 0 is legal.  grad_rows whose range intersects that of any arena is refused.
 *
 * Sizes: P >= 0 and P * D < 2^31; at P = 0 both functions check P, D (and B) and look at no pointer.  D that is not 3 K + 14
 * for a K in 1 .. 16 is refused (the Python layer further restricts K to the square numbers an SH degree gives).
 *
 * Same conventions as gsr.h: device pointers, float32, caller-owned buffers, enqueued on `stream`, 0 = ok or a GSR_ERR_* code
 * with its text in gsr_last_error(), no host synchronisation, never aborts.
 */
#ifndef GSR_ROWS_H
#define GSR_ROWS_H
#include <stddef.h>
#include <stdint.h>
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
#define GSR_ROWS_MAX_K 16
#define GSR_ROWS_MAX_B 64
int32_t gsr_rows_unpack(gsr_stream_t stream, int32_t P, int32_t D, const float *rows /*[P,D]*/,
                        float *xyz /*[P,3]*/, float *f_dc /*[P,1,3]*/, float *f_rest /*[P,K-1,3] or NULL*/,
                        float *opacity /*[P,1]*/, float *scaling /*[P,3]*/, float *rotation /*[P,4]*/);
int32_t gsr_rows_grad_pack(gsr_stream_t stream, int32_t P, int32_t D, int32_t B, const float *const *arenas /*[B] host*/,
                           float *grad_rows /*[P,D]*/);
#ifdef __cplusplus
}
#endif
#endif
