/*
 * gsr_sequence.h -- C ABI of the sequence preparation of the Gaussian transformer: the box sort that orders a splat scene
 * into a token sequence, and the visibility of every Gaussian under a set of cameras without rendering them
 * (part of libgsr_hip.so; kernels in csrc/sequence.hip).
 *
 * Box sort: `model/box_sort.py::GaussianHandler.box_sort` of the reference (train_stacked_transformer.py:72-73 calls it with
 * interval_num = 40: a Python loop over 64 000 boxes, each iteration six comparisons over all rows, two uploads and a
 * host-synchronising boolean gather).  PARITY PINNED: tests/golden/box_sort.npz holds inputs and outputs of the reference's own
 * function.
 *
 *   rows [P, D] float32; the three coordinates are columns xyz_col .. xyz_col + 2, already normalised.
 *   Boundaries b_k = (float)((1.0 / n) * k) for k = 0 .. n, the product taken in double: what the reference's
 *   torch.FloatTensor([interval_size * x, ...]) holds.  For every n in 1 .. 256, b is strictly increasing, b_0 = 0, b_n = 1.0f.
 *   A coordinate c lies in axis cell a iff b_a <= c < b_{a+1}; the cell is decided by comparisons with this very table
 *   (a first guess from c * n, then corrected), so a value one ulp below a boundary lands where the reference puts it.
 *   The row's box is ax + n ay + n n az.  Output rows are ordered by box, and inside a box by original index (a stable sort).
 *   -0.0 lies in cell 0.
 *
 * DEVIATION from the reference, deliberate: a row with any coordinate < 0, >= 1.0f or NaN belongs to no box.  After min-max
 * normalisation that is every Gaussian that attains the maximum on an axis (its coordinate is exactly 1.0).  The reference
 * drops these rows without a word and returns torch.empty garbage in the tail of its result.  Here
 *   - *out_count (device int32) is the number of rows kept (`last` in the reference);
 *   - out_rows [P, D]: rows [0, count) as the reference orders them, rows [count, P) ZERO;
 *   - out_perm [P] int32: the original index of every output row, -1 in the tail.  The dropped rows are those no entry names.
 *
 * The result is bitwise identical from run to run: the order is a stable radix sort of (box, index) and no step depends on the
 * order in which atomic operations land.  Sizes: 1 <= n <= 128, 3 <= D <= 64, 0 <= xyz_col <= D - 3, 0 <= P < 2^31 / D rows;
 * P = 0 is legal (count 0, nothing else written).  rows and out_rows must not overlap: equal pointers, and ranges of
 * P * D floats that intersect, are refused with GSR_ERR_INVALID_ARGUMENT.  Workspace: gsr_box_sort_workspace(P, n) bytes (12 P plus the radix sort's own), contents
 * irrelevant before and after; smaller: GSR_ERR_WORKSPACE.
 *
 * Visibility: both trainers render batch_size full images under no_grad in every iteration and keep only
 * `visibility_filter = radii > 0`, OR-ed over the cameras (train_stacked_transformer.py:93-96, train_transformer.py:79-81,
 * prep_cameras :121-133).  gsr_visible_union computes exactly those radii for B cameras in one pass over the Gaussians:
 *   radii_out[b, i] is, as an integer, what gsr_forward writes into radii[i] for camera b with the same means3D, scales,
 *   rotations (or cov3D_precomp), scale_modifier, raw_params, matrices, tanfov and image size: the near-plane test, det != 0
 *   and a non-empty tile rectangle decide it; SH, binning, compositing and the option exact_tile_cull do not enter.
 *   visible_out[i] = OR over b of (radii[b, i] > 0), as 0 / 1 bytes;  counts_out[b] = number of i with radii[b, i] > 0.
 * Any of the three outputs may be NULL, in every combination.  1 <= B <= 64 (callers chunk larger sets and OR the results);
 * P = 0 is legal (counts are zeroed).  viewmatrices / projmatrices are [B, 16] DEVICE arrays in the layout of gsr.h; tanfovx,
 * tanfovy, widths, heights are [B] HOST arrays, read before the call returns.  Exactly one of (scales, rotations) /
 * cov3D_precomp; raw_params = 1 (log-scales, unnormalised quaternions, as gsr_forward's fused-step extension) needs the former.
 * rotations must be 16-byte aligned (each quaternion is read as one 16-byte load, as in gsr_forward).
 * No workspace, no read-back.
 *
 * Same conventions as gsr.h: device pointers, float32, caller-owned buffers, enqueued on `stream`, 0 = ok or a GSR_ERR_* code
 * with its text in gsr_last_error(), no host synchronisation, never aborts.
 */
#ifndef GSR_SEQUENCE_H
#define GSR_SEQUENCE_H
#include <stddef.h>
#include <stdint.h>
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
#define GSR_BOX_MAX_N 128
#define GSR_BOX_MAX_D 64
#define GSR_VISIBLE_MAX_B 64
int32_t gsr_box_sort_workspace(int32_t P, int32_t n, size_t *bytes);
int32_t gsr_box_sort(gsr_stream_t stream, int32_t P, int32_t D, const float *rows /*[P,D]*/, int32_t xyz_col, int32_t n,
                     float *out_rows /*[P,D]*/, int32_t *out_perm /*[P]*/, int32_t *out_count /*[1] device*/,
                     void *ws, size_t ws_bytes);
int32_t gsr_visible_union(gsr_stream_t stream, int32_t P, int32_t B,
                          const float *means3D /*[P,3]*/, const float *scales /*[P,3] or NULL*/, float scale_modifier,
                          const float *rotations /*[P,4] or NULL*/, const float *cov3D_precomp /*[P,6] or NULL*/, int32_t raw_params,
                          const float *viewmatrices /*[B,16]*/, const float *projmatrices /*[B,16]*/,
                          const float *tanfovx /*[B] host*/, const float *tanfovy /*[B] host*/,
                          const int32_t *widths /*[B] host*/, const int32_t *heights /*[B] host*/,
                          int32_t *radii_out /*[B,P] or NULL*/, uint8_t *visible_out /*[P] or NULL*/, int32_t *counts_out /*[B] or NULL*/);
#ifdef __cplusplus
}
#endif
#endif
