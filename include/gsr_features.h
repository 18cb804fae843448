/*
 * gsr_features.h -- C ABI of N-channel feature maps of a render, with gradients
 * (part of libgsr_hip.so; kernels and entry points in csrc/feature_maps.hip).
 *
 * A feature map blends C numbers per Gaussian exactly as the colour pass blends three: semantic or language features, one-hot
 * instance ids, a learned embedding.  Both calls run AFTER the gsr_forward that filled the three workspaces (geometry, binning,
 * image) and re-use what it left on the device, as gsr_depth.h does: the per-tile lists, the 12-float records, the reachability
 * bytes per (list entry, 8x8 block), and per pixel the final transmittance and the last contributor.  No per-Gaussian stage and
 * no list build runs a second time.  The colour path (gsr_forward / gsr_backward) is not changed by this header.
 *
 *   out[c, y, x] = sum_i F[g(i), c] alpha_i T_i     over exactly the entries the colour pass blended into the pixel, front to back.
 *
 * The map is NOT normalised by alpha and has no background term.  Per entry the decisions are the colour pass's, from the same
 * expression (csrc/gsr_device.h): skipped on power > 0, alpha = min(0.99, opacity * G), skipped on alpha < 1/255; the walk ends at
 * the pixel's recorded last contributor.  A column of ones in F gives the alpha map of gsr_depth.h to rounding.  Inputs are taken
 * as finite.  1 <= C <= GSR_FEATURES_MAX_C; anything else: GSR_ERR_INVALID_ARGUMENT.
 *
 * gsr_features_forward: P == 0 or R == 0 (R = the pair count gsr_forward reported): zeros are written and no workspace is read.
 * No atomics: the result is bit-identical from run to run.
 *
 * gsr_features_backward: gradients of  L = <dL_dout, out>.  Per pixel and blended entry, with u_i = sum_c dL_dout[c, pixel] F[g(i), c]:
 *     dL/dalpha_i = u_i T_i - S_i / (1 - alpha_i),   S_i = sum_{j > i} u_j alpha_j T_j      (gsr_depth.h's recurrence with v = u, gD = 1)
 *     dL/dF[g, c] = sum over pixels and entries with g(i) = g of dL_dout[c, pixel] alpha_i T_i
 * The first feeds the same per-Gaussian chain as the colour gradient (csrc/pergauss_bwd.hip, unchanged); F does not depend on the
 * mean, so dL/dmeans3D has no further term.
 *   - exactly one of (scales, rotations) / cov3D_precomp, as gsr_backward; the gradient buffers of the form that was not given
 *     may be NULL and are not written.
 *   - accumulate = 0: dL_dmeans2D [P,3], dL_dopacity [P], dL_dmeans3D [P,3] and dL_dcov3D [P,6] or dL_dscales [P,3], dL_drots [P,4]
 *     are fully written, zeros included.
 *   - accumulate = 1: the result is ADDED element-wise (out = out + g) to buffers that a gsr_backward (and possibly a
 *     gsr_depth_backward) of the same render on the same stream has fully written.  Gaussians the forward pass never composited
 *     (gsr_composited_mask) are neither read nor written.
 *   - dL_dfeatures [P,C]: this pass's alone, so it takes no part in `accumulate`: always fully written, exact zeros for Gaussians
 *     outside gsr_composited_mask.  NULL: features that need no gradient -- the C sums per entry are not formed at all.
 *   - NOT supported by this call: raw_params (the fused-step extension) and split SH tensors.  A render made with raw_params = 1
 *     has no feature gradient through this header.
 *   - the option "deterministic_bwd" on: refused (GSR_ERR_INVALID_ARGUMENT, text naming the option).  The pass sums with float
 *     atomics and has no slot form; gradients may differ in the last bits from run to run.
 *   - workspace: gsr_features_workspace_bytes(P, C) bytes = gsr_depth_workspace_bytes(P) -- acc_rows(P) = P + P / 32 + 1024
 *     accumulator rows of 64 bytes (P taken as 1 when 0), rounded up to 256, plus 80 P bytes, rounded up to 256 -- plus
 *     acc_rows(P) rows of 4 C bytes for dL/dF, replica rows included, rounded up to 256.  Contents irrelevant before and after.
 *     Only the rows that can be added into (composited Gaussians, replica rows) are cleared.  Smaller: GSR_ERR_WORKSPACE.
 *     gsr_features_workspace_bytes needs no device.
 *   - P == 0: nothing to do.  R == 0: dL_dfeatures is zeroed; accumulate = 0 writes zeros, accumulate = 1 adds nothing.
 *
 * Same conventions as gsr.h: device pointers, float32, caller-owned buffers, matrices in gsr.h's layout, work enqueued on `stream`
 * (no host wait, no second stream), 0 = ok or a GSR_ERR_* code with its text in gsr_last_error(), never aborts.
 */
#ifndef GSR_FEATURES_H
#define GSR_FEATURES_H
#include <stddef.h>
#include <stdint.h>
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
#define GSR_FEATURES_MAX_C 64
int32_t gsr_features_workspace_bytes(int32_t P, int32_t C, size_t *bytes);
int32_t gsr_features_forward(gsr_stream_t stream, int32_t P, int32_t C, int32_t W, int32_t H, int64_t R, const float *features /*[P,C]*/,
                             const void *geom_ws, size_t geom_bytes, const void *binning_ws, size_t binning_bytes,
                             const void *img_ws, size_t img_bytes, float *out /*[C,H,W]*/);
int32_t gsr_features_backward(gsr_stream_t stream, int32_t P, int32_t C, int32_t W, int32_t H, int64_t R,
                              const float *means3D /*[P,3]*/, const int32_t *radii /*[P]*/, const float *scales /*[P,3] or NULL*/,
                              float scale_modifier, const float *rotations /*[P,4] or NULL*/, const float *cov3D_precomp /*[P,6] or NULL*/,
                              const float *viewmatrix, const float *projmatrix, const float *campos, float tanfovx, float tanfovy,
                              const float *features /*[P,C]*/, const float *dL_dout /*[C,H,W]*/,
                              const void *geom_ws, size_t geom_bytes, const void *binning_ws, size_t binning_bytes,
                              const void *img_ws, size_t img_bytes, void *ws, size_t ws_bytes, int32_t accumulate,
                              float *dL_dmeans2D /*[P,3]*/, float *dL_dopacity /*[P]*/, float *dL_dmeans3D /*[P,3]*/,
                              float *dL_dcov3D /*[P,6] or NULL*/, float *dL_dscales /*[P,3] or NULL*/, float *dL_drots /*[P,4] or NULL*/,
                              float *dL_dfeatures /*[P,C] or NULL*/);
#ifdef __cplusplus
}
#endif
#endif
