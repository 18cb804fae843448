/*
 * gsr_depth.h -- C ABI of the depth and accumulated-opacity maps of a render, with gradients
 * (part of libgsr_hip.so; kernels and entry points in csrc/depth_maps.hip).
 *
 * Both calls run AFTER the gsr_forward that filled the three workspaces (geometry, binning, image) and re-use what it left on the
 * device: the per-tile lists (ranges, point_list), the 12-float records (centre, conic, opacity, view-space depth), the
 * reachability bytes per (list entry, 8x8 block), and per pixel the final transmittance T_final and the last contributor.  No
 * per-Gaussian stage and no list build runs a second time.  The colour path (gsr_forward / gsr_backward) is not changed by this
 * header and does not know of it.
 *
 *   depth[y, x] = sum_i v_i alpha_i T_i      over the entries the colour pass blended into the pixel, front to back,
 *   alpha[y, x] = 1 - T_final[y, x]          read from the image workspace: bit for bit the factor of the colour image's background term.
 *
 * v_i by `mode`:  GSR_DEPTH_EXPECTED (0): z_i, the view-space depth gsr_forward stored in the record;
 *                 GSR_DEPTH_INVERSE  (1): 1.0f / z_i (IEEE division).            Any other mode: GSR_ERR_INVALID_ARGUMENT.
 * Depth is NOT normalised by alpha and has no background term.  Per entry the decisions are the colour pass's, from the same
 * expression (csrc/gsr_device.h): skipped on power > 0, alpha = min(0.99, opacity * G), skipped on alpha < 1/255; the walk ends at
 * the pixel's recorded last contributor, so the stop test (T < 1e-4) is not evaluated again.
 *
 * gsr_depth_forward: either output may be NULL.  P == 0 or R == 0 (R = the pair count gsr_forward reported): zeros are written and
 * no workspace is read.
 *
 * gsr_depth_backward: gradients of  L = <dL_ddepth, depth> + <dL_dalpha, alpha>  with respect to the Gaussians' inputs.  Either map
 * gradient may be NULL (that map was not used); both NULL is refused.  Per blended entry, back to front, with the 0.99 cap
 * straight-through as in gsr_backward:
 *     dL/dalpha_i = gD (v_i T_i - S_i / (1 - alpha_i)) + gA T_final / (1 - alpha_i),   S_i = sum_{j > i} v_j alpha_j T_j
 *     dL/dv_i     = gD alpha_i T_i
 * The first feeds the same per-Gaussian chain as the colour gradient (moments of opacity * G * dL/dalpha; csrc/pergauss_bwd.hip,
 * unchanged); the second reaches means3D through z:  dL/dmeans3D += dL/dv * dv/dz * (m[2], m[6], m[10]) of viewmatrix, dv/dz = 1
 * (mode 0) or -1/z^2 (mode 1), z = m[2] x + m[6] y + m[10] z + m[14].
 *   - exactly one of (scales, rotations) / cov3D_precomp, as gsr_backward; the gradient buffers of the form that was not given
 *     may be NULL (dL_dcov3D with scales/rotations; dL_dscales, dL_drots with cov3D_precomp) and are not written.
 *   - accumulate = 0: dL_dmeans2D [P,3], dL_dopacity [P], dL_dmeans3D [P,3] and dL_dcov3D [P,6] or dL_dscales [P,3], dL_drots [P,4]
 *     are fully written, zeros included.
 *   - accumulate = 1: the result is ADDED element-wise (out = out + g) to buffers that a gsr_backward on the same stream has fully
 *     written: colour, depth and alpha losses of one render then need one set of gradient tensors.  Gaussians the forward pass
 *     never composited (gsr_composited_mask) are neither read nor written.
 *   - the colour inputs take no part: there is no dL_dcolors / dL_dsh here (they are zero).
 *   - NOT supported by this call: raw_params (the fused-step extension: logits, log-scales, un-normalised quaternions) and split SH
 *     tensors.  A render made with raw_params = 1 has no depth gradient through this header.
 *   - the option "deterministic_bwd" on: refused (GSR_ERR_INVALID_ARGUMENT, text naming the option).  The pass sums with float
 *     atomics and has no slot form; gradients may differ in the last bits from run to run.
 *   - workspace: gsr_depth_workspace_bytes(P) bytes = acc_rows(P) = P + P / 32 + 1024 accumulator rows of 64 bytes (P taken as 1
 *     when 0), rounded up to 256, plus 80 P bytes (rounded up to 256) where accumulate = 1 stages the per-Gaussian chain's result.
 *     Contents irrelevant before and after.  Only the rows that can be added into (composited Gaussians, replica rows) are cleared.
 *     Smaller: GSR_ERR_WORKSPACE.  gsr_depth_workspace_bytes needs no device.
 *   - P == 0: nothing to do.  R == 0: accumulate = 0 writes zeros, accumulate = 1 adds nothing.
 *
 * Same conventions as gsr.h: device pointers, float32, caller-owned buffers, matrices in gsr.h's layout, work enqueued on `stream`
 * (no host wait, no second stream), 0 = ok or a GSR_ERR_* code with its text in gsr_last_error(), never aborts.
 */
#ifndef GSR_DEPTH_H
#define GSR_DEPTH_H
#include <stddef.h>
#include <stdint.h>
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
#define GSR_DEPTH_EXPECTED 0
#define GSR_DEPTH_INVERSE 1
int32_t gsr_depth_workspace_bytes(int32_t P, size_t *bytes);
int32_t gsr_depth_forward(gsr_stream_t stream, int32_t P, int32_t W, int32_t H, int64_t R, int32_t mode,
                          const void *geom_ws, size_t geom_bytes, const void *binning_ws, size_t binning_bytes,
                          const void *img_ws, size_t img_bytes, float *out_depth /*[H,W] or NULL*/, float *out_alpha /*[H,W] or NULL*/);
int32_t gsr_depth_backward(gsr_stream_t stream, int32_t P, int32_t W, int32_t H, int64_t R, int32_t mode,
                           const float *means3D /*[P,3]*/, const int32_t *radii /*[P]*/, const float *scales /*[P,3] or NULL*/,
                           float scale_modifier, const float *rotations /*[P,4] or NULL*/, const float *cov3D_precomp /*[P,6] or NULL*/,
                           const float *viewmatrix, const float *projmatrix, const float *campos, float tanfovx, float tanfovy,
                           const float *dL_ddepth /*[H,W] or NULL*/, const float *dL_dalpha /*[H,W] or NULL*/,
                           const void *geom_ws, size_t geom_bytes, const void *binning_ws, size_t binning_bytes,
                           const void *img_ws, size_t img_bytes, void *ws, size_t ws_bytes, int32_t accumulate,
                           float *dL_dmeans2D /*[P,3]*/, float *dL_dopacity /*[P]*/, float *dL_dmeans3D /*[P,3]*/,
                           float *dL_dcov3D /*[P,6] or NULL*/, float *dL_dscales /*[P,3] or NULL*/, float *dL_drots /*[P,4] or NULL*/);
#ifdef __cplusplus
}
#endif
#endif
