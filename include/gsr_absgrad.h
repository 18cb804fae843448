/*
 * gsr_absgrad.h -- C ABI of absgrad: per-Gaussian sums of |dL/dmeans2D| over the pixels of a render
 * (part of libgsr_hip.so; kernels and entry points in csrc/absgrad.hip).
 *
 * gsr_backward forms dL/dmeans2D as a SIGNED sum over the pixels a splat touches.  A splat too large for the detail under it is
 * pulled one way on one side and the other way on the other; the terms cancel and the norm density control thresholds stays small
 * (the over-reconstruction case of AbsGS, Ye et al. 2024; gsplat's `absgrad`).  This call sums the absolute values instead:
 *
 *     absgrad[g]          = ( sum_pixels |t_x(pixel, g)| , sum_pixels |t_y(pixel, g)| )
 *     dL/dmeans2D[g, 0:2] = ( sum_pixels  t_x            , sum_pixels  t_y            )         (what gsr_backward returns)
 *
 * The absolute value is taken per (pixel, Gaussian) pair, inside a reverse walk of its own, so nothing gsr_backward returns can
 * stand in for it.  For a pixel and a blended list entry i of Gaussian g, with the forward pass's own decisions (csrc/gsr_device.h:
 * skipped on power > 0 and on alpha < 1/255, the walk ends at the pixel's recorded last contributor) and the 0.99 cap
 * straight-through, as in gsr_backward:
 *     u_i        = sum_ch gC[ch] rgb_g[ch]                      gC = dL_dcolor at the pixel, rgb from the forward pass's record
 *     S_i        = sum_{j behind i, blended} u_j alpha_j T_j
 *     dL/dalpha_i = u_i T_i - S_i / (1 - alpha_i) - (sum_ch gC[ch] bg[ch]) T_final / (1 - alpha_i)
 *     s          = opacity_g G dL/dalpha_i                      (the alpha before the cap)
 *     d          = centre_g - pixel
 *     t_x = -0.5 W s (conic.xx d_x + conic.xy d_y),   t_y = -0.5 H s (conic.xy d_x + conic.yy d_y)
 * The units are those of gsr_backward's dL_dmeans2D[:, 0:2].
 *
 * ONLY THE COLOUR IMAGE'S LOSS ENTERS: dL_dcolor is the gradient of the loss with respect to gsr_forward's out_color.  Losses on
 * the depth, alpha and feature maps of the same render (gsr_depth.h, gsr_features.h) add nothing to absgrad, whatever graph they
 * share with the colour loss.  The clamp of an SH colour at 0 plays no part either: the record's rgb is the clamped value.
 *
 * gsr_absgrad_backward runs AFTER the gsr_forward that filled the three workspaces (geometry, binning, image) and re-reads what it
 * left on the device, as gsr_depth.h's calls do: the per-tile lists, the records, the reachability bytes, and per pixel T_final and
 * the last contributor.  No per-Gaussian stage and no list build runs again; gsr_backward is neither needed nor changed, and may
 * run before or after this call.  Works for renders made with raw_params = 1 as for any other: only the records are read.
 *
 *   - accumulate = 0: absgrad [P,2] (and signed_sum, if given) is written in full; a Gaussian that was culled or that no wave
 *     staged gets an exact +0.0.
 *   - accumulate = 1: the result is ADDED element-wise (out = out + g); rows of Gaussians without a gradient are neither read
 *     nor written.  Many views then sum into one [P,2] tensor.
 *   - signed_sum [P,2] or NULL: the same walk's sums of t_x, t_y without the absolute value, i.e. this walk's dL/dmeans2D[:, 0:2].
 *     It exists so that the walk can be held against gsr_backward; NULL selects a kernel that forms no such sums.
 *   - the option "deterministic_bwd" on: refused (GSR_ERR_INVALID_ARGUMENT, text naming the option).  The pass sums with float
 *     atomics and has no slot form; results may differ in the last bits from run to run.
 *   - workspace: gsr_absgrad_workspace_bytes(P) bytes = two buffers of acc_rows(P) = P + P / 32 + 1024 rows of 8 bytes (P taken as
 *     1 when 0), each rounded up to 256.  Contents irrelevant before and after.  Only the rows that can be added into (composited
 *     Gaussians, replica rows) are cleared.  Smaller: GSR_ERR_WORKSPACE.  gsr_absgrad_workspace_bytes needs no device.
 *   - P == 0: nothing to do.  R == 0 (R = the pair count gsr_forward reported): accumulate = 0 writes zeros, accumulate = 1 adds
 *     nothing.
 *   - refused, in this order: bad sizes or an image too large; a missing bg, dL_dcolor, geometry, image or own workspace or absgrad;
 *     a missing binning workspace with R > 0; the option above (all GSR_ERR_INVALID_ARGUMENT); a short workspace
 *     (GSR_ERR_WORKSPACE); P too large for the 28-bit accumulator row index (GSR_ERR_INVALID_ARGUMENT); a geometry, image or
 *     binning workspace smaller than gsr_forward's (GSR_ERR_WORKSPACE).  A refused call writes nothing.
 *
 * Same conventions as gsr.h: device pointers, float32, caller-owned buffers, work enqueued on `stream` (no host wait, no second
 * stream), 0 = ok or a GSR_ERR_* code with its text in gsr_last_error(), never aborts.
 */
#ifndef GSR_ABSGRAD_H
#define GSR_ABSGRAD_H
#include <stddef.h>
#include <stdint.h>
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
int32_t gsr_absgrad_workspace_bytes(int32_t P, size_t *bytes);
int32_t gsr_absgrad_backward(gsr_stream_t stream, int32_t P, int32_t W, int32_t H, int64_t R,
                             const float *bg /*[3]*/, const float *dL_dcolor /*[3,H,W]*/,
                             const void *geom_ws, size_t geom_bytes, const void *binning_ws, size_t binning_bytes,
                             const void *img_ws, size_t img_bytes, void *ws, size_t ws_bytes, int32_t accumulate,
                             float *absgrad /*[P,2]*/, float *signed_sum /*[P,2] or NULL*/);
#ifdef __cplusplus
}
#endif
#endif
