/*
 * gsr_pose.h -- C ABI of the camera gradients of a render: dL/dviewmatrix, dL/dprojmatrix, dL/dcampos
 * (part of libgsr_hip.so; kernels and entry points in csrc/pose_grad.hip).
 *
 * gsr_pose_backward runs AFTER the reverse pass whose loss it differentiates -- gsr_backward (kind GSR_POSE_COLOR = 0) or
 * gsr_depth_backward (kind GSR_POSE_DEPTH_EXPECTED = 1: expected depth, GSR_POSE_DEPTH_INVERSE = 2: inverse depth; the alpha map's
 * gradient rides with either) -- and re-uses what that call left on the device: the per-Gaussian moment sums in the accumulator rows at the
 * start of its workspace (sum s d, sum s d d^T, sum s, the colour gradient; for the maps also sum dL/dv in slot 9).  No compositing
 * runs again.  The Gaussians' own gradients, the colour path and the map path are not changed by this header and do not know of it.
 *
 * The one thing this adds to gsr.h's and gsr_depth.h's "contents irrelevant after": `acc_ws` is the workspace the matching gsr_backward
 * (kind 0) or gsr_depth_backward (kinds 1, 2) was given, UNMODIFIED since that call, and this call is enqueued on the same stream.
 * Only its first acc_rows(P) = P + P / 32 + 1024 rows of 64 bytes (P taken as 1 when 0) are read.  Every reverse route leaves each
 * Gaussian's final sums there before its per-Gaussian stage reads them: the classic, persistent and length-ordered kernels add into the
 * rows (replica rows included), the deterministic mode's slot reduction stores into them, and the dense per-Gaussian stage reads the
 * same rows as the streaming one.
 *
 * Outputs, in gsr.h's memory layout (x' = m[0] x + m[4] y + m[8] z + m[12]), fully written, zeros included; any one or two of them
 * may be NULL (all three NULL is refused):
 *     dL_dviewmatrix [16]   entries 3, 7, 11, 15 are exactly +0 (the renderer never reads the matrix's fourth column)
 *     dL_dprojmatrix [16]   entries 2, 6, 10, 14 are exactly +0 (clip-space z is never read)
 *     dL_dcampos     [3]    zero unless kind 0 with shs
 * A Gaussian contributes iff the per-Gaussian stage treats it as visible: radii > 0 and its composited byte equals the frame's mark.
 * Its accumulator row has its replica rows folded in as that stage folds them.  The terms are the ones csrc/pergauss_bwd.hip forms, in
 * float32, on the same helpers and with the same compile flags, so the camera gradient is consistent with dL/dmeans3D:
 *   projection (kinds 0, 1, 2):  ph = p Pm, mw = 1 / (ph[3] + 1e-7), g0 = dm2[0] mw, g1 = dm2[1] mw,
 *       g3 = -(dm2[0] ph[0] + dm2[1] ph[1]) mw^2;  dPm[4 j + c] += p_j g_c (j = 0..2), dPm[12 + c] += g_c, c in {0, 1, 3}
 *   EWA (inside the same 1 / (det^2 + 1e-7) != 0 guard): with dT[2][3], (dtx, dty, dtz), J00 = fx / tz, J11 = fy / tz, J02, J12 of the
 *       clamped t and Wm[r][k] = V[4 k + r]:  dWm[0][k] = J00 dT[0][k], dWm[1][k] = J11 dT[1][k], dWm[2][k] = J02 dT[0][k] + J12 dT[1][k];
 *       dV[4 k + r] += dWm[r][k] + p_k dt_r, dV[12 + r] += dt_r (r, k in 0..2); dtx, dty carry the 1.3 tanfov clamp masks
 *   view direction (kind 0 with shs): dcampos[ax] -= (ddir[ax] - dir[ax] dot) / |p - campos|, the SH clamp mask applied to the colour
 *       gradient first
 *   depth value (kinds 1, 2): g = (sum dL/dv) dv/dz, dv/dz = 1 or -1 / z^2, z as gsr_depth_backward forms it;
 *       dV[4 k + 2] += p_k g, dV[14] += g
 * Discrete decisions (cull, radius, tile membership, order, skips, stop) are constants, and the 0.99 cap and the clamped coordinate
 * are straight-through, as everywhere else.
 *
 * Summation: the 27 live sums are accumulated in float64 (per lane products in float32, converted; a fixed shuffle tree per wave, the
 * four waves of a workgroup through LDS, one row of 32 doubles per workgroup; a second kernel adds every eighth row in index order per
 * lane and a fixed tree) and rounded to float32 once.  No atomics: for identical accumulator rows the result is bit-identical from run to run, so with
 * the option "deterministic_bwd" on, kind 0 is bitwise reproducible.
 *
 *   - exactly one of (scales, rotations) / cov3D_precomp; kind 0: exactly one of shs / colors_precomp, D in 0..3, M >= (D + 1)^2 with
 *     shs; kinds 1, 2: shs and colors_precomp are not read.
 *   - workspace: gsr_pose_workspace_bytes(P) = ceil(P / 256) rows of 256 bytes (at least one), 16-byte aligned as acc_ws is (else
 *     GSR_ERR_INVALID_ARGUMENT).  Contents irrelevant before and after.
 *     Smaller, or acc_bytes below the accumulator rows: GSR_ERR_WORKSPACE.  gsr_pose_workspace_bytes needs no device.
 *   - P == 0 or R == 0 (R = the pair count gsr_forward reported): zeros are written and no workspace is read.
 *   - NOT supported by this call: raw_params (the fused-step extension: logits, log-scales, un-normalised quaternions) and split SH
 *     tensors, as in gsr_depth.h.  A render made with raw_params = 1 has no camera gradient through this header.
 *
 * Same conventions as gsr.h: device pointers, float32, caller-owned buffers, work enqueued on `stream` (no host wait, no second
 * stream), 0 = ok or a GSR_ERR_* code with its text in gsr_last_error(), never aborts.
 */
#ifndef GSR_POSE_H
#define GSR_POSE_H
#include <stddef.h>
#include <stdint.h>
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
#define GSR_POSE_COLOR 0
#define GSR_POSE_DEPTH_EXPECTED 1
#define GSR_POSE_DEPTH_INVERSE 2
int32_t gsr_pose_workspace_bytes(int32_t P, size_t *bytes);
int32_t gsr_pose_backward(gsr_stream_t stream, int32_t kind, int32_t P, int32_t D, int32_t M, int32_t W, int32_t H, int64_t R,
                          const float *means3D /*[P,3]*/, const int32_t *radii /*[P]*/, const float *shs /*[P,M,3] or NULL*/,
                          const float *colors_precomp /*[P,3] or NULL*/, const float *scales /*[P,3] or NULL*/, float scale_modifier,
                          const float *rotations /*[P,4] or NULL*/, const float *cov3D_precomp /*[P,6] or NULL*/,
                          const float *viewmatrix, const float *projmatrix, const float *campos, float tanfovx, float tanfovy,
                          const void *geom_ws, size_t geom_bytes, const void *acc_ws, size_t acc_bytes, void *ws, size_t ws_bytes,
                          float *dL_dviewmatrix /*[16] or NULL*/, float *dL_dprojmatrix /*[16] or NULL*/, float *dL_dcampos /*[3] or NULL*/);
#ifdef __cplusplus
}
#endif
#endif
