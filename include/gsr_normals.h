/*
 * gsr_normals.h -- C ABI of the surface-normal feature: per-Gaussian normals, and the fused depth-normal consistency loss of 2DGS
 * (Huang et al., SIGGRAPH 2024) on the maps a render already gives (part of libgsr_hip.so; kernels and entry points in
 * csrc/normals.hip).  Nothing here touches the colour path, a list or a record: the normal MAP is a three-channel feature map
 * (gsr_features.h blends and differentiates it), and the loss is image-space work on [H,W] tensors.
 *
 * ---- per-Gaussian normals ----
 * gsr_gaussian_normals_forward, per Gaussian g (float32, every operation rounded as written, no FMA contraction):
 *     k    = the index of the smallest of scales[g, 0..2]; the scan over 0, 1, 2 uses strict <, so ties go to the lowest index
 *     n_w  = column k of quat_to_rot(rotations[g]): the quaternion (r, x, y, z) AS GIVEN, exactly as the covariance is built from it
 *            (csrc/gsr_device.h: cov3d_from_scale_rot).  NO normalisation: a non-unit quaternion gives a non-unit normal.
 *     n_v[i] = m[i] n_w.x + m[4+i] n_w.y + m[8+i] n_w.z          m = viewmatrix in gsr.h's layout, its rotation part only
 *     p_v  = (m[i] p.x + m[4+i] p.y + m[8+i] p.z + m[12+i])_i     the mean in view space
 *     if n_v.x p_v.x + n_v.y p_v.y + n_v.z p_v.z > 0 (added left to right): n_v = -n_v, so the stored normal faces the camera;
 *            a dot product of exactly 0 does not flip
 *     out_normals[g] = n_v;   out_axis[g] = k | (flipped << 2)    (out_axis may be NULL)
 * Gaussians outside the frustum are computed like any other.  P == 0: nothing to do, nothing is looked at.
 *
 * gsr_gaussian_normals_backward writes dL_drots [P,4] IN FULL: the derivative of column k's polynomial in (r, x, y, z), taken through
 * the view rotation and the recorded sign, both read from axis[g] (bits 0-1: k; bit 2: flipped; k == 3 is read as 2).  Sums in float64,
 * rounded once.  NO GRADIENT GOES TO SCALES OR MEANS: k and the sign are piecewise constant in them, so their derivative is zero
 * wherever it exists.  None goes to the viewmatrix either (no camera gradient of the normal map is formed).
 *
 * ---- depth to normals, and the loss ----
 * depth [H,W] is the "expected" map of gsr_depth.h (sum z alpha T, NOT normalised), alpha [H,W] the accumulated opacity of the same
 * render, normals [3,H,W] the rendered, unnormalised normal map N.  With
 *     D        = depth / alpha
 *     ray(x,y) = (((2x+1)/W - 1) tanfovx, ((2y+1)/H - 1) tanfovy, 1)          (the inverse of ndc_to_pixel)
 *     Q(x,y)   = D(x,y) ray(x,y)
 *     c        = (Q(x,y+1) - Q(x,y-1)) x (Q(x+1,y) - Q(x-1,y))
 * a pixel is VALID iff it is interior (0 < x < W-1, 0 < y < H-1), it and its four neighbours have alpha >= alpha_min (a float32
 * comparison), and |c|^2 > 1e-30.  At valid pixels n~ = c / |c| (a fronto-parallel plane gives (0,0,-1): facing the camera, as the
 * Gaussians' normals do); elsewhere n~ = 0.
 *     loss = (1 / (H W)) sum_valid A (1 - N . n~)        A = the pixel's alpha TAKEN AS A CONSTANT (2DGS's alpha.detach())
 *     out2 = (loss, valid pixels / (H W))                 out_surf [3,H,W] (or NULL) = n~, exact zeros at invalid pixels
 *     dL/dN      = -A n~ / (H W)
 *     dL/dn~     = -A N / (H W), through the normalisation and the cross product to the four neighbours' Q, from there to depth
 *                  (factor 1/alpha) and alpha (factor -depth/alpha^2)
 * Invalid pixels contribute nothing.  Every output is written in full, the zeros included.  The arithmetic per pixel is float64 on
 * the float32 inputs, rounded to float32 once at the store.  Inputs are taken as finite.
 *
 *   - forward: one workgroup per 32 x 8 tile (GSR_NORMAL_TILE_X x GSR_NORMAL_TILE_Y), one-pixel halo of D in LDS; each workgroup
 *     leaves (sum, valid count) as two doubles in the workspace and a finishing kernel adds them in a FIXED order in float64 -- 256
 *     contiguous chunks of the tile index each in index order, then the chunk sums in index order -- and rounds once: the result is
 *     bit-identical from run to run.  No atomics.
 *   - backward: a GATHER -- each pixel collects from the up-to-four stencils that contain it, which its workgroup RECOMPUTES from a
 *     two-pixel halo in LDS (nothing of the forward call is kept, no workspace is needed, and the call may run without a forward
 *     call).  No atomics; bit-identical from run to run.  grad_loss: a DEVICE scalar the three outputs are multiplied with after
 *     their rounding (NULL: 1), so a power of two scales exactly.  Any of the three outputs may be NULL; all NULL: nothing runs.
 *   - workspace (forward only): gsr_normal_loss_workspace(H, W) = 16 * ceil(W/32) * ceil(H/8) bytes rounded up to 256.  Needs no
 *     device.  Contents irrelevant before and after.
 *   - an image without an interior (H < 3 or W < 3) is no error: loss 0, fraction 0, zero gradients.
 *   - refused (GSR_ERR_INVALID_ARGUMENT, the text names the call), in this order: H < 1 or W < 1 ("bad sizes"); H > 524280 or
 *     W > 1048576 ("image too large"); alpha_min <= 0 or not a number; a NULL input or out2 (forward) / a NULL input (backward);
 *     then a short workspace (GSR_ERR_WORKSPACE).  A refused call writes nothing.
 *
 * Same conventions as gsr.h: device pointers, float32, caller-owned buffers, work enqueued on `stream` (no host wait, no second
 * stream), 0 = ok or a GSR_ERR_* code with its text in gsr_last_error(), never aborts.
 */
#ifndef GSR_NORMALS_H
#define GSR_NORMALS_H
#include <stddef.h>
#include <stdint.h>
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
#define GSR_NORMAL_TILE_X 32
#define GSR_NORMAL_TILE_Y 8
int32_t gsr_gaussian_normals_forward(gsr_stream_t stream, int32_t P, const float *means3D /*[P,3]*/, const float *scales /*[P,3]*/,
                                     const float *rotations /*[P,4]*/, const float *viewmatrix /*[16]*/,
                                     float *out_normals /*[P,3]*/, int32_t *out_axis /*[P] or NULL*/);
int32_t gsr_gaussian_normals_backward(gsr_stream_t stream, int32_t P, const float *rotations /*[P,4]*/, const float *viewmatrix /*[16]*/,
                                      const int32_t *axis /*[P]*/, const float *dL_dnormals /*[P,3]*/, float *dL_drots /*[P,4]*/);
int32_t gsr_normal_loss_workspace(int32_t H, int32_t W, size_t *bytes);
int32_t gsr_normal_loss_forward(gsr_stream_t stream, int32_t H, int32_t W, float tanfovx, float tanfovy, float alpha_min,
                                const float *depth /*[H,W]*/, const float *alpha /*[H,W]*/, const float *normals /*[3,H,W]*/,
                                float *out2 /*[2]*/, float *out_surf /*[3,H,W] or NULL*/, void *ws, size_t ws_bytes);
int32_t gsr_normal_loss_backward(gsr_stream_t stream, int32_t H, int32_t W, float tanfovx, float tanfovy, float alpha_min,
                                 const float *depth /*[H,W]*/, const float *alpha /*[H,W]*/, const float *normals /*[3,H,W]*/,
                                 const float *grad_loss /*device scalar, NULL = 1*/, float *dL_ddepth /*[H,W] or NULL*/,
                                 float *dL_dalpha /*[H,W] or NULL*/, float *dL_dnormals /*[3,H,W] or NULL*/);
#ifdef __cplusplus
}
#endif
#endif
