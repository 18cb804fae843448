/*
 * gsr_loss.h -- C ABI of the fused training loss (part of libgsr_hip.so).  "Next" row 8f-1 of SURVEY.md.
 *
 * Replaces, for the train step of the reference (train.py:91-92),
 *     Ll1  = l1_loss(image, gt_image)                                   utils/loss_utils.py:17-18
 *     loss = (1 - lambda_dssim) * Ll1 + lambda_dssim * (1 - ssim(image, gt_image))   utils/loss_utils.py:33-63
 * (five grouped 11x11 convolutions + elementwise ops + their autograd, ~11.6 ms at 3x1080x1920 on MI355X)
 * with one fused kernel per direction.  Same conventions as gsr.h: device pointers, float32, caller-owned
 * buffers, work enqueued on `stream`, 0 = ok.
 */
#ifndef GSR_LOSS_H
#define GSR_LOSS_H
#include <stddef.h>
#include <stdint.h>
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif

/* bytes of the workspace written by the forward and read by the backward */
int32_t gsr_l1_ssim_workspace(int32_t C, int32_t H, int32_t W, size_t *bytes);

/* img, gt: [C,H,W].  out3 (device, 3 floats): loss, mean |img-gt|, mean SSIM. */
int32_t gsr_l1_ssim_forward(gsr_stream_t stream, int32_t C, int32_t H, int32_t W, const float *img, const float *gt,
                            float lambda_dssim, float *out3, void *ws, size_t ws_bytes);

/* grad_img [C,H,W] = grad_loss[0] * d loss / d img  (grad_loss: device scalar, NULL means 1). */
int32_t gsr_l1_ssim_backward(gsr_stream_t stream, int32_t C, int32_t H, int32_t W, const float *img, const float *gt,
                             float lambda_dssim, const float *grad_loss, const void *ws, size_t ws_bytes, float *grad_img);

/*
 * The same loss over B views of [3,H,W] each: the image loss of the stacked trainer's step (train_stacked_transformer.py:203-222).
 *     L1   = mean |s(x) - s(y)|  over all B*3*H*W entries
 *     SSIM = mean of the SSIM map over all B*3*H*W entries (padding and constants as above, per channel plane; no window crosses a
 *            view; the window's normaliser is the sum of its 11 float32 taps rounded once, as torch computes it: one place above
 *            the single-image kernel's, which adds them one by one)
 *     loss = w_l1 * L1 + w_ssim * (1 - SSIM)
 * sanitize != 0: every pixel of images and targets is read as s(x) = clamp(nan_to_num(x), 0, 1) (NaN -> 0, +inf -> 1, -inf -> 0)
 * and the gradient is exactly 0 where the image pixel is not finite or outside [0, 1] (bounds included: the gradient passes at 0 and 1),
 * as torch.clamp / torch.nan_to_num differentiate; sanitize == 0: s(x) = x.  w_l1 = 0.5 / B, w_ssim = 0.02 / B is the reference's
 * step; B = 1, w_l1 = 1 - lambda, w_ssim = lambda the loss above.
 *
 * imgs, gts, grad_imgs are HOST arrays of B DEVICE pointers, read before the call returns; all views share H and W.  One kernel
 * launch carries the pointers of GSR_VIEWS_LOSS_MAX_B views in its arguments; a larger B is served by further launches into the
 * same workspace, and one finishing kernel sums over all of them.  The sums are taken in a fixed order: results are bit-identical
 * from run to run.  B < 1, H < 1, W < 1, a NULL among imgs / gts / the workspace, or a workspace smaller than the workspace call
 * reports: GSR_ERR_INVALID_ARGUMENT with its text in the last-error string, and nothing is launched.
 */
#define GSR_VIEWS_LOSS_MAX_B 16
int32_t gsr_views_loss_workspace(int32_t B, int32_t H, int32_t W, size_t *bytes);

/* out3 (device, 3 floats): loss, L1, SSIM.  terms (device, [B,3]): per view mean |s(x)-s(y)|, mean SSIM, mean (s(x)-s(y))^2. */
int32_t gsr_views_loss_forward(gsr_stream_t stream, int32_t B, int32_t H, int32_t W, const float *const *imgs, const float *const *gts,
                               float w_l1, float w_ssim, int32_t sanitize, float *out3, float *terms, void *ws, size_t ws_bytes);

/* grad_imgs[b] [3,H,W] = grad_loss[0] * d loss / d imgs[b]  (grad_loss: device scalar, NULL means 1); grad_imgs[b] = NULL: view b
 * wants no gradient and nothing is stored for it.  Same arguments as the forward that filled ws. */
int32_t gsr_views_loss_backward(gsr_stream_t stream, int32_t B, int32_t H, int32_t W, const float *const *imgs, const float *const *gts,
                                float w_l1, float w_ssim, int32_t sanitize, const float *grad_loss, const void *ws, size_t ws_bytes,
                                float *const *grad_imgs);

#ifdef __cplusplus
}
#endif
#endif
