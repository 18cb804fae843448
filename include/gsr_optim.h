/*
 * gsr_optim.h -- C ABI of the Adam step over the Gaussian parameter groups (part of libgsr_hip.so).
 * "Next" row 8f-1 of SURVEY.md (the fused step around the rasterizer).
 *
 * Replaces, for the training loop, the `self.optimizer.step()` of train.py:126 on the optimiser the reference builds at
 * scene/gaussian_model.py:155-164: torch.optim.Adam over six one-tensor groups, lr per group, betas (0.9, 0.999),
 * eps 1e-15, no weight decay, no amsgrad.  Same update, element for element:
 *     m = m + (g - m) * (1 - beta1);  v = v * beta2 + g * g * (1 - beta2)
 *     p = p - (lr / (1 - beta1^step)) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * All groups go through ONE launch (28 bytes of traffic per element, nothing else): torch's fused path takes one
 * launch sequence per group and ~2x the time at 59 M floats.
 * Same conventions as gsr.h: device pointers, float32, caller-owned buffers, enqueued on `stream`, 0 = ok.
 *
 * The masked step (opt-in; the "sparse Adam" of the mainline 3DGS trainer).  Every group is [P, w] row-major with w = n / P
 * (the reference's groups: w = 3, 3, 3 (M - 1), 1, 3, 4), and a mask of P entries says which Gaussians a view saw:
 *   - a row whose entry is set receives exactly the update above: same formula, same float constants derived on the host in
 *     double, the group's `step`; its param / exp_avg / exp_avg_sq come out bit for bit as the dense call leaves them;
 *   - a row whose entry is clear keeps param, exp_avg and exp_avg_sq bit for bit; its grad is not needed, and a NaN or Inf in any
 *     of its four arrays stays where it is and reaches nothing else;
 *   - `step` stays one count per tensor, advanced by the caller on every call, so a row seen for the first time at step t is
 *     corrected with t (as torch.optim.SparseAdam); there is no per-row counter and the state layout is that of the dense step.
 * This is NOT dense Adam on a gradient with zero rows: there a row with an all-zero gradient decays its moments and coasts on
 * its momentum, here it stands still.  That difference is the point: the reverse pass writes exact zeros into the rows of every
 * Gaussian the view did not composite (91 % of them for one camera of BASELINE config 3), and those rows are not read at all.
 * One launch for all groups, no atomics, no workspace, no read-back: bit-identical from run to run for a given mask.  Of the
 * masks at hand, gsr_forward's radii (> 0) are reproducible; gsr_composited_mask's bytes are tighter but may mark a few extra
 * rows from stale workspace bytes, so a run that must be reproducible uses the radii.
 */
#ifndef GSR_OPTIM_H
#define GSR_OPTIM_H
#include <stddef.h>
#include <stdint.h>
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
#define GSR_ADAM_MAX_GROUPS 16
typedef struct {
    float *param;          /* [n] updated in place */
    const float *grad;     /* [n] */
    float *exp_avg;        /* [n] first moment, updated in place */
    float *exp_avg_sq;     /* [n] second moment, updated in place */
    int64_t n;
    float lr;
    int32_t step;          /* 1-based step count of this group AFTER this update (torch keeps it per tensor) */
} gsr_adam_group_t;
/* betas and eps are doubles: torch derives 1 - beta and the bias corrections in double (1 - 0.999f is 1.3e-5 off 0.001). */
int32_t gsr_adam_step(gsr_stream_t stream, int32_t n_groups, const gsr_adam_group_t *groups /* host array */, double beta1,
                      double beta2, double eps);

#define GSR_ADAM_MASK_BYTES 0   /* uint8 / bool [P]: visible iff != 0; any address */
#define GSR_ADAM_MASK_RADII 1   /* int32 [P]: visible iff > 0 (gsr_forward's radii as they are, without a `radii > 0` launch) */
/* INVALID_ARGUMENT before anything is enqueued: n_groups outside 1..GSR_ADAM_MAX_GROUPS, P < 0, a NULL mask with P > 0, an unknown
 * mask_kind, an int32 mask off a 4-byte boundary, a group whose n is no multiple of P or exceeds 2^31 - 1, a NULL pointer in a
 * group with n > 0.  P = 0 and groups with n = 0 are legal and do nothing. */
int32_t gsr_adam_step_masked(gsr_stream_t stream, int32_t n_groups, const gsr_adam_group_t *groups /* host array */, double beta1,
                             double beta2, double eps, int32_t P, const void *mask /* device */, int32_t mask_kind);
#ifdef __cplusplus
}
#endif
#endif
