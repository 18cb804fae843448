/*
 * gsr_density.h -- C ABI of adaptive density control on the device: the per-iteration statistics and the
 * clone / split / prune of all Gaussians with their Adam moments (part of libgsr_hip.so; kernels in csrc/density.hip).
 * "Next" row 8f-4 of SURVEY.md.  gaussian_transformer_amd/densify.py::DensityController, which restates the reference's
 * GaussianModel in torch index arithmetic, is the oracle of this path (tests/density_ref.py holds the rule below in torch).
 *
 * Same conventions as gsr.h: device pointers, float32, caller-owned buffers, enqueued on `stream`, 0 = ok or a GSR_ERR_* code
 * with its text in gsr_last_error(), no allocation inside, never aborts.  P = 0 is valid everywhere and launches nothing.
 *
 * ---- gsr_density_record: train.py:113-116 with scene/gaussian_model.py:405-407 (max_radii2D, add_densification_stats) ----
 * One launch, no host wait.  Row i is visible when visible[i] != 0, or, with visible == NULL, when radii[i] > 0.
 * For every visible row, in plain float32 without contraction:
 *     accum[i] += sqrtf(x * x + y * y);   denom[i] += 1;   max_radii[i] = max(max_radii[i], (float)radii[i])
 * with (x, y) = grad2d[i * grad_stride_floats + {0, 1}] (3 for means2D.grad; a view into a gradient arena is accepted through
 * its stride, grad_stride_floats >= 2).  Rows that are not visible are not touched.
 *
 * ---- gsr_densify_plan: scene/gaussian_model.py:349-403 (densify_and_clone, densify_and_split, densify_and_prune) decided
 *      once per Gaussian ----
 *     g      = accum / denom, NaN -> 0            (x / 0 with x > 0 stays +inf and is selected, as in torch)
 *     size   = max_k expf(scaling[k])
 *     hot    = g >= grad_threshold
 *     clone  = hot && size <= cut;   split = hot && size > cut                        (cut = percent_dense * extent)
 *     low    = sigmoid(opacity) < min_opacity
 *     big    = prune_world_size >= 0 && size > prune_world_size                       (0.1 * extent; negative: no size test)
 *     child_scaling[k] = logf(expf(scaling[k]) / (float)(0.8 * N))
 *     childbig = prune_world_size >= 0 && max_k expf(child_scaling[k]) > prune_world_size
 *     keep_self  = !split && !(low || big)
 *     keep_clone =  clone && !(low || big)
 *     keep_child =  split && !(low || childbig)
 * followed by ONE exclusive scan (rocPRIM, deterministic) that carries the ranks among keep_self, keep_clone, split and
 * keep_child rows at once, and a pass that files, for every row of the new state, which Gaussian it comes from.
 * Thresholds are floats: torch rounds a Python number to float32 when it compares a float32 tensor with it, so callers pass
 * float32(value).  grad_threshold must be > 0 (a clone has no statistics yet in the reference and is never split).
 * counts, four words {n_clone, n_split, n_pruned, P_new}, are kept in the workspace and copied to `counts_host` (pinned
 * host memory, 4 x uint32) on the stream; the caller waits for the stream once and reads them.  n_clone and n_split count
 * every selected row; n_pruned is what the reference's final prune removes (split parents not counted):
 *     n_pruned = (P - n_split - #keep_self) + (n_clone - #keep_clone) + N * (n_split - #keep_child).
 *
 * THE SCREEN-SIZE TEST IS NOT PART OF THE PLAN.  In the reference every append (densification_postfix :303-322) zeroes
 * max_radii2D before the final prune reads it, so `max_radii2D > max_screen_size` (:398) never selects a row:
 * max_screen_size only switches the world-size test on.  That behaviour is kept; callers pass prune_world_size < 0 when
 * max_screen_size is None and 0.1 * extent otherwise.
 *
 * ---- gsr_densify_apply: the optimiser-state surgery :258-347 (cat_tensors_to_optimizer, _prune_optimizer) in one launch ----
 * Writes the whole new state of up to GSR_DENSITY_MAX_GROUPS parameter groups from a plan.  Row order of the new state, the
 * reference's:
 *   1. surviving non-split originals in row order;
 *   2. surviving clones in the order of their originals;
 *   3. surviving children: child j of the k-th split row (k counted among all split rows, pruned or not) sits before the
 *      prune at j * n_split + k and reads noise[j * n_split + k]  (noise [N * n_split, 3], standard normal).
 * Survivors carry parameter and both moments; clones and children get the parent's parameter and zero moments, except
 *   role GSR_DENSITY_SCALING (width 3): children get child_scaling;
 *   role GSR_DENSITY_XYZ (width 3): children get R(rotation / |rotation|) . (noise * expf(scaling)) + xyz, with the rotation
 *   matrix of utils/general_utils.py:78-99 (build_rotation).
 *   Both are evaluated in float64 from the float32 inputs and rounded once (the float32 nearest to the formula's value; the
 *   plan's childbig decision uses the float32 child_scaling above).
 * src_exp_avg / src_exp_avg_sq / dst_exp_avg / dst_exp_avg_sq may all four be NULL (the optimiser has no state yet).
 * A group of width 0 is skipped.  No atomics: the output is bit-identical from run to run.  dst buffers hold P_new rows and must
 * not overlap the sources.  P, N, n_split and P_new must be those of the plan in `ws`; a kernel that finds other counts in the
 * workspace writes nothing.
 *
 * Indices are 32-bit: P * (N + 1) >= 2^31 is refused, and so is P_new * width >= 2^32.
 */
#ifndef GSR_DENSITY_H
#define GSR_DENSITY_H
#include <stddef.h>
#include <stdint.h>
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
#define GSR_DENSITY_MAX_GROUPS 16
#define GSR_DENSITY_COPY 0
#define GSR_DENSITY_XYZ 1
#define GSR_DENSITY_SCALING 2
typedef struct {
    const float *src;             /* [P, width] */
    const float *src_exp_avg;     /* [P, width] or NULL */
    const float *src_exp_avg_sq;  /* [P, width] or NULL */
    float *dst;                   /* [P_new, width] */
    float *dst_exp_avg;           /* [P_new, width] or NULL */
    float *dst_exp_avg_sq;        /* [P_new, width] or NULL */
    int32_t width_floats;
    int32_t role;                 /* GSR_DENSITY_COPY / _XYZ / _SCALING */
} gsr_density_group_t;
int32_t gsr_density_record(gsr_stream_t stream, int32_t P, const float *grad2d, int32_t grad_stride_floats, const int32_t *radii /*[P]*/,
                           const uint8_t *visible /*[P] or NULL*/, float *accum /*[P]*/, float *denom /*[P]*/, float *max_radii /*[P]*/);
int32_t gsr_densify_plan_workspace(int32_t P, int32_t N, size_t *bytes);
int32_t gsr_densify_plan(gsr_stream_t stream, int32_t P, const float *opacity /*[P] logits*/, const float *scaling /*[P,3] log*/,
                         const float *accum /*[P]*/, const float *denom /*[P]*/, float grad_threshold, float min_opacity, float cut,
                         float prune_world_size, int32_t N, uint32_t *counts_host /*[4] pinned*/, void *ws, size_t ws_bytes);
int32_t gsr_densify_apply(gsr_stream_t stream, int32_t P, int32_t N, int32_t n_split, int32_t P_new, int32_t n_groups,
                          const gsr_density_group_t *groups /* host array */, const float *scaling /*[P,3]*/, const float *rotation /*[P,4]*/,
                          const float *noise /*[N * n_split, 3]*/, const void *ws, size_t ws_bytes);
#ifdef __cplusplus
}
#endif
#endif
