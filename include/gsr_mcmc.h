/*
 * gsr_mcmc.h -- C ABI of MCMC density control on the device (part of libgsr_hip.so; kernels in csrc/mcmc.hip): relocation of dead
 * Gaussians onto live ones, growth by a factor the host knows in advance, the opacity-gated position noise and the two regularisers
 * of "3D Gaussian Splatting as Markov Chain Monte Carlo" (Kheradmand et al., 2024).  gaussian_transformer_amd/densify.py::
 * MCMCController states the same rule in torch index arithmetic and is the oracle of this path; tests/mcmc_ref.py holds it in
 * Python integers and 50-digit decimals.
 *
 * Same conventions as gsr.h: device pointers, float32, caller-owned buffers, enqueued on `stream`, 0 = ok or a GSR_ERR_* code
 * with its text in gsr_last_error(), no allocation inside, never aborts.  P = 0 is valid everywhere and launches nothing.
 * NO ENTRY POINT WAITS FOR THE HOST.
 *
 * ---- the rule (gsr_mcmc_plan) ----
 * Inputs: opacity [P] as logits, scaling [P,3] as logs.  In the formulas x is the corrected opacity, not a position.
 *   dead_i = opacity_i <= L        L = float32(log(m / (1 - m))), evaluated by the host once in float64 (m = min_opacity): the
 *                                  comparison is on the logit, neither side evaluates a transcendental for a decision
 *   w_i    = 0 for a dead row, else (uint32) floor(s64(opacity_i) * 2^20 + 0.5), s64 the sigmoid evaluated in float64
 *   C      = inclusive prefix sum of w in uint64: exact, independent of the order of summation; total = C[P-1] < 2^51
 * Draws, from caller-supplied float32 uniforms u_j in [0, 1):
 *   t_j    = min((uint64) floor((double)u_j * (double)total), total - 1)      one IEEE double multiply, no contraction
 *   src_j  = the smallest i with C_i > t_j
 * RELOCATE (GSR_MCMC_RELOCATE; P unchanged, applied in place): n = n_dead draws; u holds at least P entries of which the first n
 *   are used, so a caller that always draws P numbers consumes its generator independently of n_dead and need not know n_dead.
 *   The destination of draw j is the j-th dead row in row order.  total == 0 (every row dead): nothing is drawn, nothing changes.
 * GROW (GSR_MCMC_GROW; out of place, like gsr_densify_apply): n = n_draws draws (the host computes
 *   n = min(cap_max, (P * 105) / 100) - P in integer arithmetic); appended row P + j is the copy of src_j.  n_draws == 0 is a no-op.
 *   total == 0: the host has sized the new buffers without asking the device, so the n rows are still appended: row P + j is
 *   the plain copy of row j mod P with zero moments, nothing is drawn and no source is corrected (counts n_draws = n_sources = 0).
 * c_i = number of draws with src_j = i (an integer histogram: integer atomics, order-independent);  N_i = min(c_i + 1, n_max),
 *   n_max in 1..GSR_MCMC_N_MAX (51; all binomials up to C(51, .) are exact in double).
 * CORRECTION of every source (every row with c_i > 0), evaluated in float64 from the float32 inputs and rounded once at the end:
 *   o = s64(opacity_i)
 *   x = 1 - (1 - o)^(1 / N_i)
 *   D = sum_{k=0}^{N-1} C(N, k+1) (-1)^k x^(k+1) / sqrt(k+1)
 *       (= sum_{m=1..N} sum_{k=0..m-1} C(m-1, k) (-1)^k x^(k+1) / sqrt(k+1) by the hockey-stick identity; D > 0 on (0, 1])
 *   scaling_new[a] = float32(scaling_i[a] + log(o / D))                      a = 0, 1, 2;  D uses the unclamped x
 *   o_c = clamp(x, m, 1 - 2^-23);   opacity_new = float32(log(o_c / (1 - o_c)))
 *   For N = 1, x = o, D = o and nothing changes.  (1 - o is evaluated as s64(-opacity_i) and x as -expm1(log(1 - o) / N): the same
 *   numbers, without the cancellation of the literal form.)
 * counts, four words {n_dead, n_draws, n_sources, P_new}, are kept in the workspace and copied to `counts_host` (pinned host
 * memory, 4 x uint32) on the stream; a caller that wants them waits for the stream, nobody else has to.  n_draws is the number of
 * draws made (0 when total == 0), P_new = P for relocation and P + n_draws(argument) for growth.
 *
 * ---- what gsr_mcmc_apply writes ----
 *   every source                       : opacity_new, scaling_new; exp_avg and exp_avg_sq of ALL groups zeroed
 *   every destination (relocation) and
 *   every appended row (growth)        : its source's row in every group, with the source's NEW opacity and scaling; moments zero
 *   every other row                    : bit for bit what it was, parameter and moments (relocation does not touch it; growth copies it)
 * DEVIATION FROM THE PUBLISHED CODE, on purpose: it zeroes only the sources' moments and leaves a relocated row with the dead
 * Gaussian's stale moments.  Here every row whose parameters were replaced starts with zero moments.
 * Groups: up to GSR_MCMC_MAX_GROUPS, role GSR_MCMC_COPY, GSR_MCMC_OPACITY (width 1) or GSR_MCMC_SCALING (width 3).  The four moment
 * pointers of a group are all given or all NULL (no optimiser state yet).  A group of width 0 is skipped.
 * Relocation: dst == src, dst_exp_avg == src_exp_avg, dst_exp_avg_sq == src_exp_avg_sq (in place).  The plan has put every source's
 * new opacity and scaling into the workspace from the OLD values; the apply pass takes these two from the workspace only, reads a
 * source's row only in the plain-copy groups, which it does not modify, and never reads a source's moments: no lane can see a
 * half-updated row.  Growth: dst buffers hold P + n_draws rows and must not be the sources.
 * P, mode and n_draws must be those of the plan in `ws`; a kernel that finds another plan in the workspace writes nothing.
 * No float atomics: the output is bit-identical from run to run.
 *
 * ---- gsr_mcmc_noise: after every optimiser step, one launch, in place ----
 *   f      = 1 / (1 + exp(gate_k * (sigmoid(opacity_i) - gate_t)))
 *   xyz_i  = float32(xyz_i + (R S S R^T noise_i) * f * scale)               S = diag(exp(scaling_i)), R = build_rotation(q / |q|)
 * evaluated as R (S^2 (R^T noise_i)) IN FLOAT64 FROM THE FLOAT32 INPUTS AND ROUNDED ONCE, as the split children of gsr_density.h: the
 * float32 nearest to the formula's value.  (A float32 evaluation cannot be held to a multiple of torch's float32 error: the gate
 * multiplies the rounding of a float32 sigmoid by gate_k, and torch's own error on one set of inputs differs several times between
 * hosts.)  R as in gsr_density.h (utils/general_utils.py:78-99), noise [P,3] standard normal samples of the caller,
 * scale = noise_lr * (current xyz learning rate).  Where f * scale * |...| is far below an ulp of xyz_i, xyz_i comes back bit for bit.
 *
 * ---- gsr_mcmc_regularize: before every optimiser step ----
 *   R = lambda_o * mean_i sigmoid(opacity_i) + lambda_s * mean_{i,a} expf(scaling_i[a])
 *   grad_opacity[i * stride_o] += float32(lambda_o / P) * (s * (1 - s));   grad_scaling[i * stride_s + a] += float32(lambda_s / (3 P)) * expf(scaling_i[a])
 * The gradients are taken as they come, rows stride_o >= 1 and stride_s >= 3 floats apart (a view into a gradient arena).
 * means_out (device, 2 x double) receives {mean sigmoid, mean expf}: the float32 terms summed in float64 in a fixed two-level
 * order (256 rows per workgroup, then the workgroups in index order).  No atomics: bit-identical from run to run.
 *
 * Indices are 32-bit: P + n_draws >= 2^31 is refused, and so is (P + n_draws) * width >= 2^32.
 */
#ifndef GSR_MCMC_H
#define GSR_MCMC_H
#include <stddef.h>
#include <stdint.h>
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
#define GSR_MCMC_MAX_GROUPS 16
#define GSR_MCMC_N_MAX 51
#define GSR_MCMC_RELOCATE 0
#define GSR_MCMC_GROW 1
#define GSR_MCMC_COPY 0
#define GSR_MCMC_OPACITY 1
#define GSR_MCMC_SCALING 2
typedef struct {
    const float *src;             /* [P, width] */
    const float *src_exp_avg;     /* [P, width] or NULL */
    const float *src_exp_avg_sq;  /* [P, width] or NULL */
    float *dst;                   /* relocation: == src; growth: [P + n_draws, width] */
    float *dst_exp_avg;           /* likewise, or NULL */
    float *dst_exp_avg_sq;        /* likewise, or NULL */
    int32_t width_floats;
    int32_t role;                 /* GSR_MCMC_COPY / _OPACITY / _SCALING */
} gsr_mcmc_group_t;
int32_t gsr_mcmc_plan_workspace(int32_t P, int32_t n_draws /* growth; 0 for relocation */, size_t *bytes);
int32_t gsr_mcmc_plan(gsr_stream_t stream, int32_t mode, int32_t P, const float *opacity /*[P] logits*/, const float *scaling /*[P,3] log*/,
                      float L, double min_opacity, int32_t n_max, int32_t n_draws /* growth; 0 for relocation */,
                      const float *u /*[P] (relocation) or [n_draws] (growth)*/, uint32_t *counts_host /*[4] pinned*/, void *ws, size_t ws_bytes);
int32_t gsr_mcmc_apply(gsr_stream_t stream, int32_t mode, int32_t P, int32_t n_draws, int32_t n_groups,
                       const gsr_mcmc_group_t *groups /* host array */, const void *ws, size_t ws_bytes);
int32_t gsr_mcmc_noise(gsr_stream_t stream, int32_t P, const float *opacity /*[P]*/, const float *scaling /*[P,3]*/, const float *rotation /*[P,4]*/,
                       const float *noise /*[P,3]*/, float *xyz /*[P,3]*/, float gate_k, float gate_t, float scale);
int32_t gsr_mcmc_regularize_workspace(int32_t P, size_t *bytes);
int32_t gsr_mcmc_regularize(gsr_stream_t stream, int32_t P, const float *opacity /*[P]*/, const float *scaling /*[P,3]*/, float *grad_opacity,
                            int32_t stride_o, float *grad_scaling, int32_t stride_s, double lambda_o, double lambda_s,
                            double *means_out /*[2] device*/, void *ws, size_t ws_bytes);
#ifdef __cplusplus
}
#endif
#endif
