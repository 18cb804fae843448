/*
 * gsr_chamfer.h -- C ABI of the Chamfer distance between two sets of D-dimensional rows, forward and backward
 * (part of libgsr_hip.so; kernels in csrc/chamfer.hip).
 *
 * Replaces the reference's third native dependency, `chamfer_distance.ChamferDistance`
 * (train_stacked_transformer.py:24,184), called every optimisation step and back-propagated through (:193-196,245):
 *     dist1, dist2, idx1, idx2 = self.chd(pred[None], tgt[None]);  chamfer = dist1.mean() + dist2.mean()
 * PARITY UNPINNED: that package is not part of the reference snapshot, so the semantics below are restated from the
 * call site and cannot be compared with the original.
 *
 * Inputs x1 [B,N,D], x2 [B,M,D].  Per batch element b:
 *   dist1[b,i] = min over j of sum_k (x1[b,i,k] - x2[b,j,k])^2   (SQUARED Euclidean distance, float32), idx1[b,i] = that j;
 *   dist2 [B,M] / idx2 [B,M] the same with the roles swapped.
 * - The distance runs over ALL D features of a row, 1 <= D <= 64 (the reference passes rows of 26 floats).  A deliberate
 *   departure: the public 3-D packages hard-code three floats per point; what they would make of wider rows is not reproduced.
 * - Ties: among candidates whose float32 distances are equal the lowest index wins.  dist* and idx* are bit-identical from
 *   run to run and do not depend on launch geometry.
 * - NaN: a candidate whose distance is NaN never wins against one that is not; if every candidate's is (e.g. the query row
 *   holds a NaN), dist is NaN and idx is 0.  +-inf coordinates follow IEEE arithmetic.  No fault or hang, whatever the values.
 * - Sizes: B = 0, or N = 0 and M = 0: success, nothing written.  Exactly one of N, M zero with B > 0, or D outside 1..64:
 *   GSR_ERR_INVALID_ARGUMENT.  A workspace smaller than gsr_chamfer_workspace says: GSR_ERR_WORKSPACE.
 * - Workspace: 8 B (N + M) bytes (one packed (distance, index) word per output row), contents irrelevant before and after.
 *
 * Backward, given g1 = dL/ddist1 [B,N], g2 = dL/ddist2 [B,M] (either may be NULL = zeros) and the forward's idx1, idx2, the
 * indices treated as constants:
 *   dL/dx1[b,i] = 2 g1[b,i] (x1[b,i] - x2[b,idx1[b,i]])  +  sum over {j : idx2[b,j] = i} of 2 g2[b,j] (x1[b,i] - x2[b,j])
 * and symmetrically for x2.  dx1 [B,N,D] and dx2 [B,M,D] are FULLY WRITTEN by the call (no zeroing by the caller); either may
 * be NULL (not wanted).  An index outside its range is skipped, not followed.  The scattered term is added with float
 * atomics: its order, and so the last bits of a row that several neighbours chose, may differ from run to run.
 *
 * Same conventions as gsr.h: device pointers, float32, caller-owned buffers, enqueued on `stream`, 0 = ok, no host
 * synchronisation, never aborts.
 */
#ifndef GSR_CHAMFER_H
#define GSR_CHAMFER_H
#include <stddef.h>
#include <stdint.h>
#include "gsr.h"
#ifdef __cplusplus
extern "C" {
#endif
int32_t gsr_chamfer_workspace(int32_t B, int32_t N, int32_t M, size_t *bytes);
int32_t gsr_chamfer_forward(gsr_stream_t stream, int32_t B, int32_t N, int32_t M, int32_t D,
                            const float *x1 /*[B,N,D]*/, const float *x2 /*[B,M,D]*/,
                            float *dist1 /*[B,N]*/, float *dist2 /*[B,M]*/, int32_t *idx1 /*[B,N]*/, int32_t *idx2 /*[B,M]*/,
                            void *ws, size_t ws_bytes);
int32_t gsr_chamfer_backward(gsr_stream_t stream, int32_t B, int32_t N, int32_t M, int32_t D,
                             const float *x1, const float *x2, const int32_t *idx1, const int32_t *idx2,
                             const float *g1 /*[B,N] or NULL*/, const float *g2 /*[B,M] or NULL*/,
                             float *dx1 /*[B,N,D] or NULL*/, float *dx2 /*[B,M,D] or NULL*/);
#ifdef __cplusplus
}
#endif
#endif
