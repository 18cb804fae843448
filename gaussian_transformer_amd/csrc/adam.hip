// adam.hip -- one launch for the Adam step of all parameter groups (include/gsr_optim.h).  Pure streaming:
// 16 bytes read + 12 written per element, float4 wide where the group's length and pointers allow.
// Below it the visibility-masked step (gsr_adam_step_masked): the same update through the same adam_four / adam_at, on the visible
// rows only, over the same group plan (adam_plan).  Both entry points are at the end of the file.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gsr_optim.h"
#include "gsr_host.h"
#include "gsr_internal.h"

namespace gsr {

struct AdamGroupDev {
    float *p;
    const float *g;
    float *m, *v;
    long long n;
    float step_size, inv_sqrt_bc2;
    unsigned first_block;        // the group's blocks are [first_block, next group's first_block)
    int vec4;
};
struct AdamArgs {
    AdamGroupDev grp[GSR_ADAM_MAX_GROUPS];
    int n_groups;
    float beta2, omb1, omb2, eps;      // 1 - beta computed in double on the host (1 - 0.999f is 4.7e-5 off 0.001)
};

#define ADAM_PER_BLOCK (256 * 4 * 4)      // 256 threads x 4 float4

__device__ __forceinline__ void adam_one(float &p, float g, float &m, float &v, float omb1, float b2, float omb2, float eps, float step_size,
                                         float isb2) {
    m = m + (g - m) * omb1;
    v = v * b2 + g * g * omb2;
    const float denom = sqrtf(v) * isb2 + eps;
    p = p - step_size * (m / denom);
}

// the update of one float4 of each array, lane by lane
__device__ __forceinline__ void adam_four(float4 &p, const float4 &g, float4 &m, float4 &v, const AdamArgs &a, const AdamGroupDev &G) {
    adam_one(p.x, g.x, m.x, v.x, a.omb1, a.beta2, a.omb2, a.eps, G.step_size, G.inv_sqrt_bc2);
    adam_one(p.y, g.y, m.y, v.y, a.omb1, a.beta2, a.omb2, a.eps, G.step_size, G.inv_sqrt_bc2);
    adam_one(p.z, g.z, m.z, v.z, a.omb1, a.beta2, a.omb2, a.eps, G.step_size, G.inv_sqrt_bc2);
    adam_one(p.w, g.w, m.w, v.w, a.omb1, a.beta2, a.omb2, a.eps, G.step_size, G.inv_sqrt_bc2);
}
// element j of group G: load, update, store
template <class Index>
__device__ __forceinline__ void adam_at(const AdamArgs &a, const AdamGroupDev &G, Index j) {
    float p = G.p[j], m = G.m[j], v = G.v[j];
    adam_one(p, G.g[j], m, v, a.omb1, a.beta2, a.omb2, a.eps, G.step_size, G.inv_sqrt_bc2);
    G.p[j] = p; G.m[j] = m; G.v[j] = v;
}

__global__ __launch_bounds__(256) void adam_kernel(AdamArgs a) {
    const AdamGroupDev &G = a.grp[group_of_block(a)];
    const long long base = (long long)(blockIdx.x - G.first_block) * ADAM_PER_BLOCK;
    if (G.vec4) {
#pragma unroll
        for (int it = 0; it < 4; it++) {
            const long long i = base + ((long long)it * 256 + threadIdx.x) * 4;
            if (i + 3 < G.n) {
                float4 p = *reinterpret_cast<float4 *>(G.p + i), m = *reinterpret_cast<float4 *>(G.m + i), v = *reinterpret_cast<float4 *>(G.v + i);
                adam_four(p, *reinterpret_cast<const float4 *>(G.g + i), m, v, a, G);
                *reinterpret_cast<float4 *>(G.p + i) = p; *reinterpret_cast<float4 *>(G.m + i) = m; *reinterpret_cast<float4 *>(G.v + i) = v;
            } else {
                for (long long j = i; j < G.n && j < i + 4; j++) adam_at(a, G, j);
            }
        }
    } else {
        for (int it = 0; it < 16; it++) {
            const long long j = base + (long long)it * 256 + threadIdx.x;
            if (j < G.n) adam_at(a, G, j);
        }
    }
}

// The launch plan of both entry points: the groups that hold an element, in order, each with its bias corrections, its float4
// eligibility and its first block.  Returns the number of blocks (0: nothing to launch).
static unsigned adam_plan(int n_groups, const gsr_adam_group_t *groups, double beta1, double beta2, double eps, AdamArgs &a) {
    a.n_groups = 0; a.beta2 = (float)beta2; a.omb1 = (float)(1.0 - beta1); a.omb2 = (float)(1.0 - beta2); a.eps = (float)eps;
    unsigned blocks = 0;                         // at most 16 groups of 2^19 blocks in the masked step, whose n < 2^31
    for (int k = 0; k < n_groups; k++) {
        const gsr_adam_group_t &h = groups[k];
        if (h.n <= 0) continue;
        AdamGroupDev &d = a.grp[a.n_groups++];
        d.p = h.param; d.g = h.grad; d.m = h.exp_avg; d.v = h.exp_avg_sq; d.n = h.n;
        const double bc1 = 1.0 - pow(beta1, (double)h.step), bc2 = 1.0 - pow(beta2, (double)h.step);
        d.step_size = (float)((double)h.lr / bc1);
        d.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
        d.first_block = blocks;
        d.vec4 = ((((uintptr_t)h.param | (uintptr_t)h.grad | (uintptr_t)h.exp_avg | (uintptr_t)h.exp_avg_sq) & 15) == 0) ? 1 : 0;
        blocks += (unsigned)((h.n + ADAM_PER_BLOCK - 1) / ADAM_PER_BLOCK);
    }
    return blocks;
}

static hipError_t launch_adam(int n_groups, const gsr_adam_group_t *groups, double beta1, double beta2, double eps, hipStream_t s) {
    AdamArgs a;
    const unsigned blocks = adam_plan(n_groups, groups, beta1, beta2, eps, a);
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---- the visibility-masked step (gsr_adam_step_masked) ----
// Same grid as adam_kernel: a block owns 4096 consecutive elements of one group, a lane the same elements as there.  A group is
// [P, w] row-major, so element j lies in row j / w.  One division per thread; from one of its elements to the next the row and the
// remainder advance by the group's (step / w, step % w), step = 1024 floats in the float4 body and 256 in the scalar one.
struct AdamMaskedArgs {
    AdamArgs a;
    int w[GSR_ADAM_MAX_GROUPS];              // floats per row
    int q_step[GSR_ADAM_MAX_GROUPS];         // step / w
    int r_step[GSR_ADAM_MAX_GROUPS];         // step % w
    const void *mask;
};

template <int KIND>
__device__ __forceinline__ bool row_visible(const void *mask, unsigned row) {
    if (KIND == GSR_ADAM_MASK_RADII) return static_cast<const int32_t *>(mask)[row] > 0;
    return static_cast<const uint8_t *>(mask)[row] != 0;
}

template <int KIND>
__global__ __launch_bounds__(256) void adam_masked_kernel(AdamMaskedArgs A) {
    const AdamArgs &a = A.a;
    const int gi = group_of_block(a);
    const AdamGroupDev &G = a.grp[gi];
    const unsigned w = (unsigned)A.w[gi], q_step = (unsigned)A.q_step[gi], r_step = (unsigned)A.r_step[gi];
    const unsigned n = (unsigned)G.n;                            // n <= 2^31 - 1 (checked on the host)
    const unsigned base = (blockIdx.x - G.first_block) * ADAM_PER_BLOCK;
    if (G.vec4) {
        // pass 1: the visibility of this lane's 4 x 4 elements, one mask read per row entered (bit c of vis[it] = element i + c)
        unsigned vis[4];
        {
            const unsigned i0 = base + threadIdx.x * 4;
            unsigned row = i0 / w, rem = i0 - row * w;
#pragma unroll
            for (int it = 0; it < 4; it++) {
                const unsigned i = i0 + it * 1024;
                unsigned bits = 0;
                if (i < n) {
                    unsigned r = row, q = rem;
                    bool on = row_visible<KIND>(A.mask, r);
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        if (on) bits |= 1u << c;
                        if (++q == w && c < 3 && i + c + 1 < n) { q = 0; r++; on = row_visible<KIND>(A.mask, r); }
                    }
                }
                vis[it] = bits;
                row += q_step; rem += r_step;
                if (rem >= w) { rem -= w; row++; }
            }
        }
        // pass 2: adam_kernel's float4 body; a wave without a visible element touches neither the four arrays nor anything else
#pragma unroll
        for (int it = 0; it < 4; it++) {
            const unsigned bits = vis[it];
            if (__ballot(bits != 0) == 0) continue;              // wave-uniform
            if (bits == 0) continue;
            const unsigned i = base + (it * 256 + threadIdx.x) * 4;
            if (i + 3 < n) {
                // a float4 may straddle rows of different visibility: all four lanes of it are computed as in adam_kernel, the invisible
                // ones get their loaded bits back (a NaN there passes through v_cndmask untouched and reaches nothing)
                const float4 p0 = *reinterpret_cast<float4 *>(G.p + i), m0 = *reinterpret_cast<float4 *>(G.m + i), v0 = *reinterpret_cast<float4 *>(G.v + i);
                const float4 g = *reinterpret_cast<const float4 *>(G.g + i);
                float4 p = p0, m = m0, v = v0;
                adam_four(p, g, m, v, a, G);
                if (!(bits & 1)) { p.x = p0.x; m.x = m0.x; v.x = v0.x; }
                if (!(bits & 2)) { p.y = p0.y; m.y = m0.y; v.y = v0.y; }
                if (!(bits & 4)) { p.z = p0.z; m.z = m0.z; v.z = v0.z; }
                if (!(bits & 8)) { p.w = p0.w; m.w = m0.w; v.w = v0.w; }
                *reinterpret_cast<float4 *>(G.p + i) = p; *reinterpret_cast<float4 *>(G.m + i) = m; *reinterpret_cast<float4 *>(G.v + i) = v;
            } else {
#pragma unroll 1
                for (unsigned c = 0; c < 4 && i + c < n; c++) {
                    if (bits >> c & 1) adam_at(a, G, i + c);
                }
            }
        }
    } else {
        const unsigned j0 = base + threadIdx.x;
        unsigned row = j0 / w, rem = j0 - row * w;
        for (int it = 0; it < 16; it++) {
            const unsigned j = j0 + it * 256;
            const bool on = j < n && row_visible<KIND>(A.mask, row);
            row += q_step; rem += r_step;
            if (rem >= w) { rem -= w; row++; }
            if (__ballot(on) == 0) continue;                     // wave-uniform
            if (on) adam_at(a, G, j);
        }
    }
}

}  // namespace gsr

using namespace gsr;

extern "C" {

// ---- Adam step over all parameter groups (include/gsr_optim.h) ----
int32_t gsr_adam_step(gsr_stream_t stream, int32_t n_groups, const gsr_adam_group_t *groups, double beta1, double beta2, double eps) {
    if (n_groups < 0 || n_groups > GSR_ADAM_MAX_GROUPS || (n_groups > 0 && !groups))
        return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_adam_step: %d groups (at most %d)", n_groups, GSR_ADAM_MAX_GROUPS);
    for (int k = 0; k < n_groups; k++) {
        const gsr_adam_group_t &g = groups[k];
        if (g.n < 0 || (g.n > 0 && (!g.param || !g.grad || !g.exp_avg || !g.exp_avg_sq)) || g.step < 1)
            return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_adam_step: group %d: n=%lld step=%d or a NULL buffer", k, (long long)g.n, g.step);
    }
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_adam_step: betas");
    HIP_TRY(launch_adam(n_groups, groups, beta1, beta2, eps, (hipStream_t)stream), "adam launch");
    return GSR_OK;
}

int32_t gsr_adam_step_masked(gsr_stream_t stream, int32_t n_groups, const gsr_adam_group_t *groups, double beta1, double beta2,
                             double eps, int32_t P, const void *mask, int32_t mask_kind) {
    const char *const who = "gsr_adam_step_masked";
    if (n_groups < 1 || n_groups > GSR_ADAM_MAX_GROUPS || !groups)
        return fail(GSR_ERR_INVALID_ARGUMENT, "%s: %d groups (1 to %d)", who, n_groups, GSR_ADAM_MAX_GROUPS);
    if (P < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: P=%d is negative", who, P);
    if (mask_kind != GSR_ADAM_MASK_BYTES && mask_kind != GSR_ADAM_MASK_RADII)
        return fail(GSR_ERR_INVALID_ARGUMENT, "%s: unknown mask_kind %d", who, mask_kind);
    if (P > 0 && !mask) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: mask is NULL with P=%d", who, P);
    if (mask_kind == GSR_ADAM_MASK_RADII && ((uintptr_t)mask & 3))
        return fail(GSR_ERR_INVALID_ARGUMENT, "%s: an int32 mask must be 4-byte aligned", who);
    for (int k = 0; k < n_groups; k++) {
        const gsr_adam_group_t &g = groups[k];
        if (g.n < 0 || g.n > 0x7fffffffLL) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: group %d: n=%lld not in 0..2^31-1", who, k, (long long)g.n);
        if (g.n > 0 && (P == 0 || g.n % P != 0))
            return fail(GSR_ERR_INVALID_ARGUMENT, "%s: group %d: n=%lld is not a multiple of P=%d", who, k, (long long)g.n, P);
        if (g.n > 0 && (!g.param || !g.grad || !g.exp_avg || !g.exp_avg_sq))
            return fail(GSR_ERR_INVALID_ARGUMENT, "%s: group %d: a NULL buffer with n=%lld", who, k, (long long)g.n);
        if (g.step < 1) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: group %d: step=%d", who, k, g.step);
    }
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: betas", who);

    AdamMaskedArgs A;
    const unsigned blocks = adam_plan(n_groups, groups, beta1, beta2, eps, A.a);
    if (blocks == 0) return GSR_OK;
    A.mask = mask;
    for (int s = 0; s < GSR_ADAM_MAX_GROUPS; s++) {
        A.w[s] = A.q_step[s] = A.r_step[s] = 0;
        if (s >= A.a.n_groups) continue;
        const long long w = A.a.grp[s].n / P, step = A.a.grp[s].vec4 ? 1024 : 256;      // P >= 1: a group with elements is a multiple of it
        A.w[s] = (int)w; A.q_step[s] = (int)(step / w); A.r_step[s] = (int)(step % w);
    }
    if (mask_kind == GSR_ADAM_MASK_RADII)
        hipLaunchKernelGGL(adam_masked_kernel<GSR_ADAM_MASK_RADII>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, A);
    else
        hipLaunchKernelGGL(adam_masked_kernel<GSR_ADAM_MASK_BYTES>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, A);
    HIP_TRY(hipGetLastError(), "masked adam launch");
    return GSR_OK;
}

}  // extern "C"
