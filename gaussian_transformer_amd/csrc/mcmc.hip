// mcmc.hip -- MCMC density control on the device (include/gsr_mcmc.h):
//   plan       : weight kernel (one lane per row: dead flag, integer weight) -> one rocPRIM inclusive scan that carries the uint64 CDF and
//                the rank among the dead rows in one value -> draw kernel (one lane per draw: binary search of the CDF, integer histogram)
//                -> correction kernel (one lane per row: a source's new opacity and scaling in float64, into the workspace).
//   apply      : ONE launch over (row, column) of every group: consecutive lanes write consecutive floats of the parameter and both
//                moments; 16-byte accesses where the width is a multiple of 4 and every pointer is aligned.  In place (relocation) a
//                lane whose row is neither a source nor a destination returns without touching memory.  The group table, its filler
//                and the common group refusals are group_table.h's, shared with density.hip; the kernel, which reads from[] and
//                hist[] under a mode, is this file's.
//   noise      : one lane per Gaussian, 56 B read and 12 B written; float64 inside (the rotation is group_table.h's), rounded once.
//   regularize : one lane per Gaussian; the two means through a fixed two-level float64 sum (workgroup tree, then one workgroup).
// Compiled with -ffp-contract=off -fno-slp-vectorize like density.hip: t_j is one IEEE multiply, the regularisers round as written.
// Every row index a kernel forms (src_j, a destination, a workspace slot) is checked against its bound in every build.  The only atomics
// are integer adds (histogram, source count): bit-identical from run to run.
#include <cstring>  // ROCm 7.2 rocprim/texture_cache_iterator.hpp uses memset without including it
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "../../include/gsr_mcmc.h"
#include "group_table.h"

namespace gsr {

// ---------------------------------------------------------------- plan ----------------------------------------------------------------

enum { M_NDEAD = 0, M_NDRAWS = 1, M_NSOURCES = 2, M_PNEW = 3, M_MODE = 4, M_NARG = 5, M_WORDS = 8 };
#define MCMC_DEAD_BIT 0x80000000u      // a weight is at most 2^20

struct McmcScan { uint64_t cw; uint64_t dead; };      // inclusive: CDF of the weights, dead rows up to and including this one
struct McmcAdd {
    __host__ __device__ McmcScan operator()(const McmcScan &a, const McmcScan &b) const { return McmcScan{a.cw + b.cw, a.dead + b.dead}; }
};
struct WeightToScan {
    __host__ __device__ McmcScan operator()(uint32_t w) const { return McmcScan{(uint64_t)(w & ~MCMC_DEAD_BIT), (uint64_t)(w >> 31)}; }
};

struct McmcWs {
    uint32_t *counts;        // [M_WORDS]
    uint32_t *wd;            // [P] weight | dead << 31
    McmcScan *scan;          // [P]
    uint32_t *hist;          // [P] c_i
    uint32_t *from;          // [P + n] the row every row of the new state is a copy of (itself: not a destination)
    float *new_op;           // [P] valid where hist > 0
    float *new_sc;           // [3 P] likewise
    void *temp; size_t temp_bytes, total;
};

static hipError_t carve_mcmc_ws(void *base, int P, int n, McmcWs &w) {
    const size_t np = (size_t)(P > 0 ? P : 1);
    size_t tb = 0;
    hipError_t e = rocprim::inclusive_scan(nullptr, tb, rocprim::make_transform_iterator((const uint32_t *)nullptr, WeightToScan()), (McmcScan *)nullptr,
                                           np, McmcAdd(), (hipStream_t)0, false);
    if (e != hipSuccess) return e;
    Bump b = {(char *)base, 0};
    w.counts = b.take<uint32_t>(M_WORDS);
    w.wd = b.take<uint32_t>(np);
    w.scan = b.take<McmcScan>(np);
    w.hist = b.take<uint32_t>(np);
    w.from = b.take<uint32_t>(np + (size_t)n);
    w.new_op = b.take<float>(np);
    w.new_sc = b.take<float>(3 * np);
    w.temp = b.take<char>(tb > 0 ? tb : 1);
    w.temp_bytes = tb;
    w.total = b.off;
    return hipSuccess;
}

static hipError_t mcmc_workspace_bytes(int P, int n, size_t *bytes) {
    McmcWs w;
    hipError_t e = carve_mcmc_ws(nullptr, P, n, w);
    if (e == hipSuccess) *bytes = w.total;
    return e;
}

__device__ __forceinline__ double sigmoid64(double v) { return 1.0 / (1.0 + exp(-v)); }

__global__ __launch_bounds__(256) void mcmc_weight_kernel(int P, const float *__restrict__ opacity, float L, uint32_t *__restrict__ wd,
                                                          uint32_t *__restrict__ hist, uint32_t *__restrict__ from, uint32_t *__restrict__ counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    if (i == 0) counts[M_NSOURCES] = 0;
    const float op = opacity[i];
    const bool dead = op <= L;
    const uint32_t w = dead ? 0u : (uint32_t)floor(sigmoid64((double)op) * 1048576.0 + 0.5);
    wd[i] = (w & ~MCMC_DEAD_BIT) | (dead ? MCMC_DEAD_BIT : 0u);
    hist[i] = 0;
    from[i] = (uint32_t)i;
}

// one lane per draw.  Relocation: the lane of dead row i makes draw j = (dead rows in front of i), whose destination is i itself.
// Growth: lane j makes draw j for appended row P + j.  The first lane files the counts.
__global__ __launch_bounds__(256) void mcmc_draw_kernel(int mode, int P, int n, const float *__restrict__ u, const uint32_t *__restrict__ wd,
                                                        const McmcScan *__restrict__ scan, uint32_t *__restrict__ hist, uint32_t *__restrict__ from,
                                                        uint32_t *__restrict__ counts) {
    const int lane = blockIdx.x * 256 + threadIdx.x;
    const uint64_t total = scan[P - 1].cw, n_dead = scan[P - 1].dead;
    if (lane == 0) {
        counts[M_NDEAD] = (uint32_t)n_dead;
        counts[M_NDRAWS] = total == 0 ? 0u : (mode == GSR_MCMC_RELOCATE ? (uint32_t)n_dead : (uint32_t)n);
        counts[M_PNEW] = (uint32_t)P + (uint32_t)n;
        counts[M_MODE] = (uint32_t)mode;
        counts[M_NARG] = (uint32_t)n;
    }
    uint32_t j, dest;
    if (mode == GSR_MCMC_RELOCATE) {
        if (lane >= P || !(wd[lane] & MCMC_DEAD_BIT) || total == 0) return;
        j = (uint32_t)(scan[lane].dead - 1);
        dest = (uint32_t)lane;
        if (j >= (uint32_t)P) return;                               // u holds P entries
    } else {
        if (lane >= n) return;
        j = (uint32_t)lane;
        dest = (uint32_t)P + j;
        if (total == 0) { from[dest] = j % (uint32_t)P; return; }   // nothing to draw from: a plain copy (include/gsr_mcmc.h)
    }
    const double prod = (double)u[j] * (double)total;               // no contraction in this unit: one IEEE multiply
    uint64_t t = prod > 0.0 ? (uint64_t)floor(prod) : 0ull;
    if (t > total - 1) t = total - 1;
    uint32_t lo = 0, hi = (uint32_t)P - 1;                          // the smallest i with C_i > t; C[P-1] = total > t
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (scan[mid].cw > t) hi = mid; else lo = mid + 1;
    }
    if (lo >= (uint32_t)P || dest >= (uint32_t)P + (uint32_t)n) return;
    from[dest] = lo;
    atomicAdd(&hist[lo], 1u);
}

// one lane per row: the correction of a source, in float64, rounded once
__global__ __launch_bounds__(256) void mcmc_correct_kernel(int P, const float *__restrict__ opacity, const float *__restrict__ scaling, double m,
                                                           int n_max, const uint32_t *__restrict__ hist, float *__restrict__ new_op,
                                                           float *__restrict__ new_sc, uint32_t *__restrict__ counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const uint32_t c = i < P ? hist[i] : 0u;
    const int in_block = __syncthreads_count(c > 0);
    if (threadIdx.x == 0 && in_block) atomicAdd(&counts[M_NSOURCES], (uint32_t)in_block);
    if (c == 0) return;
    const int N = c + 1u < (uint32_t)n_max ? (int)(c + 1u) : n_max;
    const double lg = (double)opacity[i];
    const double o = sigmoid64(lg), q = sigmoid64(-lg);             // q = 1 - o without the cancellation
    const double lq = log(q) / (double)N;
    const double x = -expm1(lq);                                    // 1 - (1 - o)^(1 / N)
    double D = 0.0, binom = (double)N, xp = x;                      // C(N, 1), x^1
    for (int k = 0; k < N; k++) {
        const double term = binom * xp / sqrt((double)(k + 1));
        D += (k & 1) ? -term : term;
        binom = binom * (double)(N - k - 1) / (double)(k + 2);      // C(N, k + 2): exact in double up to N = 51
        xp *= x;
    }
    const double shift = log(o / D);
    for (int a = 0; a < 3; a++) new_sc[3 * (size_t)i + a] = (float)((double)scaling[3 * (size_t)i + a] + shift);
    const double hi = 1.0 - 1.1920928955078125e-07;                 // 1 - 2^-23
    const double oc = x < m ? m : (x > hi ? hi : x);
    const double rest = oc == x ? exp(lq) : 1.0 - oc;               // 1 - o_c; (1 - o)^(1 / N) where the clamp did not act
    new_op[i] = (float)log(oc / rest);
}

// sizes validated by the caller; P >= 1
static hipError_t launch_mcmc_plan(int mode, int P, const float *opacity, const float *scaling, float L, double m, int n_max, int n, const float *u,
                                   uint32_t *counts_host, void *ws, hipStream_t s) {
    McmcWs w;
    hipError_t e = carve_mcmc_ws(ws, P, n, w);
    if (e != hipSuccess) return e;
    const dim3 grid((P + 255) / 256), block(256);
    hipLaunchKernelGGL(mcmc_weight_kernel, grid, block, 0, s, P, opacity, L, w.wd, w.hist, w.from, w.counts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t tb = w.temp_bytes;
    e = rocprim::inclusive_scan(w.temp, tb, rocprim::make_transform_iterator((const uint32_t *)w.wd, WeightToScan()), w.scan, (size_t)P, McmcAdd(), s,
                                false);
    if (e != hipSuccess) return e;
    const int lanes = mode == GSR_MCMC_RELOCATE ? P : (n > 0 ? n : 1);
    hipLaunchKernelGGL(mcmc_draw_kernel, dim3((lanes + 255) / 256), block, 0, s, mode, P, n, u, (const uint32_t *)w.wd, (const McmcScan *)w.scan, w.hist,
                       w.from, w.counts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(mcmc_correct_kernel, grid, block, 0, s, P, opacity, scaling, m, n_max, (const uint32_t *)w.hist, w.new_op, w.new_sc, w.counts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return hipMemcpyAsync(counts_host, w.counts, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
}

// ---------------------------------------------------------------- apply ----------------------------------------------------------------

struct McmcApplyArgs {
    GroupDev grp[GSR_MCMC_MAX_GROUPS];
    int n_groups, P, mode;
    uint32_t n, p_new;
    const uint32_t *from, *hist, *counts;
    const float *new_op, *new_sc;
};

__global__ __launch_bounds__(256) void mcmc_apply_kernel(McmcApplyArgs a) {
    // the plan in the workspace must be the one the caller sized the outputs for (uniform)
    if (a.counts[M_PNEW] != a.p_new || a.counts[M_MODE] != (uint32_t)a.mode || a.counts[M_NARG] != a.n) return;
    const GroupDev &G = a.grp[group_of_block(a)];
    const uint32_t w = G.w, P = (uint32_t)a.P;
    const uint64_t total = (uint64_t)a.p_new * w;               // < 2^32 (checked by the caller)
    const uint64_t base = (uint64_t)(blockIdx.x - G.first_block) * GROUP_PER_BLOCK;
    const bool moments = G.dm != nullptr, in_place = a.mode == GSR_MCMC_RELOCATE;
    if (G.vec4) {                                               // w % 4 == 0, role copy: a float4 never leaves its row
        const uint64_t e = base + (uint64_t)threadIdx.x * 4;
        if (e >= total) return;
        const uint32_t row = (uint32_t)(e / w), c = (uint32_t)(e - (uint64_t)row * w);
        const uint32_t s = a.from[row];                         // row < p_new = P + n, the size of from[]
        if (s >= P) return;
        const bool fresh = s != row || a.hist[s] > 0;           // a destination or a source: zero moments
        if (in_place && !fresh) return;
        const size_t so = (size_t)s * w + c;
        if (!in_place || s != row) *reinterpret_cast<float4 *>(G.dst + e) = *reinterpret_cast<const float4 *>(G.src + so);
        if (moments) {
            float4 mm = make_float4(0.f, 0.f, 0.f, 0.f), vv = mm;
            if (!fresh) { mm = *reinterpret_cast<const float4 *>(G.sm + so); vv = *reinterpret_cast<const float4 *>(G.sv + so); }
            *reinterpret_cast<float4 *>(G.dm + e) = mm;
            *reinterpret_cast<float4 *>(G.dv + e) = vv;
        }
        return;
    }
#pragma unroll 1
    for (int it = 0; it < GROUP_PER_BLOCK / 256; it++) {
        const uint64_t e = base + (uint64_t)it * 256 + threadIdx.x;
        if (e >= total) return;
        const uint32_t row = (uint32_t)(e / w), c = (uint32_t)(e - (uint64_t)row * w);
        const uint32_t s = a.from[row];
        if (s >= P) continue;
        const bool corrected = a.hist[s] > 0;                   // s is a source: its opacity and scaling come from the workspace
        const bool fresh = s != row || corrected;
        if (in_place && !fresh) continue;
        const size_t so = (size_t)s * w + c;
        if (corrected && G.role == GSR_MCMC_OPACITY) G.dst[e] = a.new_op[s];
        else if (corrected && G.role == GSR_MCMC_SCALING) G.dst[e] = a.new_sc[3 * (size_t)s + c];
        else if (!in_place || s != row) G.dst[e] = G.src[so];   // in place a source keeps its plain-copy groups: not read, not written
        if (moments) {
            G.dm[e] = fresh ? 0.f : G.sm[so];
            G.dv[e] = fresh ? 0.f : G.sv[so];
        }
    }
}

// sizes, pointers and roles validated by the caller; P >= 1
static hipError_t launch_mcmc_apply(int mode, int P, int n, int n_groups, const gsr_mcmc_group_t *groups, const void *ws, hipStream_t s) {
    McmcWs w;
    hipError_t e = carve_mcmc_ws(const_cast<void *>(ws), P, n, w);
    if (e != hipSuccess) return e;
    McmcApplyArgs a;
    memset(&a, 0, sizeof(a));
    a.P = P; a.mode = mode; a.n = (uint32_t)n; a.p_new = (uint32_t)P + (uint32_t)n;
    a.from = w.from; a.hist = w.hist; a.counts = w.counts; a.new_op = w.new_op; a.new_sc = w.new_sc;
    const unsigned blocks = fill_group_table(n_groups, groups, a.p_new, GSR_MCMC_COPY, a.grp, a.n_groups);
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(mcmc_apply_kernel, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------- noise ----------------------------------------------------------------

// Evaluated in float64 from the float32 inputs and rounded once, as density.hip's split children: the result is the float32 nearest to the
// formula's value, so no float32 evaluation lies nearer to it.  A float32 evaluation cannot be held to "twice torch's float32 error": the
// gate multiplies a sigmoid's rounding by gate_k, six entries of R each carry 1e-7 into a move of up to a few hundred, and torch's own
// float32 error on one input set was 1.1e-5 on one host and 7.3e-5 on another.  About 150 double operations and five exps beside 68 bytes.
__global__ __launch_bounds__(256) void mcmc_noise_kernel(int P, const float *__restrict__ opacity, const float *__restrict__ scaling,
                                                         const float *__restrict__ rotation, const float *__restrict__ noise, float *__restrict__ xyz,
                                                         float gate_k, float gate_t, float scale) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const double f = 1.0 / (1.0 + exp((double)gate_k * (sigmoid64((double)opacity[i]) - (double)gate_t)));
    const float4 q4 = *reinterpret_cast<const float4 *>(rotation + 4 * (size_t)i);      // rows of 16 bytes: aligned with the buffer (checked by the caller)
    const Quat64 q = unit_quat64(q4.x, q4.y, q4.z, q4.w);
    const Row64 R0 = rot_row(q, 0), R1 = rot_row(q, 1), R2 = rot_row(q, 2);
    const size_t b = 3 * (size_t)i;
    const double s0 = exp((double)scaling[b]), s1 = exp((double)scaling[b + 1]), s2 = exp((double)scaling[b + 2]);
    const double n0 = noise[b], n1 = noise[b + 1], n2 = noise[b + 2];
    const double v0 = (R0.c0 * n0 + R1.c0 * n1 + R2.c0 * n2) * (s0 * s0);                // S^2 R^T noise
    const double v1 = (R0.c1 * n0 + R1.c1 * n1 + R2.c1 * n2) * (s1 * s1);
    const double v2 = (R0.c2 * n0 + R1.c2 * n1 + R2.c2 * n2) * (s2 * s2);
    const double g = f * (double)scale;
    xyz[b] = (float)((double)xyz[b] + (R0.c0 * v0 + R0.c1 * v1 + R0.c2 * v2) * g);
    xyz[b + 1] = (float)((double)xyz[b + 1] + (R1.c0 * v0 + R1.c1 * v1 + R1.c2 * v2) * g);
    xyz[b + 2] = (float)((double)xyz[b + 2] + (R2.c0 * v0 + R2.c1 * v1 + R2.c2 * v2) * g);
}

// ---------------------------------------------------------------- regularize ----------------------------------------------------------------

__global__ __launch_bounds__(256) void mcmc_regularize_kernel(int P, const float *__restrict__ opacity, const float *__restrict__ scaling,
                                                              float *__restrict__ grad_o, int stride_o, float *__restrict__ grad_s, int stride_s,
                                                              float co, float cs, double *__restrict__ partial) {
    __shared__ double sh[2][256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    double so = 0.0, ss = 0.0;
    if (i < P) {
        const float s = 1.f / (1.f + expf(-opacity[i]));
        float *go = grad_o + (size_t)i * stride_o;
        *go = *go + co * (s * (1.f - s));
        so = (double)s;
        float *gs = grad_s + (size_t)i * stride_s;
        for (int a = 0; a < 3; a++) {
            const float e = expf(scaling[3 * (size_t)i + a]);
            gs[a] = gs[a] + cs * e;
            ss += (double)e;
        }
    }
    sh[0][threadIdx.x] = so; sh[1][threadIdx.x] = ss;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {                          // a fixed tree: the same sum every run
        if ((int)threadIdx.x < h) { sh[0][threadIdx.x] += sh[0][threadIdx.x + h]; sh[1][threadIdx.x] += sh[1][threadIdx.x + h]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { partial[2 * (size_t)blockIdx.x] = sh[0][0]; partial[2 * (size_t)blockIdx.x + 1] = sh[1][0]; }
}

// one workgroup: lane t sums the partials t, t + 256, ... in that order, then the same tree
__global__ __launch_bounds__(256) void mcmc_means_kernel(int P, int nblk, const double *__restrict__ partial, double *__restrict__ means) {
    __shared__ double sh[2][256];
    double so = 0.0, ss = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) { so += partial[2 * (size_t)b]; ss += partial[2 * (size_t)b + 1]; }
    sh[0][threadIdx.x] = so; sh[1][threadIdx.x] = ss;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) { sh[0][threadIdx.x] += sh[0][threadIdx.x + h]; sh[1][threadIdx.x] += sh[1][threadIdx.x + h]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { means[0] = sh[0][0] / (double)P; means[1] = sh[1][0] / (3.0 * (double)P); }
}

// two doubles per workgroup of 256 rows
static size_t regularize_workspace_bytes(int P) { return align_up(2 * sizeof(double) * (((size_t)(P > 0 ? P : 1) + 255) / 256)); }

}  // namespace gsr

using namespace gsr;

extern "C" {

// ---- MCMC density control on the device (include/gsr_mcmc.h) ----
static int mcmc_sizes(const char *who, int32_t P, int32_t n_draws) {
    if (P < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: P=%d is negative", who, P);
    if (n_draws < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: n_draws=%d is negative", who, n_draws);
    if ((long long)P + (long long)n_draws > 0x7fffffffLL)
        return fail(GSR_ERR_INVALID_ARGUMENT, "%s: P + n_draws = %lld, must stay below 2^31", who, (long long)P + (long long)n_draws);
    return GSR_OK;
}

static int mcmc_mode(const char *who, int32_t mode, int32_t n_draws) {
    if (mode != GSR_MCMC_RELOCATE && mode != GSR_MCMC_GROW) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: unknown mode %d", who, mode);
    if (mode == GSR_MCMC_RELOCATE && n_draws != 0)
        return fail(GSR_ERR_INVALID_ARGUMENT, "%s: n_draws=%d with relocation (it draws n_dead times; pass 0)", who, n_draws);
    return GSR_OK;
}

int32_t gsr_mcmc_plan_workspace(int32_t P, int32_t n_draws, size_t *bytes) {
    if (!bytes) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_mcmc_plan_workspace: bytes is NULL");
    GSR_TRY(mcmc_sizes("gsr_mcmc_plan_workspace", P, n_draws));
    HIP_TRY(mcmc_workspace_bytes(P, n_draws, bytes), "mcmc workspace size");
    return GSR_OK;
}

int32_t gsr_mcmc_plan(gsr_stream_t stream, int32_t mode, int32_t P, const float *opacity, const float *scaling, float L, double min_opacity,
                      int32_t n_max, int32_t n_draws, const float *u, uint32_t *counts_host, void *ws, size_t ws_bytes) {
    GSR_TRY(mcmc_sizes("gsr_mcmc_plan", P, n_draws));
    GSR_TRY(mcmc_mode("gsr_mcmc_plan", mode, n_draws));
    if (!counts_host) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_mcmc_plan: counts_host is NULL");
    if (n_max < 1 || n_max > GSR_MCMC_N_MAX) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_mcmc_plan: n_max=%d not in 1..%d", n_max, GSR_MCMC_N_MAX);
    if (!(min_opacity > 0.0 && min_opacity < 1.0))
        return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_mcmc_plan: min_opacity=%g, must lie in (0, 1)", min_opacity);
    if (P == 0) {
        if (n_draws != 0) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_mcmc_plan: n_draws=%d from an empty set", n_draws);
        counts_host[0] = counts_host[1] = counts_host[2] = counts_host[3] = 0;
        return GSR_OK;
    }
    if (!opacity || !scaling || !u || !ws) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_mcmc_plan: null pointer");
    size_t need = 0;
    HIP_TRY(mcmc_workspace_bytes(P, n_draws, &need), "mcmc workspace size");
    if (ws_bytes < need) return fail(GSR_ERR_WORKSPACE, "mcmc workspace %zu < %zu", ws_bytes, need);
    HIP_TRY(launch_mcmc_plan(mode, P, opacity, scaling, L, min_opacity, n_max, n_draws, u, counts_host, ws, (hipStream_t)stream), "mcmc plan launch");
    return GSR_OK;
}

int32_t gsr_mcmc_apply(gsr_stream_t stream, int32_t mode, int32_t P, int32_t n_draws, int32_t n_groups, const gsr_mcmc_group_t *groups,
                       const void *ws, size_t ws_bytes) {
    GSR_TRY(mcmc_sizes("gsr_mcmc_apply", P, n_draws));
    GSR_TRY(mcmc_mode("gsr_mcmc_apply", mode, n_draws));
    if (n_groups < 0 || n_groups > GSR_MCMC_MAX_GROUPS || (n_groups > 0 && !groups))
        return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_mcmc_apply: %d groups (at most %d)", n_groups, GSR_MCMC_MAX_GROUPS);
    if (P == 0) return GSR_OK;
    if (!ws) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_mcmc_apply: null pointer (ws)");
    const long long p_new = (long long)P + (long long)n_draws;
    const bool in_place = mode == GSR_MCMC_RELOCATE;
    for (int k = 0; k < n_groups; k++) {
        const gsr_mcmc_group_t &g = groups[k];
        GSR_TRY(refuse_group_size("gsr_mcmc_apply", k, g, (unsigned long long)p_new, "(P + n_draws)"));
        if (g.width_floats == 0) continue;
        if (!g.src || !g.dst) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_mcmc_apply: group %d: src / dst NULL", k);
        int nm = 0;
        GSR_TRY(refuse_group_moments("gsr_mcmc_apply", k, g, &nm));
        const bool same = g.src == g.dst && g.src_exp_avg == g.dst_exp_avg && g.src_exp_avg_sq == g.dst_exp_avg_sq;
        const bool apart = g.src != g.dst && (nm == 0 || (g.src_exp_avg != g.dst_exp_avg && g.src_exp_avg_sq != g.dst_exp_avg_sq));
        if (in_place ? !same : !apart)
            return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_mcmc_apply: group %d: relocation works in place (dst == src), growth into other buffers", k);
        if (g.role != GSR_MCMC_COPY && g.role != GSR_MCMC_OPACITY && g.role != GSR_MCMC_SCALING)
            return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_mcmc_apply: group %d: role %d", k, g.role);
        const int want = g.role == GSR_MCMC_OPACITY ? 1 : 3;
        if (g.role != GSR_MCMC_COPY && g.width_floats != want)
            return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_mcmc_apply: group %d: role %d needs width %d, got %d", k, g.role, want, g.width_floats);
    }
    size_t need = 0;
    HIP_TRY(mcmc_workspace_bytes(P, n_draws, &need), "mcmc workspace size");
    if (ws_bytes < need) return fail(GSR_ERR_WORKSPACE, "mcmc workspace %zu < %zu", ws_bytes, need);
    HIP_TRY(launch_mcmc_apply(mode, P, n_draws, n_groups, groups, ws, (hipStream_t)stream), "mcmc apply launch");
    return GSR_OK;
}

int32_t gsr_mcmc_noise(gsr_stream_t stream, int32_t P, const float *opacity, const float *scaling, const float *rotation, const float *noise,
                       float *xyz, float gate_k, float gate_t, float scale) {
    if (P < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_mcmc_noise: P=%d is negative", P);
    if (P == 0) return GSR_OK;
    if (!opacity || !scaling || !rotation || !noise || !xyz) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_mcmc_noise: null pointer");
    if ((uintptr_t)rotation & 15) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_mcmc_noise: rotation must be 16-byte aligned (a quaternion is one 16-byte load)");
    hipLaunchKernelGGL(mcmc_noise_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, P, opacity, scaling, rotation, noise, xyz, gate_k,
                       gate_t, scale);
    HIP_TRY(hipGetLastError(), "mcmc noise launch");
    return GSR_OK;
}

int32_t gsr_mcmc_regularize_workspace(int32_t P, size_t *bytes) {
    if (!bytes) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_mcmc_regularize_workspace: bytes is NULL");
    if (P < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_mcmc_regularize_workspace: P=%d is negative", P);
    *bytes = regularize_workspace_bytes(P);
    return GSR_OK;
}

int32_t gsr_mcmc_regularize(gsr_stream_t stream, int32_t P, const float *opacity, const float *scaling, float *grad_opacity, int32_t stride_o,
                            float *grad_scaling, int32_t stride_s, double lambda_o, double lambda_s, double *means_out, void *ws, size_t ws_bytes) {
    if (P < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_mcmc_regularize: P=%d is negative", P);
    if (P == 0) return GSR_OK;
    if (stride_o < 1 || stride_s < 3)
        return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_mcmc_regularize: stride_o=%d stride_s=%d, at least 1 and 3", stride_o, stride_s);
    if (!opacity || !scaling || !grad_opacity || !grad_scaling || !means_out || !ws) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_mcmc_regularize: null pointer");
    if ((uintptr_t)means_out & 7) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_mcmc_regularize: means_out must be 8-byte aligned");
    const size_t need = regularize_workspace_bytes(P);
    if (ws_bytes < need) return fail(GSR_ERR_WORKSPACE, "mcmc regularize workspace %zu < %zu", ws_bytes, need);
    const int nblk = (P + 255) / 256;
    double *partial = (double *)ws;
    hipLaunchKernelGGL(mcmc_regularize_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, P, opacity, scaling, grad_opacity, stride_o, grad_scaling,
                       stride_s, (float)(lambda_o / (double)P), (float)(lambda_s / (3.0 * (double)P)), partial);
    HIP_TRY(hipGetLastError(), "mcmc regularize launch");
    hipLaunchKernelGGL(mcmc_means_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, P, nblk, (const double *)partial, means_out);
    HIP_TRY(hipGetLastError(), "mcmc means launch");
    return GSR_OK;
}

}  // extern "C"
