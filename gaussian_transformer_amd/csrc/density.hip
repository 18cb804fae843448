// density.hip -- adaptive density control on the device (include/gsr_density.h):
//   record : one lane per Gaussian, the three statistics of a view in one launch.
//   plan   : flag kernel (one lane per row: the whole clone / split / prune rule) -> one rocPRIM exclusive scan that carries
//            the four ranks (and the clone total) in one value -> map kernel (the source of every row of the new state, the counts).
//   apply  : ONE launch over (destination row, column) of every group: consecutive lanes write consecutive floats of the new
//            parameter and both new moments; 16-byte accesses where the width is a multiple of 4 and every pointer is aligned.
//            The group table, its filler, the quaternion's rotation and the common group refusals are group_table.h's, shared
//            with mcmc.hip; the kernel, which reads the map and the ranks, is this file's.
// Compiled with -ffp-contract=off -fno-slp-vectorize like the other per-Gaussian units: the norm of record and the plan's
// decisions round as written.  No float atomics anywhere: bit-identical from run to run.
#include <cstring>  // ROCm 7.2 rocprim/texture_cache_iterator.hpp uses memset without including it
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "../../include/gsr_density.h"
#include "group_table.h"

namespace gsr {

// ---------------------------------------------------------------- record ----------------------------------------------------------------

__global__ __launch_bounds__(256) void density_record_kernel(int P, const float *__restrict__ grad2d, int stride, const int32_t *__restrict__ radii,
                                                             const uint8_t *__restrict__ visible, float *__restrict__ accum,
                                                             float *__restrict__ denom, float *__restrict__ max_radii) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const int r = radii[i];
    const bool vis = visible ? visible[i] != 0 : r > 0;
    if (!vis) return;
    const float x = grad2d[(size_t)i * stride], y = grad2d[(size_t)i * stride + 1];
    accum[i] = accum[i] + sqrtf(x * x + y * y);
    denom[i] = denom[i] + 1.f;
    const float m = max_radii[i], rf = (float)r;
    max_radii[i] = rf > m ? rf : m;
}

static hipError_t launch_density_record(int P, const float *grad2d, int stride, const int32_t *radii, const uint8_t *visible, float *accum,
                                 float *denom, float *max_radii, hipStream_t s) {
    hipLaunchKernelGGL(density_record_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, grad2d, stride, radii, visible, accum, denom, max_radii);
    return hipGetLastError();
}

// ---------------------------------------------------------------- plan ----------------------------------------------------------------

enum { F_KEEP_SELF = 1, F_KEEP_CLONE = 2, F_SPLIT = 4, F_KEEP_CHILD = 8, F_CLONE = 16 };
enum { C_NCLONE = 0, C_NSPLIT = 1, C_NPRUNED = 2, C_PNEW = 3, C_KEEP_SELF = 4, C_KEEP_CLONE = 5, C_KEEP_CHILD = 6, C_WORDS = 8 };
#define MAP_KIND_SHIFT 30          // P * (N + 1) < 2^31 and N >= 1, so a row index leaves the two top bits free
#define MAP_ROW_MASK 0x3fffffffu
enum { KIND_SELF = 0, KIND_CLONE = 1, KIND_CHILD = 2 };

struct Rank5 { uint32_t self, clone, split, child, clone_all; };
struct RankAdd {
    __host__ __device__ Rank5 operator()(const Rank5 &a, const Rank5 &b) const {
        return Rank5{a.self + b.self, a.clone + b.clone, a.split + b.split, a.child + b.child, a.clone_all + b.clone_all};
    }
};
struct FlagToRank {
    __host__ __device__ Rank5 operator()(uint8_t f) const {
        return Rank5{(uint32_t)(f & F_KEEP_SELF ? 1 : 0), (uint32_t)(f & F_KEEP_CLONE ? 1 : 0), (uint32_t)(f & F_SPLIT ? 1 : 0),
                     (uint32_t)(f & F_KEEP_CHILD ? 1 : 0), (uint32_t)(f & F_CLONE ? 1 : 0)};
    }
};

struct PlanWs { uint32_t *counts; uint8_t *flags; Rank5 *ranks; uint32_t *map; void *temp; size_t temp_bytes, total; };

static hipError_t carve_plan_ws(void *base, int P, int N, PlanWs &w) {
    const size_t np = (size_t)(P > 0 ? P : 1);
    size_t tb = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, tb, rocprim::make_transform_iterator((const uint8_t *)nullptr, FlagToRank()), (Rank5 *)nullptr,
                                           Rank5{0, 0, 0, 0, 0}, np, RankAdd(), (hipStream_t)0, false);
    if (e != hipSuccess) return e;
    Bump b = {(char *)base, 0};
    w.counts = b.take<uint32_t>(C_WORDS);
    w.flags = b.take<uint8_t>(np);
    w.ranks = b.take<Rank5>(np);
    w.map = b.take<uint32_t>(np * (size_t)(N + 1));
    w.temp = b.take<char>(tb > 0 ? tb : 1);
    w.temp_bytes = tb;
    w.total = b.off;
    return hipSuccess;
}

static hipError_t densify_plan_workspace_bytes(int P, int N, size_t *bytes) {
    PlanWs w;
    hipError_t e = carve_plan_ws(nullptr, P, N, w);
    if (e == hipSuccess) *bytes = w.total;
    return e;
}

__device__ __forceinline__ float max3(float a, float b, float c) { const float m = a > b ? a : b; return m > c ? m : c; }

__global__ __launch_bounds__(256) void densify_flags_kernel(int P, const float *__restrict__ opacity, const float *__restrict__ scaling,
                                                            const float *__restrict__ accum, const float *__restrict__ denom, float grad_threshold,
                                                            float min_opacity, float cut, float prune_world, float child_div,
                                                            uint8_t *__restrict__ flags) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    float g = accum[i] / denom[i];
    if (g != g) g = 0.f;
    const float e0 = expf(scaling[3 * (size_t)i]), e1 = expf(scaling[3 * (size_t)i + 1]), e2 = expf(scaling[3 * (size_t)i + 2]);
    const float size = max3(e0, e1, e2);
    const bool hot = g >= grad_threshold;
    const bool clone = hot && size <= cut, split = hot && size > cut;
    const bool low = 1.f / (1.f + expf(-opacity[i])) < min_opacity;
    const bool test_size = prune_world >= 0.f;
    const bool big = test_size && size > prune_world;
    const float csize = max3(expf(logf(e0 / child_div)), expf(logf(e1 / child_div)), expf(logf(e2 / child_div)));
    const bool childbig = test_size && csize > prune_world;
    uint32_t f = 0;
    if (!split && !(low || big)) f |= F_KEEP_SELF;
    if (clone) f |= F_CLONE;
    if (clone && !(low || big)) f |= F_KEEP_CLONE;
    if (split) f |= F_SPLIT;
    if (split && !(low || childbig)) f |= F_KEEP_CHILD;
    flags[i] = (uint8_t)f;
}

// one lane per source row: files the row's destinations in the map; the lane of row 0 writes the counts
__global__ __launch_bounds__(256) void densify_map_kernel(int P, int N, const uint8_t *__restrict__ flags, const Rank5 *__restrict__ ranks,
                                                          uint32_t *__restrict__ map, uint32_t *__restrict__ counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const Rank5 tot = RankAdd()(ranks[P - 1], FlagToRank()(flags[P - 1]));
    const uint32_t p_new = tot.self + tot.clone + (uint32_t)N * tot.child;
    if (i == 0) {
        counts[C_NCLONE] = tot.clone_all;
        counts[C_NSPLIT] = tot.split;
        counts[C_NPRUNED] = ((uint32_t)P - tot.split - tot.self) + (tot.clone_all - tot.clone) + (uint32_t)N * (tot.split - tot.child);
        counts[C_PNEW] = p_new;
        counts[C_KEEP_SELF] = tot.self;
        counts[C_KEEP_CLONE] = tot.clone;
        counts[C_KEEP_CHILD] = tot.child;
        counts[7] = 0;
    }
    const uint32_t f = flags[i];
    const Rank5 r = ranks[i];
    const uint32_t cap = (uint32_t)P * (uint32_t)(N + 1);          // the map's size: p_new <= cap by construction
    if ((f & F_KEEP_SELF) && r.self < cap) map[r.self] = (uint32_t)i | (KIND_SELF << MAP_KIND_SHIFT);
    if (f & F_KEEP_CLONE) {
        const uint32_t d = tot.self + r.clone;
        if (d < cap) map[d] = (uint32_t)i | (KIND_CLONE << MAP_KIND_SHIFT);
    }
    if (f & F_KEEP_CHILD)
        for (int j = 0; j < N; j++) {
            const uint32_t d = tot.self + tot.clone + (uint32_t)j * tot.child + r.child;
            if (d < cap) map[d] = (uint32_t)i | ((uint32_t)KIND_CHILD << MAP_KIND_SHIFT);
        }
}

// sizes validated by the caller; P >= 1
static hipError_t launch_densify_plan(int P, const float *opacity, const float *scaling, const float *accum, const float *denom, float grad_threshold,
                               float min_opacity, float cut, float prune_world, int N, uint32_t *counts_host, void *ws, hipStream_t s) {
    PlanWs w;
    hipError_t e = carve_plan_ws(ws, P, N, w);
    if (e != hipSuccess) return e;
    const dim3 grid((P + 255) / 256), block(256);
    hipLaunchKernelGGL(densify_flags_kernel, grid, block, 0, s, P, opacity, scaling, accum, denom, grad_threshold, min_opacity, cut, prune_world,
                       (float)(0.8 * (double)N), w.flags);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t tb = w.temp_bytes;
    e = rocprim::exclusive_scan(w.temp, tb, rocprim::make_transform_iterator((const uint8_t *)w.flags, FlagToRank()), w.ranks, Rank5{0, 0, 0, 0, 0},
                                (size_t)P, RankAdd(), s, false);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(densify_map_kernel, grid, block, 0, s, P, N, (const uint8_t *)w.flags, (const Rank5 *)w.ranks, w.map, w.counts);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return hipMemcpyAsync(counts_host, w.counts, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
}

// ---------------------------------------------------------------- apply ----------------------------------------------------------------

struct ApplyArgs {
    GroupDev grp[GSR_DENSITY_MAX_GROUPS];
    int n_groups, P, N;
    uint32_t p_new, n_split;
    double child_div;            // 0.8 * N
    const float *scaling, *rotation, *noise;
    const uint32_t *map, *counts;
    const Rank5 *ranks;
};

// The values of the split children are evaluated in float64 and rounded once: each is the float32 nearest to the formula's exact
// value, so no float32 evaluation of the same formula (torch's, on either device) lies nearer to it.  Three values per child, beside
// 3 x 59 floats copied per row: the double-rate arithmetic does not show in the kernel's time.
// coordinate c of the child of Gaussian i drawn with noise row n: R(q / |q|) . (noise * exp(scaling)) + xyz
__device__ __forceinline__ float child_xyz(const ApplyArgs &a, const float *__restrict__ xyz, uint32_t i, uint32_t n, uint32_t c) {
    const Quat64 q = unit_quat64(a.rotation[4 * (size_t)i], a.rotation[4 * (size_t)i + 1], a.rotation[4 * (size_t)i + 2], a.rotation[4 * (size_t)i + 3]);
    const double s0 = (double)a.noise[3 * (size_t)n] * exp((double)a.scaling[3 * (size_t)i]),
                 s1 = (double)a.noise[3 * (size_t)n + 1] * exp((double)a.scaling[3 * (size_t)i + 1]),
                 s2 = (double)a.noise[3 * (size_t)n + 2] * exp((double)a.scaling[3 * (size_t)i + 2]);
    const Row64 m = rot_row(q, c);
    return (float)(m.c0 * s0 + m.c1 * s1 + m.c2 * s2 + (double)xyz[3 * (size_t)i + c]);
}

__global__ __launch_bounds__(256) void densify_apply_kernel(ApplyArgs a) {
    // the plan in the workspace must be the one the caller sized the outputs for (uniform)
    if (a.counts[C_PNEW] != a.p_new || a.counts[C_NSPLIT] != a.n_split) return;
    const GroupDev &G = a.grp[group_of_block(a)];
    const uint32_t w = G.w;
    const uint64_t total = (uint64_t)a.p_new * w;               // < 2^32 (checked by the caller)
    const uint64_t base = (uint64_t)(blockIdx.x - G.first_block) * GROUP_PER_BLOCK;
    const uint32_t child0 = a.counts[C_KEEP_SELF] + a.counts[C_KEEP_CLONE], keep_child = a.counts[C_KEEP_CHILD];
    const bool moments = G.dm != nullptr;
    if (G.vec4) {                                               // w % 4 == 0, role copy: a float4 never leaves its row
        const uint64_t e = base + (uint64_t)threadIdx.x * 4;
        if (e >= total) return;
        const uint32_t row = (uint32_t)(e / w), c = (uint32_t)(e - (uint64_t)row * w);
        const uint32_t m = a.map[row], i = m & MAP_ROW_MASK;
        if (i >= (uint32_t)a.P) return;
        const size_t so = (size_t)i * w + c;
        *reinterpret_cast<float4 *>(G.dst + e) = *reinterpret_cast<const float4 *>(G.src + so);
        if (moments) {
            float4 mm = make_float4(0.f, 0.f, 0.f, 0.f), vv = mm;
            if ((m >> MAP_KIND_SHIFT) == KIND_SELF) { mm = *reinterpret_cast<const float4 *>(G.sm + so); vv = *reinterpret_cast<const float4 *>(G.sv + so); }
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
        const uint32_t m = a.map[row], i = m & MAP_ROW_MASK, kind = m >> MAP_KIND_SHIFT;
        if (i >= (uint32_t)a.P) continue;
        const size_t so = (size_t)i * w + c;
        float p;
        if (kind == KIND_CHILD && G.role != GSR_DENSITY_COPY) {
            if (G.role == GSR_DENSITY_SCALING) {
                p = (float)log(exp((double)G.src[so]) / a.child_div);
            } else {
                const uint32_t j = keep_child ? (row - child0) / keep_child : 0u;
                const uint32_t n = j * a.n_split + a.ranks[i].split;
                if (j >= (uint32_t)a.N || n >= (uint32_t)a.N * a.n_split) continue;
                p = child_xyz(a, G.src, i, n, c);
            }
        } else {
            p = G.src[so];
        }
        G.dst[e] = p;
        if (moments) {
            const bool self = kind == KIND_SELF;
            G.dm[e] = self ? G.sm[so] : 0.f;
            G.dv[e] = self ? G.sv[so] : 0.f;
        }
    }
}

// sizes, pointers and roles validated by the caller; P >= 1, p_new >= 1
static hipError_t launch_densify_apply(int P, int N, uint32_t n_split, uint32_t p_new, int n_groups, const gsr_density_group_t *groups,
                                const float *scaling, const float *rotation, const float *noise, const void *ws, hipStream_t s) {
    PlanWs w;
    hipError_t e = carve_plan_ws(const_cast<void *>(ws), P, N, w);
    if (e != hipSuccess) return e;
    ApplyArgs a;
    memset(&a, 0, sizeof(a));
    a.P = P; a.N = N; a.p_new = p_new; a.n_split = n_split; a.child_div = 0.8 * (double)N;
    a.scaling = scaling; a.rotation = rotation; a.noise = noise;
    a.map = w.map; a.counts = w.counts; a.ranks = w.ranks;
    const unsigned blocks = fill_group_table(n_groups, groups, p_new, GSR_DENSITY_COPY, a.grp, a.n_groups);
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(densify_apply_kernel, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace gsr

using namespace gsr;

extern "C" {

// ---- density control on the device (include/gsr_density.h) ----
int32_t gsr_density_record(gsr_stream_t stream, int32_t P, const float *grad2d, int32_t grad_stride_floats, const int32_t *radii,
                           const uint8_t *visible, float *accum, float *denom, float *max_radii) {
    if (P < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_density_record: P=%d is negative", P);
    if (P == 0) return GSR_OK;
    if (grad_stride_floats < 2) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_density_record: grad_stride_floats=%d, at least 2", grad_stride_floats);
    if (!grad2d || !radii || !accum || !denom || !max_radii) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_density_record: null pointer");
    HIP_TRY(launch_density_record(P, grad2d, grad_stride_floats, radii, visible, accum, denom, max_radii, (hipStream_t)stream), "density record launch");
    return GSR_OK;
}

static int densify_sizes(const char *who, int32_t P, int32_t N) {
    if (P < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: P=%d is negative", who, P);
    if (N < 1) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: N=%d, at least 1", who, N);
    if ((long long)P * ((long long)N + 1) > 0x7fffffffLL)
        return fail(GSR_ERR_INVALID_ARGUMENT, "%s: P * (N + 1) = %lld, must stay below 2^31", who, (long long)P * ((long long)N + 1));
    return GSR_OK;
}

int32_t gsr_densify_plan_workspace(int32_t P, int32_t N, size_t *bytes) {
    if (!bytes) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_densify_plan_workspace: bytes is NULL");
    if (densify_sizes("gsr_densify_plan_workspace", P, N) != GSR_OK) return GSR_ERR_INVALID_ARGUMENT;
    HIP_TRY(densify_plan_workspace_bytes(P, N, bytes), "densify workspace size");
    return GSR_OK;
}

int32_t gsr_densify_plan(gsr_stream_t stream, int32_t P, const float *opacity, const float *scaling, const float *accum, const float *denom,
                         float grad_threshold, float min_opacity, float cut, float prune_world_size, int32_t N, uint32_t *counts_host, void *ws,
                         size_t ws_bytes) {
    if (densify_sizes("gsr_densify_plan", P, N) != GSR_OK) return GSR_ERR_INVALID_ARGUMENT;
    if (!counts_host) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_densify_plan: counts_host is NULL");
    if (!(grad_threshold > 0.f)) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_densify_plan: grad_threshold=%g, must be > 0", (double)grad_threshold);
    if (P == 0) {
        counts_host[0] = counts_host[1] = counts_host[2] = counts_host[3] = 0;
        return GSR_OK;
    }
    if (!opacity || !scaling || !accum || !denom || !ws) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_densify_plan: null pointer");
    size_t need = 0;
    HIP_TRY(densify_plan_workspace_bytes(P, N, &need), "densify workspace size");
    if (ws_bytes < need) return fail(GSR_ERR_WORKSPACE, "densify workspace %zu < %zu", ws_bytes, need);
    HIP_TRY(launch_densify_plan(P, opacity, scaling, accum, denom, grad_threshold, min_opacity, cut, prune_world_size, N, counts_host, ws,
                                (hipStream_t)stream), "densify plan launch");
    return GSR_OK;
}

int32_t gsr_densify_apply(gsr_stream_t stream, int32_t P, int32_t N, int32_t n_split, int32_t P_new, int32_t n_groups,
                          const gsr_density_group_t *groups, const float *scaling, const float *rotation, const float *noise, const void *ws,
                          size_t ws_bytes) {
    if (densify_sizes("gsr_densify_apply", P, N) != GSR_OK) return GSR_ERR_INVALID_ARGUMENT;
    if (n_groups < 0 || n_groups > GSR_DENSITY_MAX_GROUPS || (n_groups > 0 && !groups))
        return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_densify_apply: %d groups (at most %d)", n_groups, GSR_DENSITY_MAX_GROUPS);
    if (n_split < 0 || n_split > P || P_new < 0 || (long long)P_new > (long long)P * ((long long)N + 1))
        return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_densify_apply: n_split=%d P_new=%d do not belong to a plan of P=%d N=%d", n_split, P_new, P, N);
    if (P == 0 || P_new == 0) return GSR_OK;
    if (!ws) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_densify_apply: null pointer (ws)");
    size_t need = 0;
    HIP_TRY(densify_plan_workspace_bytes(P, N, &need), "densify workspace size");
    if (ws_bytes < need) return fail(GSR_ERR_WORKSPACE, "densify workspace %zu < %zu", ws_bytes, need);
    for (int k = 0; k < n_groups; k++) {
        const gsr_density_group_t &g = groups[k];
        GSR_TRY(refuse_group_size("gsr_densify_apply", k, g, (unsigned long long)P_new, "P_new"));
        if (g.width_floats == 0) continue;
        if (!g.src || !g.dst || g.src == g.dst) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_densify_apply: group %d: src / dst NULL or equal", k);
        GSR_TRY(refuse_group_moments("gsr_densify_apply", k, g));
        if (g.role != GSR_DENSITY_COPY && g.role != GSR_DENSITY_XYZ && g.role != GSR_DENSITY_SCALING)
            return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_densify_apply: group %d: role %d", k, g.role);
        if (g.role != GSR_DENSITY_COPY && g.width_floats != 3)
            return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_densify_apply: group %d: role %d needs width 3, got %d", k, g.role, g.width_floats);
        if (g.role == GSR_DENSITY_XYZ && n_split > 0 && (!scaling || !rotation || !noise))
            return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_densify_apply: group %d: the xyz role needs scaling, rotation and noise", k);
    }
    HIP_TRY(launch_densify_apply(P, N, (uint32_t)n_split, (uint32_t)P_new, n_groups, groups, scaling, rotation, noise, ws, (hipStream_t)stream),
            "densify apply launch");
    return GSR_OK;
}

}  // extern "C"
