// contrib_stats.hip -- per-Gaussian blend-weight statistics of a render (include/gsr_contrib.h): kernels and entry points.
//
// Built beside the colour path, which it does not touch, from map_walk.h's pieces: the walk is depth_fwd_kernel's (depth_maps.hip) with
// the depth value dropped -- a wave64 owns the two 8x8 blocks of one half tile, stages the list 64 entries at a time into its own LDS
// slice and walks the set bits of the ballot of reachable entries, front to back, to the half tile's largest last contributor -- and
// forms the same w = alpha * T per (entry, pixel), from the same expression under the same contraction setting.  What is new is the
// reduction over pixels: per entry the wave folds its 64 + 64 weights into three wave-uniform integers,
//   sum   of floor(w 2^32): the low and the high 16-bit halves are summed apart (128 x 65535 < 2^23 each) and recombined in 64 bits,
//   max   of the bit patterns (w >= 0: unsigned order is float order),
//   count = the popcount of the two blend masks, which are scalars already,
// by four DPP steps inside each row of 16 lanes and four v_readlane across the rows: the results are in SGPRs, where the row's address
// is formed.  Lane 0 then issues three vector integer atomics (add_x2, umax, add) into Gaussian g's 16-byte row, only when some lane
// blended.  Integer sums and maxima do not depend on the order, so the rows are the same bytes whatever the wave geometry, the route
// that built the lists or the order of the views.
// The loop is this file's own (map_walk.h says why the walks are not a template over callables).
#include <string.h>

#include "../../include/gsr_contrib.h"
#include "map_walk.h"

namespace gsr {
namespace {

struct ContribArgs : WalkArgs {                      // mode: unused
    gsr_contrib_row_t *rows;                         // [P]
};

// stages entry base + lane of the tile's list: (px, py, a, b) (c, opacity, g, bits); returns whether the entry reaches a block
__device__ __forceinline__ bool stage_entry(const ContribArgs &a, const HalfTile &h, float4 *my, const int tile, const int sub, const int base,
                                            const int cnt, const int lane) {
    Entry e;
    if (!gather_entry(a, h, tile, sub, base, cnt, lane, false, e)) return false;
    my[lane] = e.s0;
    my[64 + lane] = make_float4(e.s1.x, e.s1.y, __uint_as_float(e.g), __uint_as_float(e.bits));
    return e.bits != 0u;
}

// Wave-wide folds of an unsigned word with all 64 lanes active: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror and
// row_mirror leave every lane of a row of 16 with the row's result; the four rows meet in scalar registers.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
__device__ __forceinline__ uint32_t wave_fold_add(uint32_t v) {
    v += dpp_u32<0xB1>(v); v += dpp_u32<0x4E>(v); v += dpp_u32<0x141>(v); v += dpp_u32<0x140>(v);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) +
           (uint32_t)__builtin_amdgcn_readlane((int)v, 32) + (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}
__device__ __forceinline__ uint32_t wave_fold_max(uint32_t v) {
    v = max(v, dpp_u32<0xB1>(v)); v = max(v, dpp_u32<0x4E>(v)); v = max(v, dpp_u32<0x141>(v)); v = max(v, dpp_u32<0x140>(v));
    return max(max((uint32_t)__builtin_amdgcn_readlane((int)v, 0), (uint32_t)__builtin_amdgcn_readlane((int)v, 16)),
               max((uint32_t)__builtin_amdgcn_readlane((int)v, 32), (uint32_t)__builtin_amdgcn_readlane((int)v, 48)));
}

__global__ __launch_bounds__(256) void contrib_walk_kernel(ContribArgs a) {
    __shared__ __align__(16) float4 stage[4][128];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int unit = blockIdx.x * 4 + wave, tile = unit >> 1, sub = unit & 1;
    if (tile >= a.gridx * a.gridy) return;              // wave-uniform
    float4 *my = stage[wave];
    const HalfTile h = half_tile(a, tile, sub, lane);
    float Tr[2] = {1.f, 1.f};
    for (int base = 0; base < h.hi; base += 64) {
        const int cnt = min(64, h.hi - base);
        __builtin_amdgcn_wave_barrier();
        const bool live = stage_entry(a, h, my, tile, sub, base, cnt, lane);
        uint64_t todo = __ballot(live);
        __builtin_amdgcn_wave_barrier();
        while (todo) {
            const int j = __builtin_ctzll(todo);
            todo &= todo - 1;
            const float4 r0 = my[j], r1 = my[64 + j];
            const uint32_t bits = __builtin_amdgcn_readfirstlane(__float_as_uint(r1.w)) & 3u;
            const uint32_t g = __builtin_amdgcn_readfirstlane(__float_as_uint(r1.z));       // < P: gather_entry staged no other
            const int pos = base + j;
            const StagedConic kc = {r0.z, r0.w, r1.x};
            const RowTerms rt = splat_row_terms(kc, r0.y - h.fy);
            uint32_t lo = 0u, hi = 0u, mx = 0u, n = 0u;
#pragma unroll
            for (int q = 0; q < 2; q++) {
                if (!(bits & (1u << q)) || pos >= h.blk_last[q]) continue;          // scalar branch
                float araw;                                                          // the one evaluation every pass shares (gsr_device.h)
                const unsigned long long okm = splat_alpha(splat_power_log2_row(kc, rt, r0.x - h.fx[q]), r1.y, araw) &
                                               __builtin_amdgcn_ballot_w64(pos < h.last[q]);
                const float alpha = fminf(GSR_ALPHA_MAX, araw);
                const float aT = alpha * Tr[q];
                const bool ok = __builtin_amdgcn_inverse_ballot_w64(okm);
                const float w = ok ? aT : 0.f;                                       // a skipped lane's exp2 may be inf: selected away, not multiplied
                const uint32_t u = (uint32_t)(w * 4294967296.0f);                    // exact scaling, truncating conversion; w <= 0.99
                lo += u & 0xffffu; hi += u >> 16;
                mx = max(mx, __float_as_uint(w));
                n += (uint32_t)__builtin_popcountll(okm);
                if (ok) Tr[q] = Tr[q] - aT;                                          // T (1 - alpha), the colour pass's form
            }
            if (n == 0u) continue;                      // wave-uniform: no pixel of this wave blends the splat
            const unsigned long long total = ((unsigned long long)wave_fold_add(hi) << 16) + wave_fold_add(lo);
            const uint32_t top = wave_fold_max(mx);
            if (lane == 0) {
                gsr_contrib_row_t *row = a.rows + g;
                atomicAdd(reinterpret_cast<unsigned long long *>(&row->sum_q32), total);
                atomicMax(&row->max_bits, top);
                atomicAdd(&row->count, n);
            }
        }
    }
}

struct ReadArgs {
    int P;
    const gsr_contrib_row_t *rows;
    float *weight_sum, *weight_max;
    int32_t *pixel_count;
};

// one lane per row: a 16-byte load, up to three 4-byte stores
__global__ __launch_bounds__(256) void contrib_read_kernel(ReadArgs r) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= r.P) return;
    const uint4 v = reinterpret_cast<const uint4 *>(r.rows)[i];
    const unsigned long long q = (unsigned long long)v.x | ((unsigned long long)v.y << 32);
    if (r.weight_sum) r.weight_sum[i] = (float)((double)q * 0x1p-32);
    if (r.weight_max) r.weight_max[i] = __uint_as_float(v.z);
    if (r.pixel_count) r.pixel_count[i] = (int32_t)v.w;
}

// a refusal of a shared check, with this call's name in front of its text
int32_t named(const char *who, int32_t rc) {
    if (rc == GSR_OK) return rc;
    char text[GSR_ERR_TEXT_BYTES];
    const char *was = gsr_last_error();
    strncpy(text, was ? was : "", sizeof text - 1);
    text[sizeof text - 1] = 0;
    return strncmp(text, who, strlen(who)) == 0 ? rc : fail(rc, "%s: %s", who, text);
}

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

static_assert(sizeof(gsr_contrib_row_t) == 16 && offsetof(gsr_contrib_row_t, max_bits) == 8 && offsetof(gsr_contrib_row_t, count) == 12,
              "gsr_contrib_row_t is 16 bytes: sum, max, count");

int32_t gsr_contrib_accumulate(gsr_stream_t stream, int32_t P, int32_t W, int32_t H, int64_t R,
                               const void *geom_ws, size_t geom_bytes, const void *binning_ws, size_t binning_bytes,
                               const void *img_ws, size_t img_bytes, gsr_contrib_row_t *rows) {
    const char *who = "gsr_contrib_accumulate";
    GSR_TRY(named(who, map_sizes(who, P, W, H, (long long)R)));
    if (P == 0 || R == 0) return GSR_OK;
    Views v;
    GSR_TRY(named(who, view_all(v, P, W, H, (long long)R, {geom_ws, geom_bytes, binning_ws, binning_bytes, img_ws, img_bytes})));
    if (!rows || !geom_ws || !binning_ws || !img_ws) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: missing rows or workspace", who);
    ContribArgs a = walk_args<ContribArgs>(v, P, W, H, (long long)R);
    a.rows = rows;
    hipLaunchKernelGGL(contrib_walk_kernel, dim3(walk_blocks(a)), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError(), "contribution walk launch");
    return GSR_OK;
}

int32_t gsr_contrib_read(gsr_stream_t stream, int32_t P, const gsr_contrib_row_t *rows, float *weight_sum, float *weight_max, int32_t *pixel_count) {
    const char *who = "gsr_contrib_read";
    if (P < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: bad sizes", who);
    if (!weight_sum && !weight_max && !pixel_count) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: weight_sum, weight_max and pixel_count are all NULL", who);
    if (P == 0) return GSR_OK;
    if (!rows) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: missing rows", who);
    const ReadArgs r = {P, rows, weight_sum, weight_max, pixel_count};
    hipLaunchKernelGGL(contrib_read_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, r);
    HIP_TRY(hipGetLastError(), "contribution read launch");
    return GSR_OK;
}

}  // extern "C"
