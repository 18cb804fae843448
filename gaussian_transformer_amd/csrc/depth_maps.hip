// depth_maps.hip -- depth and accumulated-opacity maps of a render, with gradients (include/gsr_depth.h): kernels and entry points.
//
// Built beside the colour path, which it does not touch: both walks re-read what gsr_forward left on the device -- the per-tile lists,
// the records (centre, conic, opacity, view-space depth), the reachability bytes per (entry, 8x8 block), final_T and n_contrib per
// pixel -- so no per-Gaussian stage and no list build runs again.
//
// CDNA4 shape, as composite_bwd.hip's classic decomposition: a wave64 owns the two 8x8 blocks of one half tile (they lie side by side
// and share dy, so the exponent is formed with gsr_device.h's row terms, the form the colour pass uses: same bits, same decisions);
// lane l holds pixel l of each block.  Waves never synchronise with each other: each stages the list 64 entries at a time into its own
// LDS slice (id -> record gather, 7 of the 12 floats: px py conic x 3, opacity, depth) and walks the set bits of the ballot of
// reachable entries.  The walk ends at the half tile's largest last contributor; a pixel blends the entries in front of its own.
//   forward: front to back, D += v alpha T, T = T - alpha T.  The stop test is not evaluated: no entry in front of the last contributor
//            triggered it.  alpha map = 1 - final_T, read, not re-composited.
//   reverse: back to front with the running suffix S = sum_{j > i} v_j alpha_j T_j and T reconstructed from final_T as bwd_unit does it:
//            dL/dalpha = gD (v T_i - S / (1 - alpha)) + gA T_final / (1 - alpha); the 0.99 cap straight-through, 1 / (1 - alpha) by
//            v_rcp_f32 as there.  (bwd_unit's own recurrence for the colour (v, 1, 0) is the same sum, but forms the alpha term as
//            1 - (alpha composited behind, normalised): in a pixel that saturates that is 1 - 0.9999.., and float32 loses three digits
//            of dL/dopacity -- measured against the float64 oracle.)  Seven sums per (wave, entry): the six moments of
//            s = opacity G dL/dalpha (slots 3..8 of the 16-float accumulator row, gsr_internal.h) and dL/dv (spare slot 9), reduced
//            through LDS + two DPP steps and issued as ONE 7-lane global_atomic_add_f32 into 28 contiguous bytes of the row, only when
//            some lane blended.  A splat with replica rows adds into replica (tile mod K).
// pergauss_bwd.hip's streaming kernel then runs unchanged on these rows (no colour input at all: shs = colors_precomp = NULL is a case
// its launcher already takes), and depth_finish_kernel adds the dL/dv term to dL/dmeans3D -- and, with accumulate, the whole result
// to the caller's buffers.
// Shared with the colour passes, one copy each in composite_common.h: the staged conic pair, the replica-row rule and the LDS + DPP
// reduction (here with 7 sums, there with 9); the signed wave-wide max is gsr_device.h's.  Not its geometry and gather helpers: through
// them these two kernels come out with another instruction order (scripts/isa_diff.py).  The recurrences differ from bwd_unit's on
// purpose, see above.
// Shared with feature_maps.hip, one copy each in map_walk.h: the leading argument fields, the half tile's geometry, the record gather
// behind the range check on the id, the add of the staged result, and on the host the views, the sizes refusal, the workspace carve and
// the reverse call's common refusals, R == 0 clearing and per-Gaussian launch.  The walk loops are this file's own (map_walk.h says why).
// Zeroing: only the rows that can be added into (marked Gaussians + replica rows) are cleared, by composite_bwd.hip's
// launch_zero_marked_rows: 64 B per marked row and a byte read per Gaussian instead of a 66 P byte memset.
#include <string.h>

#include "../../include/gsr_depth.h"
#include "map_walk.h"
#include "pergauss_chain.h"

namespace gsr {
namespace {

#define DEPTH_NSUM 7                                    // s dx, s dy, s dx dx, s dx dy, s dy dy, s, dL/dv -> row slots 3..9
#define DEPTH_BWD_LDS_F4 (64 * 2 + (DEPTH_NSUM * RED_STRIDE + 3) / 4)

struct DepthArgs : WalkArgs {                        // mode: GSR_DEPTH_*
    float *out_depth, *out_alpha;           // forward (either may be NULL)
    const float *gD, *gA;                   // reverse (either may be NULL)
    float *acc;
};

// stages entry base + lane of the tile's list: (px, py, a, b) (c, opacity, v, bits | row << 4); returns whether the entry reaches a block
__device__ __forceinline__ bool stage_entry(const DepthArgs &a, const HalfTile &h, float4 *my, const int tile, const int sub, const int base,
                                            const int cnt, const int lane, const bool want_row) {
    Entry e;
    if (!gather_entry(a, h, tile, sub, base, cnt, lane, want_row, e)) return false;
    const float v = a.mode == GSR_DEPTH_INVERSE ? 1.0f / e.r2.y : e.r2.y;
    my[lane] = e.s0;
    my[64 + lane] = make_float4(e.s1.x, e.s1.y, v, entry_code(e));
    return e.bits != 0u;
}

__global__ __launch_bounds__(256) void depth_fwd_kernel(DepthArgs a) {
    __shared__ __align__(16) float4 stage[4][128];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int unit = blockIdx.x * 4 + wave, tile = unit >> 1, sub = unit & 1;
    if (tile >= a.gridx * a.gridy) return;              // wave-uniform
    float4 *my = stage[wave];
    HalfTile h = half_tile(a, tile, sub, lane);
    if (!a.out_depth) h.hi = 0;                         // the alpha map alone is a read of final_T
    float Tr[2] = {1.f, 1.f}, D[2] = {0.f, 0.f};
    for (int base = 0; base < h.hi; base += 64) {
        const int cnt = min(64, h.hi - base);
        __builtin_amdgcn_wave_barrier();
        const bool live = stage_entry(a, h, my, tile, sub, base, cnt, lane, false);
        uint64_t todo = __ballot(live);
        __builtin_amdgcn_wave_barrier();
        while (todo) {
            const int j = __builtin_ctzll(todo);
            todo &= todo - 1;
            const float4 r0 = my[j], r1 = my[64 + j];
            const uint32_t bits = __builtin_amdgcn_readfirstlane(__float_as_uint(r1.w)) & 3u;
            const int pos = base + j;
            const StagedConic kc = {r0.z, r0.w, r1.x};
            const RowTerms rt = splat_row_terms(kc, r0.y - h.fy);
#pragma unroll
            for (int q = 0; q < 2; q++) {
                if (!(bits & (1u << q)) || pos >= h.blk_last[q]) continue;          // scalar branch
                float araw;                                                          // the one evaluation every pass shares (gsr_device.h)
                const unsigned long long okm = splat_alpha(splat_power_log2_row(kc, rt, r0.x - h.fx[q]), r1.y, araw) &
                                               __builtin_amdgcn_ballot_w64(pos < h.last[q]);
                const float alpha = fminf(GSR_ALPHA_MAX, araw);
                const float aT = alpha * Tr[q];
                if (__builtin_amdgcn_inverse_ballot_w64(okm)) {
                    D[q] += r1.z * aT;
                    Tr[q] = Tr[q] - aT;                                              // T (1 - alpha), the colour pass's form
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 2; q++) {
        if (!h.inside[q]) continue;
        if (a.out_depth) a.out_depth[h.pix[q]] = D[q];
        if (a.out_alpha) a.out_alpha[h.pix[q]] = 1.f - a.final_T[h.pix[q]];
    }
}

__global__ __launch_bounds__(256) void depth_bwd_kernel(DepthArgs a) {
    __shared__ __align__(16) float4 stage[4][DEPTH_BWD_LDS_F4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int unit = blockIdx.x * 4 + wave, tile = unit >> 1, sub = unit & 1;
    if (tile >= a.gridx * a.gridy) return;              // wave-uniform
    float4 *my = stage[wave];
    float *red = reinterpret_cast<float *>(my + 128);   // [value 0..6][lane 0..63], rows of RED_STRIDE floats
    const HalfTile h = half_tile(a, tile, sub, lane);
    if (h.hi <= 0) return;
    // per pixel: Tr = transmittance behind the splats visited so far, S = sum of v alpha T over them (the running suffix of the depth
    // map), gAT = gA T_final
    float Tr[2], S[2] = {0.f, 0.f}, gD[2], gAT[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        Tr[q] = h.inside[q] ? a.final_T[h.pix[q]] : 1.f;
        gD[q] = h.inside[q] && a.gD ? a.gD[h.pix[q]] : 0.f;
        gAT[q] = h.inside[q] && a.gA ? a.gA[h.pix[q]] * Tr[q] : 0.f;
    }
    // lane 4 value + part adds red[value][16 part .. 16 part + 15]; two DPP steps fold the four parts; lanes 0, 4, .., 24 hold the totals
    const float4 *red_rd;
    bool red_lane;
    const int rvalue = reduce_setup<DEPTH_NSUM>(red, lane, red_rd, red_lane);
    const int slot = rvalue >= 0 ? 3 + rvalue : -1;

    for (int base = ((h.hi - 1) >> 6) << 6; base >= 0; base -= 64) {
        const int cnt = min(64, h.hi - base);
        __builtin_amdgcn_wave_barrier();
        const bool live = stage_entry(a, h, my, tile, sub, base, cnt, lane, true);
        uint64_t todo = __ballot(live);
        __builtin_amdgcn_wave_barrier();
        while (todo) {
            const int j = 63 - __builtin_clzll(todo);   // back to front
            todo &= ~(1ull << j);
            const float4 r0 = my[j], r1 = my[64 + j];
            const uint32_t code = __builtin_amdgcn_readfirstlane(__float_as_uint(r1.w));
            const uint32_t bits = code & 3u, row = code >> 4;
            const int pos = base + j;
            const StagedConic kc = {r0.z, r0.w, r1.x};
            const float dy = r0.y - h.fy;
            const RowTerms rt = splat_row_terms(kc, dy);
            float s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f, s5 = 0.f, s6 = 0.f, s7 = 0.f;
            unsigned long long any_ok = 0ull;
#pragma unroll
            for (int q = 0; q < 2; q++) {
                if (!(bits & (1u << q)) || pos >= h.blk_last[q]) continue;          // scalar branch
                const float dx = r0.x - h.fx[q];
                float araw;
                const unsigned long long okm = splat_alpha(splat_power_log2_row(kc, rt, dx), r1.y, araw) &
                                               __builtin_amdgcn_ballot_w64(pos < h.last[q]);
                any_ok |= okm;
                // lanes that do not blend carry alpha = 0 through the same arithmetic: every sum gets an exact 0 (exp2 of a skipped lane may be inf)
                const float araw_ok = __builtin_amdgcn_inverse_ballot_w64(okm) ? araw : 0.f;
                const float alpha = fminf(GSR_ALPHA_MAX, araw_ok);
                const float inv = __builtin_amdgcn_rcpf(1.f - alpha);
                const float Tk = Tr[q] * inv;                                        // transmittance in front of this splat
                // gD (v T_i - S / (1 - alpha)) + gA T_final / (1 - alpha) with T_i = Tr / (1 - alpha): one factor 1 / (1 - alpha).  The alpha
                // term is formed from T_final itself, not as 1 - (alpha composited behind): no cancellation where a pixel saturates
                const float dL_dalpha = (gD[q] * (r1.z * Tr[q] - S[q]) + gAT[q]) * inv;
                const float w = alpha * Tk;
                S[q] += r1.z * w;
                Tr[q] = Tk;
                s7 += w * gD[q];                                                     // dL/dv
                const float sg = araw_ok * dL_dalpha;                                // pre-cap alpha: the cap is straight-through
                s6 += sg;
                const float sx = sg * dx, sy = sg * dy;
                s1 += sx; s2 += sy;
                s3 += sx * dx; s4 += sx * dy; s5 += sy * dy;
            }
            if (any_ok == 0ull) continue;               // wave-uniform: no pixel of this wave blends the splat
            const float sums[DEPTH_NSUM] = {s1, s2, s3, s4, s5, s6, s7};
            const float sel = reduce_rows(red, red_rd, red_lane, lane, sums);
            if (slot >= 0) atomicAdd(a.acc + GSR_ACC_FLOATS * (size_t)row + slot, sel);
        }
    }
}

struct FinishArgs {
    int P, mode, accumulate;
    const float *means3D, *viewmatrix;
    const int *radii;
    const uint8_t *touched, *clamped;
    const uint32_t *touch_mark, *hot;
    const float *acc;
    StagedAdd add;               // out: the caller's buffers; accumulate: the per-Gaussian chain's result (t, staged in the workspace) is added to them
};

// One lane per Gaussian: dL/dmeans3D += dL/dv dv/dz (m[2], m[6], m[10]); with accumulate, out += staged result.  A Gaussian whose mark
// differs (or that was culled) has no gradient: pergauss_bwd wrote its zeros (accumulate = 0) or nothing is added (accumulate = 1).
__global__ __launch_bounds__(256) void depth_finish_kernel(FinishArgs f) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= f.P) return;
    const size_t si = (size_t)i;
    if (!(f.radii[si] > 0 && (uint32_t)f.touched[si] == *f.touch_mark)) return;
    float dv = f.acc[GSR_ACC_FLOATS * si + 9];
    if (f.clamped[si] & 0x80u) fold_replica_rows<9, false>(f.acc, f.P, f.hot[si], 0, nullptr, nullptr, true, dv);   // their slot 9 is folded in
    const float *m = f.viewmatrix;
    const float x = f.means3D[3 * si], y = f.means3D[3 * si + 1], z = f.means3D[3 * si + 2];
    const float zv = m[2] * x + m[6] * y + m[10] * z + m[14];
    const float g = f.mode == GSR_DEPTH_INVERSE ? -dv / (zv * zv) : dv;
    const float e0 = g * m[2], e1 = g * m[6], e2 = g * m[10];
    if (!f.accumulate) {
        float *const o = f.add.out.means3D;
        o[3 * si] += e0; o[3 * si + 1] += e1; o[3 * si + 2] += e2;
        return;
    }
    const float e[3] = {e0, e1, e2};
    add_staged(f.add, si, e);
}

// ---- host side ----
int32_t sizes_and_mode(const char *who, int P, int W, int H, long long R, int mode) {
    GSR_TRY(map_sizes(who, P, W, H, R));
    if (mode != GSR_DEPTH_EXPECTED && mode != GSR_DEPTH_INVERSE)
        return fail(GSR_ERR_INVALID_ARGUMENT, "%s: mode %d is neither 0 (expected depth) nor 1 (inverse depth)", who, mode);
    return GSR_OK;
}

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

int32_t gsr_depth_workspace_bytes(int32_t P, size_t *bytes) {
    if (P < 0 || !bytes) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_depth_workspace_bytes: bad argument");
    *bytes = carve_map_ws(nullptr, P, 0).total_bytes;
    return GSR_OK;
}

int32_t gsr_depth_forward(gsr_stream_t stream, int32_t P, int32_t W, int32_t H, int64_t R, int32_t mode,
                          const void *geom_ws, size_t geom_bytes, const void *binning_ws, size_t binning_bytes,
                          const void *img_ws, size_t img_bytes, float *out_depth, float *out_alpha) {
    hipStream_t s = (hipStream_t)stream;
    GSR_TRY(sizes_and_mode("gsr_depth_forward", P, W, H, (long long)R, mode));
    if (!out_depth && !out_alpha) return GSR_OK;
    if (P == 0 || R == 0) {
        const size_t n = (size_t)W * H * sizeof(float);
        if (out_depth) HIP_TRY(hipMemsetAsync(out_depth, 0, n, s), "clear depth map");
        if (out_alpha) HIP_TRY(hipMemsetAsync(out_alpha, 0, n, s), "clear alpha map");
        return GSR_OK;
    }
    if (!geom_ws || !binning_ws || !img_ws) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_depth_forward: missing workspace");
    Views v;
    GSR_TRY(view_all(v, P, W, H, (long long)R, {geom_ws, geom_bytes, binning_ws, binning_bytes, img_ws, img_bytes}));
    DepthArgs a = walk_args<DepthArgs>(v, P, W, H, (long long)R);
    a.mode = mode; a.out_depth = out_depth; a.out_alpha = out_alpha;
    hipLaunchKernelGGL(depth_fwd_kernel, dim3(walk_blocks(a)), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError(), "depth forward launch");
    return GSR_OK;
}

int32_t gsr_depth_backward(gsr_stream_t stream, int32_t P, int32_t W, int32_t H, int64_t R, int32_t mode,
                           const float *means3D, const int32_t *radii, const float *scales, float scale_modifier, const float *rotations,
                           const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix, const float *campos,
                           float tanfovx, float tanfovy, const float *dL_ddepth, const float *dL_dalpha,
                           const void *geom_ws, size_t geom_bytes, const void *binning_ws, size_t binning_bytes,
                           const void *img_ws, size_t img_bytes, void *ws, size_t ws_bytes, int32_t accumulate,
                           float *dL_dmeans2D, float *dL_dopacity, float *dL_dmeans3D, float *dL_dcov3D, float *dL_dscales, float *dL_drots) {
    const char *who = "gsr_depth_backward";
    hipStream_t s = (hipStream_t)stream;
    GSR_TRY(sizes_and_mode(who, P, W, H, (long long)R, mode));
    if (!dL_ddepth && !dL_dalpha) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: dL_ddepth and dL_dalpha are both NULL", who);
    if (P == 0) return GSR_OK;
    ReverseCall c = {who, P, W, H, (long long)R, means3D, radii, scales, scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, campos,
                     tanfovx, tanfovy, {geom_ws, geom_bytes, binning_ws, binning_bytes, img_ws, img_bytes}, ws, ws_bytes, accumulate,
                     {dL_dmeans2D, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dscales, dL_drots}};
    MapWs dw;
    GSR_TRY(reverse_prologue(c, true, "depth", 0, &dw));
    if (R == 0) return clear_gradients(c, nullptr, 0, s);
    Views v;
    GSR_TRY(view_all(v, P, W, H, c.R, c.fws));

    // 1. clear the rows that can be added into; 2. the reverse walk
    HIP_TRY(launch_zero_marked_rows(P, v.g.touched, v.g.touch_mark, dw.acc, acc_rows(P), v.im.seg, 0, 0, s), "zero depth accumulators");
    DepthArgs a = walk_args<DepthArgs>(v, P, W, H, c.R);
    a.mode = mode; a.gD = dL_ddepth; a.gA = dL_dalpha; a.acc = dw.acc; a.acc_rows = acc_rows(P);
    hipLaunchKernelGGL(depth_bwd_kernel, dim3(walk_blocks(a)), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError(), "depth backward launch");

    // 3. the per-Gaussian chain on these rows
    GSR_TRY(launch_chain(c, v, dw, s));

    // 4. dL/dv -> dL/dmeans3D, and the accumulation
    FinishArgs f;
    memset(&f, 0, sizeof f);
    f.P = P; f.mode = mode; f.accumulate = accumulate ? 1 : 0; f.means3D = means3D; f.viewmatrix = viewmatrix; f.radii = radii;
    f.touched = v.g.touched; f.clamped = v.g.clamped; f.touch_mark = v.g.touch_mark; f.hot = v.g.hot; f.acc = dw.acc;
    f.add = {dw.staged, c.out};
    hipLaunchKernelGGL(depth_finish_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, f);
    HIP_TRY(hipGetLastError(), "depth finish launch");
    return GSR_OK;
}

}  // extern "C"
