// absgrad.hip -- per-Gaussian sums of |dL/dmeans2D| over the pixels of a render (include/gsr_absgrad.h): kernels and entry points.
//
// Built beside the colour path, which it does not touch, from map_walk.h's pieces: a reverse walk of its own over what gsr_forward
// left on the device (lists, records, reachability bytes, final_T, n_contrib), run after -- or without -- gsr_backward.  The shape is
// depth_bwd_kernel's (depth_maps.hip): a wave64 owns the two 8x8 blocks of one half tile, lane l holds pixel l of each block, the list
// is staged 64 entries at a time into the wave's own LDS slice, the wave walks the ballot of reachable entries back to front with
// scalar branches on the reachability bits and never meets a workgroup barrier.  The recurrence is that kernel's with
//   v = u_i = sum_ch gC[ch] rgb_i[ch],  gD = 1,  gA = -sum_ch gC[ch] bg[ch]:
//   dL/dalpha_i = ((u_i Tr - S) + gA T_final) / (1 - alpha_i),   Tr = T_i (1 - alpha_i),  S = sum_{j behind i} u_j alpha_j T_j,
// the form that does not cancel where a pixel saturates.  gC is fixed per pixel, so the upstream gradient is three registers per pixel
// and block and the suffix S one scalar per pixel.
// Staged per entry, three float4 planes: (px, py, A, B) (C, opacity, r, bits | row << 4) (g, b, -, -).  The conic is staged RAW, since
// the per-pixel terms need it, and the exponent's form (-0.5 log2e A, ..) is made from it per visit by gsr_device.h's stage_conic: the
// bits composite_common.h's stage_record makes, hence the colour pass's decisions.
// Per (entry, pixel) the terms  t_x = s (A dx + B dy),  t_y = s (B dx + C dy),  s = opacity G dL/dalpha (the alpha before the cap,
// straight-through) are formed and their ABSOLUTE VALUES summed per lane over the two blocks -- before any reduction: the absolute value
// of a wave's or a tile's sum is another quantity.  The two sums (four in the instantiation that also wants the signed ones, which the
// other does not pay for) go through composite_common.h's reduce_rows and leave as ONE 2-lane (4-lane) global_atomic_add_f32 per
// (wave, entry) into the entry's row of a [acc_rows(P)][2] buffer of the workspace, only when some lane blended.  A splat with replica
// rows adds into replica (tile mod K), as in the reverse map walks.  No per-Gaussian chain runs: the factors that are constant per
// Gaussian, -0.5 W and -0.5 H, are applied by the finishing kernel, which also folds the replica rows and writes or adds [P,2].
// Zeroing: only the rows that can be added into (marked Gaussians + replica rows), by features_zero_kernel's rule.
// The walk loop is this file's own (map_walk.h says why the walks are not a template over callables).
#include <string.h>

#include "../../include/gsr_absgrad.h"
#include "map_walk.h"

namespace gsr {
namespace {

struct AbsArgs : WalkArgs {                          // mode: unused; acc_rows: rows of absacc and of sgnacc
    const float *bg;                                 // [3]
    const float *gC;                                 // dL_dcolor [3][H][W]
    float *absacc, *sgnacc;                          // [acc_rows][2] each: sums of |s (..)| and of s (..), unscaled
};

// stages entry base + lane of the tile's list; returns whether the entry reaches a block
__device__ __forceinline__ bool stage_entry(const AbsArgs &a, const HalfTile &h, float4 *my, const int tile, const int sub, const int base,
                                            const int cnt, const int lane) {
    Entry e;
    if (!gather_entry(a, h, tile, sub, base, cnt, lane, true, e)) return false;
    const float4 *rec4 = reinterpret_cast<const float4 *>(a.rec) + 3 * (size_t)e.g;       // the conic as stored (e.g < P: gather_entry checked)
    const float4 r0 = rec4[0], r1 = rec4[1];
    my[lane] = make_float4(r0.x, r0.y, r0.z, r0.w);
    my[64 + lane] = make_float4(r1.x, r1.y, r1.z, entry_code(e));
    my[128 + lane] = make_float4(r1.w, e.r2.x, 0.f, 0.f);
    return e.bits != 0u;
}

template <bool SIGNED>
__global__ __launch_bounds__(256) void absgrad_walk_kernel(AbsArgs a) {
    constexpr int NSUM = SIGNED ? 4 : 2;                // |t_x|, |t_y| (, t_x, t_y)
    __shared__ __align__(16) float4 stage[4][192 + (NSUM * RED_STRIDE + 3) / 4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int unit = blockIdx.x * 4 + wave, tile = unit >> 1, sub = unit & 1;
    if (tile >= a.gridx * a.gridy) return;              // wave-uniform
    float4 *my = stage[wave];
    float *red = reinterpret_cast<float *>(my + 192);   // [value][lane], rows of RED_STRIDE floats
    const HalfTile h = half_tile(a, tile, sub, lane);
    if (h.hi <= 0) return;
    // per pixel: Tr = transmittance behind the splats visited so far, S = sum of u alpha T over them, G = dL/dcolor,
    // gAT = -(sum_ch G[ch] bg[ch]) T_final
    const size_t plane = (size_t)a.W * a.H;
    const float bg0 = a.bg[0], bg1 = a.bg[1], bg2 = a.bg[2];
    float Tr[2], S[2] = {0.f, 0.f}, G[2][3], gAT[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        Tr[q] = h.inside[q] ? a.final_T[h.pix[q]] : 1.f;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) G[q][ch] = h.inside[q] ? a.gC[(size_t)ch * plane + h.pix[q]] : 0.f;
        gAT[q] = -(G[q][0] * bg0 + G[q][1] * bg1 + G[q][2] * bg2) * Tr[q];
    }
    // lane 4 value + part adds red[value][16 part .. 16 part + 15]; two DPP steps fold the four parts; lanes 0, 4 (, 8, 12) hold the totals
    const float4 *red_rd;
    bool red_lane;
    const int rvalue = reduce_setup<NSUM>(red, lane, red_rd, red_lane);
    float *const dst = rvalue < 0 ? nullptr : (rvalue < 2 ? a.absacc + rvalue : a.sgnacc + (rvalue - 2));

    for (int base = ((h.hi - 1) >> 6) << 6; base >= 0; base -= 64) {
        const int cnt = min(64, h.hi - base);
        __builtin_amdgcn_wave_barrier();
        const bool live = stage_entry(a, h, my, tile, sub, base, cnt, lane);
        uint64_t todo = __ballot(live);
        __builtin_amdgcn_wave_barrier();
        while (todo) {
            const int j = 63 - __builtin_clzll(todo);   // back to front
            todo &= ~(1ull << j);
            const float4 r0 = my[j], r1 = my[64 + j], r2 = my[128 + j];
            const uint32_t code = __builtin_amdgcn_readfirstlane(__float_as_uint(r1.w));
            const uint32_t bits = code & 3u, row = code >> 4;
            const int pos = base + j;
            const float cA = r0.z, cB = r0.w, cC = r1.x;
            const StagedConic kc = stage_conic(cA, cB, cC);
            const float dy = r0.y - h.fy;
            const RowTerms rt = splat_row_terms(kc, dy);
            const float By = cB * dy, Cy = cC * dy;
            float ax = 0.f, ay = 0.f, sx = 0.f, sy = 0.f;
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
                const float u = G[q][0] * r1.z + G[q][1] * r2.x + G[q][2] * r2.y;
                // ((u T_i - S / (1 - alpha)) + gA T_final / (1 - alpha)) with T_i = Tr / (1 - alpha): one factor 1 / (1 - alpha), no
                // cancellation where a pixel saturates (depth_maps.hip)
                const float dL_dalpha = ((u * Tr[q] - S[q]) + gAT[q]) * inv;
                S[q] += u * (alpha * Tk);
                Tr[q] = Tk;
                const float sg = araw_ok * dL_dalpha;                                // pre-cap alpha: the cap is straight-through
                const float tx = sg * (cA * dx + By), ty = sg * (cB * dx + Cy);
                ax += fabsf(tx); ay += fabsf(ty);                                    // per (pixel, Gaussian) pair, before any sum
                if (SIGNED) { sx += tx; sy += ty; }
            }
            if (any_ok == 0ull) continue;               // wave-uniform: no pixel of this wave blends the splat
            float sel;
            if (SIGNED) {
                const float sums[4] = {ax, ay, sx, sy};
                sel = reduce_rows(red, red_rd, red_lane, lane, sums);
            } else {
                const float sums[2] = {ax, ay};
                sel = reduce_rows(red, red_rd, red_lane, lane, sums);
            }
            if (dst) atomicAdd(dst + 2 * (size_t)row, sel);
        }
    }
}

// clears the rows that can be added into: those of the Gaussians the forward pass marked, and the replica rows (features_zero_kernel's
// rule); one thread per float of a row pair, both buffers when the signed sums are wanted
__global__ __launch_bounds__(256) void absgrad_zero_kernel(int P, const uint8_t *__restrict__ touched, const uint32_t *__restrict__ mark,
                                                           float *__restrict__ absacc, float *__restrict__ sgnacc, size_t rows_total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows_total * 2) return;
    const size_t row = i >> 1;
    if (row < (size_t)P && touched[row] != (uint8_t)*mark) return;
    absacc[i] = 0.f;
    if (sgnacc) sgnacc[i] = 0.f;
}

struct FinishArgs {
    int P, accumulate;
    float kx, ky;                // 0.5 W, 0.5 H
    const uint32_t *tiles;
    const uint8_t *touched, *clamped;
    const uint32_t *touch_mark, *hot;
    const float *absacc, *sgnacc;
    size_t rows_total;
    float *absgrad, *signed_sum; // [P,2]; signed_sum may be NULL
};

// a Gaussian's own row plus its replica rows (rows at or beyond rows_total are not read: a code can only name rows of the workspace)
__device__ __forceinline__ float2 folded_row(const float *acc, const FinishArgs &f, size_t si, bool replicas) {
    float2 v = reinterpret_cast<const float2 *>(acc)[si];
    if (replicas) {
        const uint32_t code = f.hot[si];
        const size_t first = (size_t)f.P + (code >> 4);
        for (uint32_t k = 0; k < (1u << (code & 15u)); k++) {
            if (first + k >= f.rows_total) break;
            const float2 r = reinterpret_cast<const float2 *>(acc)[first + k];
            v.x += r.x; v.y += r.y;
        }
    }
    return v;
}

// One lane per Gaussian.  A Gaussian that emitted no pair or whose mark differs has no gradient: an exact +0.0 (accumulate = 0) or
// nothing read or written (accumulate = 1)
__global__ __launch_bounds__(256) void absgrad_finish_kernel(FinishArgs f) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= f.P) return;
    const size_t si = (size_t)i;
    const bool has = f.tiles[si] > 0u && (uint32_t)f.touched[si] == *f.touch_mark;
    if (!has && f.accumulate) return;
    float2 av = make_float2(0.f, 0.f), sv = make_float2(0.f, 0.f);
    if (has) {
        const bool replicas = (f.clamped[si] & 0x80u) != 0u;
        av = folded_row(f.absacc, f, si, replicas);
        av.x *= f.kx; av.y *= f.ky;
        if (f.signed_sum) {
            sv = folded_row(f.sgnacc, f, si, replicas);
            sv.x = 0.f - sv.x * f.kx; sv.y = 0.f - sv.y * f.ky;      // (a row nothing was added into stays +0.0)
        }
    }
    float2 *const oa = reinterpret_cast<float2 *>(f.absgrad) + si;
    float2 *const os = f.signed_sum ? reinterpret_cast<float2 *>(f.signed_sum) + si : nullptr;
    if (f.accumulate) {
        const float2 a0 = *oa;
        *oa = make_float2(a0.x + av.x, a0.y + av.y);
        if (os) {
            const float2 s0 = *os;
            *os = make_float2(s0.x + sv.x, s0.y + sv.y);
        }
    } else {
        *oa = av;
        if (os) *os = sv;
    }
}

struct AbsWs { float *absacc, *sgnacc; size_t total_bytes; };
AbsWs carve_abs_ws(void *ws, int P) {
    Bump w = {(char *)ws, 0};
    float *const a = w.take<float>(2 * acc_rows(P));
    float *const s = w.take<float>(2 * acc_rows(P));
    return {a, s, w.off};
}

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

int32_t gsr_absgrad_workspace_bytes(int32_t P, size_t *bytes) {
    if (P < 0 || !bytes) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_absgrad_workspace_bytes: bad argument");
    *bytes = carve_abs_ws(nullptr, P).total_bytes;
    return GSR_OK;
}

int32_t gsr_absgrad_backward(gsr_stream_t stream, int32_t P, int32_t W, int32_t H, int64_t R, const float *bg, const float *dL_dcolor,
                             const void *geom_ws, size_t geom_bytes, const void *binning_ws, size_t binning_bytes,
                             const void *img_ws, size_t img_bytes, void *ws, size_t ws_bytes, int32_t accumulate,
                             float *absgrad, float *signed_sum) {
    const char *who = "gsr_absgrad_backward";
    hipStream_t s = (hipStream_t)stream;
    GSR_TRY(map_sizes(who, P, W, H, (long long)R));
    if (P == 0) return GSR_OK;
    if (!bg || !dL_dcolor || !geom_ws || !img_ws || !ws || !absgrad)
        return fail(GSR_ERR_INVALID_ARGUMENT, "%s: missing input, workspace or output buffer", who);
    if (R > 0 && !binning_ws) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: binning workspace missing", who);
    int32_t det = 0;
    GSR_TRY(gsr_get_option("deterministic_bwd", &det));
    if (det) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: not available while the option deterministic_bwd is on (this pass sums with float atomics and has no slot form)", who);
    const AbsWs aw = carve_abs_ws(ws, P);
    if (ws_bytes < aw.total_bytes) return fail(GSR_ERR_WORKSPACE, "absgrad workspace %zu < %zu", ws_bytes, aw.total_bytes);
    const size_t rows = acc_rows(P);
    if (rows >= (1u << 28)) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: P too large for the 28-bit accumulator row index", who);
    if (R == 0) {                                       // nothing was composited: every sum is zero
        if (accumulate) return GSR_OK;
        HIP_TRY(hipMemsetAsync(absgrad, 0, 2 * (size_t)P * sizeof(float), s), "clear absgrad");
        if (signed_sum) HIP_TRY(hipMemsetAsync(signed_sum, 0, 2 * (size_t)P * sizeof(float), s), "clear signed sums");
        return GSR_OK;
    }
    Views v;
    GSR_TRY(view_all(v, P, W, H, (long long)R, {geom_ws, geom_bytes, binning_ws, binning_bytes, img_ws, img_bytes}));

    // 1. clear the rows that can be added into; 2. the reverse walk; 3. fold, scale, write or add
    hipLaunchKernelGGL(absgrad_zero_kernel, dim3((unsigned)((2 * rows + 255) / 256)), dim3(256), 0, s, P, v.g.touched, v.g.touch_mark, aw.absacc,
                       signed_sum ? aw.sgnacc : nullptr, rows);
    HIP_TRY(hipGetLastError(), "zero absgrad rows");
    AbsArgs a = walk_args<AbsArgs>(v, P, W, H, (long long)R);
    a.bg = bg; a.gC = dL_dcolor; a.absacc = aw.absacc; a.sgnacc = aw.sgnacc; a.acc_rows = rows;
    if (signed_sum) hipLaunchKernelGGL(absgrad_walk_kernel<true>, dim3(walk_blocks(a)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(absgrad_walk_kernel<false>, dim3(walk_blocks(a)), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError(), "absgrad walk launch");

    FinishArgs f;
    memset(&f, 0, sizeof f);
    f.P = P; f.accumulate = accumulate ? 1 : 0; f.kx = 0.5f * (float)W; f.ky = 0.5f * (float)H;
    f.tiles = v.g.tiles; f.touched = v.g.touched; f.clamped = v.g.clamped; f.touch_mark = v.g.touch_mark; f.hot = v.g.hot;
    f.absacc = aw.absacc; f.sgnacc = aw.sgnacc; f.rows_total = rows; f.absgrad = absgrad; f.signed_sum = signed_sum;
    hipLaunchKernelGGL(absgrad_finish_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, f);
    HIP_TRY(hipGetLastError(), "absgrad finish launch");
    return GSR_OK;
}

}  // extern "C"
