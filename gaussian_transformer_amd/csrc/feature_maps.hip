// feature_maps.hip -- N-channel feature maps of a render, with gradients (include/gsr_features.h): kernels and entry points.
//
// depth_maps.hip with a C-vector per Gaussian in place of a scalar: both walks re-read what gsr_forward left on the device (lists,
// records, reachability bytes, final_T, n_contrib), so no per-Gaussian stage and no list build runs again, and the colour path is not
// touched.  The decomposition is depth_maps.hip's: a wave64 owns the two 8x8 blocks of one half tile, lane l holds pixel l of each
// block, the list is staged 64 entries at a time into the wave's own LDS slice, the wave walks the ballot of reachable entries and
// never meets a workgroup barrier.  New here:
//   channels:  C is cut into chunks of CH = 4, 8 or 16 channels (the smallest that holds C, else 16), and chunk k is blockIdx.y = k: a
//              wave walks its half tile for ONE chunk, with 2 CH registers of accumulators (forward) or of upstream gradients
//              (reverse).  Every quantity the chunks share is linear in the chunk's part of u_i = sum_c G[c] F[g(i), c] -- the suffix
//              S_i, dL/dalpha_i and with it the six moments -- so each chunk adds its partial moments into the same accumulator row;
//              no wave ever needs the whole of u_i, and the serial chain per splat visit does not grow with C.  The chunks of one
//              half tile run side by side (C = 64: four walks across the grid), each re-deriving alpha from the same expressions.
//   staging:   the CH features of a staged entry go into LDS beside its record, as CH / 4 float4 planes [plane][entry]: lane e writes
//              entry e (conflict-free), the walk reads entry j in every lane (one address: a broadcast read).
//   forward:   acc[c] += F[c] alpha T, the colour pass's decisions from the colour pass's expressions; no atomics, bit-identical
//              from run to run.
//   reverse:   depth_bwd_kernel's recurrence with v = u (the form that does not cancel where a pixel saturates).  Two reductions
//              per (wave, entry) through composite_common.h's reduce_rows: the six moments (slots 3..8 of the accumulator row, ONE
//              6-lane atomic) and, only when dL/dF is wanted, the CH sums  sum_pixel G[c] alpha T  (ONE CH-lane atomic into CH
//              contiguous floats of the entry's row in a [rows][C] buffer of the workspace, replica rows included).
// pergauss_bwd.hip's streaming kernel then runs unchanged on the accumulator rows; features_df_kernel folds the replica rows and
// writes dL/dF [P,C] in full, features_add_kernel adds the staged per-Gaussian result with accumulate.
// Shared with depth_maps.hip, one copy each in map_walk.h: the leading argument fields, the half tile's geometry, the record gather
// behind the range check on the id, the add of the staged result, and on the host the views, the sizes refusal, the workspace carve and
// the reverse call's common refusals, R == 0 clearing and per-Gaussian launch.  The walk loops are this file's own (map_walk.h says
// why).  With the colour passes it shares what depth_maps.hip shares with them (composite_common.h), and no more.
#include <string.h>

#include "../../include/gsr_features.h"
#include "map_walk.h"
#include "pergauss_chain.h"

namespace gsr {
namespace {

#define FEAT_NMOM 6                                     // s dx, s dy, s dx dx, s dx dy, s dy dy, s -> row slots 3..8

struct FeatArgs : WalkArgs {     // C: channels; acc_rows: rows of acc and of dfacc
    const float *features;       // [P][C]
    float *out;                  // forward: [C][H][W]
    const float *G;              // reverse: dL_dout [C][H][W]
    float *acc;                  // [acc_rows][GSR_ACC_FLOATS]
    float *dfacc;                // [acc_rows][C]
};

// stages entry base + lane of the tile's list: (px, py, a, b) (c, opacity, -, bits | row << 4) and its CH features from channel c0 on
// (zeros from channel C on); returns whether the entry reaches a block
template <int CH>
__device__ __forceinline__ bool stage_entry(const FeatArgs &a, const HalfTile &h, float4 *my, float4 *ft, const int tile, const int sub,
                                            const int base, const int cnt, const int lane, const int c0, const bool want_row) {
    Entry e;
    if (!gather_entry(a, h, tile, sub, base, cnt, lane, want_row, e)) return false;
    my[lane] = e.s0;
    my[64 + lane] = make_float4(e.s1.x, e.s1.y, 0.f, entry_code(e));
    const float *fr = a.features + (size_t)e.g * a.C;
#pragma unroll
    for (int k = 0; k < CH / 4; k++) {
        const int c = c0 + 4 * k;
        ft[64 * k + lane] = make_float4(c < a.C ? fr[c] : 0.f, c + 1 < a.C ? fr[c + 1] : 0.f, c + 2 < a.C ? fr[c + 2] : 0.f,
                                        c + 3 < a.C ? fr[c + 3] : 0.f);
    }
    return e.bits != 0u;
}

template <int CH>
__device__ __forceinline__ void read_features(const float4 *ft, const int j, float (&f)[CH]) {
#pragma unroll
    for (int k = 0; k < CH / 4; k++) {
        const float4 v = ft[64 * k + j];                         // one address in every lane
        f[4 * k] = v.x; f[4 * k + 1] = v.y; f[4 * k + 2] = v.z; f[4 * k + 3] = v.w;
    }
}

template <int CH>
__global__ __launch_bounds__(256) void features_fwd_kernel(FeatArgs a) {
    __shared__ __align__(16) float4 stage[4][128 + 16 * CH];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int unit = blockIdx.x * 4 + wave, tile = unit >> 1, sub = unit & 1;
    if (tile >= a.gridx * a.gridy) return;              // wave-uniform
    const int c0 = blockIdx.y * CH;
    float4 *my = stage[wave], *ft = my + 128;
    const HalfTile h = half_tile(a, tile, sub, lane);
    float Tr[2] = {1.f, 1.f}, acc[2][CH];
#pragma unroll
    for (int k = 0; k < CH; k++) acc[0][k] = acc[1][k] = 0.f;
    for (int base = 0; base < h.hi; base += 64) {
        const int cnt = min(64, h.hi - base);
        __builtin_amdgcn_wave_barrier();
        const bool live = stage_entry<CH>(a, h, my, ft, tile, sub, base, cnt, lane, c0, false);
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
            float f[CH];
            read_features<CH>(ft, j, f);
#pragma unroll
            for (int q = 0; q < 2; q++) {
                if (!(bits & (1u << q)) || pos >= h.blk_last[q]) continue;          // scalar branch
                float araw;                                                          // the one evaluation every pass shares (gsr_device.h)
                const unsigned long long okm = splat_alpha(splat_power_log2_row(kc, rt, r0.x - h.fx[q]), r1.y, araw) &
                                               __builtin_amdgcn_ballot_w64(pos < h.last[q]);
                const float alpha = fminf(GSR_ALPHA_MAX, araw);
                const float aT = alpha * Tr[q];
                if (__builtin_amdgcn_inverse_ballot_w64(okm)) {
#pragma unroll
                    for (int k = 0; k < CH; k++) acc[q][k] += f[k] * aT;
                    Tr[q] = Tr[q] - aT;                                              // T (1 - alpha), the colour pass's form
                }
            }
        }
    }
    const size_t plane = (size_t)a.W * a.H;
#pragma unroll
    for (int q = 0; q < 2; q++) {
        if (!h.inside[q]) continue;
#pragma unroll
        for (int k = 0; k < CH; k++)
            if (c0 + k < a.C) a.out[(size_t)(c0 + k) * plane + h.pix[q]] = acc[q][k];
    }
}

template <int CH, bool WANT_DF>
__global__ __launch_bounds__(256) void features_bwd_kernel(FeatArgs a) {
    constexpr int NRED = WANT_DF && CH > FEAT_NMOM ? CH : FEAT_NMOM;
    __shared__ __align__(16) float4 stage[4][128 + 16 * CH + (NRED * RED_STRIDE + 3) / 4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int unit = blockIdx.x * 4 + wave, tile = unit >> 1, sub = unit & 1;
    if (tile >= a.gridx * a.gridy) return;              // wave-uniform
    const int c0 = blockIdx.y * CH;
    float4 *my = stage[wave], *ft = my + 128;
    float *red = reinterpret_cast<float *>(ft + 16 * CH);       // [value][lane], rows of RED_STRIDE floats; the two reductions take turns
    const HalfTile h = half_tile(a, tile, sub, lane);
    if (h.hi <= 0) return;
    // per pixel: Tr = transmittance behind the splats visited so far, S = sum of u alpha T over them, G = this chunk's upstream gradients
    const size_t plane = (size_t)a.W * a.H;
    float Tr[2], S[2] = {0.f, 0.f}, G[2][CH];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        Tr[q] = h.inside[q] ? a.final_T[h.pix[q]] : 1.f;
#pragma unroll
        for (int k = 0; k < CH; k++) G[q][k] = h.inside[q] && c0 + k < a.C ? a.G[(size_t)(c0 + k) * plane + h.pix[q]] : 0.f;
    }
    const float4 *mom_rd, *df_rd = nullptr;
    bool mom_lane, df_lane = false;
    const int mvalue = reduce_setup<FEAT_NMOM>(red, lane, mom_rd, mom_lane);
    const int slot = mvalue >= 0 ? 3 + mvalue : -1;
    int dchan = -1;                                     // the channel whose total this lane ends up holding
    if (WANT_DF) {
        const int dvalue = reduce_setup<CH>(red, lane, df_rd, df_lane);
        dchan = dvalue >= 0 && c0 + dvalue < a.C ? c0 + dvalue : -1;
    }

    for (int base = ((h.hi - 1) >> 6) << 6; base >= 0; base -= 64) {
        const int cnt = min(64, h.hi - base);
        __builtin_amdgcn_wave_barrier();
        const bool live = stage_entry<CH>(a, h, my, ft, tile, sub, base, cnt, lane, c0, true);
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
            float f[CH];
            read_features<CH>(ft, j, f);
            float s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f, s5 = 0.f, s6 = 0.f, d[CH];
#pragma unroll
            for (int k = 0; k < CH; k++) d[k] = 0.f;
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
                const float inv = __builtin_amdgcn_rcpf(1.f - alpha);                // (an IEEE division here moves no gradient closer to the oracle: measured)
                const float Tk = Tr[q] * inv;                                        // transmittance in front of this splat
                float u = 0.f;                                                      // this chunk's part of sum_c G[c] F[c]
#pragma unroll
                for (int k = 0; k < CH; k++) u += G[q][k] * f[k];
                // (u T_i - S / (1 - alpha)) with T_i = Tr / (1 - alpha): one factor 1 / (1 - alpha), no cancellation where a pixel saturates
                const float dL_dalpha = (u * Tr[q] - S[q]) * inv;
                const float w = alpha * Tk;
                S[q] += u * w;
                Tr[q] = Tk;
                if (WANT_DF) {
#pragma unroll
                    for (int k = 0; k < CH; k++) d[k] += G[q][k] * w;               // dL/dF[c]
                }
                const float sg = araw_ok * dL_dalpha;                                // pre-cap alpha: the cap is straight-through
                s6 += sg;
                const float sx = sg * dx, sy = sg * dy;
                s1 += sx; s2 += sy;
                s3 += sx * dx; s4 += sx * dy; s5 += sy * dy;
            }
            if (any_ok == 0ull) continue;               // wave-uniform: no pixel of this wave blends the splat
            const float sums[FEAT_NMOM] = {s1, s2, s3, s4, s5, s6};
            const float sel = reduce_rows(red, mom_rd, mom_lane, lane, sums);
            if (slot >= 0) atomicAdd(a.acc + GSR_ACC_FLOATS * (size_t)row + slot, sel);
            if (WANT_DF) {
                const float dsel = reduce_rows(red, df_rd, df_lane, lane, d);
                if (dchan >= 0) atomicAdd(a.dfacc + (size_t)row * a.C + dchan, dsel);
            }
        }
    }
}

// clears the rows of dfacc that can be added into: those of the Gaussians the forward pass marked, and the replica rows
// (launch_zero_marked_rows' rule); one thread per float
__global__ __launch_bounds__(256) void features_zero_kernel(int P, int C, const uint8_t *__restrict__ touched, const uint32_t *__restrict__ mark,
                                                            float *__restrict__ dfacc, size_t rows_total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows_total * (size_t)C) return;
    const size_t row = i / (size_t)C;
    if (row < (size_t)P && touched[row] != (uint8_t)*mark) return;
    dfacc[i] = 0.f;
}

// dL/dF [P,C], fully written: the Gaussian's own row plus its replica rows; an exact zero for a Gaussian without a gradient
__global__ __launch_bounds__(256) void features_df_kernel(int P, int C, const int *__restrict__ radii, const uint8_t *__restrict__ touched,
                                                          const uint8_t *__restrict__ clamped, const uint32_t *__restrict__ mark,
                                                          const uint32_t *__restrict__ hot, const float *__restrict__ dfacc, size_t rows_total,
                                                          float *__restrict__ dL_dfeatures) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)P * (size_t)C) return;
    const size_t g = i / (size_t)C, c = i - g * (size_t)C;
    float v = 0.f;
    if (radii[g] > 0 && (uint32_t)touched[g] == *mark) {
        v = dfacc[i];
        if (clamped[g] & 0x80u) {
            const uint32_t code = hot[g];
            const size_t first = (size_t)P + (code >> 4);
            for (uint32_t k = 0; k < (1u << (code & 15u)); k++) {
                if (first + k >= rows_total) break;     // a code can only name rows of the workspace
                v += dfacc[(first + k) * (size_t)C + c];
            }
        }
    }
    dL_dfeatures[i] = v;
}

struct AddArgs {
    int P;
    const int *radii;
    const uint8_t *touched;
    const uint32_t *touch_mark;
    StagedAdd add;
};

// accumulate: out += the per-Gaussian chain's result staged in the workspace, one lane per Gaussian.  A Gaussian whose mark differs
// (or that was culled) has no gradient: nothing is read or added
__global__ __launch_bounds__(256) void features_add_kernel(AddArgs f) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= f.P) return;
    const size_t si = (size_t)i;
    if (!(f.radii[si] > 0 && (uint32_t)f.touched[si] == *f.touch_mark)) return;
    add_staged(f.add, si, nullptr);
}

// ---- host side ----
int32_t sizes_and_channels(const char *who, int P, int C, int W, int H, long long R) {
    GSR_TRY(map_sizes(who, P, W, H, R));
    if (C < 1 || C > GSR_FEATURES_MAX_C) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: C = %d channels, must be 1 .. %d", who, C, GSR_FEATURES_MAX_C);
    return GSR_OK;
}

// the chunk a call's C is cut into, and the grid: x = half tiles / 4 (a wave each), y = chunks
inline int chunk_of(int C) { return C <= 4 ? 4 : (C <= 8 ? 8 : 16); }
inline dim3 walk_grid(const FeatArgs &a) {
    const int ch = chunk_of(a.C);
    return dim3(walk_blocks(a), (unsigned)((a.C + ch - 1) / ch));
}

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

int32_t gsr_features_workspace_bytes(int32_t P, int32_t C, size_t *bytes) {
    if (P < 0 || C < 1 || C > GSR_FEATURES_MAX_C || !bytes) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_features_workspace_bytes: bad argument");
    *bytes = carve_map_ws(nullptr, P, C).total_bytes;
    return GSR_OK;
}

int32_t gsr_features_forward(gsr_stream_t stream, int32_t P, int32_t C, int32_t W, int32_t H, int64_t R, const float *features,
                             const void *geom_ws, size_t geom_bytes, const void *binning_ws, size_t binning_bytes,
                             const void *img_ws, size_t img_bytes, float *out) {
    const char *who = "gsr_features_forward";
    hipStream_t s = (hipStream_t)stream;
    GSR_TRY(sizes_and_channels(who, P, C, W, H, (long long)R));
    if (!out) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: out is NULL", who);
    if (P == 0 || R == 0) {
        HIP_TRY(hipMemsetAsync(out, 0, (size_t)C * W * H * sizeof(float), s), "clear feature map");
        return GSR_OK;
    }
    if (!features || !geom_ws || !binning_ws || !img_ws) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: missing features or workspace", who);
    Views v;
    GSR_TRY(view_all(v, P, W, H, (long long)R, {geom_ws, geom_bytes, binning_ws, binning_bytes, img_ws, img_bytes}));
    FeatArgs a = walk_args<FeatArgs>(v, P, W, H, (long long)R);
    a.C = C; a.features = features; a.out = out;
    switch (chunk_of(C)) {
        case 4: hipLaunchKernelGGL(features_fwd_kernel<4>, walk_grid(a), dim3(256), 0, s, a); break;
        case 8: hipLaunchKernelGGL(features_fwd_kernel<8>, walk_grid(a), dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL(features_fwd_kernel<16>, walk_grid(a), dim3(256), 0, s, a); break;
    }
    HIP_TRY(hipGetLastError(), "features forward launch");
    return GSR_OK;
}

int32_t gsr_features_backward(gsr_stream_t stream, int32_t P, int32_t C, int32_t W, int32_t H, int64_t R,
                              const float *means3D, const int32_t *radii, const float *scales, float scale_modifier, const float *rotations,
                              const float *cov3D_precomp, const float *viewmatrix, const float *projmatrix, const float *campos,
                              float tanfovx, float tanfovy, const float *features, const float *dL_dout,
                              const void *geom_ws, size_t geom_bytes, const void *binning_ws, size_t binning_bytes,
                              const void *img_ws, size_t img_bytes, void *ws, size_t ws_bytes, int32_t accumulate,
                              float *dL_dmeans2D, float *dL_dopacity, float *dL_dmeans3D, float *dL_dcov3D, float *dL_dscales, float *dL_drots,
                              float *dL_dfeatures) {
    const char *who = "gsr_features_backward";
    hipStream_t s = (hipStream_t)stream;
    GSR_TRY(sizes_and_channels(who, P, C, W, H, (long long)R));
    if (!dL_dout) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: dL_dout is NULL", who);
    if (P == 0) return GSR_OK;
    ReverseCall c = {who, P, W, H, (long long)R, means3D, radii, scales, scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, campos,
                     tanfovx, tanfovy, {geom_ws, geom_bytes, binning_ws, binning_bytes, img_ws, img_bytes}, ws, ws_bytes, accumulate,
                     {dL_dmeans2D, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dscales, dL_drots}};
    MapWs fw;
    GSR_TRY(reverse_prologue(c, features != nullptr, "features", C, &fw));
    if (R == 0) return clear_gradients(c, dL_dfeatures, C, s);
    Views v;
    GSR_TRY(view_all(v, P, W, H, c.R, c.fws));

    // 1. clear the rows that can be added into; 2. the reverse walk, one wave per (half tile, chunk)
    const size_t rows = acc_rows(P), cells = rows * (size_t)C;
    HIP_TRY(launch_zero_marked_rows(P, v.g.touched, v.g.touch_mark, fw.acc, rows, v.im.seg, 0, 0, s), "zero feature accumulators");
    if (dL_dfeatures) {
        hipLaunchKernelGGL(features_zero_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, P, C, v.g.touched, v.g.touch_mark, fw.dfacc, rows);
        HIP_TRY(hipGetLastError(), "zero dL/dF rows");
    }
    FeatArgs a = walk_args<FeatArgs>(v, P, W, H, c.R);
    a.C = C; a.features = features; a.G = dL_dout; a.acc = fw.acc; a.dfacc = fw.dfacc; a.acc_rows = rows;
#define LAUNCH_BWD(CH) \
    if (dL_dfeatures) hipLaunchKernelGGL((features_bwd_kernel<CH, true>), walk_grid(a), dim3(256), 0, s, a); \
    else hipLaunchKernelGGL((features_bwd_kernel<CH, false>), walk_grid(a), dim3(256), 0, s, a)
    switch (chunk_of(C)) {
        case 4: LAUNCH_BWD(4); break;
        case 8: LAUNCH_BWD(8); break;
        default: LAUNCH_BWD(16); break;
    }
#undef LAUNCH_BWD
    HIP_TRY(hipGetLastError(), "features backward launch");

    // 3. the per-Gaussian chain on these rows
    GSR_TRY(launch_chain(c, v, fw, s));

    // 4. dL/dF: replica rows folded, [P,C] written in full; 5. the accumulation
    if (dL_dfeatures) {
        const size_t n = (size_t)P * (size_t)C;
        hipLaunchKernelGGL(features_df_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, P, C, radii, v.g.touched, v.g.clamped, v.g.touch_mark,
                           v.g.hot, fw.dfacc, rows, dL_dfeatures);
        HIP_TRY(hipGetLastError(), "dL/dF finish launch");
    }
    if (accumulate) {
        AddArgs f;
        memset(&f, 0, sizeof f);
        f.P = P; f.radii = radii; f.touched = v.g.touched; f.touch_mark = v.g.touch_mark; f.add = {fw.staged, c.out};
        hipLaunchKernelGGL(features_add_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, f);
        HIP_TRY(hipGetLastError(), "features accumulate launch");
    }
    return GSR_OK;
}

}  // extern "C"
