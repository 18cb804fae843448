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
// Kept here as copies of depth_maps.hip's lines and not shared with it: the half tile's geometry and the record gather -- that file's
// two kernels come out in another instruction order through shared helpers (its header; scripts/isa_diff.py), and they stay as they are.
#include <string.h>

#include "../../include/gsr_features.h"
#include "composite_common.h"
#include "gsr_host.h"
#include "gsr_internal.h"
#include "pergauss_chain.h"

namespace gsr {
namespace {

#define FEAT_NMOM 6                                     // s dx, s dy, s dx dx, s dx dy, s dy dy, s -> row slots 3..8

struct FeatArgs {
    int W, H, gridx, gridy, P, C;
    size_t list_len;             // R: entries of point_list, stride of contrib
    size_t acc_rows;             // rows of acc and of dfacc (reverse pass)
    const uint8_t *contrib;      // [4][list_len]
    const uint2 *ranges;
    const uint32_t *point_list;
    const float *rec;
    const float *final_T;
    const uint32_t *n_contrib;
    const float *features;       // [P][C]
    float *out;                  // forward: [C][H][W]
    const float *G;              // reverse: dL_dout [C][H][W]
    float *acc;                  // [acc_rows][GSR_ACC_FLOATS]
    float *dfacc;                // [acc_rows][C]
};

// what a wave knows of its half tile before it walks (depth_maps.hip's HalfTile)
struct HalfTile {
    float fx[2], fy;
    bool inside[2];
    size_t pix[2];
    int last[2], blk_last[2], hi;
    uint2 range;
};
__device__ __forceinline__ HalfTile half_tile(const FeatArgs &a, const int tile, const int sub, const int lane) {
    HalfTile h;
    const int tx = tile % a.gridx, ty = tile / a.gridx;
    h.range = a.ranges[tile];
    const int y = ty * GSR_TILE + sub * 8 + (lane >> 3);
    h.fy = (float)y;
    int hi = 0;
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int x = tx * GSR_TILE + q * 8 + (lane & 7);
        h.inside[q] = x < a.W && y < a.H;
        h.pix[q] = (size_t)(h.inside[q] ? y : 0) * a.W + (h.inside[q] ? x : 0);
        h.fx[q] = (float)x;
        h.last[q] = h.inside[q] ? (int)a.n_contrib[h.pix[q]] : 0;
        int m = h.last[q];
        GSR_WAVE_MAX_I32(m);
        h.blk_last[q] = __builtin_amdgcn_readfirstlane(m);
        hi = max(hi, h.blk_last[q]);
    }
    const long long n = (long long)h.range.y - (long long)h.range.x;
    h.hi = (int)min((long long)hi, max(n, 0ll));      // a garbage n_contrib cannot send the walk past the tile's range
    return h;
}

// stages entry base + lane of the tile's list: (px, py, a, b) (c, opacity, -, bits | row << 4) and its CH features from channel c0 on
// (zeros from channel C on); returns whether the entry reaches a block
template <int CH>
__device__ __forceinline__ bool stage_entry(const FeatArgs &a, const HalfTile &h, float4 *my, float4 *ft, const int tile, const int sub,
                                            const int base, const int cnt, const int lane, const int c0, const bool want_row) {
    if (lane >= cnt) return false;
    const size_t at = (size_t)h.range.x + base + lane;
    if (at >= a.list_len) return false;
    const uint32_t g = a.point_list[at];
    if (g >= (uint32_t)a.P) return false;
    const float4 *rec4 = reinterpret_cast<const float4 *>(a.rec) + 3 * (size_t)g;
    const float4 r0 = rec4[0], r1 = rec4[1], r2 = rec4[2];
    uint32_t bits = 0u;
#pragma unroll
    for (int q = 0; q < 2; q++) bits |= a.contrib[(size_t)(sub * 2 + q) * a.list_len + at] ? (1u << q) : 0u;
    uint32_t row = g;
    if (want_row) {
        row = replica_row(__float_as_uint(r2.w), g, a.P, tile);
        if ((size_t)row >= a.acc_rows) return false;
    }
    float4 s0, s1;
    stage_record(r0, r1, s0, s1);                                // as the colour pass stages it
    my[lane] = s0;
    my[64 + lane] = make_float4(s1.x, s1.y, 0.f, __uint_as_float(bits | (row << 4)));      // row < 2^28 (checked by the entry point)
    const float *fr = a.features + (size_t)g * a.C;
#pragma unroll
    for (int k = 0; k < CH / 4; k++) {
        const int c = c0 + 4 * k;
        ft[64 * k + lane] = make_float4(c < a.C ? fr[c] : 0.f, c + 1 < a.C ? fr[c + 1] : 0.f, c + 2 < a.C ? fr[c + 2] : 0.f,
                                        c + 3 < a.C ? fr[c + 3] : 0.f);
    }
    return bits != 0u;
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
    const float *t_means2D, *t_opacity, *t_means3D, *t_cov3D, *t_scales, *t_rots;
    float *dL_dmeans2D, *dL_dopacity, *dL_dmeans3D, *dL_dcov3D, *dL_dscales, *dL_drots;
};

// accumulate: out += the per-Gaussian chain's result staged in the workspace, one lane per Gaussian.  A Gaussian whose mark differs
// (or that was culled) has no gradient: nothing is read or added
__global__ __launch_bounds__(256) void features_add_kernel(AddArgs f) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= f.P) return;
    const size_t si = (size_t)i;
    if (!(f.radii[si] > 0 && (uint32_t)f.touched[si] == *f.touch_mark)) return;
#pragma unroll
    for (int k = 0; k < 3; k++) f.dL_dmeans3D[3 * si + k] += f.t_means3D[3 * si + k];
    f.dL_dmeans2D[3 * si] += f.t_means2D[3 * si]; f.dL_dmeans2D[3 * si + 1] += f.t_means2D[3 * si + 1];
    f.dL_dopacity[si] += f.t_opacity[si];
    if (f.dL_dcov3D) {
#pragma unroll
        for (int k = 0; k < 6; k++) f.dL_dcov3D[6 * si + k] += f.t_cov3D[6 * si + k];
    }
    if (f.dL_dscales) {
#pragma unroll
        for (int k = 0; k < 3; k++) f.dL_dscales[3 * si + k] += f.t_scales[3 * si + k];
#pragma unroll
        for (int k = 0; k < 4; k++) f.dL_drots[4 * si + k] += f.t_rots[4 * si + k];
    }
}

// ---- host side ----
// gsr_features_backward's workspace: gsr_depth_backward's (the accumulator rows where gsr_backward's has them, then the staging area
// `accumulate` sends the per-Gaussian stage's results through: rots 4 | means2D 3 | means3D 3 | opacity 1 | scales 3 | cov3D 6 floats
// per Gaussian), then the dL/dF rows: acc_rows(P) x C floats
struct FeatWs { float *acc, *t_rots, *t_m2, *t_m3, *t_op, *t_sc, *t_cov, *dfacc; size_t total_bytes; };
FeatWs carve_features_ws(void *ws, int P, int C) {
    const BackwardView rows = carve_backward(ws, P, 0);
    const size_t n = (size_t)(P > 0 ? P : 0);
    Bump w = {(char *)ws, rows.vis_off};
    float *const st = w.take<float>(20 * n);
    float *const df = w.take<float>(acc_rows(P) * (size_t)C);
    return {rows.acc, st, st + 4 * n, st + 7 * n, st + 10 * n, st + 11 * n, st + 14 * n, df, w.off};
}

int32_t sizes_and_channels(const char *who, int P, int C, int W, int H, long long R) {
    if (P < 0 || W <= 0 || H <= 0 || R < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: bad sizes", who);
    if (W > 65535 * GSR_TILE_HOST || H > 65535 * GSR_TILE_HOST || (long long)grid_dim(W) * grid_dim(H) > (1ll << 28)) return fail(GSR_ERR_INVALID_ARGUMENT, "image too large");
    if (C < 1 || C > GSR_FEATURES_MAX_C) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: C = %d channels, must be 1 .. %d", who, C, GSR_FEATURES_MAX_C);
    return GSR_OK;
}

// the three workspaces of the gsr_forward before this call (gsr_internal.h: view_geom, view_image, view_lists, refused in this order)
struct Views { GeomView g; ImageView im; BinningView b; };
int32_t view_all(Views &v, int P, int W, int H, long long R, const void *geom_ws, size_t geom_bytes, const void *binning_ws, size_t binning_bytes,
                 const void *img_ws, size_t img_bytes) {
    GSR_TRY(view_geom(geom_ws, geom_bytes, P, &v.g));
    GSR_TRY(view_image(img_ws, img_bytes, W, H, &v.im));
    GSR_TRY(view_lists(binning_ws, binning_bytes, R, &v.b));
    return GSR_OK;
}
FeatArgs walk_args(const Views &v, int P, int C, int W, int H, long long R, const float *features) {
    FeatArgs a;
    memset(&a, 0, sizeof a);
    a.W = W; a.H = H; a.gridx = grid_dim(W); a.gridy = grid_dim(H); a.P = P; a.C = C; a.list_len = (size_t)R;
    a.contrib = v.b.contrib; a.ranges = v.im.ranges; a.point_list = v.b.point_list; a.rec = v.g.rec;
    a.final_T = v.im.final_T; a.n_contrib = v.im.n_contrib; a.features = features;
    return a;
}
// the chunk a call's C is cut into, and the grid: x = half tiles / 4 (a wave each), y = chunks
inline int chunk_of(int C) { return C <= 4 ? 4 : (C <= 8 ? 8 : 16); }
inline dim3 walk_grid(const FeatArgs &a) {
    const int ch = chunk_of(a.C);
    return dim3((unsigned)((2ll * a.gridx * a.gridy + 3) / 4), (unsigned)((a.C + ch - 1) / ch));
}

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

int32_t gsr_features_workspace_bytes(int32_t P, int32_t C, size_t *bytes) {
    if (P < 0 || C < 1 || C > GSR_FEATURES_MAX_C || !bytes) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_features_workspace_bytes: bad argument");
    *bytes = carve_features_ws(nullptr, P, C).total_bytes;
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
    GSR_TRY(view_all(v, P, W, H, (long long)R, geom_ws, geom_bytes, binning_ws, binning_bytes, img_ws, img_bytes));
    FeatArgs a = walk_args(v, P, C, W, H, (long long)R, features);
    a.out = out;
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
    if (!means3D || !radii || !viewmatrix || !projmatrix || !features || !geom_ws || !img_ws || !ws || !dL_dmeans2D || !dL_dopacity || !dL_dmeans3D)
        return fail(GSR_ERR_INVALID_ARGUMENT, "%s: missing input, workspace or gradient buffer", who);
    if (((scales != nullptr) && (rotations != nullptr)) == (cov3D_precomp != nullptr) || ((scales != nullptr) != (rotations != nullptr)))
        return fail(GSR_ERR_INVALID_ARGUMENT, "%s: exactly one of (scales, rotations) / cov3D_precomp must be given", who);
    if ((cov3D_precomp && !dL_dcov3D) || (scales && (!dL_dscales || !dL_drots)))
        return fail(GSR_ERR_INVALID_ARGUMENT, "%s: dL_dcov3D required with cov3D_precomp, dL_dscales and dL_drots with scales and rotations", who);
    if (R > 0 && !binning_ws) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: binning workspace missing", who);
    int32_t det = 0;
    GSR_TRY(gsr_get_option("deterministic_bwd", &det));
    if (det) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: not available while the option deterministic_bwd is on (this pass sums with float atomics and has no slot form)", who);
    const FeatWs fw = carve_features_ws(ws, P, C);
    if (ws_bytes < fw.total_bytes) return fail(GSR_ERR_WORKSPACE, "features workspace %zu < %zu", ws_bytes, fw.total_bytes);
    if (acc_rows(P) >= (1u << 28)) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: P too large for the 28-bit accumulator row index", who);
    float *const d_scales = scales ? dL_dscales : nullptr, *const d_rots = scales ? dL_drots : nullptr;      // the form that was not given is not written
    if (R == 0) {                                       // nothing was composited: every gradient is zero
        const size_t n = (size_t)P * sizeof(float);
        if (dL_dfeatures) HIP_TRY(hipMemsetAsync(dL_dfeatures, 0, (size_t)C * n, s), "clear gradients");
        if (accumulate) return GSR_OK;
        HIP_TRY(hipMemsetAsync(dL_dmeans2D, 0, 3 * n, s), "clear gradients");
        HIP_TRY(hipMemsetAsync(dL_dopacity, 0, n, s), "clear gradients");
        HIP_TRY(hipMemsetAsync(dL_dmeans3D, 0, 3 * n, s), "clear gradients");
        if (dL_dcov3D) HIP_TRY(hipMemsetAsync(dL_dcov3D, 0, 6 * n, s), "clear gradients");
        if (d_scales) { HIP_TRY(hipMemsetAsync(d_scales, 0, 3 * n, s), "clear gradients"); HIP_TRY(hipMemsetAsync(d_rots, 0, 4 * n, s), "clear gradients"); }
        return GSR_OK;
    }
    Views v;
    GSR_TRY(view_all(v, P, W, H, (long long)R, geom_ws, geom_bytes, binning_ws, binning_bytes, img_ws, img_bytes));

    // 1. clear the rows that can be added into; 2. the reverse walk, one wave per (half tile, chunk)
    const size_t rows = acc_rows(P), cells = rows * (size_t)C;
    HIP_TRY(launch_zero_marked_rows(P, v.g.touched, v.g.touch_mark, fw.acc, rows, v.im.seg, 0, 0, s), "zero feature accumulators");
    if (dL_dfeatures) {
        hipLaunchKernelGGL(features_zero_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, P, C, v.g.touched, v.g.touch_mark, fw.dfacc, rows);
        HIP_TRY(hipGetLastError(), "zero dL/dF rows");
    }
    FeatArgs a = walk_args(v, P, C, W, H, (long long)R, features);
    a.G = dL_dout; a.acc = fw.acc; a.dfacc = fw.dfacc; a.acc_rows = rows;
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

    // 3. the per-Gaussian chain S11-S13 on these rows: pergauss_bwd.hip's streaming kernel, no colour input, into the caller's buffers or
    //    -- with accumulate -- into the staging area behind the rows
    PergaussBwdArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.P = P; pa.W = W; pa.H = H; pa.rec = v.g.rec; pa.means3D = means3D; pa.scales = scales; pa.rotations = rotations; pa.cov3D_precomp = cov3D_precomp;
    pa.opac = v.g.opac; pa.viewmatrix = viewmatrix; pa.projmatrix = projmatrix; pa.campos = campos;
    pa.scale_modifier = scale_modifier; pa.tanfovx = tanfovx; pa.tanfovy = tanfovy; pa.radii = radii; pa.clamped = v.g.clamped;
    pa.acc = fw.acc; pa.hot = v.g.hot; pa.touched = v.g.touched; pa.touch_mark = v.g.touch_mark;
    pa.dL_dmeans2D = accumulate ? fw.t_m2 : dL_dmeans2D; pa.dL_dopacity = accumulate ? fw.t_op : dL_dopacity; pa.dL_dmeans3D = accumulate ? fw.t_m3 : dL_dmeans3D;
    pa.dL_dcov3D = dL_dcov3D ? (accumulate ? fw.t_cov : dL_dcov3D) : nullptr;
    pa.dL_dscales = d_scales ? (accumulate ? fw.t_sc : d_scales) : nullptr; pa.dL_drots = d_rots ? (accumulate ? fw.t_rots : d_rots) : nullptr;
    HIP_TRY(launch_pergauss_bwd(pa, s), "per-Gaussian backward launch");

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
        f.P = P; f.radii = radii; f.touched = v.g.touched; f.touch_mark = v.g.touch_mark;
        f.t_means2D = fw.t_m2; f.t_opacity = fw.t_op; f.t_means3D = fw.t_m3; f.t_cov3D = fw.t_cov; f.t_scales = fw.t_sc; f.t_rots = fw.t_rots;
        f.dL_dmeans2D = dL_dmeans2D; f.dL_dopacity = dL_dopacity; f.dL_dmeans3D = dL_dmeans3D; f.dL_dcov3D = dL_dcov3D; f.dL_dscales = d_scales; f.dL_drots = d_rots;
        hipLaunchKernelGGL(features_add_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, f);
        HIP_TRY(hipGetLastError(), "features accumulate launch");
    }
    return GSR_OK;
}

}  // extern "C"
