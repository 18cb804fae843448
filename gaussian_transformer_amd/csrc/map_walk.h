// map_walk.h -- what depth_maps.hip and feature_maps.hip share, one copy of each: the two files walk the same half tiles over the
// same lists and end their reverse calls in the same per-Gaussian chain; they differ in what a splat carries (a scalar v, a C-vector).
//   device: the leading kernel-argument fields (WalkArgs), the half tile's geometry (its y is formed once for both blocks), the record
//           gather behind the range check on the id (gather_entry: each file keeps only what it writes into LDS), and the add of the
//           staged per-Gaussian result that `accumulate` asks for (add_staged).
//   host:   the three workspaces of the gsr_forward before the call (view_all), the filler of WalkArgs, the half-tile block count, the
//           size and image-limit refusal, the workspace carve (depth's layout is the one without dL/dF rows), and of the reverse calls
//           the common refusals, the R == 0 clearing and the per-Gaussian launch with its `accumulate` selection.
// Every device function is inlined, and every kernel of the two files compiles to the instructions it compiled to with these lines
// written out in it (scripts/isa_diff.py, profiles/isa/map_walk_refactor.txt): WalkArgs keeps the fields' order, so the
// kernel-argument offsets are the same.
// NOT shared, on purpose: the four walk loops.  As templates that take the per-entry work as callables all eleven walk kernels come
// out different (features_fwd_kernel<16>: 77 -> 110 VGPRs, 40 -> 73 s_waitcnt; features_bwd_kernel<16, true>: 126 -> 116 VGPRs with
// other branching): a performance change nobody has measured.  The recurrences stay apart as well: depth's
// gD (v T - S) + gA T_final folded into the features' u T - S rounds differently.
// With the colour passes these walks share what composite_common.h holds, and no more: through its geometry and gather helpers the
// depth kernels come out in another instruction order.
#pragma once
#include <string.h>

#include "composite_common.h"
#include "gsr_host.h"
#include "gsr_internal.h"

namespace gsr {

// ---- device ----
struct WalkArgs {
    int W, H, gridx, gridy, P;
    union { int mode; int C; };  // depth_maps.hip: GSR_DEPTH_*; feature_maps.hip: channels
    size_t list_len;             // R: entries of point_list, stride of contrib
    size_t acc_rows;             // rows of acc (reverse pass)
    const uint8_t *contrib;      // [4][list_len]
    const uint2 *ranges;
    const uint32_t *point_list;
    const float *rec;
    const float *final_T;
    const uint32_t *n_contrib;
};

// what a wave knows of its half tile before it walks: pixel coordinates, each pixel's last contributor (0 outside the image), the
// largest one per block and overall (clamped to the list: a garbage n_contrib cannot send the walk past the tile's range)
struct HalfTile {
    float fx[2], fy;
    bool inside[2];
    size_t pix[2];
    int last[2], blk_last[2], hi;
    uint2 range;
};
__device__ __forceinline__ HalfTile half_tile(const WalkArgs &a, const int tile, const int sub, const int lane) {
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
    h.hi = (int)min((long long)hi, max(n, 0ll));
    return h;
}

// entry base + lane of the tile's list: its Gaussian, the staged record (px, py, a, b) (c, opacity, -, -) as the colour pass stages it,
// the record's third word, which of the half tile's two blocks it reaches and -- want_row -- its accumulator row (else g)
struct Entry {
    uint32_t g, bits, row;
    float4 s0, s1, r2;
};
// false: the lane has no entry (past cnt, past the list, an id or a row out of range)
__device__ __forceinline__ bool gather_entry(const WalkArgs &a, const HalfTile &h, const int tile, const int sub, const int base, const int cnt,
                                             const int lane, const bool want_row, Entry &e) {
    if (lane >= cnt) return false;
    const size_t at = (size_t)h.range.x + base + lane;
    if (at >= a.list_len) return false;
    e.g = a.point_list[at];
    if (e.g >= (uint32_t)a.P) return false;
    const float4 *rec4 = reinterpret_cast<const float4 *>(a.rec) + 3 * (size_t)e.g;
    const float4 r0 = rec4[0], r1 = rec4[1];
    e.r2 = rec4[2];
    e.bits = 0u;
#pragma unroll
    for (int q = 0; q < 2; q++) e.bits |= a.contrib[(size_t)(sub * 2 + q) * a.list_len + at] ? (1u << q) : 0u;
    e.row = e.g;
    if (want_row) {
        e.row = replica_row(__float_as_uint(e.r2.w), e.g, a.P, tile);
        if ((size_t)e.row >= a.acc_rows) return false;
    }
    stage_record(r0, r1, e.s0, e.s1);
    return true;
}
// the fourth float of an entry's second staged word; row < 2^28 (checked by the entry point)
__device__ __forceinline__ float entry_code(const Entry &e) { return __uint_as_float(e.bits | (e.row << 4)); }

// the six gradients of the per-Gaussian chain: the caller's buffers, or their staging area in the workspace
struct Grads { float *means2D, *opacity, *means3D, *cov3D, *scales, *rots; };
struct StagedAdd { Grads t, out; };
// accumulate: out += t for Gaussian si.  e: three floats the caller adds to dL/dmeans3D in the same statement (out += t + e), or NULL
__device__ __forceinline__ void add_staged(const StagedAdd &f, const size_t si, const float *e) {
    if (e) {
#pragma unroll
        for (int k = 0; k < 3; k++) f.out.means3D[3 * si + k] += f.t.means3D[3 * si + k] + e[k];
    } else {
#pragma unroll
        for (int k = 0; k < 3; k++) f.out.means3D[3 * si + k] += f.t.means3D[3 * si + k];
    }
    f.out.means2D[3 * si] += f.t.means2D[3 * si]; f.out.means2D[3 * si + 1] += f.t.means2D[3 * si + 1];
    f.out.opacity[si] += f.t.opacity[si];
    if (f.out.cov3D) {
#pragma unroll
        for (int k = 0; k < 6; k++) f.out.cov3D[6 * si + k] += f.t.cov3D[6 * si + k];
    }
    if (f.out.scales) {
#pragma unroll
        for (int k = 0; k < 3; k++) f.out.scales[3 * si + k] += f.t.scales[3 * si + k];
#pragma unroll
        for (int k = 0; k < 4; k++) f.out.rots[4 * si + k] += f.t.rots[4 * si + k];
    }
}

// ---- host ----
static inline int32_t map_sizes(const char *who, int P, int W, int H, long long R) {
    if (P < 0 || W <= 0 || H <= 0 || R < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: bad sizes", who);
    if (W > 65535 * GSR_TILE_HOST || H > 65535 * GSR_TILE_HOST || (long long)grid_dim(W) * grid_dim(H) > (1ll << 28)) return fail(GSR_ERR_INVALID_ARGUMENT, "image too large");
    return GSR_OK;
}

// the three workspaces of the gsr_forward before this call (gsr_internal.h: view_geom, view_image, view_lists, refused in this order)
struct ForwardWs { const void *geom; size_t geom_bytes; const void *binning; size_t binning_bytes; const void *img; size_t img_bytes; };
struct Views { GeomView g; ImageView im; BinningView b; };
static inline int32_t view_all(Views &v, int P, int W, int H, long long R, const ForwardWs &f) {
    GSR_TRY(view_geom(f.geom, f.geom_bytes, P, &v.g));
    GSR_TRY(view_image(f.img, f.img_bytes, W, H, &v.im));
    GSR_TRY(view_lists(f.binning, f.binning_bytes, R, &v.b));
    return GSR_OK;
}
// A: DepthArgs or FeatArgs, zeroed, with WalkArgs' fields but mode / C and acc_rows
template <class A>
inline A walk_args(const Views &v, int P, int W, int H, long long R) {
    A a;
    memset(&a, 0, sizeof a);
    a.W = W; a.H = H; a.gridx = grid_dim(W); a.gridy = grid_dim(H); a.P = P; a.list_len = (size_t)R;
    a.contrib = v.b.contrib; a.ranges = v.im.ranges; a.point_list = v.b.point_list; a.rec = v.g.rec;
    a.final_T = v.im.final_T; a.n_contrib = v.im.n_contrib;
    return a;
}
static inline unsigned walk_blocks(const WalkArgs &a) { return (unsigned)((2ll * a.gridx * a.gridy + 3) / 4); }      // half tiles / 4: a wave each

// A reverse call's workspace: the accumulator rows where gsr_backward's has them, then the staging area `accumulate` sends the
// per-Gaussian stage's results through, one piece of 20 floats per Gaussian: rots 4 | means2D 3 | means3D 3 | opacity 1 | scales 3 |
// cov3D 6, then -- gsr_features_backward, C > 0 -- the dL/dF rows: acc_rows(P) x C floats
struct MapWs { float *acc; Grads staged; float *dfacc; size_t total_bytes; };
static inline MapWs carve_map_ws(void *ws, int P, int C) {
    const BackwardView rows = carve_backward(ws, P, 0);
    const size_t n = (size_t)(P > 0 ? P : 0);
    Bump w = {(char *)ws, rows.vis_off};
    float *const st = w.take<float>(20 * n);
    float *const df = w.take<float>(acc_rows(P) * (size_t)C);
    return {rows.acc, {st + 4 * n, st + 10 * n, st + 7 * n, st + 14 * n, st + 11 * n, st}, df, w.off};
}

// what gsr_depth_backward and gsr_features_backward are both handed, in the order of their parameters
struct ReverseCall {
    const char *who;
    int P, W, H;
    long long R;
    const float *means3D; const int32_t *radii; const float *scales; float scale_modifier; const float *rotations, *cov3D_precomp;
    const float *viewmatrix, *projmatrix, *campos;
    float tanfovx, tanfovy;
    ForwardWs fws;
    void *ws; size_t ws_bytes;
    int accumulate;
    Grads out;                   // dL_dmeans2D .. dL_drots; after reverse_prologue scales and rots are NULL unless scales were given
};

// The refusals both reverse calls make once their own arguments are checked and P > 0, and the carve.  own_inputs: the call's own
// input pointers are all there; ws_name: "depth" or "features"; C: channels of the dL/dF rows, 0 for none
static inline int32_t reverse_prologue(ReverseCall &c, bool own_inputs, const char *ws_name, int C, MapWs *w) {
    if (!c.means3D || !c.radii || !c.viewmatrix || !c.projmatrix || !own_inputs || !c.fws.geom || !c.fws.img || !c.ws || !c.out.means2D || !c.out.opacity || !c.out.means3D)
        return fail(GSR_ERR_INVALID_ARGUMENT, "%s: missing input, workspace or gradient buffer", c.who);
    if (((c.scales != nullptr) && (c.rotations != nullptr)) == (c.cov3D_precomp != nullptr) || ((c.scales != nullptr) != (c.rotations != nullptr)))
        return fail(GSR_ERR_INVALID_ARGUMENT, "%s: exactly one of (scales, rotations) / cov3D_precomp must be given", c.who);
    if ((c.cov3D_precomp && !c.out.cov3D) || (c.scales && (!c.out.scales || !c.out.rots)))
        return fail(GSR_ERR_INVALID_ARGUMENT, "%s: dL_dcov3D required with cov3D_precomp, dL_dscales and dL_drots with scales and rotations", c.who);
    if (c.R > 0 && !c.fws.binning) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: binning workspace missing", c.who);
    int32_t det = 0;
    GSR_TRY(gsr_get_option("deterministic_bwd", &det));
    if (det) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: not available while the option deterministic_bwd is on (this pass sums with float atomics and has no slot form)", c.who);
    *w = carve_map_ws(c.ws, c.P, C);
    if (c.ws_bytes < w->total_bytes) return fail(GSR_ERR_WORKSPACE, "%s workspace %zu < %zu", ws_name, c.ws_bytes, w->total_bytes);
    if (acc_rows(c.P) >= (1u << 28)) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: P too large for the 28-bit accumulator row index", c.who);
    if (!c.scales) c.out.scales = c.out.rots = nullptr;      // the form that was not given is not written
    return GSR_OK;
}

// R == 0, nothing was composited: every gradient is zero.  own: the call's own gradient output of own_floats per Gaussian (dL/dF) or NULL;
// it is written in full by every call, so it is cleared first and with `accumulate` too, which leaves the six others as they are
static inline int32_t clear_gradients(const ReverseCall &c, float *own, int own_floats, hipStream_t s) {
    const struct { float *p; int floats; } buf[7] = {{own, own_floats}, {c.out.means2D, 3}, {c.out.opacity, 1}, {c.out.means3D, 3},
                                                     {c.out.cov3D, 6}, {c.out.scales, 3}, {c.out.rots, 4}};
    for (int k = 0; k < (c.accumulate ? 1 : 7); k++)
        if (buf[k].p) HIP_TRY(hipMemsetAsync(buf[k].p, 0, (size_t)buf[k].floats * c.P * sizeof(float), s), "clear gradients");
    return GSR_OK;
}

// the per-Gaussian chain S11-S13 on the walk's rows: pergauss_bwd.hip's streaming kernel, no colour input, into the caller's buffers or
// -- with accumulate -- into the staging area behind the rows
static inline int32_t launch_chain(const ReverseCall &c, const Views &v, const MapWs &w, hipStream_t s) {
    const Grads &to = c.accumulate ? w.staged : c.out;
    PergaussBwdArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.P = c.P; pa.W = c.W; pa.H = c.H; pa.rec = v.g.rec; pa.means3D = c.means3D; pa.scales = c.scales; pa.rotations = c.rotations; pa.cov3D_precomp = c.cov3D_precomp;
    pa.opac = v.g.opac; pa.viewmatrix = c.viewmatrix; pa.projmatrix = c.projmatrix; pa.campos = c.campos;
    pa.scale_modifier = c.scale_modifier; pa.tanfovx = c.tanfovx; pa.tanfovy = c.tanfovy; pa.radii = c.radii; pa.clamped = v.g.clamped;
    pa.acc = w.acc; pa.hot = v.g.hot; pa.touched = v.g.touched; pa.touch_mark = v.g.touch_mark;
    pa.dL_dmeans2D = to.means2D; pa.dL_dopacity = to.opacity; pa.dL_dmeans3D = to.means3D;
    pa.dL_dcov3D = c.out.cov3D ? to.cov3D : nullptr; pa.dL_dscales = c.out.scales ? to.scales : nullptr; pa.dL_drots = c.out.rots ? to.rots : nullptr;
    HIP_TRY(launch_pergauss_bwd(pa, s), "per-Gaussian backward launch");
    return GSR_OK;
}

}  // namespace gsr
