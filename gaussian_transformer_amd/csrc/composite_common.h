// composite_common.h -- the pieces the three per-pixel walks share (composite_fwd.hip, composite_bwd.hip, depth_maps.hip): device
// code only, one copy of each.  Every function is inlined into its callers, and each is used exactly where the caller still compiles
// to the instructions it compiled to with the code written out (scripts/isa_diff.py is the check; a helper's parameter order, or
// whether it takes a value or fills references, decides that -- change one only with that tool at hand).  Where a kernel came out in
// another instruction order the caller keeps its own lines: depth_maps.hip its geometry and its record gather, fwd_unit_pair its
// gather and staging.  The signed wave-wide max the walks use is gsr_device.h's GSR_WAVE_MAX_I32.
#pragma once
#include "gsr_device.h"

namespace gsr {

// ---- block geometry: which 8x8 block of its tile a wave's q-th block is, and the lane's pixel in it ----
// NPX blocks per wave: 4 = the whole tile, 2 = its upper or lower half (`sub`), 1 = one quadrant.  blk 0..3: (bx = blk & 1, by = blk >> 1)
template <int NPX>
__device__ __forceinline__ int block_index(int sub, int q) { return NPX == 4 ? q : (NPX == 2 ? sub * 2 + q : sub); }
struct BlockGeom {
    int x0, y0;       // the block's origin
    int x, y;         // the lane's pixel (lane l holds pixel l of the block, row-major)
    bool inside;      // ... lies in the image
    size_t pix;       // its index there; 0 when outside, so that it can be formed before it is known to be needed
};
__device__ __forceinline__ BlockGeom block_geom(int tx, int ty, int blk, int lane, int W, int H) {      // (tx, ty): the tile
    BlockGeom g;
    g.x0 = tx * GSR_TILE + (blk & 1) * 8; g.y0 = ty * GSR_TILE + (blk >> 1) * 8;
    g.x = g.x0 + (lane & 7); g.y = g.y0 + (lane >> 3);
    g.inside = g.x < W && g.y < H;
    g.pix = (size_t)(g.inside ? g.y : 0) * W + (g.inside ? g.x : 0);
    return g;
}

// ---- staging: one Gaussian's record as every walk keeps it in LDS ----
// gather_record: the record as stored; stage_record: (px, py, -0.5*log2e*A, -log2e*B) (-0.5*log2e*C, opacity, r, g), formed where the
// caller stores them (after its own use of the record: the order the kernels were tuned in).  Built as new vectors: overwriting
// components of the loaded ones sent them through scratch memory (16 bytes of private segment per lane, set up at every wave's start).
// The guards on the list index and on g, the third word and the LDS layout are the caller's.
__device__ __forceinline__ void gather_record(const float *rec, uint32_t g, float4 &r0, float4 &r1, float4 &r2) {
    const float4 *rec4 = reinterpret_cast<const float4 *>(rec) + 3 * (size_t)g;
    r0 = rec4[0]; r1 = rec4[1]; r2 = rec4[2];
}
__device__ __forceinline__ void stage_record(const float4 &r0, const float4 &r1, float4 &s0, float4 &s1) {
    const StagedConic sc = stage_conic(r0.z, r0.w, r1.x);
    s0 = make_float4(r0.x, r0.y, sc.a, sc.b);
    s1 = make_float4(sc.c, r1.y, r1.z, r1.w);
}
// accumulator row of Gaussian g in a reverse pass: its own, or -- for a splat with replica rows (`hot` is the record's replica code,
// gsr_internal.h: first replica << 4 | log2 K) -- replica (tile mod K), behind the P rows of the Gaussians
__device__ __forceinline__ uint32_t replica_row(uint32_t hot, uint32_t g, int P, int tile) {
    return hot ? (uint32_t)P + (hot >> 4) + ((uint32_t)tile & ((1u << (hot & 15u)) - 1u)) : g;
}

// ---- cross-lane reduction of N per-lane sums through LDS ----
// The LDS pipe is idle in the reverse walks, the VALU is their bottleneck: every lane stores its N values as red[value][lane], lane
// 4 value + part adds the 16 floats red[value][16 part .. 16 part + 15] (four ds_read_b128), two DPP steps fold the four parts, and
// lanes 0, 4, .., 4 (N - 1) hold the totals: they leave as ONE N-lane global_atomic_add_f32 per (wave, splat).
// Rows of 68 floats: with 64 the rows start in the same LDS bank and the reading lanes collide N-way.
#define RED_STRIDE 68
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
    const int moved = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true);
    return v + __int_as_float(moved);
}
// the lane's part in reduce_rows: where it reads, whether it reads at all; returns the value whose total it ends up holding, or -1
template <int N>
__device__ __forceinline__ int reduce_setup(const float *red, int lane, const float4 *&red_rd, bool &red_lane) {
    const int rvalue = lane >> 2, rpart = lane & 3;
    red_lane = rvalue < N;
    red_rd = reinterpret_cast<const float4 *>(red + (red_lane ? rvalue : 0) * RED_STRIDE + rpart * 16);
    return (red_lane && rpart == 0) ? rvalue : -1;
}
template <int N>
__device__ __forceinline__ float reduce_rows(float *red, const float4 *red_rd, bool red_lane, int lane, const float (&v)[N]) {
#pragma unroll
    for (int k = 0; k < N; k++) red[k * RED_STRIDE + lane] = v[k];
    __builtin_amdgcn_wave_barrier();
    float sel = 0.f;
    if (red_lane) {
        const float4 p0 = red_rd[0], p1 = red_rd[1], p2 = red_rd[2], p3 = red_rd[3];       // (v_pk_add_f32 pairs here: 2 % slower)
        sel = ((p0.x + p0.y) + (p0.z + p0.w)) + ((p1.x + p1.y) + (p1.z + p1.w)) +
              (((p2.x + p2.y) + (p2.z + p2.w)) + ((p3.x + p3.y) + (p3.z + p3.w)));
    }
    __builtin_amdgcn_wave_barrier();
    sel = dpp_add<0xB1>(sel);   // quad_perm [1,0,3,2]
    return dpp_add<0x4E>(sel);  // quad_perm [2,3,0,1]
}

// ---- the last word of a wave-timeline record (CompositeCounters::trace): splat visits, capped, and where the wave ran ----
__device__ __forceinline__ uint32_t wave_trace_word(unsigned long long visits) {
    return (uint32_t)min(visits, 4095ull) | (__builtin_amdgcn_s_getreg(30724) & 0xffffu) << 12 |   // HW_ID[15:0]: wave, simd, pipe, cu, sh, se
           (__builtin_amdgcn_s_getreg(6164) & 0xfu) << 28;                                          // XCC_ID
}

}  // namespace gsr
