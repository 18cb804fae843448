// pergauss_chain.h -- the per-Gaussian chain, one copy of each stage that several kernels run: S2 (covariance from scale and rotation,
// with the raw-parameter activations) and the perspective divide for all four, the radius (S4) and the pixel centre (S5) for
// preprocess_fwd_kernel (preprocess.hip) and visible_union_kernel (sequence.hip), S11-S12b (oracle/gsr_ref.c) for pergauss_one
// (pergauss_bwd.hip) and pose_terms_kernel (pose_grad.hip); depth_finish_kernel (depth_maps.hip) shares the replica-row fold.
// Every helper is inlined and spells its arithmetic as the kernels spelled it; where a function would have changed a kernel's
// instruction list, the helper is a statement (a macro), as GSR_WAVE_MAX_I32 in gsr_device.h.  The gate is scripts/isa_diff.py against
// the commit before this header: every kernel of the five files `identical` or `reordered` (profiles/isa/pergauss_chain_refactor.txt).
// The three tests of the forward footprint (near plane, det != 0, area != 0) stay written out in both forward kernels, around calls of
// these stages: one helper for the whole footprint changed preprocess_fwd_kernel's control flow or loads in every form tried.
#pragma once
#include "gsr_device.h"
#include "gsr_internal.h"

namespace gsr {

// ---- covariance of one Gaussian ----
// The inputs of Gaussian si from the kernel's arguments `a` (cov3D_precomp, or scales and rotations): c6 if the caller supplies
// covariances, (s, q) otherwise (uniform branch).  A statement, not a function: through a function's parameters the four kernels come
// out with other address arithmetic (3 si is then no longer shared with the load of the mean) -- scripts/isa_diff.py
#define GSR_LOAD_COV_INPUTS(a, si, c6, s, q)                                                    \
    if ((a).cov3D_precomp) {                                                                    \
        _Pragma("unroll") for (int k_ = 0; k_ < 6; k_++) (c6)[k_] = (a).cov3D_precomp[6 * (si) + k_]; \
    } else {                                                                                    \
        (s)[0] = (a).scales[3 * (si)]; (s)[1] = (a).scales[3 * (si) + 1]; (s)[2] = (a).scales[3 * (si) + 2]; \
        const float4 q4_ = reinterpret_cast<const float4 *>((a).rotations)[si];                 \
        (q)[0] = q4_.x; (q)[1] = q4_.y; (q)[2] = q4_.z; (q)[3] = q4_.w;                         \
    }
// S2 from loaded values.  RAW: s and q are the raw parameters and are activated in place (exp / normalize, scene/gaussian_model.py:33-41),
// as the reverse chain needs them; returns 1 / |q| of the raw quaternion (1 without RAW)
template <bool RAW>
__device__ __forceinline__ float cov3d_activated(float s[3], float q[4], float scale_modifier, float c6[6]) {
    float inv_norm = 1.f;
    if (RAW) {
        s[0] = expf(s[0]); s[1] = expf(s[1]); s[2] = expf(s[2]);
        act_normalize4(q, inv_norm);
    }
    cov3d_from_scale_rot(s, scale_modifier, q, c6);
    return inv_norm;
}

// S1 / S12a: clip-space position of p and the perspective-divide factor 1 / (w + eps)
__device__ __forceinline__ float persp_divide(const float *__restrict__ projmatrix, const float p[3], float ph[4]) {
    xform4x4(projmatrix, p, ph);
    return 1.f / (ph[3] + GSR_W_EPS);
}

// S4: the splat's radius in pixels, 3 sigma of the larger eigenvalue of the 2D covariance (a b; b c) with determinant det
__device__ __forceinline__ int splat_radius(const Ewa &e, float det) {
    const float mid = 0.5f * (e.a + e.c);
    float disc = mid * mid - det;
    if (disc < GSR_LAMBDA_FLOOR) disc = GSR_LAMBDA_FLOOR;
    const float l1 = mid + sqrtf(disc), l2 = mid - sqrtf(disc);
    const float lmax = l1 > l2 ? l1 : l2;
    return (int)ceilf(GSR_SIGMA_EXTENT * sqrtf(lmax));
}
// S5: pixel coordinate of an NDC coordinate on an axis of `size` pixels
__device__ __forceinline__ float ndc_to_pixel(float ndc, int size) { return ((ndc + 1.f) * (float)size - 1.f) * 0.5f; }

// ---- the reverse chain ----
// A splat over hundreds of tiles had its waves add into replica accumulator rows (gsr_internal.h): rows P + (hot >> 4) ... of `acc`,
// 2^(hot & 15) of them, are added to the Gaussian's own.  A0 / A1 (floats 0-7; null: not wanted) and float SLOT (`extra`, if with_extra).
// GUARDED: rows at or beyond acc_rows are not read.
template <int SLOT, bool GUARDED>
__device__ __forceinline__ void fold_replica_rows(const float *acc, int P, uint32_t hot, size_t acc_rows, float4 *A0, float4 *A1,
                                                  bool with_extra, float &extra) {
    const size_t first = (size_t)P + (hot >> 4);
    for (uint32_t k = 0; k < (1u << (hot & 15u)); k++) {
        if (GUARDED && first + k >= acc_rows) break;      // a code can only name rows of the workspace: nothing beyond it is read
        if (A0) {
            const float4 *r4 = reinterpret_cast<const float4 *>(acc) + 4 * (first + k);
            const float4 B0 = r4[0], B1 = r4[1];
            A0->x += B0.x; A0->y += B0.y; A0->z += B0.z; A0->w += B0.w;
            A1->x += B1.x; A1->y += B1.y; A1->z += B1.z; A1->w += B1.w;
        }
        if (with_extra) extra += acc[GSR_ACC_FLOATS * (first + k) + SLOT];
    }
}

// S11, first step.  The compositing kernel (composite_bwd.hip) accumulates moments of s = opacity * G * dL/dalpha over the pixels:
// A0.w, A1.x = sum s*d;  A1.yzw = sum s * d d^T.  The factors that are constant per Gaussian are applied here:
//   mean2D gradient w.r.t. NDC = -(W/2, H/2) * conic * sum s*d;   conic gradient = -1/2 * sum s * d d^T
__device__ __forceinline__ void conic_moments(const Ewa &e, const float4 &A0, const float4 &A1, int W, int H, float &det, float dm2[2],
                                              float &gA, float &gB, float &gC, float &d2inv) {
    const float ea = e.a, eb = e.b, ec = e.c;
    det = ea * ec - eb * eb;
    const float det_inv = 1.f / det;                        // the conic as the forward pass formed it (S4)
    const float cA = ec * det_inv, cB = -eb * det_inv, cC = ea * det_inv;
    dm2[0] = -0.5f * (float)W * (cA * A0.w + cB * A1.x); dm2[1] = -0.5f * (float)H * (cB * A0.w + cC * A1.x);
    gA = -0.5f * A1.y; gB = -0.5f * A1.z; gC = -0.5f * A1.w;
    d2inv = 1.f / (det * det + GSR_DENOM_EPS);
}
// conic gradient -> gradient of the 2D covariance (a b; b c)
struct Cov2dGrad { float a, b, c; };
__device__ __forceinline__ Cov2dGrad cov2d_grad(const Ewa &e, float det, float d2inv, float gA, float gB, float gC) {
    const float ea = e.a, eb = e.b, ec = e.c;
    Cov2dGrad d;
    d.a = d2inv * (-ec * ec * gA + 2.f * eb * ec * gB + (det - ea * ec) * gC);
    d.c = d2inv * (-ea * ea * gC + 2.f * ea * eb * gB + (det - ea * ec) * gA);
    d.b = d2inv * 2.f * (eb * ec * gA - (det + 2.f * eb * eb) * gB + ea * eb * gC);
    return d;
}
// 2D covariance = T Sigma T^T with T = J Wm: its gradient w.r.t. T and, through the Jacobian J(t), w.r.t. the (clamped) view-space mean t
__device__ __forceinline__ void ewa_T_grad(const Ewa &e, float dL_da, float dL_db, float dL_dc, float dT[2][3], float dt[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        dT[0][k] = 2.f * dL_da * e.TS[0][k] + dL_db * e.TS[1][k];
        dT[1][k] = dL_db * e.TS[0][k] + 2.f * dL_dc * e.TS[1][k];
    }
    float dJ00 = 0.f, dJ02 = 0.f, dJ11 = 0.f, dJ12 = 0.f;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        dJ00 += dT[0][k] * e.Wm[0][k]; dJ02 += dT[0][k] * e.Wm[2][k];
        dJ11 += dT[1][k] * e.Wm[1][k]; dJ12 += dT[1][k] * e.Wm[2][k];
    }
    const float tz = 1.f / e.t[2], tz2 = tz * tz, tz3 = tz2 * tz;
    dt[0] = (e.clampx ? 0.f : 1.f) * (-e.fx * tz2 * dJ02);
    dt[1] = (e.clampy ? 0.f : 1.f) * (-e.fy * tz2 * dJ12);
    dt[2] = -e.fx * tz2 * dJ00 - e.fy * tz2 * dJ11 + 2.f * e.fx * e.t[0] * tz3 * dJ02 + 2.f * e.fy * e.t[1] * tz3 * dJ12;
}

// S6 / S12b: dir = (p - campos) / |p - campos|; returns il = 1 / |p - campos|
__device__ __forceinline__ float view_dir(const float p[3], const float *campos, float dir[3]) {
    const float v[3] = {p[0] - campos[0], p[1] - campos[1], p[2] - campos[2]};
    const float len2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], il = 1.f / sqrtf(len2);
    dir[0] = v[0] * il; dir[1] = v[1] * il; dir[2] = v[2] * il;
    return il;
}
// S12b: colour -> view direction dir, for SH degree D and the Gaussian's SH row c.  Declares in the caller's scope: gch[3] =
// dL/dcolour (dcol) with the channels the forward pass clamped (bits 0-2 of cl) switched off; ddir[3] = the gradient w.r.t. dir.
// sh_dir_project then gives g, the gradient w.r.t. p: dL/dmeans3D gains g, dL/dcampos gains -g.
// A statement, not a function: behind a function the compiler folds the sign of -SH_C1 into six subtractions where the kernels add
// today (the same sums, but another instruction list) -- scripts/isa_diff.py
#define GSR_SH_DIR_GRAD(D, c, cl, dcol, dir, gch, ddir)                                                                  \
    float bg3_[16][3];                                                                                                  \
    sh_basis_grad<D>(dir, bg3_);                                                                                        \
    float ddir[3] = {0.f, 0.f, 0.f};                                                                                    \
    float gch[3];                                                                                                       \
    _Pragma("unroll") for (int ch_ = 0; ch_ < 3; ch_++) gch[ch_] = (((cl) >> ch_) & 1) ? 0.f : (dcol)[ch_];             \
    _Pragma("unroll") for (int ch_ = 0; ch_ < 3; ch_++)                                                                 \
        _Pragma("unroll") for (int k_ = 0; k_ < ((D) + 1) * ((D) + 1); k_++)                                            \
            _Pragma("unroll") for (int ax_ = 0; ax_ < 3; ax_++) ddir[ax_] += bg3_[k_][ax_] * (c)[k_ * 3 + ch_] * gch[ch_]
// ... and through the normalisation: the part of ddir along dir is projected off
__device__ __forceinline__ void sh_dir_project(const float dir[3], const float ddir[3], float il, float g[3]) {
    const float dot = dir[0] * ddir[0] + dir[1] * ddir[1] + dir[2] * ddir[2];
#pragma unroll
    for (int ax = 0; ax < 3; ax++) g[ax] = (ddir[ax] - dir[ax] * dot) * il;
}

}  // namespace gsr
