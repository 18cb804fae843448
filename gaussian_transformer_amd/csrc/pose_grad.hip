// pose_grad.hip -- camera gradients of a render (include/gsr_pose.h): dL/dviewmatrix, dL/dprojmatrix, dL/dcampos; kernels and entry points.
//
// Built beside the reverse passes, which it does not touch: it reads the accumulator rows gsr_backward or gsr_depth_backward left at the
// start of their workspace and calls pergauss_bwd.hip's chain (S11, S12a, S12b: the stages of pergauss_chain.h), with the same flags
// (-ffp-contract=off -fno-slp-vectorize), up to the intermediate terms that reach dL/dmeans3D there: the same terms times the camera-side
// factors are the camera gradient.  Nothing per Gaussian is written: 27 sums over P Gaussians leave as 35 floats.
//
// CDNA4 shape:
//   pose_terms_kernel: one lane per Gaussian, 256-lane workgroups.  A lane without a gradient (culled, or not composited: 91 % at
//       BASELINE config 3) issues the radii / composited-byte loads only, and a wave without any skips the chain and the tree
//       (wave-uniform branch).  Contributing lanes form the 27 products in float32 and convert to double; the wave adds them in a fixed
//       xor-shuffle tree, the four waves meet in LDS (1 KiB), the workgroup stores one row of 32 doubles.  HBM-streaming: per Gaussian with
//       a gradient 48 B of accumulator row + 40 B of inputs + 12 K B of SH row, as the streaming pergauss_bwd_kernel; writes 256 B per 256.
//   pose_sum_kernel: one workgroup.  Lane l adds rows l >> 5, (l >> 5) + 8, ... of column l & 31 in index order (coalesced: a row per 32
//       lanes), then a fixed tree over the eight row groups through LDS; rounds to float32 once and writes the 35 outputs, structural
//       zeros included.
// No atomics, no scratch: for identical accumulator rows the result is bit-identical from run to run.
#include <string.h>

#include "../../include/gsr_pose.h"
#include "gsr_host.h"
#include "pergauss_chain.h"

namespace gsr {
namespace {

#define POSE_NSUM 27             // 12 of viewmatrix (columns 0..2 of its four rows) | 12 of projmatrix (columns 0, 1, 3) | 3 of campos
#define POSE_ROW 32              // doubles per workspace row (256 bytes)

struct PoseArgs {
    int P, M, W, H, kind;
    size_t acc_rows;
    const float *means3D, *shs, *scales, *rotations, *cov3D_precomp;
    const float *viewmatrix, *projmatrix, *campos;
    float scale_modifier, tanfovx, tanfovy;
    const int *radii;
    const uint8_t *clamped, *touched;
    const uint32_t *touch_mark, *hot;
    const float *acc;
    double *rows;                // [ceil(P / 256)][POSE_ROW]
};

__device__ __forceinline__ double wave_tree_sum(double v) {
#pragma unroll
    for (int sft = 32; sft > 0; sft >>= 1) v += __shfl_xor(v, sft);
    return v;
}

// the four waves' totals -> out[0..31] (zeros behind the live sums); `part` is the workgroup's LDS
__device__ __forceinline__ void block_tree_store(double v[POSE_NSUM], const bool wave_any, double (*part)[POSE_ROW], double *out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave_any) {                                       // wave-uniform
#pragma unroll
        for (int k = 0; k < POSE_NSUM; k++) v[k] = wave_tree_sum(v[k]);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < POSE_NSUM; k++) part[wave][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < POSE_ROW) {
        const int t = threadIdx.x;
        out[t] = t < POSE_NSUM ? ((part[0][t] + part[1][t]) + (part[2][t] + part[3][t])) : 0.0;
    }
}

// SH: kind 0 with an SH tensor (degree D); otherwise D = 0 and no colour input is read
template <int D, bool SH>
__global__ __launch_bounds__(256) void pose_terms_kernel(PoseArgs a) {
    __shared__ double part[4][POSE_ROW];
    constexpr int K = (D + 1) * (D + 1);
    const int i_in = blockIdx.x * 256 + threadIdx.x;
    const bool inside = i_in < a.P;
    const size_t si = inside ? (size_t)i_in : 0;
    int rad = a.radii[si];
    uint32_t cl = a.clamped[si];
    uint32_t tch = a.touched[si];
    asm volatile("" : "+v"(rad), "+v"(cl), "+v"(tch));   // requested together, awaited together (as pergauss_bwd.hip)
    const bool visible = inside && rad > 0 && tch == *a.touch_mark;
    const bool wave_any = __builtin_amdgcn_ballot_w64(visible) != 0ull;

    float sV[12], sP[12], sC[3];
#pragma unroll
    for (int k = 0; k < 12; k++) { sV[k] = 0.f; sP[k] = 0.f; }
    sC[0] = sC[1] = sC[2] = 0.f;

    if (visible) {
        const float4 *acc4 = reinterpret_cast<const float4 *>(a.acc) + 4 * si;
        float4 A0 = acc4[0], A1 = acc4[1];
        float A9 = a.kind != GSR_POSE_COLOR ? a.acc[GSR_ACC_FLOATS * si + 9] : 0.f;
        float p[3], c6[6], s[3] = {0.f, 0.f, 0.f}, q[4] = {1.f, 0.f, 0.f, 0.f}, c[3 * K + 3];
        p[0] = a.means3D[3 * si]; p[1] = a.means3D[3 * si + 1]; p[2] = a.means3D[3 * si + 2];
        GSR_LOAD_COV_INPUTS(a, si, c6, s, q)
        if (SH) {
            if constexpr ((3 * K) % 4 == 0) load_sh_row<K>(a.shs, si, a.M, c);
            else load_sh_row_exact<K>(a.shs, si, a.M, c);
        }
        if (cl & 0x80u) fold_replica_rows<9, true>(a.acc, a.P, a.hot[si], a.acc_rows, &A0, &A1, a.kind != GSR_POSE_COLOR, A9);
        float pv[3];
        xform4x3(a.viewmatrix, p, pv);
        if (!a.cov3D_precomp) cov3d_activated<false>(s, q, a.scale_modifier, c6);
        // ---- S11: conic -> 2D covariance -> T = J Wm and t = Wm p + translation ----
        Ewa e;
        ewa_project(pv, c6, a.viewmatrix, a.tanfovx, a.tanfovy, a.W, a.H, e);
        float det, dm2[2], gA, gB, gC, d2inv;
        conic_moments(e, A0, A1, a.W, a.H, det, dm2, gA, gB, gC, d2inv);
        if (d2inv != 0.f) {
            const Cov2dGrad d2 = cov2d_grad(e, det, d2inv, gA, gB, gC);
            float dT[2][3], dt[3];
            ewa_T_grad(e, d2.a, d2.b, d2.c, dT, dt);
            // the Jacobian as ewa_project forms it (clamped t)
            const float J00 = e.fx / e.t[2], J02 = -(e.fx * e.t[0]) / (e.t[2] * e.t[2]);
            const float J11 = e.fy / e.t[2], J12 = -(e.fy * e.t[1]) / (e.t[2] * e.t[2]);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const float dW[3] = {J00 * dT[0][k], J11 * dT[1][k], J02 * dT[0][k] + J12 * dT[1][k]};
#pragma unroll
                for (int r = 0; r < 3; r++) sV[3 * k + r] = dW[r] + p[k] * dt[r];
            }
#pragma unroll
            for (int r = 0; r < 3; r++) sV[9 + r] = dt[r];
        }
        // ---- S12a: NDC mean -> projmatrix ----
        {
            float ph[4];
            const float mw = persp_divide(a.projmatrix, p, ph);
            const float g[3] = {dm2[0] * mw, dm2[1] * mw, -(dm2[0] * ph[0] + dm2[1] * ph[1]) * mw * mw};
#pragma unroll
            for (int j = 0; j < 3; j++)
#pragma unroll
                for (int cc = 0; cc < 3; cc++) sP[3 * j + cc] = p[j] * g[cc];
#pragma unroll
            for (int cc = 0; cc < 3; cc++) sP[9 + cc] = g[cc];
        }
        // ---- S12b: colour -> view direction -> campos ----
        if (SH) {
            const float dcol[3] = {A0.x, A0.y, A0.z};
            float dir[3], g[3];
            const float il = view_dir(p, a.campos, dir);
            GSR_SH_DIR_GRAD(D, c, cl, dcol, dir, gch, ddir);
            sh_dir_project(dir, ddir, il, g);
#pragma unroll
            for (int ax = 0; ax < 3; ax++) sC[ax] = -g[ax];
        }
        // ---- the maps' depth value: dL/dv dv/dz into the z row of viewmatrix ----
        if (a.kind != GSR_POSE_COLOR) {
            const float zv = pv[2];
            const float g = a.kind == GSR_POSE_DEPTH_INVERSE ? -A9 / (zv * zv) : A9;
#pragma unroll
            for (int k = 0; k < 3; k++) sV[3 * k + 2] += p[k] * g;
            sV[9 + 2] += g;
        }
    }
    double v[POSE_NSUM];
#pragma unroll
    for (int k = 0; k < 12; k++) { v[k] = (double)sV[k]; v[12 + k] = (double)sP[k]; }
    v[24] = (double)sC[0]; v[25] = (double)sC[1]; v[26] = (double)sC[2];
    block_tree_store(v, wave_any, part, a.rows + (size_t)blockIdx.x * POSE_ROW);
}

__global__ __launch_bounds__(256) void pose_sum_kernel(const double *rows, int nrows, float *dV, float *dPm, float *dC) {
    // lane l owns column l & 31 and adds rows l >> 5, (l >> 5) + 8, ... of it in index order: 32 lanes read one 256-byte row, a wave two
    // rows per load (with a row per lane every load touched 64 lines: 27.6 us for 3907 rows, one CU's request rate)
    __shared__ double part[8][POSE_ROW];
    __shared__ double tot[POSE_ROW];
    const int col = threadIdx.x & 31, grp = threadIdx.x >> 5;
    // eight running sums per lane over rows 64 apart, four rounds unrolled: 32 loads in flight per lane -- one dependent chain waited
    // for the memory latency 61 times over 3907 rows (24.8 us); the order of the adds stays fixed
    double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int r = grp;
#pragma unroll 4
    for (; r + 56 < nrows; r += 64) {
#pragma unroll
        for (int j = 0; j < 8; j++) s[j] += rows[(size_t)(r + 8 * j) * POSE_ROW + col];
    }
    for (; r < nrows; r += 8) s[0] += rows[(size_t)r * POSE_ROW + col];
    part[grp][col] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
    __syncthreads();
    if (threadIdx.x < POSE_ROW) {                         // a fixed tree over the eight row groups
        const int c = threadIdx.x;
        tot[c] = ((part[0][c] + part[1][c]) + (part[2][c] + part[3][c])) + ((part[4][c] + part[5][c]) + (part[6][c] + part[7][c]));
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < 16) {                                         // viewmatrix entry 4 k + r: column 3 is never read by the renderer
        const int k = t >> 2, r = t & 3;
        if (dV) dV[t] = r == 3 ? 0.f : (float)tot[3 * k + r];
    } else if (t < 32) {                                  // projmatrix entry 4 j + c: column 2 (clip z) is never read
        const int e = t - 16, j = e >> 2, c = e & 3;
        if (dPm) dPm[e] = c == 2 ? 0.f : (float)tot[12 + 3 * j + (c == 3 ? 2 : c)];
    } else if (t < 35) {
        if (dC) dC[t - 32] = (float)tot[24 + (t - 32)];
    }
}

inline size_t pose_rows(int P) { return (size_t)((P > 0 ? P : 1) + 255) / 256; }
inline size_t workspace_bytes(int P) { return pose_rows(P) * POSE_ROW * sizeof(double); }

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

int32_t gsr_pose_workspace_bytes(int32_t P, size_t *bytes) {
    if (P < 0 || !bytes) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_pose_workspace_bytes: bad argument");
    *bytes = workspace_bytes(P);
    return GSR_OK;
}

int32_t gsr_pose_backward(gsr_stream_t stream, int32_t kind, int32_t P, int32_t D, int32_t M, int32_t W, int32_t H, int64_t R,
                          const float *means3D, const int32_t *radii, const float *shs, const float *colors_precomp,
                          const float *scales, float scale_modifier, const float *rotations, const float *cov3D_precomp,
                          const float *viewmatrix, const float *projmatrix, const float *campos, float tanfovx, float tanfovy,
                          const void *geom_ws, size_t geom_bytes, const void *acc_ws, size_t acc_bytes, void *ws, size_t ws_bytes,
                          float *dL_dviewmatrix, float *dL_dprojmatrix, float *dL_dcampos) {
    const char *who = "gsr_pose_backward";
    hipStream_t s = (hipStream_t)stream;
    if (kind != GSR_POSE_COLOR && kind != GSR_POSE_DEPTH_EXPECTED && kind != GSR_POSE_DEPTH_INVERSE)
        return fail(GSR_ERR_INVALID_ARGUMENT, "%s: kind %d is none of 0 (colour), 1 (expected depth), 2 (inverse depth)", who, kind);
    if (P < 0 || W <= 0 || H <= 0 || R < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: bad sizes", who);
    if (!dL_dviewmatrix && !dL_dprojmatrix && !dL_dcampos)
        return fail(GSR_ERR_INVALID_ARGUMENT, "%s: dL_dviewmatrix, dL_dprojmatrix and dL_dcampos are all NULL", who);
    if (P == 0 || R == 0) {                               // nothing was composited: every gradient is zero
        if (dL_dviewmatrix) HIP_TRY(hipMemsetAsync(dL_dviewmatrix, 0, 16 * sizeof(float), s), "clear camera gradients");
        if (dL_dprojmatrix) HIP_TRY(hipMemsetAsync(dL_dprojmatrix, 0, 16 * sizeof(float), s), "clear camera gradients");
        if (dL_dcampos) HIP_TRY(hipMemsetAsync(dL_dcampos, 0, 3 * sizeof(float), s), "clear camera gradients");
        return GSR_OK;
    }
    if (!means3D || !radii || !viewmatrix || !projmatrix || !geom_ws || !acc_ws || !ws)
        return fail(GSR_ERR_INVALID_ARGUMENT, "%s: missing input or workspace", who);
    if (((scales != nullptr) && (rotations != nullptr)) == (cov3D_precomp != nullptr) || ((scales != nullptr) != (rotations != nullptr)))
        return fail(GSR_ERR_INVALID_ARGUMENT, "%s: exactly one of (scales, rotations) / cov3D_precomp must be given", who);
    const bool sh = kind == GSR_POSE_COLOR && shs != nullptr;
    if (kind == GSR_POSE_COLOR) {
        if ((shs != nullptr) == (colors_precomp != nullptr))
            return fail(GSR_ERR_INVALID_ARGUMENT, "%s: exactly one of shs / colors_precomp must be given with kind 0", who);
        if (shs && (!campos || D < 0 || D > 3 || M < (D + 1) * (D + 1))) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: SH inputs inconsistent", who);
    }
    if ((reinterpret_cast<uintptr_t>(acc_ws) | reinterpret_cast<uintptr_t>(ws)) & 15) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: workspaces must be 16-byte aligned", who);
    const BackwardView rows = carve_backward(const_cast<void *>(acc_ws), P, 0);      // the backward (or depth) workspace a reverse pass has filled
    if (acc_bytes < rows.acc_bytes) return fail(GSR_ERR_WORKSPACE, "accumulator workspace %zu < %zu", acc_bytes, rows.acc_bytes);
    if (ws_bytes < workspace_bytes(P)) return fail(GSR_ERR_WORKSPACE, "pose workspace %zu < %zu", ws_bytes, workspace_bytes(P));
    GeomView g; GSR_TRY(view_geom(geom_ws, geom_bytes, P, &g));

    PoseArgs a;
    memset(&a, 0, sizeof a);
    a.P = P; a.M = M; a.W = W; a.H = H; a.kind = kind; a.acc_rows = acc_rows(P);
    a.means3D = means3D; a.shs = sh ? shs : nullptr; a.scales = scales; a.rotations = rotations; a.cov3D_precomp = cov3D_precomp;
    a.viewmatrix = viewmatrix; a.projmatrix = projmatrix; a.campos = campos;
    a.scale_modifier = scale_modifier; a.tanfovx = tanfovx; a.tanfovy = tanfovy;
    a.radii = radii; a.clamped = g.clamped; a.touched = g.touched; a.touch_mark = g.touch_mark; a.hot = g.hot;
    a.acc = rows.acc; a.rows = (double *)ws;
    const dim3 grid((unsigned)pose_rows(P)), block(256);
    if (!sh) hipLaunchKernelGGL((pose_terms_kernel<0, false>), grid, block, 0, s, a);
    else with_sh_degree(D, [&](auto DD) { hipLaunchKernelGGL((pose_terms_kernel<decltype(DD)::value, true>), grid, block, 0, s, a); });
    HIP_TRY(hipGetLastError(), "pose terms launch");
    hipLaunchKernelGGL(pose_sum_kernel, dim3(1), block, 0, s, (const double *)ws, (int)pose_rows(P), dL_dviewmatrix, dL_dprojmatrix, dL_dcampos);
    HIP_TRY(hipGetLastError(), "pose sum launch");
    return GSR_OK;
}

}  // extern "C"
