// normals.hip -- per-Gaussian normals and the fused depth-normal consistency loss (include/gsr_normals.h): kernels and entry points.
//
// Beside the colour path, which it does not touch: no list, no record and no workspace of gsr_forward is read.  Two independent pieces.
//
// 1. Per Gaussian, one lane each: the shortest axis' column of quat_to_rot, turned into view space and towards the camera.  Float32,
//    built without FMA contraction so that the two decisions (argmin of the scales, the sign of n_v . p_v) round as the header writes
//    them.  The reverse kernel is the column's polynomial differentiated by hand, in float64, rounded once.
//
// 2. The loss, a bandwidth-bound stencil pair over [H,W] maps: one 256-thread workgroup per 32 x 8 tile, rows coalesced.
//    Staged in LDS per pixel of the tile and its halo: D = depth / alpha as a double and one byte "alpha >= alpha_min, inside the image".
//    All arithmetic of a stencil is float64 on the float32 inputs: the cross product of two differences of neighbouring Q's cancels
//    6 to 7 digits at image sizes of interest, which float32 does not have to give; the kernels stay bound by their 20 to 40 bytes per
//    pixel (DESIGN.md section 7 has the measured figures).
//    forward : one-pixel halo; every thread forms its pixel's stencil, stores n~ (optional), and the block's sum of A (1 - N . n~) and
//              its count of valid pixels go to the workspace as two doubles: wave reduction by shuffles, then the four waves' values in
//              order.  A finishing kernel adds the blocks' values in a fixed order.
//    backward: a gather.  The workgroup RECOMPUTES the stencils of its tile and of a one-pixel ring around it (340 stencils for 256
//              pixels, from a two-pixel halo of D) and leaves each stencil's dL/da and dL/db -- the gradients of its two difference
//              vectors -- in LDS; every pixel then collects the four that its Q entered, with the signs it entered them with.  Nothing
//              is kept from the forward call: seeds in the workspace would cost 24 bytes per pixel written and read again, more than
//              the 20 the forward kernel reads, to save arithmetic the kernel has to spare.
#include <string.h>

#include "../../include/gsr_normals.h"
#include "gsr_device.h"
#include "gsr_host.h"
#include "gsr_internal.h"

namespace gsr {
namespace {

// ------------------------------------------------------------ per-Gaussian normals ------------------------------------------------------------

__global__ __launch_bounds__(256) void gaussian_normals_fwd_kernel(int P, const float *__restrict__ means3D, const float *__restrict__ scales,
                                                                   const float *__restrict__ rotations, const float *__restrict__ vm,
                                                                   float *__restrict__ out_normals, int32_t *__restrict__ out_axis) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const size_t g = (size_t)i;
    const float s[3] = {scales[3 * g], scales[3 * g + 1], scales[3 * g + 2]};
    int k = 0;
    if (s[1] < s[k]) k = 1;
    if (s[2] < s[k]) k = 2;
    const float q[4] = {rotations[4 * g], rotations[4 * g + 1], rotations[4 * g + 2], rotations[4 * g + 3]};
    float Rm[3][3];
    quat_to_rot(q, Rm);
    const float nw[3] = {k == 0 ? Rm[0][0] : (k == 1 ? Rm[0][1] : Rm[0][2]), k == 0 ? Rm[1][0] : (k == 1 ? Rm[1][1] : Rm[1][2]),
                         k == 0 ? Rm[2][0] : (k == 1 ? Rm[2][1] : Rm[2][2])};
    float nv[3], pv[3];
#pragma unroll
    for (int c = 0; c < 3; c++) nv[c] = vm[c] * nw[0] + vm[4 + c] * nw[1] + vm[8 + c] * nw[2];
    const float p[3] = {means3D[3 * g], means3D[3 * g + 1], means3D[3 * g + 2]};
    xform4x3(vm, p, pv);
    const float dot = nv[0] * pv[0] + nv[1] * pv[1] + nv[2] * pv[2];
    const bool flip = dot > 0.f;
#pragma unroll
    for (int c = 0; c < 3; c++) out_normals[3 * g + c] = flip ? -nv[c] : nv[c];
    if (out_axis) out_axis[g] = k | (flip ? 4 : 0);
}

__global__ __launch_bounds__(256) void gaussian_normals_bwd_kernel(int P, const float *__restrict__ rotations, const float *__restrict__ vm,
                                                                   const int32_t *__restrict__ axis, const float *__restrict__ dL_dn,
                                                                   float *__restrict__ dL_drots) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const size_t g = (size_t)i;
    const int code = axis[g], k = min(code & 3, 2);
    const double sgn = (code & 4) ? -1.0 : 1.0;
    const double gv[3] = {sgn * (double)dL_dn[3 * g], sgn * (double)dL_dn[3 * g + 1], sgn * (double)dL_dn[3 * g + 2]};
    double gw[3];                                        // dL/dn_w = R_view^T dL/dn_v
#pragma unroll
    for (int j = 0; j < 3; j++) gw[j] = (double)vm[4 * j] * gv[0] + (double)vm[4 * j + 1] * gv[1] + (double)vm[4 * j + 2] * gv[2];
    const double r = rotations[4 * g], x = rotations[4 * g + 1], y = rotations[4 * g + 2], z = rotations[4 * g + 3];
    double dr, dx, dy, dz;
    if (k == 0) {            // (1 - 2 (yy + zz), 2 (xy + rz), 2 (xz - ry))
        dr = 2.0 * (z * gw[1] - y * gw[2]);
        dx = 2.0 * (y * gw[1] + z * gw[2]);
        dy = -4.0 * y * gw[0] + 2.0 * (x * gw[1] - r * gw[2]);
        dz = -4.0 * z * gw[0] + 2.0 * (r * gw[1] + x * gw[2]);
    } else if (k == 1) {     // (2 (xy - rz), 1 - 2 (xx + zz), 2 (yz + rx))
        dr = 2.0 * (x * gw[2] - z * gw[0]);
        dx = -4.0 * x * gw[1] + 2.0 * (y * gw[0] + r * gw[2]);
        dy = 2.0 * (x * gw[0] + z * gw[2]);
        dz = -4.0 * z * gw[1] + 2.0 * (y * gw[2] - r * gw[0]);
    } else {                 // (2 (xz + ry), 2 (yz - rx), 1 - 2 (xx + yy))
        dr = 2.0 * (y * gw[0] - x * gw[1]);
        dx = -4.0 * x * gw[2] + 2.0 * (z * gw[0] - r * gw[1]);
        dy = -4.0 * y * gw[2] + 2.0 * (r * gw[0] + z * gw[1]);
        dz = 2.0 * (x * gw[0] + y * gw[1]);
    }
    reinterpret_cast<float4 *>(dL_drots)[g] = make_float4((float)dr, (float)dx, (float)dy, (float)dz);
}

// ------------------------------------------------------------ depth to normals, and the loss ------------------------------------------------------------

constexpr int NT_X = GSR_NORMAL_TILE_X, NT_Y = GSR_NORMAL_TILE_Y;      // 256 threads: one pixel each
static_assert(NT_X * NT_Y == 256, "one thread per pixel of a tile");

struct LossArgs {
    int H, W;
    float alpha_min;
    double tx, ty, inv_w, inv_h, inv_n;                  // tanfovx, tanfovy, 1/W, 1/H, 1/(H W)
    const float *depth, *alpha, *normals;                // [H,W] [H,W] [3,H,W]
    float *out_surf;                                     // forward: [3,H,W] or NULL
    double2 *partial;                                    // forward: [blocks] (sum, valid pixels)
    const float *grad_loss;                              // backward: device scalar or NULL
    float *g_depth, *g_alpha, *g_normals;                // backward: each may be NULL
};

// Stages D and the validity byte of the tile's pixels and a HALO-pixel ring around them: entry [ly][lx] is pixel (x0 - HALO + lx, y0 - HALO + ly)
template <int HALO>
__device__ __forceinline__ void stage_depth(const LossArgs &a, int x0, int y0, double (*sD)[NT_X + 2 * HALO], uint8_t (*sOK)[NT_X + 2 * HALO]) {
    constexpr int SW = NT_X + 2 * HALO, SH = NT_Y + 2 * HALO;
    for (int i = threadIdx.x; i < SW * SH; i += 256) {
        const int ly = i / SW, lx = i - ly * SW;
        const int x = x0 - HALO + lx, y = y0 - HALO + ly;
        double D = 0.0;
        uint8_t ok = 0;
        if (x >= 0 && x < a.W && y >= 0 && y < a.H) {
            const size_t p = (size_t)y * a.W + x;
            const float al = a.alpha[p];
            if (al >= a.alpha_min) { ok = 1; D = (double)a.depth[p] / (double)al; }
        }
        sD[ly][lx] = D;
        sOK[ly][lx] = ok;
    }
}

struct Stencil { double a[3], b[3], c[3], n2; };

// The stencil of pixel (x, y), whose staged entry is [ly][lx]; false: not valid (s is then not to be used)
template <int SW>
__device__ __forceinline__ bool stencil_at(const LossArgs &a, int x, int y, int lx, int ly, const double (*sD)[SW], const uint8_t (*sOK)[SW], Stencil &s) {
    if (!(x > 0 && x < a.W - 1 && y > 0 && y < a.H - 1)) return false;
    if (!(sOK[ly][lx] & sOK[ly - 1][lx] & sOK[ly + 1][lx] & sOK[ly][lx - 1] & sOK[ly][lx + 1])) return false;
    const double rx = ((2.0 * x + 1.0) * a.inv_w - 1.0) * a.tx, ry = ((2.0 * y + 1.0) * a.inv_h - 1.0) * a.ty;
    const double rxl = ((2.0 * (x - 1) + 1.0) * a.inv_w - 1.0) * a.tx, rxr = ((2.0 * (x + 1) + 1.0) * a.inv_w - 1.0) * a.tx;
    const double ryu = ((2.0 * (y - 1) + 1.0) * a.inv_h - 1.0) * a.ty, ryd = ((2.0 * (y + 1) + 1.0) * a.inv_h - 1.0) * a.ty;
    const double Du = sD[ly - 1][lx], Dd = sD[ly + 1][lx], Dl = sD[ly][lx - 1], Dr = sD[ly][lx + 1];
    s.a[0] = Dd * rx - Du * rx; s.a[1] = Dd * ryd - Du * ryu; s.a[2] = Dd - Du;
    s.b[0] = Dr * rxr - Dl * rxl; s.b[1] = Dr * ry - Dl * ry; s.b[2] = Dr - Dl;
    s.c[0] = s.a[1] * s.b[2] - s.a[2] * s.b[1];
    s.c[1] = s.a[2] * s.b[0] - s.a[0] * s.b[2];
    s.c[2] = s.a[0] * s.b[1] - s.a[1] * s.b[0];
    s.n2 = s.c[0] * s.c[0] + s.c[1] * s.c[1] + s.c[2] * s.c[2];
    return s.n2 > 1e-30;
}

__global__ __launch_bounds__(256) void normal_loss_fwd_kernel(LossArgs a) {
    __shared__ double sD[NT_Y + 2][NT_X + 2];
    __shared__ uint8_t sOK[NT_Y + 2][NT_X + 2];
    __shared__ double wsum[4];
    __shared__ unsigned wcnt[4];
    const int x0 = blockIdx.x * NT_X, y0 = blockIdx.y * NT_Y;
    stage_depth<1>(a, x0, y0, sD, sOK);
    __syncthreads();
    const int tx = threadIdx.x & (NT_X - 1), ty = threadIdx.x / NT_X;
    const int x = x0 + tx, y = y0 + ty;
    const bool inside = x < a.W && y < a.H;
    const size_t plane = (size_t)a.H * a.W, p = (size_t)y * a.W + x;
    Stencil s;
    const bool valid = inside && stencil_at<NT_X + 2>(a, x, y, tx + 1, ty + 1, sD, sOK, s);
    double term = 0.0, n[3] = {0.0, 0.0, 0.0};
    if (valid) {
        const double inv = 1.0 / sqrt(s.n2);
        n[0] = s.c[0] * inv; n[1] = s.c[1] * inv; n[2] = s.c[2] * inv;
        const double N0 = a.normals[p], N1 = a.normals[plane + p], N2 = a.normals[2 * plane + p];
        term = (double)a.alpha[p] * (1.0 - (N0 * n[0] + N1 * n[1] + N2 * n[2]));
    }
    if (inside && a.out_surf) {
        a.out_surf[p] = (float)n[0]; a.out_surf[plane + p] = (float)n[1]; a.out_surf[2 * plane + p] = (float)n[2];
    }
    // the block's sum: the wave's by shuffles (a fixed tree), the four waves' in order
    const unsigned cnt = (unsigned)__popcll(__ballot(valid));
#pragma unroll
    for (int sft = 32; sft > 0; sft >>= 1) term += __shfl_xor(term, sft);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { wsum[wave] = term; wcnt[wave] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0)
        a.partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] =
            make_double2(((wsum[0] + wsum[1]) + wsum[2]) + wsum[3], (double)(wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3]));
}

// One block: thread t adds the partials of the t-th of 256 contiguous chunks in index order, thread 0 the chunk sums in index order
__global__ __launch_bounds__(256) void normal_loss_finish_kernel(size_t nblocks, double n, const double2 *__restrict__ partial, float *__restrict__ out2) {
    __shared__ double cs[256], cc[256];
    const size_t chunk = (nblocks + 255) / 256, lo = min(nblocks, chunk * threadIdx.x), hi = min(nblocks, lo + chunk);
    double s = 0.0, c = 0.0;
    for (size_t i = lo; i < hi; i++) { const double2 v = partial[i]; s += v.x; c += v.y; }
    cs[threadIdx.x] = s; cc[threadIdx.x] = c;
    __syncthreads();
    if (threadIdx.x != 0) return;
    s = 0.0; c = 0.0;
    for (int t = 0; t < 256; t++) { s += cs[t]; c += cc[t]; }
    out2[0] = (float)(s / n);
    out2[1] = (float)(c / n);
}

__global__ __launch_bounds__(256) void normal_loss_bwd_kernel(LossArgs a) {
    constexpr int RW = NT_X + 2, RH = NT_Y + 2;          // the stencils recomputed: the tile's and a one-pixel ring's
    __shared__ double sD[NT_Y + 4][NT_X + 4];
    __shared__ uint8_t sOK[NT_Y + 4][NT_X + 4];
    __shared__ double sA[RH][RW][3], sB[RH][RW][3];      // dL/da, dL/db of each stencil (zero: not valid)
    const int x0 = blockIdx.x * NT_X, y0 = blockIdx.y * NT_Y;
    const float up = a.grad_loss ? *a.grad_loss : 1.f;
    stage_depth<2>(a, x0, y0, sD, sOK);
    __syncthreads();
    const size_t plane = (size_t)a.H * a.W;
    for (int i = threadIdx.x; i < RW * RH; i += 256) {
        const int sy = i / RW, sx = i - sy * RW;
        const int x = x0 - 1 + sx, y = y0 - 1 + sy;
        const bool inside = x >= 0 && x < a.W && y >= 0 && y < a.H;
        Stencil s;
        const bool valid = inside && stencil_at<NT_X + 4>(a, x, y, sx + 1, sy + 1, sD, sOK, s);
        double da[3] = {0.0, 0.0, 0.0}, db[3] = {0.0, 0.0, 0.0}, gN[3] = {0.0, 0.0, 0.0};
        if (valid) {
            const size_t p = (size_t)y * a.W + x;
            const double inv = 1.0 / sqrt(s.n2);
            const double n[3] = {s.c[0] * inv, s.c[1] * inv, s.c[2] * inv};
            const double w = -(double)a.alpha[p] * a.inv_n;                          // dL/dn~ = w N, dL/dN = w n~
            const double g[3] = {w * (double)a.normals[p], w * (double)a.normals[plane + p], w * (double)a.normals[2 * plane + p]};
            const double ng = n[0] * g[0] + n[1] * g[1] + n[2] * g[2];
            const double gc[3] = {(g[0] - n[0] * ng) * inv, (g[1] - n[1] * ng) * inv, (g[2] - n[2] * ng) * inv};      // dL/dc
            // c = a x b:  dL/da = b x dL/dc,  dL/db = dL/dc x a
            da[0] = s.b[1] * gc[2] - s.b[2] * gc[1]; da[1] = s.b[2] * gc[0] - s.b[0] * gc[2]; da[2] = s.b[0] * gc[1] - s.b[1] * gc[0];
            db[0] = gc[1] * s.a[2] - gc[2] * s.a[1]; db[1] = gc[2] * s.a[0] - gc[0] * s.a[2]; db[2] = gc[0] * s.a[1] - gc[1] * s.a[0];
            gN[0] = w * n[0]; gN[1] = w * n[1]; gN[2] = w * n[2];
        }
#pragma unroll
        for (int c = 0; c < 3; c++) { sA[sy][sx][c] = da[c]; sB[sy][sx][c] = db[c]; }
        if (a.g_normals && inside && sx >= 1 && sx <= NT_X && sy >= 1 && sy <= NT_Y) {      // the tile's own pixels
            const size_t p = (size_t)y * a.W + x;
#pragma unroll
            for (int c = 0; c < 3; c++) a.g_normals[c * plane + p] = (float)gN[c] * up;
        }
    }
    if (!a.g_depth && !a.g_alpha) return;                // block-uniform
    __syncthreads();
    const int tx = threadIdx.x & (NT_X - 1), ty = threadIdx.x / NT_X;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= a.W || y >= a.H) return;
    const size_t p = (size_t)y * a.W + x;
    double gd = 0.0, ga = 0.0;
    if (sOK[ty + 2][tx + 2]) {
        // Q(x,y) is the (y+1) end of the stencil above, the (y-1) end of the one below, the (x+1) end of the left one, the (x-1) end of the right one
        double gQ[3];
#pragma unroll
        for (int c = 0; c < 3; c++) gQ[c] = ((sA[ty][tx + 1][c] - sA[ty + 2][tx + 1][c]) + sB[ty + 1][tx][c]) - sB[ty + 1][tx + 2][c];
        const double rx = ((2.0 * x + 1.0) * a.inv_w - 1.0) * a.tx, ry = ((2.0 * y + 1.0) * a.inv_h - 1.0) * a.ty;
        const double gD = (gQ[0] * rx + gQ[1] * ry) + gQ[2];
        const double inv_al = 1.0 / (double)a.alpha[p];
        gd = gD * inv_al;
        ga = -(gD * sD[ty + 2][tx + 2]) * inv_al;
    }
    if (a.g_depth) a.g_depth[p] = (float)gd * up;
    if (a.g_alpha) a.g_alpha[p] = (float)ga * up;
}

struct LossWs { double2 *partial; size_t blocks, total_bytes; };
LossWs carve_loss_ws(void *ws, int H, int W) {
    Bump w = {(char *)ws, 0};
    const size_t blocks = (size_t)((W + NT_X - 1) / NT_X) * (size_t)((H + NT_Y - 1) / NT_Y);
    double2 *const partial = w.take<double2>(blocks);
    return {partial, blocks, w.off};
}

int32_t loss_sizes(const char *who, int32_t H, int32_t W) {
    if (H < 1 || W < 1) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: bad sizes", who);
    if (H > NT_Y * 65535 || W > (1 << 20)) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: image too large", who);
    return GSR_OK;
}

LossArgs loss_args(int32_t H, int32_t W, float tanfovx, float tanfovy, float alpha_min, const float *depth, const float *alpha, const float *normals) {
    LossArgs a;
    memset(&a, 0, sizeof a);
    a.H = H; a.W = W; a.alpha_min = alpha_min; a.tx = (double)tanfovx; a.ty = (double)tanfovy;
    a.inv_w = 1.0 / (double)W; a.inv_h = 1.0 / (double)H; a.inv_n = 1.0 / ((double)H * (double)W);
    a.depth = depth; a.alpha = alpha; a.normals = normals;
    return a;
}

inline dim3 loss_grid(int32_t H, int32_t W) { return dim3((unsigned)((W + NT_X - 1) / NT_X), (unsigned)((H + NT_Y - 1) / NT_Y)); }

}  // namespace
}  // namespace gsr

using namespace gsr;

extern "C" {

int32_t gsr_gaussian_normals_forward(gsr_stream_t stream, int32_t P, const float *means3D, const float *scales, const float *rotations,
                                     const float *viewmatrix, float *out_normals, int32_t *out_axis) {
    const char *who = "gsr_gaussian_normals_forward";
    if (P < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: bad sizes", who);
    if (P == 0) return GSR_OK;
    if (!means3D || !scales || !rotations || !viewmatrix || !out_normals)
        return fail(GSR_ERR_INVALID_ARGUMENT, "%s: missing input or output buffer", who);
    hipLaunchKernelGGL(gaussian_normals_fwd_kernel, dim3((unsigned)(((long long)P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P, means3D,
                       scales, rotations, viewmatrix, out_normals, out_axis);
    HIP_TRY(hipGetLastError(), "gaussian normals forward launch");
    return GSR_OK;
}

int32_t gsr_gaussian_normals_backward(gsr_stream_t stream, int32_t P, const float *rotations, const float *viewmatrix, const int32_t *axis,
                                      const float *dL_dnormals, float *dL_drots) {
    const char *who = "gsr_gaussian_normals_backward";
    if (P < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: bad sizes", who);
    if (P == 0) return GSR_OK;
    if (!rotations || !viewmatrix || !axis || !dL_dnormals || !dL_drots)
        return fail(GSR_ERR_INVALID_ARGUMENT, "%s: missing input or output buffer", who);
    hipLaunchKernelGGL(gaussian_normals_bwd_kernel, dim3((unsigned)(((long long)P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P, rotations,
                       viewmatrix, axis, dL_dnormals, dL_drots);
    HIP_TRY(hipGetLastError(), "gaussian normals backward launch");
    return GSR_OK;
}

int32_t gsr_normal_loss_workspace(int32_t H, int32_t W, size_t *bytes) {
    const char *who = "gsr_normal_loss_workspace";
    if (!bytes) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: bad argument", who);
    GSR_TRY(loss_sizes(who, H, W));
    *bytes = carve_loss_ws(nullptr, H, W).total_bytes;
    return GSR_OK;
}

int32_t gsr_normal_loss_forward(gsr_stream_t stream, int32_t H, int32_t W, float tanfovx, float tanfovy, float alpha_min, const float *depth,
                                const float *alpha, const float *normals, float *out2, float *out_surf, void *ws, size_t ws_bytes) {
    const char *who = "gsr_normal_loss_forward";
    hipStream_t s = (hipStream_t)stream;
    GSR_TRY(loss_sizes(who, H, W));
    if (!(alpha_min > 0.f)) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: alpha_min must be positive (D = depth / alpha is formed where alpha >= alpha_min)", who);
    if (!depth || !alpha || !normals || !out2 || !ws) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: missing input, output or workspace", who);
    const LossWs w = carve_loss_ws(ws, H, W);
    if (ws_bytes < w.total_bytes) return fail(GSR_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, ws_bytes, w.total_bytes);
    LossArgs a = loss_args(H, W, tanfovx, tanfovy, alpha_min, depth, alpha, normals);
    a.out_surf = out_surf; a.partial = w.partial;
    hipLaunchKernelGGL(normal_loss_fwd_kernel, loss_grid(H, W), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError(), "normal loss forward launch");
    hipLaunchKernelGGL(normal_loss_finish_kernel, dim3(1), dim3(256), 0, s, w.blocks, (double)H * (double)W, (const double2 *)w.partial, out2);
    HIP_TRY(hipGetLastError(), "normal loss finish launch");
    return GSR_OK;
}

int32_t gsr_normal_loss_backward(gsr_stream_t stream, int32_t H, int32_t W, float tanfovx, float tanfovy, float alpha_min, const float *depth,
                                 const float *alpha, const float *normals, const float *grad_loss, float *dL_ddepth, float *dL_dalpha,
                                 float *dL_dnormals) {
    const char *who = "gsr_normal_loss_backward";
    GSR_TRY(loss_sizes(who, H, W));
    if (!(alpha_min > 0.f)) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: alpha_min must be positive (D = depth / alpha is formed where alpha >= alpha_min)", who);
    if (!depth || !alpha || !normals) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: missing input", who);
    if (!dL_ddepth && !dL_dalpha && !dL_dnormals) return GSR_OK;
    LossArgs a = loss_args(H, W, tanfovx, tanfovy, alpha_min, depth, alpha, normals);
    a.grad_loss = grad_loss; a.g_depth = dL_ddepth; a.g_alpha = dL_dalpha; a.g_normals = dL_dnormals;
    hipLaunchKernelGGL(normal_loss_bwd_kernel, loss_grid(H, W), dim3(256), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError(), "normal loss backward launch");
    return GSR_OK;
}

}  // extern "C"
