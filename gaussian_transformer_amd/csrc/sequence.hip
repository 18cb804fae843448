// sequence.hip -- sequence preparation of the Gaussian transformer (include/gsr_sequence.h):
//   box sort : key kernel (box of every row, decided against the boundary table in LDS) -> stable rocPRIM radix sort of
//              (box, index) over just the bits the boxes need -> gather kernel (rows, permutation, count, zero tail).
//              Dropped rows carry the key n^3, so the stable sort leaves them behind every box: no compaction step, no atomic.
//   visible_union : one lane per Gaussian, 3-D covariance built once (pergauss_chain.h's cov3d_activated, as preprocess.hip calls it),
//              then the geometry stages S1-S5 of preprocess.hip per camera.
// Compiled with -ffp-contract=off -fno-slp-vectorize like preprocess.hip: the radii round exactly as gsr_forward's.
#include <cstring>  // ROCm 7.2 rocprim/texture_cache_iterator.hpp uses memset without including it
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "../../include/gsr_sequence.h"
#include "gsr_host.h"
#include "gsr_internal.h"
#include "pergauss_chain.h"

namespace gsr {

#define GSR_SEQ_MAX_N 128   // == GSR_BOX_MAX_N
#define GSR_SEQ_MAX_B 64    // == GSR_VISIBLE_MAX_B
static_assert(GSR_SEQ_MAX_N == GSR_BOX_MAX_N && GSR_SEQ_MAX_B == GSR_VISIBLE_MAX_B, "limits of sequence.hip and gsr_sequence.h");
struct VisibleArgs {
    int P, B, raw_params;
    float scale_modifier;
    const float *means3D, *scales, *rotations, *cov3D_precomp, *viewmatrices, *projmatrices;
    int32_t *radii_out;
    uint8_t *visible_out;
    int32_t *counts_out;
    float tanfovx[GSR_SEQ_MAX_B], tanfovy[GSR_SEQ_MAX_B];
    int W[GSR_SEQ_MAX_B], H[GSR_SEQ_MAX_B];
};

// ---------------------------------------------------------------- box sort ----------------------------------------------------------------

struct BoxKeyArgs {
    int P, D, xyz_col, n;
    const float *rows;
    uint32_t *keys;
    float b[GSR_SEQ_MAX_N + 1];     // (float)((1.0 / n) * k), computed by the host in double
};

// axis cell of c among the n cells [b_a, b_{a+1}), -1 if none (c < b_0, c >= b_n, NaN).  The guess from c * n is off by at most a
// cell near a boundary; the comparisons against the table decide.
__device__ __forceinline__ int box_cell(float c, int n, const float *__restrict__ b) {
    if (!(c >= b[0] && c < b[n])) return -1;
    int g = (int)(c * (float)n);
    g = g < 0 ? 0 : (g > n - 1 ? n - 1 : g);
    while (g > 0 && c < b[g]) g--;
    while (g < n - 1 && c >= b[g + 1]) g++;
    return g;
}

__global__ __launch_bounds__(256) void box_key_kernel(BoxKeyArgs a) {
    __shared__ float s_b[GSR_SEQ_MAX_N + 1];
    for (int k = threadIdx.x; k <= a.n; k += 256) s_b[k] = a.b[k];
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.P) return;
    const float *r = a.rows + (size_t)i * a.D + a.xyz_col;
    const int cx = box_cell(r[0], a.n, s_b), cy = box_cell(r[1], a.n, s_b), cz = box_cell(r[2], a.n, s_b);
    const uint32_t n = (uint32_t)a.n;
    a.keys[i] = (cx < 0 || cy < 0 || cz < 0) ? n * n * n : (uint32_t)cx + n * ((uint32_t)cy + n * (uint32_t)cz);
}

// one thread per output float: consecutive lanes read consecutive floats of a source row and write consecutive floats of the output.
// P * D < 2^31 (checked by the caller), so the index arithmetic is 32-bit.
__global__ __launch_bounds__(256) void box_gather_kernel(int P, int D, uint32_t nbox, const float *__restrict__ rows,
                                                         const uint32_t *__restrict__ skeys, const uint32_t *__restrict__ sidx,
                                                         float *__restrict__ out_rows, int32_t *__restrict__ out_perm,
                                                         int32_t *__restrict__ out_count) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= (uint32_t)P * (uint32_t)D) return;
    const uint32_t j = e / (uint32_t)D, c = e - j * (uint32_t)D;
    const bool kept = skeys[j] < nbox;
    const uint32_t src = sidx[j];
    out_rows[e] = kept ? rows[src * (uint32_t)D + c] : 0.f;
    if (c == 0) {
        out_perm[j] = kept ? (int32_t)src : -1;
        // the kept rows are a prefix: exactly one j sees its end
        if (kept && (j + 1 == (uint32_t)P || !(skeys[j + 1] < nbox))) *out_count = (int32_t)(j + 1);
        if (!kept && j == 0) *out_count = 0;
    }
}

struct BoxWs { uint32_t *keys, *skeys, *sidx; void *temp; size_t temp_bytes, total; };

static int box_bits(int n) { return ceil_log2_u32((uint32_t)n * n * n + 1u); }      // keys 0 .. n^3 inclusive

static hipError_t carve_box_ws(void *base, int P, int n, BoxWs &w) {
    const size_t np = (size_t)(P > 0 ? P : 1);
    size_t tb = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, tb, (const uint32_t *)nullptr, (uint32_t *)nullptr,
                                             rocprim::counting_iterator<uint32_t>(0), (uint32_t *)nullptr, np, 0u,
                                             (unsigned)box_bits(n), (hipStream_t)0, false);
    if (e != hipSuccess) return e;
    Bump b = {(char *)base, 0};
    w.keys = b.take<uint32_t>(np); w.skeys = b.take<uint32_t>(np); w.sidx = b.take<uint32_t>(np);
    w.temp = b.take<char>(tb > 0 ? tb : 1);
    w.temp_bytes = tb;
    w.total = b.off;
    return hipSuccess;
}

static hipError_t box_sort_workspace_bytes(int P, int n, size_t *bytes) {
    BoxWs w;
    hipError_t e = carve_box_ws(nullptr, P, n, w);
    if (e == hipSuccess) *bytes = w.total;
    return e;
}

// sizes validated by the caller; P >= 1
static hipError_t launch_box_sort(int P, int D, const float *rows, int xyz_col, int n, float *out_rows, int32_t *out_perm, int32_t *out_count,
                           void *ws, hipStream_t s) {
    BoxWs w;
    hipError_t e = carve_box_ws(ws, P, n, w);
    if (e != hipSuccess) return e;
    BoxKeyArgs ka;
    ka.P = P; ka.D = D; ka.xyz_col = xyz_col; ka.n = n; ka.rows = rows; ka.keys = w.keys;
    const double interval = 1.0 / (double)n;
    for (int k = 0; k <= GSR_SEQ_MAX_N; k++) ka.b[k] = k <= n ? (float)(interval * (double)k) : 0.f;
    hipLaunchKernelGGL(box_key_kernel, dim3((P + 255) / 256), dim3(256), 0, s, ka);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t tb = w.temp_bytes;
    e = rocprim::radix_sort_pairs(w.temp, tb, (const uint32_t *)w.keys, w.skeys, rocprim::counting_iterator<uint32_t>(0), w.sidx,
                                  (size_t)P, 0u, (unsigned)box_bits(n), s, false);
    if (e != hipSuccess) return e;
    const uint32_t total = (uint32_t)P * (uint32_t)D;
    hipLaunchKernelGGL(box_gather_kernel, dim3((total + 255u) / 256u), dim3(256), 0, s, P, D, (uint32_t)n * n * n, rows,
                       (const uint32_t *)w.skeys, (const uint32_t *)w.sidx, out_rows, out_perm, out_count);
    return hipGetLastError();
}

// ---------------------------------------------------------------- visibility ----------------------------------------------------------------

// 256 threads, one Gaussian per lane; the cameras' matrices sit in LDS (8 KB at B = 64), their scalars in the kernel arguments.
// Per camera the sequence of operations is that of preprocess_fwd_kernel up to `area != 0`: the same three tests around calls of the
// same stages (pergauss_chain.h: persp_divide, ewa_project, splat_radius, ndc_to_pixel, tile_rect).
template <bool RAW>
__global__ __launch_bounds__(256) void visible_union_kernel(VisibleArgs a) {
    __shared__ float s_vm[GSR_SEQ_MAX_B * 16], s_pm[GSR_SEQ_MAX_B * 16];
    for (int k = threadIdx.x; k < a.B * 16; k += 256) { s_vm[k] = a.viewmatrices[k]; s_pm[k] = a.projmatrices[k]; }
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < a.P;
    const size_t si = (size_t)(live ? i : a.P - 1);       // lanes past the end recompute Gaussian P-1 and store nothing
    const float p[3] = {a.means3D[3 * si], a.means3D[3 * si + 1], a.means3D[3 * si + 2]};
    float c6[6];
    if (a.cov3D_precomp) {                                // uniform
#pragma unroll
        for (int k = 0; k < 6; k++) c6[k] = a.cov3D_precomp[6 * si + k];
    } else {                                              // S2, once for all cameras
        float s[3] = {a.scales[3 * si], a.scales[3 * si + 1], a.scales[3 * si + 2]};
        const float4 q4 = reinterpret_cast<const float4 *>(a.rotations)[si];
        float q[4] = {q4.x, q4.y, q4.z, q4.w};
        cov3d_activated<RAW>(s, q, a.scale_modifier, c6);
    }
    bool any = false;
    for (int b = 0; b < a.B; b++) {
        float vm[16], pm[16];
#pragma unroll
        for (int k = 0; k < 16; k++) { vm[k] = s_vm[b * 16 + k]; pm[k] = s_pm[b * 16 + k]; }
        const int W = a.W[b], H = a.H[b];
        const int gridx = (W + GSR_TILE - 1) / GSR_TILE, gridy = (H + GSR_TILE - 1) / GSR_TILE;
        int radius_out = 0;
        float pv[3];
        xform4x3(vm, p, pv);
        if (pv[2] > GSR_NEAR_Z) {                                                       // S1
            float ph[4];
            const float pw = persp_divide(pm, p, ph);
            const float ndcx = ph[0] * pw, ndcy = ph[1] * pw;
            Ewa e;
            ewa_project(pv, c6, vm, a.tanfovx[b], a.tanfovy[b], W, H, e);               // S3
            const float det = e.a * e.c - e.b * e.b;                                    // S4
            if (det != 0.f) {
                const int radius = splat_radius(e, det);
                const float px = ndc_to_pixel(ndcx, W), py = ndc_to_pixel(ndcy, H);                // S5
                int x0, y0, x1, y1;
                tile_rect(px, py, radius, gridx, gridy, x0, y0, x1, y1);
                if ((x1 - x0) * (y1 - y0) != 0) radius_out = radius;
            }
        }
        const bool vis = live && radius_out > 0;
        any |= vis;
        if (a.radii_out && live) a.radii_out[(size_t)b * a.P + si] = radius_out;
        if (a.counts_out) {                               // one integer atomic per wave and camera
            const unsigned long long m = __ballot(vis);
            if ((threadIdx.x & 63) == 0 && m) atomicAdd(&a.counts_out[b], (int)__popcll(m));
        }
    }
    if (a.visible_out && live) a.visible_out[si] = any ? 1 : 0;
}

// sizes validated by the caller; P >= 1; counts_out zeroed by the caller on the same stream
static hipError_t launch_visible_union(const VisibleArgs &a, hipStream_t s) {
    const dim3 grid((a.P + 255) / 256), block(256);
    if (a.raw_params) hipLaunchKernelGGL((visible_union_kernel<true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((visible_union_kernel<false>), grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace gsr

using namespace gsr;

extern "C" {

// ---- sequence preparation: box sort and multi-camera visibility (include/gsr_sequence.h) ----
static int box_sizes(const char *who, int32_t P, int32_t n) {
    if (P < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: P=%d is negative", who, P);
    if (n < 1 || n > GSR_BOX_MAX_N) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: n=%d not in 1..%d", who, n, GSR_BOX_MAX_N);
    return GSR_OK;
}

int32_t gsr_box_sort_workspace(int32_t P, int32_t n, size_t *bytes) {
    if (!bytes) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_box_sort_workspace: bytes is NULL");
    if (box_sizes("gsr_box_sort_workspace", P, n) != GSR_OK) return GSR_ERR_INVALID_ARGUMENT;
    HIP_TRY(box_sort_workspace_bytes(P, n, bytes), "box sort workspace size");
    return GSR_OK;
}

int32_t gsr_box_sort(gsr_stream_t stream, int32_t P, int32_t D, const float *rows, int32_t xyz_col, int32_t n, float *out_rows,
                     int32_t *out_perm, int32_t *out_count, void *ws, size_t ws_bytes) {
    if (box_sizes("gsr_box_sort", P, n) != GSR_OK) return GSR_ERR_INVALID_ARGUMENT;
    if (D < 3 || D > GSR_BOX_MAX_D) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_box_sort: D=%d not in 3..%d", D, GSR_BOX_MAX_D);
    if (xyz_col < 0 || xyz_col > D - 3) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_box_sort: xyz_col=%d not in 0..D-3=%d", xyz_col, D - 3);
    if ((long long)P * D > 0x7fffffffLL) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_box_sort: P * D = %lld too large", (long long)P * D);
    if (!out_count) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_box_sort: out_count is NULL");
    if (P == 0) {
        HIP_TRY(hipMemsetAsync(out_count, 0, sizeof(int32_t), (hipStream_t)stream), "box sort: clear count");
        return GSR_OK;
    }
    if (!rows || !out_rows || !out_perm || !ws) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_box_sort: null pointer");
    if (rows == out_rows) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_box_sort: rows and out_rows must not overlap (same pointer)");
    if (rows < out_rows + (size_t)P * D && out_rows < rows + (size_t)P * D)
        return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_box_sort: rows and out_rows must not overlap (the ranges of P * D floats intersect)");
    size_t need = 0;
    HIP_TRY(box_sort_workspace_bytes(P, n, &need), "box sort workspace size");
    if (ws_bytes < need) return fail(GSR_ERR_WORKSPACE, "box sort workspace %zu < %zu", ws_bytes, need);
    HIP_TRY(launch_box_sort(P, D, rows, xyz_col, n, out_rows, out_perm, out_count, ws, (hipStream_t)stream), "box sort launch");
    return GSR_OK;
}

int32_t gsr_visible_union(gsr_stream_t stream, int32_t P, int32_t B, const float *means3D, const float *scales, float scale_modifier,
                          const float *rotations, const float *cov3D_precomp, int32_t raw_params, const float *viewmatrices,
                          const float *projmatrices, const float *tanfovx, const float *tanfovy, const int32_t *widths,
                          const int32_t *heights, int32_t *radii_out, uint8_t *visible_out, int32_t *counts_out) {
    if (P < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_visible_union: P=%d is negative", P);
    if (B < 1 || B > GSR_VISIBLE_MAX_B) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_visible_union: B=%d not in 1..%d", B, GSR_VISIBLE_MAX_B);
    if (!tanfovx || !tanfovy || !widths || !heights) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_visible_union: tanfovx/tanfovy/widths/heights (host) required");
    VisibleArgs a;
    memset(&a, 0, sizeof(a));
    for (int b = 0; b < B; b++) {
        if (widths[b] <= 0 || heights[b] <= 0 || widths[b] > 65535 * GSR_TILE_HOST || heights[b] > 65535 * GSR_TILE_HOST)
            return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_visible_union: camera %d: image size %d x %d", b, widths[b], heights[b]);
        a.tanfovx[b] = tanfovx[b]; a.tanfovy[b] = tanfovy[b]; a.W[b] = widths[b]; a.H[b] = heights[b];
    }
    if (counts_out) HIP_TRY(hipMemsetAsync(counts_out, 0, (size_t)B * sizeof(int32_t), (hipStream_t)stream), "visible union: clear counts");
    if (P == 0) return GSR_OK;
    if (!means3D || !viewmatrices || !projmatrices) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_visible_union: missing means3D or matrices");
    if ((cov3D_precomp != nullptr) == (scales != nullptr || rotations != nullptr) || (!cov3D_precomp && (!scales || !rotations)))
        return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_visible_union: exactly one of (scales, rotations) / cov3D_precomp must be given");
    if (raw_params && cov3D_precomp) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_visible_union: raw_params needs scales/rotations, not cov3D_precomp");
    a.P = P; a.B = B; a.raw_params = raw_params ? 1 : 0; a.scale_modifier = scale_modifier;
    a.means3D = means3D; a.scales = scales; a.rotations = rotations; a.cov3D_precomp = cov3D_precomp;
    a.viewmatrices = viewmatrices; a.projmatrices = projmatrices;
    a.radii_out = radii_out; a.visible_out = visible_out; a.counts_out = counts_out;
    HIP_TRY(launch_visible_union(a, (hipStream_t)stream), "visible union launch");
    return GSR_OK;
}

}  // extern "C"
