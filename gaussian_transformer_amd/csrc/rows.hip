// rows.hip -- the row glue of the Gaussian transformer (include/gsr_rows.h), kernels and C entry points:
//   rows_unpack : rows [P, D] -> xyz, f_dc, f_rest, opacity, scaling, rotation (the raw inputs of gsr_forward's fused form), a bit copy
//   grad_pack   : B per-camera gradient arenas -> grad_rows [P, D], summed over the cameras in index order
// Both are an AoS <-> SoA transpose of a tile of ROWS_TILE rows through LDS.  The tile's rows are ONE contiguous run of n * D floats
// of `rows` / `grad_rows` and, per column group of width w, one contiguous run of n * w floats of that group's buffer: every global
// access is flat and coalesced (16 bytes per lane on the row side when the base pointer allows it, consecutive dwords per lane on
// the group side, whose runs start at multiples of w floats only).  The LDS tile has an odd pitch (D | 1 dwords): with the even
// pitches 26 and 62, rows r and r + 16 would share a bank (ds_write_b32 / ds_read_b32 bank on dword address mod 32).
// No floating-point contraction question: grad_pack only adds.  The entry points live here, next to their kernels, as those of
// every header but gsr.h do; refusals go through gsr::fail (gsr_host.h).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gsr_rows.h"
#include "gsr_host.h"

namespace gsr {

#define ROWS_TILE 64                                  // rows per workgroup
#define ROWS_MAX_PITCH (3 * GSR_ROWS_MAX_K + 14 + 1)  // 63 dwords: 15.75 KiB of LDS per workgroup at most

// column groups of a row with K SH coefficients (include/gsr_rows.h)
__host__ __device__ __forceinline__ int col_rot(int K) { return 3 * K; }
__host__ __device__ __forceinline__ int col_opacity(int K) { return 3 * K + 4; }
__host__ __device__ __forceinline__ int col_xyz(int K) { return 3 * K + 5; }
__host__ __device__ __forceinline__ int col_scaling(int K) { return 3 * K + 8; }
__host__ __device__ __forceinline__ int col_flags(int K) { return 3 * K + 11; }

struct RowsUnpackArgs {
    int P, D, K;
    int vec;                 // rows is 16-byte aligned: the tile is read 16 bytes per lane
    const uint32_t *rows;
    uint32_t *xyz, *f_dc, *f_rest, *opacity, *scaling, *rotation;
};

struct RowsPackArgs {
    int P, D, K, B;
    int vec;                 // grad_rows is 16-byte aligned
    float *grad_rows;
    const float *arena[GSR_ROWS_MAX_B];
};

// one column group of the tile, LDS -> its dense buffer: lane j of the run writes float r0 * w + j
__device__ __forceinline__ void unpack_group(const uint32_t *s, int pitch, int col, int w, int r0, int n, uint32_t *__restrict__ dst) {
    uint32_t *d = dst + (size_t)r0 * w;
    for (int j = threadIdx.x; j < n * w; j += 256) {
        const int r = j / w, c = j - r * w;
        d[j] = s[r * pitch + col + c];
    }
}

// 256 threads, ROWS_TILE rows.  The words are moved as integers: no value is ever interpreted.
__global__ __launch_bounds__(256) void rows_unpack_kernel(RowsUnpackArgs a) {
    __shared__ uint32_t s[ROWS_TILE * ROWS_MAX_PITCH];
    const int D = a.D, K = a.K, pitch = D | 1;
    const int r0 = blockIdx.x * ROWS_TILE;
    const int n = a.P - r0 < ROWS_TILE ? a.P - r0 : ROWS_TILE;
    const int len = n * D;
    const uint32_t *src = a.rows + (size_t)r0 * D;     // r0 * D * 4 bytes is a multiple of 256: as aligned as a.rows
    const int nq = a.vec ? len >> 2 : 0;
    for (int q = threadIdx.x; q < nq; q += 256) {
        const uint4 v = reinterpret_cast<const uint4 *>(src)[q];
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
        int r = (4 * q) / D, c = 4 * q - r * D;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            s[r * pitch + c] = w4[i];
            if (++c == D) { c = 0; r++; }
        }
    }
    for (int e = 4 * nq + threadIdx.x; e < len; e += 256) {
        const int r = e / D, c = e - r * D;
        s[r * pitch + c] = src[e];
    }
    __syncthreads();
    unpack_group(s, pitch, col_xyz(K), 3, r0, n, a.xyz);
    unpack_group(s, pitch, 0, 3, r0, n, a.f_dc);
    if (K > 1) unpack_group(s, pitch, 3, 3 * (K - 1), r0, n, a.f_rest);
    unpack_group(s, pitch, col_opacity(K), 1, r0, n, a.opacity);
    unpack_group(s, pitch, col_scaling(K), 3, r0, n, a.scaling);
    unpack_group(s, pitch, col_rot(K), 4, r0, n, a.rotation);
}

// one column group of the tile, the cameras' arenas -> LDS: block `off` floats into every arena, summed in camera order from
// a_0 itself (B = 1 copies bits; -0.0 + -0.0 stays -0.0)
__device__ __forceinline__ void pack_group(float *s, int pitch, int col, int w, int r0, int n, const RowsPackArgs &a, size_t off) {
    const size_t base = off + (size_t)r0 * w;
    for (int j = threadIdx.x; j < n * w; j += 256) {
        const int r = j / w, c = j - r * w;
        float v = a.arena[0][base + j];
#pragma unroll 4
        for (int b = 1; b < a.B; b++) v = v + a.arena[b][base + j];
        s[r * pitch + col + c] = v;
    }
}

__global__ __launch_bounds__(256) void rows_grad_pack_kernel(RowsPackArgs a) {
    __shared__ float s[ROWS_TILE * ROWS_MAX_PITCH];
    const int D = a.D, K = a.K, pitch = D | 1;
    const int r0 = blockIdx.x * ROWS_TILE;
    const int n = a.P - r0 < ROWS_TILE ? a.P - r0 : ROWS_TILE;
    const size_t P = (size_t)a.P;
    // arena layout: xyz 3 P | f_dc 3 P | f_rest 3 (K - 1) P | opacity P | scaling 3 P | rotation 4 P
    pack_group(s, pitch, col_xyz(K), 3, r0, n, a, 0);
    pack_group(s, pitch, 0, 3, r0, n, a, 3 * P);
    if (K > 1) pack_group(s, pitch, 3, 3 * (K - 1), r0, n, a, 6 * P);
    pack_group(s, pitch, col_opacity(K), 1, r0, n, a, 3 * P * (K + 1));
    pack_group(s, pitch, col_scaling(K), 3, r0, n, a, 3 * P * (K + 1) + P);
    pack_group(s, pitch, col_rot(K), 4, r0, n, a, 3 * P * (K + 1) + 4 * P);
    for (int j = threadIdx.x; j < n * 3; j += 256) {
        const int r = j / 3, c = j - r * 3;
        s[r * pitch + col_flags(K) + c] = 0.f;
    }
    __syncthreads();
    const int len = n * D;
    float *dst = a.grad_rows + (size_t)r0 * D;         // as aligned as a.grad_rows (r0 * D * 4 bytes is a multiple of 256)
    const int nq = a.vec ? len >> 2 : 0;
    for (int q = threadIdx.x; q < nq; q += 256) {
        int r = (4 * q) / D, c = 4 * q - r * D;
        float w4[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            w4[i] = s[r * pitch + c];
            if (++c == D) { c = 0; r++; }
        }
        reinterpret_cast<float4 *>(dst)[q] = make_float4(w4[0], w4[1], w4[2], w4[3]);
    }
    for (int e = 4 * nq + threadIdx.x; e < len; e += 256) {
        const int r = e / D, c = e - r * D;
        dst[e] = s[r * pitch + c];
    }
}

// ---------------------------------------------------------------- host ----------------------------------------------------------------

// K of a D-column row, 0 if D is no row width
static int rows_K(int D) {
    if (D < 17 || (D - 14) % 3) return 0;
    const int K = (D - 14) / 3;
    return K <= GSR_ROWS_MAX_K ? K : 0;
}

static bool ranges_meet(const void *a, size_t a_floats, const void *b, size_t b_floats) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + 4 * b_floats && b0 < a0 + 4 * a_floats;
}

static int rows_sizes(const char *who, int32_t P, int32_t D) {
    if (P < 0) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: P=%d is negative", who, P);
    if (!rows_K(D))
        return fail(GSR_ERR_INVALID_ARGUMENT, "%s: D=%d is not 3 K + 14 for K in 1..%d SH coefficients", who, D, GSR_ROWS_MAX_K);
    if ((long long)P * D > 0x7fffffffLL) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: P * D = %lld too large", who, (long long)P * D);
    return GSR_OK;
}

}  // namespace gsr

using namespace gsr;

extern "C" {

int32_t gsr_rows_unpack(gsr_stream_t stream, int32_t P, int32_t D, const float *rows, float *xyz, float *f_dc, float *f_rest,
                        float *opacity, float *scaling, float *rotation) {
    if (rows_sizes("gsr_rows_unpack", P, D) != GSR_OK) return GSR_ERR_INVALID_ARGUMENT;
    if (P == 0) return GSR_OK;                       // nothing to read or write: no pointer is looked at
    const int K = rows_K(D);
    if ((f_rest == nullptr) != (K == 1))
        return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_rows_unpack: f_rest must be NULL if and only if K = 1 (D=%d holds K=%d)", D, K);
    if (!rows || !xyz || !f_dc || !opacity || !scaling || !rotation) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_rows_unpack: null pointer");
    if ((uintptr_t)rotation & 15)
        return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_rows_unpack: rotation must be 16-byte aligned (gsr_forward reads a quaternion as one 16-byte load)");
    const struct { const char *name; const float *p; size_t w; } outs[6] = {
        {"xyz", xyz, 3}, {"f_dc", f_dc, 3}, {"f_rest", f_rest, (size_t)3 * (K - 1)}, {"opacity", opacity, 1}, {"scaling", scaling, 3}, {"rotation", rotation, 4}};
    for (const auto &o : outs)
        if (o.p && ranges_meet(rows, (size_t)P * D, o.p, (size_t)P * o.w))
            return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_rows_unpack: %s overlaps rows", o.name);
    RowsUnpackArgs a;
    a.P = P; a.D = D; a.K = K; a.vec = ((uintptr_t)rows & 15) == 0;
    a.rows = (const uint32_t *)rows;
    a.xyz = (uint32_t *)xyz; a.f_dc = (uint32_t *)f_dc; a.f_rest = (uint32_t *)f_rest;
    a.opacity = (uint32_t *)opacity; a.scaling = (uint32_t *)scaling; a.rotation = (uint32_t *)rotation;
    hipLaunchKernelGGL(rows_unpack_kernel, dim3((P + ROWS_TILE - 1) / ROWS_TILE), dim3(256), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(GSR_ERR_HIP, "rows unpack launch: %s (%d)", hipGetErrorString(e), (int)e);
    return GSR_OK;
}

int32_t gsr_rows_grad_pack(gsr_stream_t stream, int32_t P, int32_t D, int32_t B, const float *const *arenas, float *grad_rows) {
    if (rows_sizes("gsr_rows_grad_pack", P, D) != GSR_OK) return GSR_ERR_INVALID_ARGUMENT;
    if (B < 1 || B > GSR_ROWS_MAX_B) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_rows_grad_pack: B=%d not in 1..%d", B, GSR_ROWS_MAX_B);
    if (P == 0) return GSR_OK;                       // likewise
    if (!arenas) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_rows_grad_pack: arenas (host array) required");
    if (!grad_rows) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_rows_grad_pack: grad_rows is NULL");
    const int K = rows_K(D);
    const size_t arena_floats = (size_t)P * (3 * K + 11);
    RowsPackArgs a;
    for (int b = 0; b < GSR_ROWS_MAX_B; b++) a.arena[b] = nullptr;
    for (int b = 0; b < B; b++) {
        if (!arenas[b]) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_rows_grad_pack: arenas[%d] is NULL", b);
        if ((uintptr_t)arenas[b] & 3) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_rows_grad_pack: arenas[%d] is not 4-byte aligned", b);
        if (ranges_meet(grad_rows, (size_t)P * D, arenas[b], arena_floats))
            return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_rows_grad_pack: grad_rows overlaps arenas[%d]", b);
        a.arena[b] = arenas[b];
    }
    a.P = P; a.D = D; a.K = K; a.B = B; a.vec = ((uintptr_t)grad_rows & 15) == 0;
    a.grad_rows = grad_rows;
    hipLaunchKernelGGL(rows_grad_pack_kernel, dim3((P + ROWS_TILE - 1) / ROWS_TILE), dim3(256), 0, (hipStream_t)stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(GSR_ERR_HIP, "rows grad pack launch: %s (%d)", hipGetErrorString(e), (int)e);
    return GSR_OK;
}

}  // extern "C"
