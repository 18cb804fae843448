// chamfer.hip -- Chamfer distance between two sets of D-dimensional rows, forward and backward (include/gsr_chamfer.h).
//
// The reference's third native dependency, `chamfer_distance.ChamferDistance` (train_stacked_transformer.py:24,184,193-196):
// every optimisation step calls it on rows of 26 floats (flattened Gaussians) and back-propagates through it.  Semantics restated
// from that call site (the package itself is not in the snapshot): squared Euclidean distance over ALL D features, nearest row of
// the other set and its index, both ways.
//
// gfx950 shape.  The reference's sizes (B = 1, N ~ M ~ 5 000 - 20 000, D = 26) give only 80 - 300 query waves, so the CANDIDATE set
// is split over workgroups as well: workgroup (query block, chunk, direction) holds two query rows per lane in registers, streams
// its chunk of the other set through a 16 KB LDS tile that every lane reads at the same address (broadcast, no bank conflicts), and
// merges its partial minimum with one 64-bit atomicMin on (distance bits << 32 | index).  Distances are >= +0, so their bits order
// like the values, NaN bits sort above +inf, and the lower index wins among equal bits: the tie rule and run-to-run determinism
// come with the merge.  Distances are sums of (a - b)^2 in float32, k ascending -- never |a|^2 + |b|^2 - 2ab, whose cancellation
// breaks the (D + 3) ulp bound the tests assert -- so there is no MFMA formulation.
#include <stdint.h>

#include "../../include/gsr_chamfer.h"
#include "gsr_host.h"
#include "gsr_internal.h"

namespace gsr {

#define CH_THREADS 256
#define CH_ROWS 2                    // query rows per lane: halves the LDS reads per distance
#define CH_QBLOCK (CH_THREADS * CH_ROWS)
#define CH_LDS_FLOATS 4096           // the candidate tile
#define CH_MIN_CHUNK 64              // candidates per workgroup, at least
#define CH_TARGET_BLOCKS 2048        // workgroups of 4 waves the split aims at (256 CUs x 8)
#define CH_NAN_BITS 0x7fc00000u

// compile-time row widths: 3 and 26 exact (the classic and the reference's shape); any other D runs in the next wider one, both
// sides padded with zeros (a padded column adds (0 - 0)^2 = +0: the sum is unchanged bit for bit)
template <int DP> struct ChShape {
    static constexpr int DPL = (DP + 3) & ~3;                   // LDS row stride: float4 reads
    static constexpr int TILE = CH_LDS_FLOATS / DPL >= 1024 ? 1024 : CH_LDS_FLOATS / DPL >= 512 ? 512 : CH_LDS_FLOATS / DPL >= 256 ? 256
                              : CH_LDS_FLOATS / DPL >= 128 ? 128 : 64;
};

struct ChamferFwdArgs {
    int B, N, M, D;
    int nqb;                 // query blocks per batch element = ceil(max(N, M) / CH_QBLOCK)
    int chunk1, chunk2;      // candidates per workgroup: of x2 (direction 0: queries x1), of x1 (direction 1)
    const float *x1, *x2;
    unsigned long long *keys;   // [B * N] direction 0, then [B * M] direction 1; all ones on entry
};

template <int DP>
__global__ __launch_bounds__(CH_THREADS) void chamfer_fwd_kernel(ChamferFwdArgs a) {
    constexpr int DPL = ChShape<DP>::DPL, TILE = ChShape<DP>::TILE;
    __shared__ float4 tile4[TILE * DPL / 4];
    float *tile = reinterpret_cast<float *>(tile4);
    const int dir = blockIdx.z;
    const int b = blockIdx.x / a.nqb, qb = blockIdx.x % a.nqb;
    const int nq = dir ? a.M : a.N, nc = dir ? a.N : a.M, D = a.D;
    const int chunk = dir ? a.chunk2 : a.chunk1;
    const long long c0 = (long long)blockIdx.y * chunk;
    if ((long long)qb * CH_QBLOCK >= nq || c0 >= nc) return;          // uniform over the workgroup
    const int c1 = (int)min((long long)nc, c0 + chunk);
    const float *__restrict__ Q = (dir ? a.x2 : a.x1) + (size_t)b * nq * D;
    const float *__restrict__ C = (dir ? a.x1 : a.x2) + (size_t)b * nc * D;
    unsigned long long *keys = a.keys + (dir ? (size_t)a.B * a.N : 0) + (size_t)b * nq;

    float q[CH_ROWS][DP];
    uint32_t best[CH_ROWS], bidx[CH_ROWS];
    int qi[CH_ROWS];
#pragma unroll
    for (int r = 0; r < CH_ROWS; r++) {
        qi[r] = qb * CH_QBLOCK + r * CH_THREADS + (int)threadIdx.x;
        const int row = min(qi[r], nq - 1);                           // a lane past the end computes a copy and stores nothing
#pragma unroll
        for (int k = 0; k < DP; k++) q[r][k] = k < D ? Q[(size_t)row * D + k] : 0.f;
        best[r] = 0xffffffffu; bidx[r] = 0u;
    }
    for (int e = threadIdx.x; e < TILE * DPL; e += CH_THREADS) tile[e] = 0.f;     // the padding columns stay zero

    for (int j0 = (int)c0; j0 < c1; j0 += TILE) {
        const int nt = min(TILE, c1 - j0);
        __syncthreads();
        for (int e = threadIdx.x; e < nt * D; e += CH_THREADS) {      // coalesced: the tile is contiguous in memory
            const int j = e / D, k = e - j * D;
            tile[j * DPL + k] = C[(size_t)j0 * D + e];
        }
        __syncthreads();
#pragma unroll 2
        for (int j = 0; j < nt; j++) {
            float c[DPL];
#pragma unroll
            for (int v = 0; v < DPL / 4; v++) {
                const float4 t = tile4[j * (DPL / 4) + v];
                c[4 * v] = t.x; c[4 * v + 1] = t.y; c[4 * v + 2] = t.z; c[4 * v + 3] = t.w;
            }
#pragma unroll
            for (int r = 0; r < CH_ROWS; r++) {
                float d = 0.f;
#pragma unroll
                for (int k = 0; k < DP; k++) { const float t = q[r][k] - c[k]; d += t * t; }
                // d is +0, positive, +inf or NaN: with the sign bit cleared every NaN compares above +inf as an integer
                const uint32_t u = __float_as_uint(d) & 0x7fffffffu;
                const bool w = u < best[r];                           // strict: the first of equal distances stays
                best[r] = w ? u : best[r];
                bidx[r] = w ? (uint32_t)(j0 + j) : bidx[r];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < CH_ROWS; r++)
        if (qi[r] < nq) {
            // one canonical NaN with index 0: a row whose every candidate is NaN ends as (NaN, 0) whatever the chunks
            const unsigned long long key = best[r] > 0x7f800000u ? ((unsigned long long)CH_NAN_BITS << 32)
                                                                  : ((unsigned long long)best[r] << 32 | bidx[r]);
            atomicMin(&keys[qi[r]], key);
        }
}

__global__ __launch_bounds__(256) void chamfer_unpack_kernel(size_t n, const unsigned long long *__restrict__ keys,
                                                             size_t split, float *__restrict__ dist1, int32_t *__restrict__ idx1,
                                                             float *__restrict__ dist2, int32_t *__restrict__ idx2) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const unsigned long long k = keys[i];
        const float d = __uint_as_float((uint32_t)(k >> 32));
        const int32_t j = (int32_t)(uint32_t)k;
        if (i < split) { dist1[i] = d; idx1[i] = j; } else { dist2[i - split] = d; idx2[i - split] = j; }
    }
}

template <int DP>
static hipError_t launch_fwd_t(const ChamferFwdArgs &a, int nchunk, hipStream_t s) {
    hipLaunchKernelGGL(chamfer_fwd_kernel<DP>, dim3((unsigned)a.nqb * (unsigned)a.B, (unsigned)nchunk, 2), dim3(CH_THREADS), 0, s, a);
    return hipGetLastError();
}

// B, N, M >= 1 and 1 <= D <= 64 (checked by gsr_chamfer_forward); ws holds 8 B (N + M) bytes
static hipError_t launch_chamfer_forward(int B, int N, int M, int D, const float *x1, const float *x2, float *dist1, float *dist2,
                                  int32_t *idx1, int32_t *idx2, void *ws, hipStream_t s) {
    const size_t nkeys = (size_t)B * ((size_t)N + (size_t)M);
    hipError_t e = hipMemsetAsync(ws, 0xff, nkeys * 8, s);
    if (e != hipSuccess) return e;
    ChamferFwdArgs a;
    a.B = B; a.N = N; a.M = M; a.D = D; a.x1 = x1; a.x2 = x2; a.keys = (unsigned long long *)ws;
    const int big = N > M ? N : M;
    a.nqb = (big + CH_QBLOCK - 1) / CH_QBLOCK;
    // split the candidates until the launch has CH_TARGET_BLOCKS workgroups, but keep CH_MIN_CHUNK rows per workgroup
    long long nchunk = CH_TARGET_BLOCKS / ((long long)a.nqb * B * 2);
    const long long most = ((long long)big + CH_MIN_CHUNK - 1) / CH_MIN_CHUNK;
    if (nchunk > most) nchunk = most;
    if (nchunk > 65535) nchunk = 65535;
    if (nchunk < 1) nchunk = 1;
    a.chunk1 = (int)(((long long)M + nchunk - 1) / nchunk);
    a.chunk2 = (int)(((long long)N + nchunk - 1) / nchunk);
    if (a.chunk1 < CH_MIN_CHUNK) a.chunk1 = CH_MIN_CHUNK;      // the smaller set: its surplus workgroups return at once
    if (a.chunk2 < CH_MIN_CHUNK) a.chunk2 = CH_MIN_CHUNK;
    if (D == 3) e = launch_fwd_t<3>(a, (int)nchunk, s);
    else if (D == 26) e = launch_fwd_t<26>(a, (int)nchunk, s);
    else if (D <= 4) e = launch_fwd_t<4>(a, (int)nchunk, s);
    else if (D <= 8) e = launch_fwd_t<8>(a, (int)nchunk, s);
    else if (D <= 16) e = launch_fwd_t<16>(a, (int)nchunk, s);
    else if (D <= 32) e = launch_fwd_t<32>(a, (int)nchunk, s);
    else if (D <= 48) e = launch_fwd_t<48>(a, (int)nchunk, s);
    else e = launch_fwd_t<64>(a, (int)nchunk, s);
    if (e != hipSuccess) return e;
    const size_t blocks = (nkeys + 255) / 256;
    hipLaunchKernelGGL(chamfer_unpack_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, s, nkeys,
                       (const unsigned long long *)ws, (size_t)B * N, dist1, idx1, dist2, idx2);
    return hipGetLastError();
}

// ---- backward ----
// dL/dx1[b,i] = 2 g1[b,i] (x1[b,i] - x2[b,idx1[b,i]])  +  sum over {j : idx2[b,j] = i} of 2 g2[b,j] (x1[b,i] - x2[b,j]), and the
// same with the roles swapped.  The first (direct) term is a plain store per element and writes the WHOLE buffer (zeros where g is
// NULL or the index is out of range); the second is scattered with float atomics by a second kernel behind it on the stream.
struct ChamferBwdArgs {
    int B, N, M, D;
    const float *x1, *x2;
    const int32_t *idx1, *idx2;
    const float *g1, *g2;
    float *dx1, *dx2;        // NULL: not wanted
    size_t n1, n2;           // elements the kernel covers for x1, x2 (0: side skipped)
};

// one element (row, k) per lane: neighbouring lanes read and write neighbouring floats of a row
__global__ __launch_bounds__(256) void chamfer_bwd_direct_kernel(ChamferBwdArgs a) {
    const size_t total = a.n1 + a.n2;
    for (size_t e0 = (size_t)blockIdx.x * 256 + threadIdx.x; e0 < total; e0 += (size_t)gridDim.x * 256) {
        const bool second = e0 >= a.n1;
        const size_t e = second ? e0 - a.n1 : e0;
        const int nq = second ? a.M : a.N, nc = second ? a.N : a.M;
        const float *xq = second ? a.x2 : a.x1, *xc = second ? a.x1 : a.x2, *g = second ? a.g2 : a.g1;
        const int32_t *idx = second ? a.idx2 : a.idx1;
        float *out = second ? a.dx2 : a.dx1;
        const size_t row = e / (size_t)a.D;              // b * nq + i
        const int k = (int)(e - row * a.D);
        const size_t b = row / (size_t)nq;
        float v = 0.f;
        if (g) {
            const int32_t j = idx[row];
            if (j >= 0 && j < nc) v = 2.f * g[row] * (xq[e] - xc[(b * nc + (size_t)j) * a.D + k]);
        }
        out[e] = v;
    }
}

// n1 / n2 here: elements of the SOURCE side whose term lands in the other side's gradient
//   e < n1: row i of x1 (with g1, idx1) adds 2 g1[i] (x2[j] - x1[i]) into dx2[j];  then row j of x2 (g2, idx2) into dx1[idx2[j]]
__global__ __launch_bounds__(256) void chamfer_bwd_scatter_kernel(ChamferBwdArgs a) {
    const size_t total = a.n1 + a.n2;
    for (size_t e0 = (size_t)blockIdx.x * 256 + threadIdx.x; e0 < total; e0 += (size_t)gridDim.x * 256) {
        const bool second = e0 >= a.n1;
        const size_t e = second ? e0 - a.n1 : e0;
        const int nq = second ? a.M : a.N, nc = second ? a.N : a.M;
        const float *xq = second ? a.x2 : a.x1, *xc = second ? a.x1 : a.x2, *g = second ? a.g2 : a.g1;
        const int32_t *idx = second ? a.idx2 : a.idx1;
        float *out = second ? a.dx1 : a.dx2;
        const size_t row = e / (size_t)a.D;
        const int k = (int)(e - row * a.D);
        const size_t b = row / (size_t)nq;
        const int32_t j = idx[row];
        if (j < 0 || j >= nc) continue;                  // an index that is not one: skipped, not followed
        const size_t t = (b * nc + (size_t)j) * a.D + k;
        atomicAdd(&out[t], 2.f * g[row] * (xc[t] - xq[e]));
    }
}

static unsigned grid_for(size_t n) { const size_t b = (n + 255) / 256; return (unsigned)(b < 8192 ? b : 8192); }

static hipError_t launch_chamfer_backward(int B, int N, int M, int D, const float *x1, const float *x2, const int32_t *idx1, const int32_t *idx2,
                                   const float *g1, const float *g2, float *dx1, float *dx2, hipStream_t s) {
    ChamferBwdArgs a;
    a.B = B; a.N = N; a.M = M; a.D = D; a.x1 = x1; a.x2 = x2; a.idx1 = idx1; a.idx2 = idx2; a.g1 = g1; a.g2 = g2; a.dx1 = dx1; a.dx2 = dx2;
    const size_t e1 = (size_t)B * N * D, e2 = (size_t)B * M * D;
    a.n1 = dx1 ? e1 : 0; a.n2 = dx2 ? e2 : 0;
    if (a.n1 + a.n2 == 0) return hipSuccess;
    hipLaunchKernelGGL(chamfer_bwd_direct_kernel, dim3(grid_for(a.n1 + a.n2)), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    a.n1 = (dx2 && g1) ? e1 : 0; a.n2 = (dx1 && g2) ? e2 : 0;
    if (a.n1 + a.n2 == 0) return hipSuccess;
    hipLaunchKernelGGL(chamfer_bwd_scatter_kernel, dim3(grid_for(a.n1 + a.n2)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace gsr

using namespace gsr;

extern "C" {

// ---- chamfer_distance.ChamferDistance equivalent (include/gsr_chamfer.h) ----
// 0: nothing to do, 1: work, < 0: invalid (message set)
static int chamfer_sizes(const char *who, int32_t B, int32_t N, int32_t M, int32_t D) {
    if (B < 0 || N < 0 || M < 0) { fail(GSR_ERR_INVALID_ARGUMENT, "%s: negative size (B=%d N=%d M=%d)", who, B, N, M); return -1; }
    if (D < 1 || D > 64) { fail(GSR_ERR_INVALID_ARGUMENT, "%s: D=%d not in 1..64", who, D); return -1; }
    if (B == 0 || (N == 0 && M == 0)) return 0;
    if (N == 0 || M == 0) { fail(GSR_ERR_INVALID_ARGUMENT, "%s: N=%d, M=%d: an empty set has no nearest neighbour", who, N, M); return -1; }
    if (((long long)(N > M ? N : M) + 511) / 512 * B > 0x7fffffffLL) { fail(GSR_ERR_INVALID_ARGUMENT, "%s: B * max(N, M) too large", who); return -1; }
    return 1;
}

int32_t gsr_chamfer_workspace(int32_t B, int32_t N, int32_t M, size_t *bytes) {
    if (B < 0 || N < 0 || M < 0 || !bytes) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_chamfer_workspace: bad argument");
    *bytes = (size_t)8 * (size_t)B * ((size_t)N + (size_t)M);
    return GSR_OK;
}

int32_t gsr_chamfer_forward(gsr_stream_t stream, int32_t B, int32_t N, int32_t M, int32_t D, const float *x1, const float *x2,
                            float *dist1, float *dist2, int32_t *idx1, int32_t *idx2, void *ws, size_t ws_bytes) {
    const int k = chamfer_sizes("gsr_chamfer_forward", B, N, M, D);
    if (k <= 0) return k < 0 ? GSR_ERR_INVALID_ARGUMENT : GSR_OK;
    if (!x1 || !x2 || !dist1 || !dist2 || !idx1 || !idx2 || !ws) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_chamfer_forward: null pointer");
    const size_t need = (size_t)8 * (size_t)B * ((size_t)N + (size_t)M);
    if (ws_bytes < need) return fail(GSR_ERR_WORKSPACE, "chamfer workspace %zu < %zu", ws_bytes, need);
    HIP_TRY(launch_chamfer_forward(B, N, M, D, x1, x2, dist1, dist2, idx1, idx2, ws, (hipStream_t)stream), "chamfer forward launch");
    return GSR_OK;
}

int32_t gsr_chamfer_backward(gsr_stream_t stream, int32_t B, int32_t N, int32_t M, int32_t D, const float *x1, const float *x2,
                             const int32_t *idx1, const int32_t *idx2, const float *g1, const float *g2, float *dx1, float *dx2) {
    const int k = chamfer_sizes("gsr_chamfer_backward", B, N, M, D);
    if (k <= 0) return k < 0 ? GSR_ERR_INVALID_ARGUMENT : GSR_OK;
    if (!x1 || !x2 || !idx1 || !idx2) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_chamfer_backward: null pointer");
    HIP_TRY(launch_chamfer_backward(B, N, M, D, x1, x2, idx1, idx2, g1, g2, dx1, dx2, (hipStream_t)stream), "chamfer backward launch");
    return GSR_OK;
}

}  // extern "C"
