// ssim_loss.hip -- fused training loss  (1-lambda) * L1 + lambda * (1 - SSIM)  and its gradient.
//
// "Next" row 8f-1 of SURVEY.md: the loss that produces dL/dimage for the rasterizer backward.  Follows the
// reference's utils/loss_utils.py:17-63 (l1_loss; ssim: 11x11 Gaussian window sigma 1.5 built as the
// outer product of a normalised 1-D kernel, zero padding 5, C1 = 0.01^2, C2 = 0.03^2, mean over all
// C*H*W map entries) combined as in train.py:91-92.  The reference runs it as five grouped 11x11
// convolutions + elementwise ops (and their autograd); here ONE kernel per direction:
//   forward : 16x16 tile + 5-pixel halo of both images staged in LDS, separable 11-tap blur of the five
//             moments (x, y, x^2, y^2, xy), SSIM map value, the three partial-derivative maps
//             (df/dmu1, df/dm11, df/dm12) written for the backward, deterministic two-stage sum.
//   backward: separable blur of the three derivative maps (zero outside the image) and
//             dL/dx = (1-lambda)/N sign(x-y) - lambda/N (G*A + 2x G*B + y G*C), scaled by the upstream scalar.
// HBM-bound: forward reads 8 and writes 12 bytes per map entry, backward reads 20 and writes 4.
//
// The multi-view form (gsr_views_loss_*, include/gsr_loss.h; the image loss of train_stacked_transformer.py:203-222) runs the same
// tile code over B views of 3 planes each: the plane index b * 3 + c is the grid's z, the B prediction / target / gradient pointers
// travel by value in the kernel arguments (GSR_VIEWS_LOSS_MAX_B views per launch, the launcher loops over larger B), the sanitising
// s(x) = clamp(nan_to_num(x), 0, 1) is applied while the tile is staged into LDS, and the backward masks its final store with the
// raw pixel it reads anyway.  A third partial, sum (s(x) - s(y))^2, gives the per-view PSNR.  Same traffic: forward reads 8 and
// writes 12 bytes per map entry (plus 12 bytes per 256-entry tile of partials), backward reads 20 and writes 4 (0 for a view
// whose gradient pointer is NULL: its blocks return at once).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gsr_loss.h"
#include "gsr_host.h"
#include "gsr_internal.h"

namespace gsr {

#define SSIM_R 5
#define SSIM_K 11
#define SSIM_T 16
#define SSIM_HALO (SSIM_T + 2 * SSIM_R)   // 26
#define SSIM_C1 (0.01 * 0.01)
#define SSIM_C2 (0.03 * 0.03)
// The moments and everything derived from them are carried in float64.  In float32 the variance s11 - m1*m1 of a flat or smooth
// patch of level c is the difference of two numbers of size c^2 and comes out with an absolute error of ~2^-24 c^2, which stands
// against C2 = 9e-4 alone: 1e-4 relative on SSIM and, through the three derivative maps of size 1/C2 that cancel in the backward
// pass, on the gradient (tests/test_gpu_loss_edges.py: flat backgrounds, one bright pixel).  The images, the derivative maps and
// the gradient stay float32 in memory: the kernels remain bound by the same HBM traffic.

struct SsimWeights { float g[SSIM_K]; };

// float32 1-D kernel exactly as utils/loss_utils.py:23-25 builds it: exp() in double, stored as float32,
// divided by the float32 sum
// exact_sum: the normaliser is the sum of the 11 float32 numbers rounded ONCE, 3.7592328, which is what torch's sum gives
// (loss._window, the reference); added one by one in float32 it comes out one place lower, 3.7592325, and the single-image
// kernels keep that (tests/test_aux_references.py: one place of the normaliser moves SSIM of smooth images by ~1e-5, and
// 1 - SSIM of noise by 4e-7 relative: twice what the multi-view tests allow the loss against torch's float64).
static SsimWeights make_weights(bool exact_sum = false) {
    SsimWeights w;
    float s = 0.f;
    double sd = 0.0;
    for (int i = 0; i < SSIM_K; i++) {
        const double d = (double)(i - SSIM_K / 2);
        w.g[i] = (float)exp(-(d * d) / (2.0 * 1.5 * 1.5));
        s += w.g[i];
        sd += (double)w.g[i];
    }
    if (exact_sum) s = (float)sd;
    for (int i = 0; i < SSIM_K; i++) w.g[i] = w.g[i] / s;
    return w;
}

// The window of the multi-view kernels.  The reference's 2-D window is g g^T with every one of its 121 products rounded to float32
// (utils/loss_utils.py:28-31, loss._window), so it is not quite separable and sums to 1 - 6.94e-8 where the exact products of the
// same g sum to 1 - 6.24e-8.  A window sum of 1 + e moves sigma12 = E[xy] - mu1 mu2 by -e mu1 mu2 in every map entry alike: for
// images of level 0.5 those 7e-9 of difference move the SSIM mean by ~1e-8 absolute, which does not average out and is 3e-7
// of the SSIM of uncorrelated noise (0.03).  So the separable blur runs with u = r / sqrt(S) in float64, r the row sums of the
// reference's float32 window (it is symmetric: its column sums too) and S its total: u u^T has the reference window's total and
// marginals exactly; what remains is a zero-sum, zero-marginal difference of <= 3e-8 of the largest tap.
struct SsimWeightsD { double g[SSIM_K]; };
static SsimWeightsD make_view_weights() {
    const SsimWeights w = make_weights(true);
    SsimWeightsD u;
    double total = 0.0;
    for (int i = 0; i < SSIM_K; i++) {
        double row = 0.0;
        for (int j = 0; j < SSIM_K; j++) {
            const float prod = w.g[i] * w.g[j];          // one float32 rounding per entry, as the reference's g.mm(g.t())
            row += (double)prod;
        }
        u.g[i] = row;
        total += row;
    }
    const double inv = 1.0 / sqrt(total);
    for (int i = 0; i < SSIM_K; i++) u.g[i] *= inv;
    return u;
}

// ---- tile code shared by the single-image and the multi-view kernels ----
typedef float SsimTile[SSIM_HALO][SSIM_HALO + 1];
typedef double SsimRows[SSIM_HALO][SSIM_T + 1];

// s(x) = clamp(nan_to_num(x), 0, 1): NaN -> 0, +inf -> 1, -inf -> 0
__device__ __forceinline__ float ssim_sanitize(float x) { return x != x ? 0.f : fminf(fmaxf(x, 0.f), 1.f); }

// 16x16 tile + 5-pixel halo of one plane of both images into LDS; zero padding (conv2d padding = 5)
template <bool SAN>
__device__ __forceinline__ void ssim_stage_pair(SsimTile sx, SsimTile sy, const float *__restrict__ img, const float *__restrict__ gt,
                                                int H, int W, int x0, int y0, int tid) {
    for (int i = tid; i < SSIM_HALO * SSIM_HALO; i += 256) {
        const int r = i / SSIM_HALO, q = i - r * SSIM_HALO;
        const int y = y0 + r - SSIM_R, x = x0 + q - SSIM_R;
        const bool in = x >= 0 && x < W && y >= 0 && y < H;
        float xv = in ? img[(size_t)y * W + x] : 0.f;
        float yv = in ? gt[(size_t)y * W + x] : 0.f;
        if (SAN) { xv = ssim_sanitize(xv); yv = ssim_sanitize(yv); }
        sx[r][q] = xv;
        sy[r][q] = yv;
    }
}

struct SsimMoments { double m1, m2, s11, s22, s12; };

// separable 11-tap blur of x, y, x^2, y^2, xy at this thread's pixel (lx, ly); the tile must be staged (no barrier needed before)
template <class Weights /*SsimWeights or SsimWeightsD*/>
__device__ __forceinline__ SsimMoments ssim_blur_moments(const SsimTile sx, const SsimTile sy, SsimRows *hz /*[5]*/,
                                                         const Weights &wts, int tid, int lx, int ly) {
    __syncthreads();
    for (int i = tid; i < SSIM_HALO * SSIM_T; i += 256) {            // horizontal pass on 26 rows x 16 columns
        const int r = i >> 4, q = i & 15;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
#pragma unroll
        for (int k = 0; k < SSIM_K; k++) {
            const double xv = sx[r][q + k], yv = sy[r][q + k], w = wts.g[k];
            a0 += w * xv; a1 += w * yv; a2 += w * (xv * xv); a3 += w * (yv * yv); a4 += w * (xv * yv);
        }
        hz[0][r][q] = a0; hz[1][r][q] = a1; hz[2][r][q] = a2; hz[3][r][q] = a3; hz[4][r][q] = a4;
    }
    __syncthreads();
    SsimMoments m = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < SSIM_K; k++) {
        const double w = wts.g[k];
        m.m1 += w * hz[0][ly + k][lx]; m.m2 += w * hz[1][ly + k][lx]; m.s11 += w * hz[2][ly + k][lx];
        m.s22 += w * hz[3][ly + k][lx]; m.s12 += w * hz[4][ly + k][lx];
    }
    return m;
}

// SSIM map entry; the three partial-derivative maps go to dA (d f / d mu1, total), dB (d f / d E[x^2]), dC (d f / d E[xy])
__device__ __forceinline__ float ssim_entry(const SsimMoments &m, float *__restrict__ dA, float *__restrict__ dB, float *__restrict__ dC) {
    const double m1 = m.m1, m2 = m.m2;
    const double a1 = 2.0 * m1 * m2 + SSIM_C1, sig12 = m.s12 - m1 * m2, a2 = 2.0 * sig12 + SSIM_C2;
    const double b1 = m1 * m1 + m2 * m2 + SSIM_C1, b2 = (m.s11 - m1 * m1) + (m.s22 - m2 * m2) + SSIM_C2;
    const double invD = 1.0 / (b1 * b2);
    const double f = a1 * a2 * invD;
    *dA = (float)((2.0 * m2 * (a2 - a1) - f * 2.0 * m1 * (b2 - b1)) * invD);
    *dB = (float)(-f / b2);
    *dC = (float)(2.0 * a1 * invD);
    return (float)f;
}

// sum over the 256 threads of a block in a fixed order (deterministic); the result is valid in thread 0.  red: 4 floats of LDS.
__device__ __forceinline__ float ssim_block_sum(float v, float *red, int tid) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void l1_ssim_fwd_kernel(int C, int H, int W, const float *__restrict__ img,
                                                          const float *__restrict__ gt, SsimWeights wts,
                                                          float *__restrict__ dmaps /*[3][C][H][W]*/,
                                                          float *__restrict__ partial /*[blocks][2]*/) {
    __shared__ SsimTile sx, sy;
    __shared__ SsimRows hz[5];
    __shared__ float red[2][4];
    const int tid = threadIdx.x, lx = tid & 15, ly = tid >> 4;
    const int c = blockIdx.z, x0 = blockIdx.x * SSIM_T, y0 = blockIdx.y * SSIM_T;
    const size_t plane = (size_t)H * W, base = (size_t)c * plane;
    ssim_stage_pair<false>(sx, sy, img + base, gt + base, H, W, x0, y0, tid);
    const SsimMoments m = ssim_blur_moments(sx, sy, hz, wts, tid, lx, ly);
    const int x = x0 + lx, y = y0 + ly;
    const bool in = x < W && y < H;
    float l1 = 0.f, ss = 0.f;
    if (in) {
        const size_t p = base + (size_t)y * W + x, CHW = (size_t)C * plane;
        ss = ssim_entry(m, dmaps + p, dmaps + CHW + p, dmaps + 2 * CHW + p);
        l1 = fabsf(sx[ly + SSIM_R][lx + SSIM_R] - sy[ly + SSIM_R][lx + SSIM_R]);
    }
    l1 = ssim_block_sum(l1, red[0], tid);
    ss = ssim_block_sum(ss, red[1], tid);
    if (tid == 0) {
        const size_t b = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partial[2 * b] = l1;
        partial[2 * b + 1] = ss;
    }
}

// out[0] = loss, out[1] = L1 mean, out[2] = SSIM mean
__global__ __launch_bounds__(1024) void l1_ssim_finish_kernel(int nblocks, double inv_n, float lambda,
                                                              const float *__restrict__ partial, float *__restrict__ out) {
    __shared__ double r0[16], r1[16];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 1024) { a += (double)partial[2 * i]; b += (double)partial[2 * i + 1]; }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) { a += __shfl_xor(a, m); b += __shfl_xor(b, m); }
    if ((threadIdx.x & 63) == 0) { r0[threadIdx.x >> 6] = a; r1[threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sa = 0.0, sb = 0.0;
        for (int i = 0; i < 16; i++) { sa += r0[i]; sb += r1[i]; }
        const float l1 = (float)(sa * inv_n), ssim = (float)(sb * inv_n);
        out[0] = (1.f - lambda) * l1 + lambda * (1.f - ssim);
        out[1] = l1;
        out[2] = ssim;
    }
}

// the three derivative maps of one plane (zero outside the image) into LDS, then their separable blur at this thread's pixel
// (the plane's d f / d mu1 map starts at dm[base]; the other two lie `stride` and 2 `stride` floats behind it)
struct SsimBlurred { double gA, gB, gC; };
template <class Weights>
__device__ __forceinline__ SsimBlurred ssim_blur_dmaps(SsimTile *sm /*[3]*/, SsimRows *hz /*[3]*/, const float *__restrict__ dm, size_t base,
                                                       size_t stride, const Weights &wts, int H, int W, int x0, int y0, int tid, int lx,
                                                       int ly) {
    for (int i = tid; i < SSIM_HALO * SSIM_HALO; i += 256) {
        const int r = i / SSIM_HALO, q = i - r * SSIM_HALO;
        const int y = y0 + r - SSIM_R, x = x0 + q - SSIM_R;
        const bool in = x >= 0 && x < W && y >= 0 && y < H;
        const size_t p = base + (size_t)(in ? y : 0) * W + (in ? x : 0);
        sm[0][r][q] = in ? dm[p] : 0.f;
        sm[1][r][q] = in ? dm[stride + p] : 0.f;
        sm[2][r][q] = in ? dm[2 * stride + p] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < SSIM_HALO * SSIM_T; i += 256) {
        const int r = i >> 4, q = i & 15;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
        for (int k = 0; k < SSIM_K; k++) {
            const double w = wts.g[k];
            a0 += w * sm[0][r][q + k]; a1 += w * sm[1][r][q + k]; a2 += w * sm[2][r][q + k];
        }
        hz[0][r][q] = a0; hz[1][r][q] = a1; hz[2][r][q] = a2;
    }
    __syncthreads();
    double gA = 0.0, gB = 0.0, gC = 0.0;
#pragma unroll
    for (int k = 0; k < SSIM_K; k++) {
        const double w = wts.g[k];
        gA += w * hz[0][ly + k][lx]; gB += w * hz[1][ly + k][lx]; gC += w * hz[2][ly + k][lx];
    }
    return {gA, gB, gC};
}

__global__ __launch_bounds__(256) void l1_ssim_bwd_kernel(int C, int H, int W, const float *__restrict__ img,
                                                          const float *__restrict__ gt, SsimWeights wts,
                                                          const float *__restrict__ dmaps, float lambda, float inv_n,
                                                          const float *__restrict__ grad_loss /*[1] or null*/,
                                                          float *__restrict__ grad_img) {
    __shared__ SsimTile sm[3];
    __shared__ SsimRows hz[3];
    const int tid = threadIdx.x, lx = tid & 15, ly = tid >> 4;
    const int c = blockIdx.z, x0 = blockIdx.x * SSIM_T, y0 = blockIdx.y * SSIM_T;
    const size_t plane = (size_t)H * W, base = (size_t)c * plane, CHW = (size_t)C * plane;
    const SsimBlurred g = ssim_blur_dmaps(sm, hz, dmaps, base, CHW, wts, H, W, x0, y0, tid, lx, ly);
    const double gA = g.gA, gB = g.gB, gC = g.gC;
    const int x = x0 + lx, y = y0 + ly;
    if (x < W && y < H) {
        const size_t p = base + (size_t)y * W + x;
        const float xv = img[p], yv = gt[p];
        const float d = xv - yv;
        const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);           // torch.abs backward: sign(0) = 0
        const float up = grad_loss ? grad_loss[0] : 1.f;
        grad_img[p] = (float)((double)up * inv_n * ((1.0 - lambda) * sgn - (double)lambda * (gA + 2.0 * xv * gB + (double)yv * gC)));
    }
}

static hipError_t launch_l1_ssim_forward(int C, int H, int W, const float *img, const float *gt, float lambda, float *dmaps,
                                  float *partial, float *out, hipStream_t s) {
    const SsimWeights w = make_weights();
    const dim3 grid((W + SSIM_T - 1) / SSIM_T, (H + SSIM_T - 1) / SSIM_T, C);
    hipLaunchKernelGGL(l1_ssim_fwd_kernel, grid, dim3(256), 0, s, C, H, W, img, gt, w, dmaps, partial);
    const int nblocks = (int)(grid.x * grid.y * grid.z);
    hipLaunchKernelGGL(l1_ssim_finish_kernel, dim3(1), dim3(1024), 0, s, nblocks, 1.0 / ((double)C * H * W), lambda, partial, out);
    return hipGetLastError();
}

static hipError_t launch_l1_ssim_backward(int C, int H, int W, const float *img, const float *gt, float lambda, const float *dmaps,
                                   const float *grad_loss, float *grad_img, hipStream_t s) {
    const SsimWeights w = make_weights();
    const dim3 grid((W + SSIM_T - 1) / SSIM_T, (H + SSIM_T - 1) / SSIM_T, C);
    hipLaunchKernelGGL(l1_ssim_bwd_kernel, grid, dim3(256), 0, s, C, H, W, img, gt, w, dmaps, lambda,
                       (float)(1.0 / ((double)C * H * W)), grad_loss, grad_img);
    return hipGetLastError();
}

// ---- B views in one launch (gsr_views_loss_*) ----
// workspace: dmaps [3][B*3][H][W] | partial [B*3*tiles][3] | view_sums [B][3] double | ticket (one int on a line of its own)
struct ViewsWs { float *dmaps, *partial; double *view_sums; int *ticket; size_t total_bytes; };
static inline size_t ssim_tiles(int H, int W) { return (size_t)((W + SSIM_T - 1) / SSIM_T) * ((H + SSIM_T - 1) / SSIM_T); }      // blocks per image plane
static inline ViewsWs views_carve(void *ws, int B, int H, int W) {
    Bump w = {(char *)ws, 0};
    float *const dmaps = w.take<float>((size_t)9 * B * H * W), *const partial = w.take<float>((size_t)9 * B * ssim_tiles(H, W));
    double *const view_sums = w.take<double>((size_t)3 * B); int *const ticket = w.take<int>(1);      // the ticket's piece is a 256-byte line: nothing shares it
    return {dmaps, partial, view_sums, ticket, w.off};
}
// one image (gsr_l1_ssim_*): dmaps [3][C][H][W] (the backward pass reads them: first) | partial [C*tiles][2]
struct L1Ws { float *dmaps, *partial; size_t total_bytes; };
static inline L1Ws l1_carve(void *ws, int C, int H, int W) {
    Bump w = {(char *)ws, 0};
    float *const dmaps = w.take<float>((size_t)3 * C * H * W), *const partial = w.take<float>(ssim_tiles(H, W) * C * 2);
    return {dmaps, partial, w.off};
}

struct ViewsFwdArgs {
    const float *img[GSR_VIEWS_MAX_B], *gt[GSR_VIEWS_MAX_B];   // the views of this launch
    float *dmaps, *partial;
    int *ticket;
    int H, W, plane0;          // plane0: 3 * (first view of this launch)
    size_t n_all;              // B * 3 * H * W
    SsimWeightsD wts;
};

// grid (tiles x, tiles y, 3 * views of this launch)
template <bool SAN>
__global__ __launch_bounds__(256) void views_loss_fwd_kernel(ViewsFwdArgs a) {
    __shared__ SsimTile sx, sy;
    __shared__ SsimRows hz[5];
    __shared__ float red[3][4];
    const int tid = threadIdx.x, lx = tid & 15, ly = tid >> 4;
    const int v = blockIdx.z / 3, c = blockIdx.z - 3 * v, x0 = blockIdx.x * SSIM_T, y0 = blockIdx.y * SSIM_T;
    const int H = a.H, W = a.W;
    const size_t plane = (size_t)H * W, gplane = (size_t)(a.plane0 + blockIdx.z);
    if (tid == 0 && (blockIdx.x | blockIdx.y | blockIdx.z) == 0) *a.ticket = 0;    // the finishing kernel counts its blocks in it
    ssim_stage_pair<SAN>(sx, sy, a.img[v] + (size_t)c * plane, a.gt[v] + (size_t)c * plane, H, W, x0, y0, tid);
    const SsimMoments m = ssim_blur_moments(sx, sy, hz, a.wts, tid, lx, ly);
    const int x = x0 + lx, y = y0 + ly;
    float l1 = 0.f, ss = 0.f, sq = 0.f;
    if (x < W && y < H) {
        const size_t p = gplane * plane + (size_t)y * W + x;
        ss = ssim_entry(m, a.dmaps + p, a.dmaps + a.n_all + p, a.dmaps + 2 * a.n_all + p);
        const float d = sx[ly + SSIM_R][lx + SSIM_R] - sy[ly + SSIM_R][lx + SSIM_R];
        l1 = fabsf(d);
        sq = d * d;
    }
    l1 = ssim_block_sum(l1, red[0], tid);
    ss = ssim_block_sum(ss, red[1], tid);
    sq = ssim_block_sum(sq, red[2], tid);
    if (tid == 0) {
        const size_t b = (gplane * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        a.partial[3 * b] = l1;
        a.partial[3 * b + 1] = ss;
        a.partial[3 * b + 2] = sq;
    }
}

// One block per view: terms[b] = (mean |d|, mean SSIM, mean d^2) of view b from its 3 * tiles partials, in a fixed order.  The block
// that takes the last ticket adds the B view sums, again in a fixed order: out[0] = loss, out[1] = L1 mean, out[2] = SSIM mean.
__global__ __launch_bounds__(1024) void views_loss_finish_kernel(int B, int per_view, double inv_nv, float w_l1, float w_ssim,
                                                                 const float *__restrict__ partial, double *view_sums, int *ticket,
                                                                 float *__restrict__ out, float *__restrict__ terms) {
    __shared__ double r[3][16];
    const int b = blockIdx.x;
    const float *p = partial + (size_t)3 * per_view * b;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < per_view; i += 1024) { s0 += (double)p[3 * i]; s1 += (double)p[3 * i + 1]; s2 += (double)p[3 * i + 2]; }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) { s0 += __shfl_xor(s0, m); s1 += __shfl_xor(s1, m); s2 += __shfl_xor(s2, m); }
    if ((threadIdx.x & 63) == 0) { r[0][threadIdx.x >> 6] = s0; r[1][threadIdx.x >> 6] = s1; r[2][threadIdx.x >> 6] = s2; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double t[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < 3; k++) {
        for (int i = 0; i < 16; i++) t[k] += r[k][i];
        terms[3 * b + k] = (float)(t[k] * inv_nv);
        view_sums[3 * b + k] = t[k];
    }
    __threadfence();                                   // the sums of this view before its ticket
    if (atomicAdd(ticket, 1) != B - 1) return;
    __threadfence();
    const volatile double *vs = view_sums;             // written by other blocks of this launch
    double sa = 0.0, sb = 0.0;
    for (int i = 0; i < B; i++) { sa += vs[3 * i]; sb += vs[3 * i + 1]; }
    const double l1 = sa * inv_nv / B, ssim = sb * inv_nv / B;
    out[0] = (float)((double)w_l1 * l1 + (double)w_ssim * (1.0 - ssim));       // rounded once
    out[1] = (float)l1;
    out[2] = (float)ssim;
}

struct ViewsBwdArgs {
    const float *img[GSR_VIEWS_MAX_B], *gt[GSR_VIEWS_MAX_B];
    float *grad[GSR_VIEWS_MAX_B];      // NULL: this view wants no gradient
    const float *dmaps, *grad_loss;    // grad_loss: [1] or NULL (= 1)
    int H, W, plane0;
    size_t n_all;
    float w_l1, w_ssim;
    double inv_n;                      // 1 / (B * 3 * H * W)
    SsimWeightsD wts;
};

template <bool SAN>
__global__ __launch_bounds__(256) void views_loss_bwd_kernel(ViewsBwdArgs a) {
    __shared__ SsimTile sm[3];
    __shared__ SsimRows hz[3];
    const int v = blockIdx.z / 3, c = blockIdx.z - 3 * v;
    float *__restrict__ grad = a.grad[v];
    if (!grad) return;                                 // the whole block
    const int tid = threadIdx.x, lx = tid & 15, ly = tid >> 4;
    const int x0 = blockIdx.x * SSIM_T, y0 = blockIdx.y * SSIM_T, H = a.H, W = a.W;
    const size_t plane = (size_t)H * W, gbase = (size_t)(a.plane0 + blockIdx.z) * plane;
    const SsimBlurred bl = ssim_blur_dmaps(sm, hz, a.dmaps, gbase, a.n_all, a.wts, H, W, x0, y0, tid, lx, ly);
    const double gA = bl.gA, gB = bl.gB, gC = bl.gC;
    const int x = x0 + lx, y = y0 + ly;
    if (x < W && y < H) {
        const size_t p = (size_t)c * plane + (size_t)y * W + x;
        const float raw = a.img[v][p];
        const float xv = SAN ? ssim_sanitize(raw) : raw, yv = SAN ? ssim_sanitize(a.gt[v][p]) : a.gt[v][p];
        const float d = xv - yv;
        const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        const float up = a.grad_loss ? a.grad_loss[0] : 1.f;
        const float g = (float)((double)up * a.inv_n * ((double)a.w_l1 * sgn - (double)a.w_ssim * (gA + 2.0 * xv * gB + (double)yv * gC)));
        // clamp passes its gradient on [0, 1], bounds included, nan_to_num where the input is finite: exactly 0 elsewhere
        grad[p] = (!SAN || (raw >= 0.f && raw <= 1.f)) ? g : 0.f;
    }
}

// B, H, W >= 1 and no NULL among imgs / gts (checked by gsr_views_loss_forward); ws holds views_carve(., B, H, W).total_bytes
static hipError_t launch_views_loss_forward(int B, int H, int W, const float *const *imgs, const float *const *gts, float w_l1, float w_ssim,
                                     int sanitize, float *out3, float *terms, void *ws, hipStream_t s) {
    const ViewsWs w = views_carve(ws, B, H, W);
    ViewsFwdArgs a;
    a.dmaps = w.dmaps; a.partial = w.partial; a.ticket = w.ticket; a.H = H; a.W = W; a.n_all = (size_t)3 * B * H * W;
    a.wts = make_view_weights();
    const unsigned gx = (W + SSIM_T - 1) / SSIM_T, gy = (H + SSIM_T - 1) / SSIM_T;
    for (int b0 = 0; b0 < B; b0 += GSR_VIEWS_MAX_B) {
        const int nb = B - b0 < GSR_VIEWS_MAX_B ? B - b0 : GSR_VIEWS_MAX_B;
        for (int i = 0; i < GSR_VIEWS_MAX_B; i++) { a.img[i] = i < nb ? imgs[b0 + i] : nullptr; a.gt[i] = i < nb ? gts[b0 + i] : nullptr; }
        a.plane0 = 3 * b0;
        const dim3 grid(gx, gy, 3 * nb);
        if (sanitize) hipLaunchKernelGGL(views_loss_fwd_kernel<true>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(views_loss_fwd_kernel<false>, grid, dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(views_loss_finish_kernel, dim3(B), dim3(1024), 0, s, B, (int)(3 * gx * gy), 1.0 / ((double)3 * H * W), w_l1, w_ssim,
                       w.partial, w.view_sums, w.ticket, out3, terms);
    return hipGetLastError();
}

static hipError_t launch_views_loss_backward(int B, int H, int W, const float *const *imgs, const float *const *gts, float w_l1, float w_ssim,
                                      int sanitize, const float *grad_loss, const void *ws, float *const *grad_imgs, hipStream_t s) {
    const ViewsWs w = views_carve(const_cast<void *>(ws), B, H, W);
    ViewsBwdArgs a;
    a.dmaps = w.dmaps; a.grad_loss = grad_loss; a.H = H; a.W = W; a.n_all = (size_t)3 * B * H * W;
    a.w_l1 = w_l1; a.w_ssim = w_ssim; a.inv_n = 1.0 / ((double)3 * B * H * W);
    a.wts = make_view_weights();
    const unsigned gx = (W + SSIM_T - 1) / SSIM_T, gy = (H + SSIM_T - 1) / SSIM_T;
    for (int b0 = 0; b0 < B; b0 += GSR_VIEWS_MAX_B) {
        const int nb = B - b0 < GSR_VIEWS_MAX_B ? B - b0 : GSR_VIEWS_MAX_B;
        bool any = false;
        for (int i = 0; i < GSR_VIEWS_MAX_B; i++) {
            a.img[i] = i < nb ? imgs[b0 + i] : nullptr; a.gt[i] = i < nb ? gts[b0 + i] : nullptr;
            a.grad[i] = i < nb && grad_imgs ? grad_imgs[b0 + i] : nullptr;
            any = any || a.grad[i];
        }
        if (!any) continue;
        a.plane0 = 3 * b0;
        const dim3 grid(gx, gy, 3 * nb);
        if (sanitize) hipLaunchKernelGGL(views_loss_bwd_kernel<true>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(views_loss_bwd_kernel<false>, grid, dim3(256), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace gsr

using namespace gsr;

extern "C" {

// ---- fused training loss (include/gsr_loss.h) ----
int32_t gsr_l1_ssim_workspace(int32_t C, int32_t H, int32_t W, size_t *bytes) {
    if (C <= 0 || H <= 0 || W <= 0 || !bytes) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_l1_ssim_workspace: bad argument");
    *bytes = l1_carve(nullptr, C, H, W).total_bytes;
    return GSR_OK;
}

int32_t gsr_l1_ssim_forward(gsr_stream_t stream, int32_t C, int32_t H, int32_t W, const float *img, const float *gt,
                            float lambda_dssim, float *out3, void *ws, size_t ws_bytes) {
    size_t need = 0;
    if (gsr_l1_ssim_workspace(C, H, W, &need) != GSR_OK) return GSR_ERR_INVALID_ARGUMENT;
    if (!img || !gt || !out3 || !ws) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_l1_ssim_forward: null pointer");
    if (ws_bytes < need) return fail(GSR_ERR_WORKSPACE, "loss workspace %zu < %zu", ws_bytes, need);
    const L1Ws w = l1_carve(ws, C, H, W);
    HIP_TRY(launch_l1_ssim_forward(C, H, W, img, gt, lambda_dssim, w.dmaps, w.partial, out3, (hipStream_t)stream), "l1+ssim forward launch");
    return GSR_OK;
}

int32_t gsr_l1_ssim_backward(gsr_stream_t stream, int32_t C, int32_t H, int32_t W, const float *img, const float *gt,
                             float lambda_dssim, const float *grad_loss, const void *ws, size_t ws_bytes, float *grad_img) {
    size_t need = 0;
    if (gsr_l1_ssim_workspace(C, H, W, &need) != GSR_OK) return GSR_ERR_INVALID_ARGUMENT;
    if (!img || !gt || !ws || !grad_img) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_l1_ssim_backward: null pointer");
    if (ws_bytes < need) return fail(GSR_ERR_WORKSPACE, "loss workspace %zu < %zu", ws_bytes, need);
    HIP_TRY(launch_l1_ssim_backward(C, H, W, img, gt, lambda_dssim, l1_carve(const_cast<void *>(ws), C, H, W).dmaps, grad_loss, grad_img, (hipStream_t)stream),
            "l1+ssim backward launch");
    return GSR_OK;
}

// ---- the same loss over B views (include/gsr_loss.h) ----
static_assert(GSR_VIEWS_MAX_B == GSR_VIEWS_LOSS_MAX_B, "per-launch view limit of ssim_loss.hip and gsr_loss.h");
// 0 = ok; everything the forward and the backward check alike, before anything is launched
static int views_loss_check(const char *who, int32_t B, int32_t H, int32_t W, const float *const *imgs, const float *const *gts,
                            const void *ws, size_t ws_bytes) {
    size_t need = 0;
    if (gsr_views_loss_workspace(B, H, W, &need) != GSR_OK) return GSR_ERR_INVALID_ARGUMENT;
    if (!imgs || !gts || !ws) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: null pointer (imgs, gts or workspace)", who);
    for (int b = 0; b < B; b++)
        if (!imgs[b] || !gts[b]) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: view %d: null %s pointer", who, b, imgs[b] ? "target" : "image");
    if (ws_bytes < need) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: workspace %zu < %zu", who, ws_bytes, need);
    return GSR_OK;
}

int32_t gsr_views_loss_workspace(int32_t B, int32_t H, int32_t W, size_t *bytes) {
    if (B < 1 || H < 1 || W < 1 || !bytes) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_views_loss_workspace: bad argument (B=%d H=%d W=%d)", B, H, W);
    if ((H + 15) / 16 > 65535 || (size_t)3 * ssim_tiles(H, W) > (size_t)INT32_MAX)
        return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_views_loss_workspace: image %d x %d too large", W, H);
    *bytes = views_carve(nullptr, B, H, W).total_bytes;
    return GSR_OK;
}

int32_t gsr_views_loss_forward(gsr_stream_t stream, int32_t B, int32_t H, int32_t W, const float *const *imgs, const float *const *gts,
                               float w_l1, float w_ssim, int32_t sanitize, float *out3, float *terms, void *ws, size_t ws_bytes) {
    const int rc = views_loss_check("gsr_views_loss_forward", B, H, W, imgs, gts, ws, ws_bytes);
    if (rc != GSR_OK) return rc;
    if (!out3 || !terms) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_views_loss_forward: null pointer (out3 or terms)");
    HIP_TRY(launch_views_loss_forward(B, H, W, imgs, gts, w_l1, w_ssim, sanitize ? 1 : 0, out3, terms, ws, (hipStream_t)stream),
            "views loss forward launch");
    return GSR_OK;
}

int32_t gsr_views_loss_backward(gsr_stream_t stream, int32_t B, int32_t H, int32_t W, const float *const *imgs, const float *const *gts,
                                float w_l1, float w_ssim, int32_t sanitize, const float *grad_loss, const void *ws, size_t ws_bytes,
                                float *const *grad_imgs) {
    const int rc = views_loss_check("gsr_views_loss_backward", B, H, W, imgs, gts, ws, ws_bytes);
    if (rc != GSR_OK) return rc;
    if (!grad_imgs) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_views_loss_backward: null pointer (grad_imgs)");
    HIP_TRY(launch_views_loss_backward(B, H, W, imgs, gts, w_l1, w_ssim, sanitize ? 1 : 0, grad_loss, ws, grad_imgs, (hipStream_t)stream),
            "views loss backward launch");
    return GSR_OK;
}

}  // extern "C"
