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
// Each direction is ONE tile body, ssim_fwd_tile / ssim_bwd_tile, templated on the sanitising, the number of partial sums and the
// window's type; the four kernels around them only find their plane's pointers (and the multi-view forward resets the ticket).  The
// two finishing kernels share ssim_sum_partials and differ in what they make of the totals.
//
// The multi-view form (gsr_views_loss_*, include/gsr_loss.h; the image loss of train_stacked_transformer.py:203-222) runs that
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

// The forward pass of one block, for both forward kernels: this block's tile of the plane img / gt ([H][W] each) staged and blurred, the
// plane's three derivative-map entries written (d f / d mu1 at dm, the other two `stride` and 2 `stride` floats behind it), and the
// block's sums of |d|, SSIM and (NPART == 3) d^2, d = x - y as staged, stored by thread 0 at slot[0 .. NPART).
template <bool SAN, int NPART, class Weights>
__device__ __forceinline__ void ssim_fwd_tile(const float *__restrict__ img, const float *__restrict__ gt, int H, int W, const Weights &wts,
                                              float *__restrict__ dm, size_t stride, float *__restrict__ slot) {
    __shared__ SsimTile sx, sy;
    __shared__ SsimRows hz[5];
    __shared__ float red[NPART][4];
    const int tid = threadIdx.x, lx = tid & 15, ly = tid >> 4;
    const int x0 = blockIdx.x * SSIM_T, y0 = blockIdx.y * SSIM_T;
    ssim_stage_pair<SAN>(sx, sy, img, gt, H, W, x0, y0, tid);
    const SsimMoments m = ssim_blur_moments(sx, sy, hz, wts, tid, lx, ly);
    const int x = x0 + lx, y = y0 + ly;
    float part[3] = {0.f, 0.f, 0.f};                       // |d|, SSIM, d^2
    if (x < W && y < H) {
        const size_t p = (size_t)y * W + x;
        part[1] = ssim_entry(m, dm + p, dm + stride + p, dm + 2 * stride + p);
        const float d = sx[ly + SSIM_R][lx + SSIM_R] - sy[ly + SSIM_R][lx + SSIM_R];
        part[0] = fabsf(d);
        part[2] = d * d;
    }
    for (int k = 0; k < NPART; k++) part[k] = ssim_block_sum(part[k], red[k], tid);
    if (tid == 0)
        for (int k = 0; k < NPART; k++) slot[k] = part[k];
}

// grid (tiles x, tiles y, C)
__global__ __launch_bounds__(256) void l1_ssim_fwd_kernel(int C, int H, int W, const float *__restrict__ img, const float *__restrict__ gt,
                                                          SsimWeights wts, float *__restrict__ dmaps /*[3][C][H][W]*/,
                                                          float *__restrict__ partial /*[blocks][2]*/) {
    const size_t plane = (size_t)H * W, base = (size_t)blockIdx.z * plane;
    const size_t b = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    ssim_fwd_tile<false, 2>(img + base, gt + base, H, W, wts, dmaps + base, (size_t)C * plane, partial + 2 * b);
}

// Sums n interleaved partials p[n][NPART] over the 1024 threads of the block, in double and in a fixed order (strided accumulate,
// shuffles, 16 LDS slots per value added in index order); the totals are valid in thread 0, t[0 .. NPART).
template <int NPART>
__device__ __forceinline__ void ssim_sum_partials(const float *__restrict__ p, int n, double *t) {
    __shared__ double r[NPART][16];
    double s[NPART];
    for (int k = 0; k < NPART; k++) s[k] = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024)
        for (int k = 0; k < NPART; k++) s[k] += (double)p[NPART * i + k];
    for (int m = 32; m > 0; m >>= 1)
        for (int k = 0; k < NPART; k++) s[k] += __shfl_xor(s[k], m);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < NPART; k++) r[k][threadIdx.x >> 6] = s[k];
    __syncthreads();
    for (int k = 0; k < NPART; k++) {
        t[k] = 0.0;
        if (threadIdx.x == 0)
            for (int i = 0; i < 16; i++) t[k] += r[k][i];
    }
}

// out[0] = loss, out[1] = L1 mean, out[2] = SSIM mean
__global__ __launch_bounds__(1024) void l1_ssim_finish_kernel(int nblocks, double inv_n, float lambda,
                                                              const float *__restrict__ partial, float *__restrict__ out) {
    double t[2];
    ssim_sum_partials<2>(partial, nblocks, t);
    if (threadIdx.x != 0) return;
    const float l1 = (float)(t[0] * inv_n), ssim = (float)(t[1] * inv_n);
    out[0] = (1.f - lambda) * l1 + lambda * (1.f - ssim);
    out[1] = l1;
    out[2] = ssim;
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

// The reverse pass of one block, for both backward kernels: the blurred derivative maps of the plane that starts at dm[base] (strides
// as ssim_blur_dmaps) and, at this thread's pixel of the planes img / gt / grad,
//   dL/dx = up * inv_n * (w_l1 sign(x - y) - w_ssim (G*A + 2 x G*B + y G*C)),   x, y sanitised first when SAN,
// rounded to float32 once.  Both weights and inv_n are doubles: the single-image kernel's 1 - lambda is no float32 number.
template <bool SAN, class Weights>
__device__ __forceinline__ void ssim_bwd_tile(const float *__restrict__ img, const float *__restrict__ gt, float *__restrict__ grad, int H, int W,
                                              const Weights &wts, const float *__restrict__ dm, size_t base, size_t stride, double w_l1,
                                              double w_ssim, double inv_n, const float *__restrict__ grad_loss /*[1] or null (= 1)*/) {
    __shared__ SsimTile sm[3];
    __shared__ SsimRows hz[3];
    const int tid = threadIdx.x, lx = tid & 15, ly = tid >> 4;
    const int x0 = blockIdx.x * SSIM_T, y0 = blockIdx.y * SSIM_T;
    const SsimBlurred bl = ssim_blur_dmaps(sm, hz, dm, base, stride, wts, H, W, x0, y0, tid, lx, ly);
    const int x = x0 + lx, y = y0 + ly;
    if (x < W && y < H) {
        const size_t p = (size_t)y * W + x;
        const float raw = img[p];
        const float xv = SAN ? ssim_sanitize(raw) : raw, yv = SAN ? ssim_sanitize(gt[p]) : gt[p];
        const float d = xv - yv;
        const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);           // torch.abs backward: sign(0) = 0
        const float up = grad_loss ? grad_loss[0] : 1.f;
        const float g = (float)((double)up * inv_n * (w_l1 * sgn - w_ssim * (bl.gA + 2.0 * xv * bl.gB + (double)yv * bl.gC)));
        // clamp passes its gradient on [0, 1], bounds included, nan_to_num where the input is finite: exactly 0 elsewhere
        grad[p] = (!SAN || (raw >= 0.f && raw <= 1.f)) ? g : 0.f;
    }
}

__global__ __launch_bounds__(256) void l1_ssim_bwd_kernel(int C, int H, int W, const float *__restrict__ img, const float *__restrict__ gt,
                                                          SsimWeights wts, const float *__restrict__ dmaps, float lambda, float inv_n,
                                                          const float *__restrict__ grad_loss /*[1] or null*/, float *__restrict__ grad_img) {
    const size_t plane = (size_t)H * W, base = (size_t)blockIdx.z * plane;
    ssim_bwd_tile<false>(img + base, gt + base, grad_img + base, H, W, wts, dmaps, base, (size_t)C * plane, 1.0 - lambda, (double)lambda,
                         (double)inv_n, grad_loss);
}

// the tile grid of `planes` image planes, for the launchers and the workspace layouts
static inline dim3 ssim_grid(int H, int W, int planes) { return dim3((W + SSIM_T - 1) / SSIM_T, (H + SSIM_T - 1) / SSIM_T, planes); }
static inline size_t ssim_tiles(int H, int W) { const dim3 g = ssim_grid(H, W, 1); return (size_t)g.x * g.y; }      // blocks per image plane

static hipError_t launch_l1_ssim_forward(int C, int H, int W, const float *img, const float *gt, float lambda, float *dmaps,
                                  float *partial, float *out, hipStream_t s) {
    hipLaunchKernelGGL(l1_ssim_fwd_kernel, ssim_grid(H, W, C), dim3(256), 0, s, C, H, W, img, gt, make_weights(), dmaps, partial);
    hipLaunchKernelGGL(l1_ssim_finish_kernel, dim3(1), dim3(1024), 0, s, (int)(ssim_tiles(H, W) * C), 1.0 / ((double)C * H * W), lambda,
                       partial, out);
    return hipGetLastError();
}

static hipError_t launch_l1_ssim_backward(int C, int H, int W, const float *img, const float *gt, float lambda, const float *dmaps,
                                   const float *grad_loss, float *grad_img, hipStream_t s) {
    hipLaunchKernelGGL(l1_ssim_bwd_kernel, ssim_grid(H, W, C), dim3(256), 0, s, C, H, W, img, gt, make_weights(), dmaps, lambda,
                       (float)(1.0 / ((double)C * H * W)), grad_loss, grad_img);
    return hipGetLastError();
}

// ---- B views in one launch (gsr_views_loss_*) ----
// workspace: dmaps [3][B*3][H][W] | partial [B*3*tiles][3] | view_sums [B][3] double | ticket (one int on a line of its own)
struct ViewsWs { float *dmaps, *partial; double *view_sums; int *ticket; size_t total_bytes; };
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
    const int v = blockIdx.z / 3, c = blockIdx.z - 3 * v;
    const size_t plane = (size_t)a.H * a.W, gplane = (size_t)(a.plane0 + blockIdx.z);
    if (threadIdx.x == 0 && (blockIdx.x | blockIdx.y | blockIdx.z) == 0) *a.ticket = 0;    // the finishing kernel counts its blocks in it
    const size_t b = (gplane * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    ssim_fwd_tile<SAN, 3>(a.img[v] + (size_t)c * plane, a.gt[v] + (size_t)c * plane, a.H, a.W, a.wts, a.dmaps + gplane * plane, a.n_all,
                          a.partial + 3 * b);
}

// One block per view: terms[b] = (mean |d|, mean SSIM, mean d^2) of view b from its 3 * tiles partials, in a fixed order.  The block
// that takes the last ticket adds the B view sums, again in a fixed order: out[0] = loss, out[1] = L1 mean, out[2] = SSIM mean.
__global__ __launch_bounds__(1024) void views_loss_finish_kernel(int B, int per_view, double inv_nv, float w_l1, float w_ssim,
                                                                 const float *__restrict__ partial, double *view_sums, int *ticket,
                                                                 float *__restrict__ out, float *__restrict__ terms) {
    const int b = blockIdx.x;
    double t[3];
    ssim_sum_partials<3>(partial + (size_t)3 * per_view * b, per_view, t);
    if (threadIdx.x != 0) return;
    for (int k = 0; k < 3; k++) {
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
    const int v = blockIdx.z / 3, c = blockIdx.z - 3 * v;
    if (!a.grad[v]) return;                            // the whole block
    const size_t plane = (size_t)a.H * a.W, off = (size_t)c * plane;
    ssim_bwd_tile<SAN>(a.img[v] + off, a.gt[v] + off, a.grad[v] + off, a.H, a.W, a.wts, a.dmaps, (size_t)(a.plane0 + blockIdx.z) * plane,
                       a.n_all, (double)a.w_l1, (double)a.w_ssim, a.inv_n, a.grad_loss);
}

// Walks the B views in chunks of GSR_VIEWS_MAX_B, one launch each: the chunk's pointers into img / gt (and grad, the backward pass's;
// NULL in the slots behind the last view), then launch(3 * first view, grid).  A chunk of the backward pass in which no view wants a
// gradient is skipped.
template <class Launch>
static void views_in_chunks(int B, int H, int W, const float *const *imgs, const float *const *gts, float *const *grad_imgs,
                            const float **img, const float **gt, float **grad /*NULL: forward*/, Launch &&launch) {
    for (int b0 = 0; b0 < B; b0 += GSR_VIEWS_MAX_B) {
        const int nb = B - b0 < GSR_VIEWS_MAX_B ? B - b0 : GSR_VIEWS_MAX_B;
        bool any = !grad;
        for (int i = 0; i < GSR_VIEWS_MAX_B; i++) {
            img[i] = i < nb ? imgs[b0 + i] : nullptr; gt[i] = i < nb ? gts[b0 + i] : nullptr;
            if (!grad) continue;
            grad[i] = i < nb && grad_imgs ? grad_imgs[b0 + i] : nullptr;
            any = any || grad[i];
        }
        if (any) launch(3 * b0, ssim_grid(H, W, 3 * nb));
    }
}

// B, H, W >= 1 and no NULL among imgs / gts (checked by gsr_views_loss_forward); ws holds views_carve(., B, H, W).total_bytes
static hipError_t launch_views_loss_forward(int B, int H, int W, const float *const *imgs, const float *const *gts, float w_l1, float w_ssim,
                                     int sanitize, float *out3, float *terms, void *ws, hipStream_t s) {
    const ViewsWs w = views_carve(ws, B, H, W);
    ViewsFwdArgs a;
    a.dmaps = w.dmaps; a.partial = w.partial; a.ticket = w.ticket; a.H = H; a.W = W; a.n_all = (size_t)3 * B * H * W;
    a.wts = make_view_weights();
    views_in_chunks(B, H, W, imgs, gts, nullptr, a.img, a.gt, nullptr, [&](int plane0, dim3 grid) {
        a.plane0 = plane0;
        if (sanitize) hipLaunchKernelGGL(views_loss_fwd_kernel<true>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(views_loss_fwd_kernel<false>, grid, dim3(256), 0, s, a);
    });
    hipLaunchKernelGGL(views_loss_finish_kernel, dim3(B), dim3(1024), 0, s, B, (int)(3 * ssim_tiles(H, W)), 1.0 / ((double)3 * H * W), w_l1,
                       w_ssim, w.partial, w.view_sums, w.ticket, out3, terms);
    return hipGetLastError();
}

static hipError_t launch_views_loss_backward(int B, int H, int W, const float *const *imgs, const float *const *gts, float w_l1, float w_ssim,
                                      int sanitize, const float *grad_loss, const void *ws, float *const *grad_imgs, hipStream_t s) {
    const ViewsWs w = views_carve(const_cast<void *>(ws), B, H, W);
    ViewsBwdArgs a;
    a.dmaps = w.dmaps; a.grad_loss = grad_loss; a.H = H; a.W = W; a.n_all = (size_t)3 * B * H * W;
    a.w_l1 = w_l1; a.w_ssim = w_ssim; a.inv_n = 1.0 / ((double)3 * B * H * W);
    a.wts = make_view_weights();
    views_in_chunks(B, H, W, imgs, gts, grad_imgs, a.img, a.gt, a.grad, [&](int plane0, dim3 grid) {
        a.plane0 = plane0;
        if (sanitize) hipLaunchKernelGGL(views_loss_bwd_kernel<true>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(views_loss_bwd_kernel<false>, grid, dim3(256), 0, s, a);
    });
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

// 0 = ok; everything the forward and the backward check alike, before anything is launched (out: out3 or grad_img)
static int l1_ssim_check(const char *who, int32_t C, int32_t H, int32_t W, const float *img, const float *gt, const float *out, const void *ws,
                         size_t ws_bytes) {
    size_t need = 0;
    if (gsr_l1_ssim_workspace(C, H, W, &need) != GSR_OK) return GSR_ERR_INVALID_ARGUMENT;
    if (!img || !gt || !out || !ws) return fail(GSR_ERR_INVALID_ARGUMENT, "%s: null pointer", who);
    if (ws_bytes < need) return fail(GSR_ERR_WORKSPACE, "loss workspace %zu < %zu", ws_bytes, need);
    return GSR_OK;
}

int32_t gsr_l1_ssim_forward(gsr_stream_t stream, int32_t C, int32_t H, int32_t W, const float *img, const float *gt,
                            float lambda_dssim, float *out3, void *ws, size_t ws_bytes) {
    GSR_TRY(l1_ssim_check("gsr_l1_ssim_forward", C, H, W, img, gt, out3, ws, ws_bytes));
    const L1Ws w = l1_carve(ws, C, H, W);
    HIP_TRY(launch_l1_ssim_forward(C, H, W, img, gt, lambda_dssim, w.dmaps, w.partial, out3, (hipStream_t)stream), "l1+ssim forward launch");
    return GSR_OK;
}

int32_t gsr_l1_ssim_backward(gsr_stream_t stream, int32_t C, int32_t H, int32_t W, const float *img, const float *gt,
                             float lambda_dssim, const float *grad_loss, const void *ws, size_t ws_bytes, float *grad_img) {
    GSR_TRY(l1_ssim_check("gsr_l1_ssim_backward", C, H, W, img, gt, grad_img, ws, ws_bytes));
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
    if (ssim_grid(H, W, 1).y > 65535 || (size_t)3 * ssim_tiles(H, W) > (size_t)INT32_MAX)
        return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_views_loss_workspace: image %d x %d too large", W, H);
    *bytes = views_carve(nullptr, B, H, W).total_bytes;
    return GSR_OK;
}

int32_t gsr_views_loss_forward(gsr_stream_t stream, int32_t B, int32_t H, int32_t W, const float *const *imgs, const float *const *gts,
                               float w_l1, float w_ssim, int32_t sanitize, float *out3, float *terms, void *ws, size_t ws_bytes) {
    GSR_TRY(views_loss_check("gsr_views_loss_forward", B, H, W, imgs, gts, ws, ws_bytes));
    if (!out3 || !terms) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_views_loss_forward: null pointer (out3 or terms)");
    HIP_TRY(launch_views_loss_forward(B, H, W, imgs, gts, w_l1, w_ssim, sanitize ? 1 : 0, out3, terms, ws, (hipStream_t)stream),
            "views loss forward launch");
    return GSR_OK;
}

int32_t gsr_views_loss_backward(gsr_stream_t stream, int32_t B, int32_t H, int32_t W, const float *const *imgs, const float *const *gts,
                                float w_l1, float w_ssim, int32_t sanitize, const float *grad_loss, const void *ws, size_t ws_bytes,
                                float *const *grad_imgs) {
    GSR_TRY(views_loss_check("gsr_views_loss_backward", B, H, W, imgs, gts, ws, ws_bytes));
    if (!grad_imgs) return fail(GSR_ERR_INVALID_ARGUMENT, "gsr_views_loss_backward: null pointer (grad_imgs)");
    HIP_TRY(launch_views_loss_backward(B, H, W, imgs, gts, w_l1, w_ssim, sanitize ? 1 : 0, grad_loss, ws, grad_imgs, (hipStream_t)stream),
            "views loss backward launch");
    return GSR_OK;
}

}  // extern "C"
