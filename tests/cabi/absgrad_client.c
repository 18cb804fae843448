/* Plain-C client of absgrad of libgsr_hip.so (include/gsr_absgrad.h): no torch, no C++ types.
 * Built and run by tests/test_gpu_absgrad_cabi.py on the GPU box:
 *   gcc absgrad_client.c -I<repo>/include -I/opt/rocm/include -L<pkg> -lgsr_hip -L/opt/rocm/lib -lamdhip64
 *   absgrad_client <problem file> <result file>
 * The problem file is written by the Python side: int32 P D M W H, float32 tanfovx tanfovy, then float32 bg [3], means3D [P,3],
 * shs [P,M,3], opacities [P], scales [P,3], rotations [P,4], viewmatrix [16], projmatrix [16], campos [3], dL_dcolor [3,H,W].  The
 * client renders once (gsr_forward), makes every refusal of the call on outputs that hold a pattern -- each must come with its code and
 * its text and leave the outputs as they were -- then P == 0, R == 0 with and without accumulate, and the call itself: accumulate = 0
 * with the signed sums, then accumulate = 1 without them onto the first result.  It writes int64 R, absgrad [P,2], signed_sum [P,2],
 * the accumulated absgrad [P,2] and the R == 0 output [P,2].  The Python side judges the numbers. */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gsr_absgrad.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at line %d\n", (int)e_, __LINE__); return 2; } } while (0)
/* the call returns `code`; a refusal's text starts with `text`, and both outputs still hold the pattern */
#define EXPECT(call, code, text) do { const int rc_ = (call); const char *said_ = gsr_last_error(); \
    if (rc_ != (code) || ((code) != GSR_OK && strncmp(said_, text, strlen(text)) != 0)) { \
        printf("line %d: expected %d \"%s\", got %d \"%s\"\n", __LINE__, (int)(code), text, rc_, said_); return 1; } \
    if (changed(out, P) || changed(sgn, P)) { printf("line %d: an output was written\n", __LINE__); return 1; } } while (0)
#define PATTERN 0xA5

static void *rd(FILE *f, size_t bytes) {
    void *p = malloc(bytes ? bytes : 1);
    if (!p || fread(p, 1, bytes, f) != bytes) { printf("short problem file\n"); exit(3); }
    return p;
}
static float *dev_copy(const void *h, size_t bytes) {
    void *d;
    if (hipMalloc(&d, bytes ? bytes : 1) != hipSuccess) return NULL;
    hipMemcpy(d, h, bytes, hipMemcpyHostToDevice);
    return (float *)d;
}
static int dump(FILE *f, const void *d, size_t bytes) {
    void *h = malloc(bytes ? bytes : 1);
    if (hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost) != hipSuccess) return 1;
    const int bad = fwrite(h, 1, bytes, f) != bytes;
    free(h);
    return bad;
}
static int changed(const float *out, int32_t P) {
    const size_t n = (size_t)P * 8;
    unsigned char *h = (unsigned char *)malloc(n);
    int bad = hipMemcpy(h, out, n, hipMemcpyDeviceToHost) != hipSuccess;      /* synchronises with the null stream */
    for (size_t k = 0; k < n && !bad; k++) bad = h[k] != PATTERN;
    free(h);
    return bad;
}

static void *binning;
static size_t binning_bytes;
static void *alloc_binning(void *user, size_t bytes) {
    (void)user;
    binning_bytes = bytes;
    return hipMalloc(&binning, bytes ? bytes : 1) == hipSuccess ? binning : NULL;
}

int main(int argc, char **argv) {
    if (argc < 3) { printf("usage: absgrad_client <problem file> <result file>\n"); return 3; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 3; }
    int32_t hdr[5];
    float tanfov[2];
    if (fread(hdr, 4, 5, f) != 5 || fread(tanfov, 4, 2, f) != 2) return 3;
    const int32_t P = hdr[0], D = hdr[1], M = hdr[2], W = hdr[3], H = hdr[4];
    if (P < 1 || M < 1 || W < 1 || H < 1) { printf("bad problem header\n"); return 3; }
    const size_t n = (size_t)P, px = (size_t)3 * W * H * 4;
    float *bg = dev_copy(rd(f, 12), 12), *means = dev_copy(rd(f, n * 12), n * 12), *shs = dev_copy(rd(f, n * M * 12), n * M * 12);
    float *opac = dev_copy(rd(f, n * 4), n * 4), *scales = dev_copy(rd(f, n * 12), n * 12), *rots = dev_copy(rd(f, n * 16), n * 16);
    float *view = dev_copy(rd(f, 64), 64), *proj = dev_copy(rd(f, 64), 64), *campos = dev_copy(rd(f, 12), 12), *dL = dev_copy(rd(f, px), px);
    fclose(f);
    if (!bg || !means || !shs || !opac || !scales || !rots || !view || !proj || !campos || !dL) { printf("hipMalloc failed\n"); return 2; }
    if (gsr_abi_version() != GSR_ABI_VERSION) { printf("ABI version mismatch\n"); return 1; }

    size_t gb = 0, ib = 0, bb = 0, wb = 0;
    if (gsr_workspace_sizes(P, W, H, &gb, &ib, &bb) != GSR_OK) { printf("workspace sizes: %s\n", gsr_last_error()); return 1; }
    if (gsr_absgrad_workspace_bytes(P, &wb) != GSR_OK || wb == 0) { printf("absgrad workspace size: %s\n", gsr_last_error()); return 1; }
    void *geom, *img, *ws;
    float *color, *out, *sgn, *first;
    int32_t *radii;
    CK(hipMalloc(&geom, gb)); CK(hipMalloc(&img, ib)); CK(hipMalloc(&ws, wb)); CK(hipMalloc((void **)&color, px)); CK(hipMalloc((void **)&radii, n * 4));
    CK(hipMalloc((void **)&out, n * 8)); CK(hipMalloc((void **)&sgn, n * 8)); CK(hipMalloc((void **)&first, n * 8));
    int64_t R = 0;
    if (gsr_forward(NULL, P, D, M, W, H, bg, means, shs, NULL, opac, scales, 1.0f, rots, NULL, view, proj, campos, tanfov[0], tanfov[1], 0, 0,
                    color, radii, geom, gb, alloc_binning, NULL, img, ib, &R, NULL, 0) != GSR_OK) { printf("gsr_forward: %s\n", gsr_last_error()); return 1; }
    if (R < 1 || !binning) { printf("nothing was rendered\n"); return 3; }

    /* ---- refusals, and the calls with nothing to do: the outputs keep the pattern ---- */
#define WHO "gsr_absgrad_backward: "
#define MISSING WHO "missing input, workspace or output buffer"
#define CALL(P_, W_, H_, R_, bg_, dL_, g_, gb_, b_, bb_, i_, ib_, ws_, wb_, acc_, out_, sgn_) \
    gsr_absgrad_backward(NULL, P_, W_, H_, R_, bg_, dL_, g_, gb_, b_, bb_, i_, ib_, ws_, wb_, acc_, out_, sgn_)
    CK(hipMemset(out, PATTERN, n * 8)); CK(hipMemset(sgn, PATTERN, n * 8));
    EXPECT(CALL(-1, W, H, R, bg, dL, geom, gb, binning, binning_bytes, img, ib, ws, wb, 0, out, sgn), GSR_ERR_INVALID_ARGUMENT, WHO "bad sizes");
    EXPECT(CALL(P, 0, H, R, bg, dL, geom, gb, binning, binning_bytes, img, ib, ws, wb, 0, out, sgn), GSR_ERR_INVALID_ARGUMENT, WHO "bad sizes");
    EXPECT(CALL(P, W, H, -1, bg, dL, geom, gb, binning, binning_bytes, img, ib, ws, wb, 0, out, sgn), GSR_ERR_INVALID_ARGUMENT, WHO "bad sizes");
    EXPECT(CALL(P, 65536 * 16, H, R, bg, dL, geom, gb, binning, binning_bytes, img, ib, ws, wb, 0, out, sgn), GSR_ERR_INVALID_ARGUMENT, "image too large");
    EXPECT(CALL(P, W, H, R, NULL, dL, geom, gb, binning, binning_bytes, img, ib, ws, wb, 0, out, sgn), GSR_ERR_INVALID_ARGUMENT, MISSING);
    EXPECT(CALL(P, W, H, R, bg, NULL, geom, gb, binning, binning_bytes, img, ib, ws, wb, 0, out, sgn), GSR_ERR_INVALID_ARGUMENT, MISSING);
    EXPECT(CALL(P, W, H, R, bg, dL, NULL, gb, binning, binning_bytes, img, ib, ws, wb, 0, out, sgn), GSR_ERR_INVALID_ARGUMENT, MISSING);
    EXPECT(CALL(P, W, H, R, bg, dL, geom, gb, binning, binning_bytes, NULL, ib, ws, wb, 0, out, sgn), GSR_ERR_INVALID_ARGUMENT, MISSING);
    EXPECT(CALL(P, W, H, R, bg, dL, geom, gb, binning, binning_bytes, img, ib, NULL, wb, 0, out, sgn), GSR_ERR_INVALID_ARGUMENT, MISSING);
    EXPECT(CALL(P, W, H, R, bg, dL, geom, gb, binning, binning_bytes, img, ib, ws, wb, 0, NULL, sgn), GSR_ERR_INVALID_ARGUMENT, MISSING);
    EXPECT(CALL(P, W, H, R, bg, dL, geom, gb, NULL, binning_bytes, img, ib, ws, wb, 0, out, sgn), GSR_ERR_INVALID_ARGUMENT, WHO "binning workspace missing");
    EXPECT(CALL(P, W, H, R, bg, dL, geom, gb, binning, binning_bytes, img, ib, ws, wb - 1, 0, out, sgn), GSR_ERR_WORKSPACE, "absgrad workspace ");
    EXPECT(CALL(P, W, H, R, bg, dL, geom, gb - 1, binning, binning_bytes, img, ib, ws, wb, 0, out, sgn), GSR_ERR_WORKSPACE, "geom workspace ");
    EXPECT(CALL(P, W, H, R, bg, dL, geom, gb, binning, binning_bytes, img, ib - 1, ws, wb, 0, out, sgn), GSR_ERR_WORKSPACE, "image workspace ");
    EXPECT(CALL(P, W, H, R, bg, dL, geom, gb, binning, (size_t)R * 5 - 1, img, ib, ws, wb, 0, out, sgn), GSR_ERR_WORKSPACE, "binning workspace too small for R=");
    if (gsr_set_option("deterministic_bwd", 1) != GSR_OK) { printf("set option: %s\n", gsr_last_error()); return 1; }
    EXPECT(CALL(P, W, H, R, bg, dL, geom, gb, binning, binning_bytes, img, ib, ws, wb, 0, out, sgn), GSR_ERR_INVALID_ARGUMENT,
           WHO "not available while the option deterministic_bwd is on");
    if (gsr_set_option("deterministic_bwd", 0) != GSR_OK) { printf("set option: %s\n", gsr_last_error()); return 1; }
    /* the order: sizes, pointers, own workspace, then the three views (geometry, image, binning) */
    EXPECT(CALL(P, W, -2, R, bg, dL, geom, 0, binning, 0, img, 0, ws, 0, 0, NULL, sgn), GSR_ERR_INVALID_ARGUMENT, WHO "bad sizes");
    EXPECT(CALL(P, W, H, R, bg, dL, geom, 0, binning, 0, img, 0, ws, 0, 0, NULL, sgn), GSR_ERR_INVALID_ARGUMENT, MISSING);
    EXPECT(CALL(P, W, H, R, bg, dL, geom, 0, binning, 0, img, 0, ws, 0, 0, out, sgn), GSR_ERR_WORKSPACE, "absgrad workspace 0 < ");
    EXPECT(CALL(P, W, H, R, bg, dL, geom, 0, binning, 0, img, 0, ws, wb, 0, out, sgn), GSR_ERR_WORKSPACE, "geom workspace 0 < ");
    EXPECT(CALL(P, W, H, R, bg, dL, geom, gb, binning, 0, img, 0, ws, wb, 0, out, sgn), GSR_ERR_WORKSPACE, "image workspace 0 < ");
    EXPECT(CALL(P, W, H, R, bg, dL, geom, gb, binning, 0, img, ib, ws, wb, 0, out, sgn), GSR_ERR_WORKSPACE, "binning workspace too small");
    EXPECT(CALL(0, W, H, R, NULL, NULL, NULL, 0, NULL, 0, NULL, 0, NULL, 0, 0, out, sgn), GSR_OK, "");          /* P == 0: nothing */
    EXPECT(CALL(P, W, H, 0, bg, dL, geom, gb, NULL, 0, img, ib, ws, wb, 1, out, sgn), GSR_OK, "");             /* R == 0, accumulate: nothing */

    FILE *res = fopen(argv[2], "wb");
    if (!res) { printf("cannot write %s\n", argv[2]); return 3; }
    int bad = fwrite(&R, 8, 1, res) != 1;
    /* ---- the call: with the signed sums; then accumulated onto its own result, without them ---- */
    if (CALL(P, W, H, R, bg, dL, geom, gb, binning, binning_bytes, img, ib, ws, wb, 0, out, sgn) != GSR_OK) { printf("absgrad: %s\n", gsr_last_error()); return 1; }
    CK(hipDeviceSynchronize());
    bad |= dump(res, out, n * 8) | dump(res, sgn, n * 8);
    CK(hipMemcpy(first, out, n * 8, hipMemcpyDeviceToDevice));
    if (CALL(P, W, H, R, bg, dL, geom, gb, binning, binning_bytes, img, ib, ws, wb, 1, first, NULL) != GSR_OK) { printf("absgrad: %s\n", gsr_last_error()); return 1; }
    CK(hipDeviceSynchronize());
    bad |= dump(res, first, n * 8);
    /* ---- R == 0 without accumulate: zeros ---- */
    CK(hipMemset(out, PATTERN, n * 8));
    if (CALL(P, W, H, 0, bg, dL, geom, gb, NULL, 0, img, ib, ws, wb, 0, out, NULL) != GSR_OK) { printf("absgrad, R = 0: %s\n", gsr_last_error()); return 1; }
    CK(hipDeviceSynchronize());
    bad |= dump(res, out, n * 8);
    if (fclose(res) || bad) { printf("could not write the results\n"); return 3; }
    printf("absgrad C client ok\n");
    return 0;
}
