/* Plain-C client of the blend-weight statistics of libgsr_hip.so (include/gsr_contrib.h): no torch, no C++ types.
 * Built and run by tests/test_gpu_contrib_cabi.py on the GPU box:
 *   gcc contrib_client.c -I<repo>/include -I/opt/rocm/include -L<pkg> -lgsr_hip -L/opt/rocm/lib -lamdhip64
 *   contrib_client <problem file> <result file>
 * The problem file is written by the Python side: int32 P D M W H, float32 tanfovx tanfovy, then float32 bg [3], means3D [P,3],
 * shs [P,M,3], opacities [P], scales [P,3], rotations [P,4], viewmatrix [16], projmatrix [16], campos [3].  The client renders once
 * (gsr_forward), makes every refusal of the two calls on rows that hold a pattern -- each must come with its code and its text and
 * leave the rows as they were -- then clears the rows, adds the view twice and reads them.  It writes int64 R, the rows after one view
 * [P,16 bytes], after two, and weight_sum [P], weight_max [P], pixel_count [P] of the two.  The Python side judges the numbers. */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gsr_contrib.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at line %d\n", (int)e_, __LINE__); return 2; } } while (0)
/* the call returns `code`; a refusal's text starts with `text`, and the rows still hold the pattern */
#define EXPECT(call, code, text) do { const int rc_ = (call); const char *said_ = gsr_last_error(); \
    if (rc_ != (code) || ((code) != GSR_OK && strncmp(said_, text, strlen(text)) != 0)) { \
        printf("line %d: expected %d \"%s\", got %d \"%s\"\n", __LINE__, (int)(code), text, rc_, said_); return 1; } \
    if (rows_changed(rows, P)) { printf("line %d: the rows were written\n", __LINE__); return 1; } } while (0)
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
static int rows_changed(const gsr_contrib_row_t *rows, int32_t P) {
    const size_t n = (size_t)P * sizeof(gsr_contrib_row_t);
    unsigned char *h = (unsigned char *)malloc(n);
    int bad = hipMemcpy(h, rows, n, hipMemcpyDeviceToHost) != hipSuccess;      /* synchronises with the null stream */
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
    if (argc < 3) { printf("usage: contrib_client <problem file> <result file>\n"); return 3; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 3; }
    int32_t hdr[5];
    float tanfov[2];
    if (fread(hdr, 4, 5, f) != 5 || fread(tanfov, 4, 2, f) != 2) return 3;
    const int32_t P = hdr[0], D = hdr[1], M = hdr[2], W = hdr[3], H = hdr[4];
    if (P < 1 || M < 1 || W < 1 || H < 1) { printf("bad problem header\n"); return 3; }
    const size_t n = (size_t)P;
    float *bg = dev_copy(rd(f, 12), 12), *means = dev_copy(rd(f, n * 12), n * 12), *shs = dev_copy(rd(f, n * M * 12), n * M * 12);
    float *opac = dev_copy(rd(f, n * 4), n * 4), *scales = dev_copy(rd(f, n * 12), n * 12), *rots = dev_copy(rd(f, n * 16), n * 16);
    float *view = dev_copy(rd(f, 64), 64), *proj = dev_copy(rd(f, 64), 64), *campos = dev_copy(rd(f, 12), 12);
    fclose(f);
    if (!bg || !means || !shs || !opac || !scales || !rots || !view || !proj || !campos) { printf("hipMalloc failed\n"); return 2; }
    if (gsr_abi_version() != GSR_ABI_VERSION) { printf("ABI version mismatch\n"); return 1; }

    size_t gb = 0, ib = 0, bb = 0;
    if (gsr_workspace_sizes(P, W, H, &gb, &ib, &bb) != GSR_OK) { printf("workspace sizes: %s\n", gsr_last_error()); return 1; }
    void *geom, *img;
    float *color;
    int32_t *radii;
    gsr_contrib_row_t *rows;
    CK(hipMalloc(&geom, gb)); CK(hipMalloc(&img, ib)); CK(hipMalloc((void **)&color, (size_t)3 * W * H * 4)); CK(hipMalloc((void **)&radii, n * 4));
    CK(hipMalloc((void **)&rows, n * sizeof(gsr_contrib_row_t)));
    int64_t R = 0;
    if (gsr_forward(NULL, P, D, M, W, H, bg, means, shs, NULL, opac, scales, 1.0f, rots, NULL, view, proj, campos, tanfov[0], tanfov[1], 0, 0,
                    color, radii, geom, gb, alloc_binning, NULL, img, ib, &R, NULL, 0) != GSR_OK) { printf("gsr_forward: %s\n", gsr_last_error()); return 1; }
    if (R < 1 || !binning) { printf("nothing was rendered\n"); return 3; }
    float *wsum, *wmax;
    int32_t *npix;
    CK(hipMalloc((void **)&wsum, n * 4)); CK(hipMalloc((void **)&wmax, n * 4)); CK(hipMalloc((void **)&npix, n * 4));

    /* ---- refusals, and the calls with nothing to do: the rows keep the pattern ---- */
    CK(hipMemset(rows, PATTERN, n * sizeof(gsr_contrib_row_t)));
    EXPECT(gsr_contrib_accumulate(NULL, -1, W, H, R, geom, gb, binning, binning_bytes, img, ib, rows), GSR_ERR_INVALID_ARGUMENT, "gsr_contrib_accumulate: bad sizes");
    EXPECT(gsr_contrib_accumulate(NULL, P, 0, H, R, geom, gb, binning, binning_bytes, img, ib, rows), GSR_ERR_INVALID_ARGUMENT, "gsr_contrib_accumulate: bad sizes");
    EXPECT(gsr_contrib_accumulate(NULL, P, W, H, -1, geom, gb, binning, binning_bytes, img, ib, rows), GSR_ERR_INVALID_ARGUMENT, "gsr_contrib_accumulate: bad sizes");
    EXPECT(gsr_contrib_accumulate(NULL, P, 65536 * 16, H, R, geom, gb, binning, binning_bytes, img, ib, rows), GSR_ERR_INVALID_ARGUMENT, "gsr_contrib_accumulate: image too large");
    EXPECT(gsr_contrib_accumulate(NULL, P, W, H, R, geom, gb - 1, binning, binning_bytes, img, ib, rows), GSR_ERR_WORKSPACE, "gsr_contrib_accumulate: geom workspace ");
    EXPECT(gsr_contrib_accumulate(NULL, P, W, H, R, geom, gb, binning, binning_bytes, img, ib - 1, rows), GSR_ERR_WORKSPACE, "gsr_contrib_accumulate: image workspace ");
    EXPECT(gsr_contrib_accumulate(NULL, P, W, H, R, geom, gb, binning, (size_t)R * 5 - 1, img, ib, rows), GSR_ERR_WORKSPACE, "gsr_contrib_accumulate: binning workspace too small for R=");
    EXPECT(gsr_contrib_accumulate(NULL, P, W, H, R, geom, gb, binning, binning_bytes, img, ib, NULL), GSR_ERR_INVALID_ARGUMENT, "gsr_contrib_accumulate: missing rows or workspace");
    EXPECT(gsr_contrib_accumulate(NULL, P, W, H, R, NULL, gb, binning, binning_bytes, img, ib, rows), GSR_ERR_INVALID_ARGUMENT, "gsr_contrib_accumulate: missing rows or workspace");
    EXPECT(gsr_contrib_accumulate(NULL, P, W, H, R, geom, gb, NULL, binning_bytes, img, ib, rows), GSR_ERR_INVALID_ARGUMENT, "gsr_contrib_accumulate: missing rows or workspace");
    EXPECT(gsr_contrib_accumulate(NULL, P, W, H, R, geom, gb, binning, binning_bytes, NULL, ib, rows), GSR_ERR_INVALID_ARGUMENT, "gsr_contrib_accumulate: missing rows or workspace");
    /* the order: sizes, then the three views (geometry, image, binning), then the pointers */
    EXPECT(gsr_contrib_accumulate(NULL, P, W, -2, R, geom, 0, binning, 0, img, 0, NULL), GSR_ERR_INVALID_ARGUMENT, "gsr_contrib_accumulate: bad sizes");
    EXPECT(gsr_contrib_accumulate(NULL, P, W, H, R, geom, 0, binning, 0, img, 0, NULL), GSR_ERR_WORKSPACE, "gsr_contrib_accumulate: geom workspace 0 < ");
    EXPECT(gsr_contrib_accumulate(NULL, P, W, H, R, geom, gb, binning, 0, img, 0, NULL), GSR_ERR_WORKSPACE, "gsr_contrib_accumulate: image workspace 0 < ");
    EXPECT(gsr_contrib_accumulate(NULL, P, W, H, R, geom, gb, binning, 0, img, ib, NULL), GSR_ERR_WORKSPACE, "gsr_contrib_accumulate: binning workspace too small");
    EXPECT(gsr_contrib_accumulate(NULL, 0, W, H, R, NULL, 0, NULL, 0, NULL, 0, rows), GSR_OK, "");
    EXPECT(gsr_contrib_accumulate(NULL, P, W, H, 0, geom, gb, NULL, 0, img, ib, rows), GSR_OK, "");
    EXPECT(gsr_contrib_accumulate(NULL, P, W, H, 0, NULL, 0, NULL, 0, NULL, 0, NULL), GSR_OK, "");
    EXPECT(gsr_contrib_read(NULL, P, rows, NULL, NULL, NULL), GSR_ERR_INVALID_ARGUMENT, "gsr_contrib_read: weight_sum, weight_max and pixel_count are all NULL");
    EXPECT(gsr_contrib_read(NULL, 0, rows, NULL, NULL, NULL), GSR_ERR_INVALID_ARGUMENT, "gsr_contrib_read: weight_sum, weight_max and pixel_count are all NULL");
    EXPECT(gsr_contrib_read(NULL, -1, rows, wsum, wmax, npix), GSR_ERR_INVALID_ARGUMENT, "gsr_contrib_read: bad sizes");
    EXPECT(gsr_contrib_read(NULL, P, NULL, wsum, wmax, npix), GSR_ERR_INVALID_ARGUMENT, "gsr_contrib_read: missing rows");
    EXPECT(gsr_contrib_read(NULL, 0, NULL, wsum, NULL, NULL), GSR_OK, "");
    EXPECT(gsr_contrib_read(NULL, P, rows, wsum, wmax, npix), GSR_OK, "");        /* reading leaves the rows alone too */

    /* ---- one view, then the same view again ---- */
    FILE *out = fopen(argv[2], "wb");
    if (!out) { printf("cannot write %s\n", argv[2]); return 3; }
    int bad = fwrite(&R, 8, 1, out) != 1;
    CK(hipMemset(rows, 0, n * sizeof(gsr_contrib_row_t)));
    if (gsr_contrib_accumulate(NULL, P, W, H, R, geom, gb, binning, binning_bytes, img, ib, rows) != GSR_OK) { printf("accumulate: %s\n", gsr_last_error()); return 1; }
    CK(hipDeviceSynchronize());
    bad |= dump(out, rows, n * sizeof(gsr_contrib_row_t));
    if (gsr_contrib_accumulate(NULL, P, W, H, R, geom, gb, binning, binning_bytes, img, ib, rows) != GSR_OK) { printf("accumulate: %s\n", gsr_last_error()); return 1; }
    if (gsr_contrib_read(NULL, P, rows, wsum, NULL, NULL) != GSR_OK || gsr_contrib_read(NULL, P, rows, NULL, wmax, npix) != GSR_OK) {
        printf("read: %s\n", gsr_last_error()); return 1; }
    CK(hipDeviceSynchronize());
    bad |= dump(out, rows, n * sizeof(gsr_contrib_row_t)) | dump(out, wsum, n * 4) | dump(out, wmax, n * 4) | dump(out, npix, n * 4);
    if (fclose(out) || bad) { printf("could not write the results\n"); return 3; }
    printf("contrib C client ok\n");
    return 0;
}
