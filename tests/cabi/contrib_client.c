/* Plain-C client of the blend-weight statistics of libgsr_hip.so (include/gsr_contrib.h): no torch, no C++ types.
 * Built and run by tests/test_gpu_contrib_cabi.py on the GPU box:
 *   gcc contrib_client.c -I<repo>/include -I/opt/rocm/include -L<pkg> -lgsr_hip -L/opt/rocm/lib -lamdhip64
 *   contrib_client <problem file> <result file>
 * The problem file is written by the Python side: the scene block of client_common.h (int32 P D M W H, float32 tanfovx tanfovy
 * scale_modifier, then float32 bg [3], means3D [P,3], shs [P,M,3], opacities [P], scales [P,3], rotations [P,4], viewmatrix [16],
 * projmatrix [16], campos [3]) and nothing else.  The client renders once
 * (gsr_forward), makes every refusal of the two calls on rows that hold a pattern -- each must come with its code and its text and
 * leave the rows as they were -- then clears the rows, adds the view twice and reads them.  It writes int64 R, the rows after one view
 * [P,16 bytes], after two, and weight_sum [P], weight_max [P], pixel_count [P] of the two.  The Python side judges the numbers. */
#include "gsr_contrib.h"
#include "client_common.h"

int main(int argc, char **argv) {
    if (argc < 3) { printf("usage: contrib_client <problem file> <result file>\n"); return 3; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 3; }
    struct cabi_scene s = {0};
    struct cabi_render r;
    int rc = cabi_scene_read(f, &s);
    fclose(f);
    if (rc) return rc;
    if (gsr_abi_version() != GSR_ABI_VERSION) { printf("ABI version mismatch\n"); return 1; }

    if ((rc = cabi_render(&s, &r)) != 0) return rc;
    const int32_t P = s.P, W = s.W, H = s.H;
    const size_t n = (size_t)P, gb = r.gb, ib = r.ib, binning_bytes = r.binning_bytes;
    void *geom = r.geom, *img = r.img, *binning = r.binning;
    const int64_t R = r.R;
    gsr_contrib_row_t *rows = dev_out(n * sizeof(gsr_contrib_row_t));         /* the one output the refusals are held against */
    if (!rows) { printf("hipMalloc failed\n"); return 2; }
    float *wsum, *wmax;
    int32_t *npix;
    CK(hipMalloc((void **)&wsum, n * 4)); CK(hipMalloc((void **)&wmax, n * 4)); CK(hipMalloc((void **)&npix, n * 4));

    /* ---- refusals, and the calls with nothing to do: the rows keep the pattern ---- */
    EXPECT_PREFIX(gsr_contrib_accumulate(NULL, -1, W, H, R, geom, gb, binning, binning_bytes, img, ib, rows), GSR_ERR_INVALID_ARGUMENT, "gsr_contrib_accumulate: bad sizes");
    EXPECT_PREFIX(gsr_contrib_accumulate(NULL, P, 0, H, R, geom, gb, binning, binning_bytes, img, ib, rows), GSR_ERR_INVALID_ARGUMENT, "gsr_contrib_accumulate: bad sizes");
    EXPECT_PREFIX(gsr_contrib_accumulate(NULL, P, W, H, -1, geom, gb, binning, binning_bytes, img, ib, rows), GSR_ERR_INVALID_ARGUMENT, "gsr_contrib_accumulate: bad sizes");
    EXPECT_PREFIX(gsr_contrib_accumulate(NULL, P, 65536 * 16, H, R, geom, gb, binning, binning_bytes, img, ib, rows), GSR_ERR_INVALID_ARGUMENT, "gsr_contrib_accumulate: image too large");
    EXPECT_PREFIX(gsr_contrib_accumulate(NULL, P, W, H, R, geom, gb - 1, binning, binning_bytes, img, ib, rows), GSR_ERR_WORKSPACE, "gsr_contrib_accumulate: geom workspace ");
    EXPECT_PREFIX(gsr_contrib_accumulate(NULL, P, W, H, R, geom, gb, binning, binning_bytes, img, ib - 1, rows), GSR_ERR_WORKSPACE, "gsr_contrib_accumulate: image workspace ");
    EXPECT_PREFIX(gsr_contrib_accumulate(NULL, P, W, H, R, geom, gb, binning, (size_t)R * 5 - 1, img, ib, rows), GSR_ERR_WORKSPACE, "gsr_contrib_accumulate: binning workspace too small for R=");
    EXPECT_PREFIX(gsr_contrib_accumulate(NULL, P, W, H, R, geom, gb, binning, binning_bytes, img, ib, NULL), GSR_ERR_INVALID_ARGUMENT, "gsr_contrib_accumulate: missing rows or workspace");
    EXPECT_PREFIX(gsr_contrib_accumulate(NULL, P, W, H, R, NULL, gb, binning, binning_bytes, img, ib, rows), GSR_ERR_INVALID_ARGUMENT, "gsr_contrib_accumulate: missing rows or workspace");
    EXPECT_PREFIX(gsr_contrib_accumulate(NULL, P, W, H, R, geom, gb, NULL, binning_bytes, img, ib, rows), GSR_ERR_INVALID_ARGUMENT, "gsr_contrib_accumulate: missing rows or workspace");
    EXPECT_PREFIX(gsr_contrib_accumulate(NULL, P, W, H, R, geom, gb, binning, binning_bytes, NULL, ib, rows), GSR_ERR_INVALID_ARGUMENT, "gsr_contrib_accumulate: missing rows or workspace");
    /* the order: sizes, then the three views (geometry, image, binning), then the pointers */
    EXPECT_PREFIX(gsr_contrib_accumulate(NULL, P, W, -2, R, geom, 0, binning, 0, img, 0, NULL), GSR_ERR_INVALID_ARGUMENT, "gsr_contrib_accumulate: bad sizes");
    EXPECT_PREFIX(gsr_contrib_accumulate(NULL, P, W, H, R, geom, 0, binning, 0, img, 0, NULL), GSR_ERR_WORKSPACE, "gsr_contrib_accumulate: geom workspace 0 < ");
    EXPECT_PREFIX(gsr_contrib_accumulate(NULL, P, W, H, R, geom, gb, binning, 0, img, 0, NULL), GSR_ERR_WORKSPACE, "gsr_contrib_accumulate: image workspace 0 < ");
    EXPECT_PREFIX(gsr_contrib_accumulate(NULL, P, W, H, R, geom, gb, binning, 0, img, ib, NULL), GSR_ERR_WORKSPACE, "gsr_contrib_accumulate: binning workspace too small");
    EXPECT_PREFIX(gsr_contrib_accumulate(NULL, 0, W, H, R, NULL, 0, NULL, 0, NULL, 0, rows), GSR_OK, "");
    EXPECT_PREFIX(gsr_contrib_accumulate(NULL, P, W, H, 0, geom, gb, NULL, 0, img, ib, rows), GSR_OK, "");
    EXPECT_PREFIX(gsr_contrib_accumulate(NULL, P, W, H, 0, NULL, 0, NULL, 0, NULL, 0, NULL), GSR_OK, "");
    EXPECT_PREFIX(gsr_contrib_read(NULL, P, rows, NULL, NULL, NULL), GSR_ERR_INVALID_ARGUMENT, "gsr_contrib_read: weight_sum, weight_max and pixel_count are all NULL");
    EXPECT_PREFIX(gsr_contrib_read(NULL, 0, rows, NULL, NULL, NULL), GSR_ERR_INVALID_ARGUMENT, "gsr_contrib_read: weight_sum, weight_max and pixel_count are all NULL");
    EXPECT_PREFIX(gsr_contrib_read(NULL, -1, rows, wsum, wmax, npix), GSR_ERR_INVALID_ARGUMENT, "gsr_contrib_read: bad sizes");
    EXPECT_PREFIX(gsr_contrib_read(NULL, P, NULL, wsum, wmax, npix), GSR_ERR_INVALID_ARGUMENT, "gsr_contrib_read: missing rows");
    EXPECT_PREFIX(gsr_contrib_read(NULL, 0, NULL, wsum, NULL, NULL), GSR_OK, "");
    EXPECT_PREFIX(gsr_contrib_read(NULL, P, rows, wsum, wmax, npix), GSR_OK, "");        /* reading leaves the rows alone too */

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
