/* Plain-C client of absgrad of libgsr_hip.so (include/gsr_absgrad.h): no torch, no C++ types.
 * Built and run by tests/test_gpu_absgrad_cabi.py on the GPU box:
 *   gcc absgrad_client.c -I<repo>/include -I/opt/rocm/include -L<pkg> -lgsr_hip -L/opt/rocm/lib -lamdhip64
 *   absgrad_client <problem file> <result file>
 * The problem file is written by the Python side: the scene block of client_common.h (int32 P D M W H, float32 tanfovx tanfovy
 * scale_modifier, then float32 bg [3], means3D [P,3], shs [P,M,3], opacities [P], scales [P,3], rotations [P,4], viewmatrix [16],
 * projmatrix [16], campos [3]), then dL_dcolor [3,H,W].  The client renders once (gsr_forward), makes every refusal of the call on outputs that hold a pattern -- each must come with its code and
 * its text and leave the outputs as they were -- then P == 0, R == 0 with and without accumulate, and the call itself: accumulate = 0
 * with the signed sums, then accumulate = 1 without them onto the first result.  It writes int64 R, absgrad [P,2], signed_sum [P,2],
 * the accumulated absgrad [P,2] and the R == 0 output [P,2].  The Python side judges the numbers. */
#include "gsr_absgrad.h"
#include "client_common.h"

int main(int argc, char **argv) {
    if (argc < 3) { printf("usage: absgrad_client <problem file> <result file>\n"); return 3; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 3; }
    struct cabi_scene s = {0};
    struct cabi_render r;
    int rc = cabi_scene_read(f, &s);
    if (rc) return rc;
    const int32_t P = s.P, W = s.W, H = s.H;
    const size_t n = (size_t)P, px = (size_t)3 * W * H * 4;
    const float *bg = s.bg, *dL = dev_copy(rd(f, px), px);
    fclose(f);
    if (!dL) { printf("hipMalloc failed\n"); return 2; }
    if (gsr_abi_version() != GSR_ABI_VERSION) { printf("ABI version mismatch\n"); return 1; }

    if ((rc = cabi_render(&s, &r)) != 0) return rc;
    void *geom = r.geom, *img = r.img, *binning = r.binning, *ws;
    const size_t gb = r.gb, ib = r.ib, binning_bytes = r.binning_bytes;
    const int64_t R = r.R;
    size_t wb = 0;
    if (gsr_absgrad_workspace_bytes(P, &wb) != GSR_OK || wb == 0) { printf("absgrad workspace size: %s\n", gsr_last_error()); return 1; }
    CK(hipMalloc(&ws, wb));
    float *out = dev_out(n * 8), *sgn = dev_out(n * 8), *first;
    if (!out || !sgn) { printf("hipMalloc failed\n"); return 2; }
    CK(hipMalloc((void **)&first, n * 8));

    /* ---- refusals, and the calls with nothing to do: the outputs keep the pattern ---- */
#define WHO "gsr_absgrad_backward: "
#define MISSING WHO "missing input, workspace or output buffer"
#define CALL(P_, W_, H_, R_, bg_, dL_, g_, gb_, b_, bb_, i_, ib_, ws_, wb_, acc_, out_, sgn_) \
    gsr_absgrad_backward(NULL, P_, W_, H_, R_, bg_, dL_, g_, gb_, b_, bb_, i_, ib_, ws_, wb_, acc_, out_, sgn_)
    EXPECT_PREFIX(CALL(-1, W, H, R, bg, dL, geom, gb, binning, binning_bytes, img, ib, ws, wb, 0, out, sgn), GSR_ERR_INVALID_ARGUMENT, WHO "bad sizes");
    EXPECT_PREFIX(CALL(P, 0, H, R, bg, dL, geom, gb, binning, binning_bytes, img, ib, ws, wb, 0, out, sgn), GSR_ERR_INVALID_ARGUMENT, WHO "bad sizes");
    EXPECT_PREFIX(CALL(P, W, H, -1, bg, dL, geom, gb, binning, binning_bytes, img, ib, ws, wb, 0, out, sgn), GSR_ERR_INVALID_ARGUMENT, WHO "bad sizes");
    EXPECT_PREFIX(CALL(P, 65536 * 16, H, R, bg, dL, geom, gb, binning, binning_bytes, img, ib, ws, wb, 0, out, sgn), GSR_ERR_INVALID_ARGUMENT, "image too large");
    EXPECT_PREFIX(CALL(P, W, H, R, NULL, dL, geom, gb, binning, binning_bytes, img, ib, ws, wb, 0, out, sgn), GSR_ERR_INVALID_ARGUMENT, MISSING);
    EXPECT_PREFIX(CALL(P, W, H, R, bg, NULL, geom, gb, binning, binning_bytes, img, ib, ws, wb, 0, out, sgn), GSR_ERR_INVALID_ARGUMENT, MISSING);
    EXPECT_PREFIX(CALL(P, W, H, R, bg, dL, NULL, gb, binning, binning_bytes, img, ib, ws, wb, 0, out, sgn), GSR_ERR_INVALID_ARGUMENT, MISSING);
    EXPECT_PREFIX(CALL(P, W, H, R, bg, dL, geom, gb, binning, binning_bytes, NULL, ib, ws, wb, 0, out, sgn), GSR_ERR_INVALID_ARGUMENT, MISSING);
    EXPECT_PREFIX(CALL(P, W, H, R, bg, dL, geom, gb, binning, binning_bytes, img, ib, NULL, wb, 0, out, sgn), GSR_ERR_INVALID_ARGUMENT, MISSING);
    EXPECT_PREFIX(CALL(P, W, H, R, bg, dL, geom, gb, binning, binning_bytes, img, ib, ws, wb, 0, NULL, sgn), GSR_ERR_INVALID_ARGUMENT, MISSING);
    EXPECT_PREFIX(CALL(P, W, H, R, bg, dL, geom, gb, NULL, binning_bytes, img, ib, ws, wb, 0, out, sgn), GSR_ERR_INVALID_ARGUMENT, WHO "binning workspace missing");
    EXPECT_PREFIX(CALL(P, W, H, R, bg, dL, geom, gb, binning, binning_bytes, img, ib, ws, wb - 1, 0, out, sgn), GSR_ERR_WORKSPACE, "absgrad workspace ");
    EXPECT_PREFIX(CALL(P, W, H, R, bg, dL, geom, gb - 1, binning, binning_bytes, img, ib, ws, wb, 0, out, sgn), GSR_ERR_WORKSPACE, "geom workspace ");
    EXPECT_PREFIX(CALL(P, W, H, R, bg, dL, geom, gb, binning, binning_bytes, img, ib - 1, ws, wb, 0, out, sgn), GSR_ERR_WORKSPACE, "image workspace ");
    EXPECT_PREFIX(CALL(P, W, H, R, bg, dL, geom, gb, binning, (size_t)R * 5 - 1, img, ib, ws, wb, 0, out, sgn), GSR_ERR_WORKSPACE, "binning workspace too small for R=");
    if (gsr_set_option("deterministic_bwd", 1) != GSR_OK) { printf("set option: %s\n", gsr_last_error()); return 1; }
    EXPECT_PREFIX(CALL(P, W, H, R, bg, dL, geom, gb, binning, binning_bytes, img, ib, ws, wb, 0, out, sgn), GSR_ERR_INVALID_ARGUMENT,
           WHO "not available while the option deterministic_bwd is on");
    if (gsr_set_option("deterministic_bwd", 0) != GSR_OK) { printf("set option: %s\n", gsr_last_error()); return 1; }
    /* the order: sizes, pointers, own workspace, then the three views (geometry, image, binning) */
    EXPECT_PREFIX(CALL(P, W, -2, R, bg, dL, geom, 0, binning, 0, img, 0, ws, 0, 0, NULL, sgn), GSR_ERR_INVALID_ARGUMENT, WHO "bad sizes");
    EXPECT_PREFIX(CALL(P, W, H, R, bg, dL, geom, 0, binning, 0, img, 0, ws, 0, 0, NULL, sgn), GSR_ERR_INVALID_ARGUMENT, MISSING);
    EXPECT_PREFIX(CALL(P, W, H, R, bg, dL, geom, 0, binning, 0, img, 0, ws, 0, 0, out, sgn), GSR_ERR_WORKSPACE, "absgrad workspace 0 < ");
    EXPECT_PREFIX(CALL(P, W, H, R, bg, dL, geom, 0, binning, 0, img, 0, ws, wb, 0, out, sgn), GSR_ERR_WORKSPACE, "geom workspace 0 < ");
    EXPECT_PREFIX(CALL(P, W, H, R, bg, dL, geom, gb, binning, 0, img, 0, ws, wb, 0, out, sgn), GSR_ERR_WORKSPACE, "image workspace 0 < ");
    EXPECT_PREFIX(CALL(P, W, H, R, bg, dL, geom, gb, binning, 0, img, ib, ws, wb, 0, out, sgn), GSR_ERR_WORKSPACE, "binning workspace too small");
    EXPECT_PREFIX(CALL(0, W, H, R, NULL, NULL, NULL, 0, NULL, 0, NULL, 0, NULL, 0, 0, out, sgn), GSR_OK, "");          /* P == 0: nothing */
    EXPECT_PREFIX(CALL(P, W, H, 0, bg, dL, geom, gb, NULL, 0, img, ib, ws, wb, 1, out, sgn), GSR_OK, "");             /* R == 0, accumulate: nothing */

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
    CK(outs_fill());
    if (CALL(P, W, H, 0, bg, dL, geom, gb, NULL, 0, img, ib, ws, wb, 0, out, NULL) != GSR_OK) { printf("absgrad, R = 0: %s\n", gsr_last_error()); return 1; }
    CK(hipDeviceSynchronize());
    bad |= dump(res, out, n * 8);
    if (fclose(res) || bad) { printf("could not write the results\n"); return 3; }
    printf("absgrad C client ok\n");
    return 0;
}
