/* Plain-C client of the camera-gradient entry points of libgsr_hip.so (include/gsr_pose.h): no torch, no C++ types.
 * Built and run by tests/test_gpu_pose_cabi.py on the GPU box:
 *   gcc pose_client.c -I<repo>/include -I/opt/rocm/include -L<pkg> -lgsr_hip -L/opt/rocm/lib -lamdhip64
 *   pose_client <problem file>
 * The problem file is written by the Python side: the scene block of client_common.h (int32 P D M W H, float32 tanfovx tanfovy
 * scale_modifier, then float32 bg [3], means3D [P,3], shs [P,M,3], opacities [P], scales [P,3], rotations [P,4], viewmatrix [16],
 * projmatrix [16], campos [3]), then float32 dL_dpix [3,H,W]; then float64 the reference's dL_dviewmatrix [16], dL_dprojmatrix [16], dL_dcampos [3] (tests/pose_ref.py, float64)
 * and three float64 bounds on the error of each tensor relative to the reference's largest entry. */
#include <math.h>
#include "gsr_pose.h"
#include "client_common.h"

static int compare(const char *name, const float *got, const double *want, int n, double bound) {
    double big = 0, err = 0;
    for (int i = 0; i < n; i++) { if (fabs(want[i]) > big) big = fabs(want[i]); }
    for (int i = 0; i < n; i++) { const double d = fabs((double)got[i] - want[i]); if (!(d <= err)) err = d; }
    const double rel = big > 0 ? err / big : err;
    printf("%s: error %.3e of the largest entry, bound %.3e\n", name, rel, bound);
    return rel <= bound ? 0 : 1;
}

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: pose_client <problem file>\n"); return 3; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 3; }
    struct cabi_scene s = {.spare = 4};               /* one float past every input: a read past an array's end stays inside its allocation */
    struct cabi_render r;
    int rc = cabi_scene_read(f, &s);
    if (rc) return rc;
    const int32_t P = s.P, D = s.D, M = s.M, W = s.W, H = s.H;
    const float tanx = s.tanfovx, tany = s.tanfovy, mod = s.scale_modifier;
    const size_t px = (size_t)3 * W * H * 4;
    float *dl = rd(f, px);
    double *want = rd(f, 35 * 8), *bound = rd(f, 3 * 8);
    fclose(f);
    if (gsr_abi_version() != GSR_ABI_VERSION) { printf("ABI version mismatch\n"); return 1; }

    float *d_bg = s.bg, *d_means = s.means3D, *d_shs = s.shs, *d_sc = s.scales, *d_rot = s.rotations, *d_view = s.viewmatrix, *d_proj = s.projmatrix;
    float *d_cam = s.campos, *d_dl = dev_copy_spare(dl, px, s.spare);
    if (!d_dl) { printf("hipMalloc failed\n"); return 2; }
    if ((rc = cabi_render(&s, &r)) != 0) return rc;
    void *geom = r.geom, *img = r.img, *bwd, *pws;
    int32_t *radii = r.radii;
    const size_t gb = r.gb, ib = r.ib;
    const int64_t n = r.R;
    size_t wb, pb;
    EXPECT_CODE(gsr_pose_workspace_bytes(P, &pb), GSR_OK, "pose workspace size");
    if (pb != (size_t)((P + 255) / 256) * 256) { printf("pose workspace %zu\n", pb); return 1; }
    CK(hipMalloc(&pws, pb));
    EXPECT_CODE(gsr_backward_workspace_bytes(P, n, &wb), GSR_OK, "backward workspace size");
    CK(hipMalloc(&bwd, wb));
    float *g2, *go, *g3, *gsh, *gs, *gr;
    CK(hipMalloc((void **)&g2, (size_t)P * 12)); CK(hipMalloc((void **)&go, (size_t)P * 4)); CK(hipMalloc((void **)&g3, (size_t)P * 12));
    CK(hipMalloc((void **)&gsh, (size_t)P * M * 12)); CK(hipMalloc((void **)&gs, (size_t)P * 12)); CK(hipMalloc((void **)&gr, (size_t)P * 16));
    EXPECT_CODE(gsr_backward(NULL, P, D, M, n, W, H, d_bg, d_means, radii, d_shs, NULL, d_sc, mod, d_rot, NULL, d_view, d_proj, d_cam, tanx, tany, d_dl,
                        geom, gb, r.binning, r.binning_bytes, img, ib, bwd, wb, g2, go, NULL, g3, NULL, gsh, gs, gr, 0, NULL, 0, NULL), GSR_OK, "backward");

    float *d_out;                       /* 16 + 16 + 3 outputs between two guard floats each */
    float h_out[41];
    for (int i = 0; i < 41; i++) h_out[i] = NAN;
    CK(hipMalloc((void **)&d_out, sizeof h_out));
    CK(hipMemcpy(d_out, h_out, sizeof h_out, hipMemcpyHostToDevice));
    float *gV = d_out + 1, *gP = d_out + 19, *gC = d_out + 37;
#define POSE(kind, p, d, m, shs_, col_, sc_, rot_, cov_, accb, wsb, o1, o2, o3) \
    gsr_pose_backward(NULL, kind, p, d, m, W, H, n, d_means, radii, shs_, col_, sc_, mod, rot_, cov_, d_view, d_proj, d_cam, tanx, tany, geom, gb, \
                      bwd, accb, pws, wsb, o1, o2, o3)
    /* refusals: nothing is enqueued, nothing is written */
    EXPECT_CODE(POSE(3, P, D, M, d_shs, NULL, d_sc, d_rot, NULL, wb, pb, gV, gP, gC), GSR_ERR_INVALID_ARGUMENT, "kind 3");
    EXPECT_CODE(POSE(0, P, D, M, d_shs, NULL, d_sc, d_rot, NULL, wb, pb, NULL, NULL, NULL), GSR_ERR_INVALID_ARGUMENT, "no output");
    EXPECT_CODE(POSE(0, P, D, M, d_shs, d_shs, d_sc, d_rot, NULL, wb, pb, gV, gP, gC), GSR_ERR_INVALID_ARGUMENT, "shs and colors");
    EXPECT_CODE(POSE(0, P, D, M, d_shs, NULL, d_sc, NULL, NULL, wb, pb, gV, gP, gC), GSR_ERR_INVALID_ARGUMENT, "scales without rotations");
    EXPECT_CODE(POSE(0, P, 4, M, d_shs, NULL, d_sc, d_rot, NULL, wb, pb, gV, gP, gC), GSR_ERR_INVALID_ARGUMENT, "D = 4");
    EXPECT_CODE(POSE(0, P, D, M, d_shs, NULL, d_sc, d_rot, NULL, 64, pb, gV, gP, gC), GSR_ERR_WORKSPACE, "accumulator workspace too small");
    EXPECT_CODE(POSE(0, P, D, M, d_shs, NULL, d_sc, d_rot, NULL, wb, pb - 1, gV, gP, gC), GSR_ERR_WORKSPACE, "pose workspace too small");
    EXPECT_CODE(gsr_pose_backward(NULL, 0, P, D, M, W, H, n, d_means, radii, d_shs, NULL, d_sc, mod, d_rot, NULL, d_view, d_proj, d_cam, tanx, tany, geom, gb / 2,
                             bwd, wb, pws, pb, gV, gP, gC), GSR_ERR_WORKSPACE, "geometry workspace too small");
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h_out, d_out, sizeof h_out, hipMemcpyDeviceToHost));
    for (int i = 0; i < 41; i++) if (!isnan(h_out[i])) { printf("a refused call wrote output %d\n", i); return 1; }

    /* the call, twice: same bits; the guards stay */
    float first[41];
    EXPECT_CODE(POSE(0, P, D, M, d_shs, NULL, d_sc, d_rot, NULL, wb, pb, gV, gP, gC), GSR_OK, "pose backward");
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(first, d_out, sizeof first, hipMemcpyDeviceToHost));
    EXPECT_CODE(POSE(0, P, D, M, d_shs, NULL, d_sc, d_rot, NULL, wb, pb, gV, gP, gC), GSR_OK, "pose backward again");
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h_out, d_out, sizeof h_out, hipMemcpyDeviceToHost));
    if (memcmp(first, h_out, sizeof first)) { printf("two calls on one workspace differ\n"); return 1; }
    if (!isnan(h_out[0]) || !isnan(h_out[17]) || !isnan(h_out[18]) || !isnan(h_out[35]) || !isnan(h_out[36]) || !isnan(h_out[40])) { printf("a guard float was written\n"); return 1; }
    int bad = compare("dL_dviewmatrix", h_out + 1, want, 16, bound[0]) + compare("dL_dprojmatrix", h_out + 19, want + 16, 16, bound[1]) +
              compare("dL_dcampos", h_out + 37, want + 32, 3, bound[2]);
    if (bad) return 1;
    for (int k = 0; k < 4; k++) {
        const float zv = h_out[1 + 4 * k + 3], zp = h_out[19 + 4 * k + 2];
        if (zv != 0.f || signbit(zv) || zp != 0.f || signbit(zp)) { printf("structural zero %d is not +0\n", k); return 1; }
    }

    /* one output alone: the same bits, the others untouched */
    float h2[41];
    for (int i = 0; i < 41; i++) h2[i] = NAN;
    CK(hipMemcpy(d_out, h2, sizeof h2, hipMemcpyHostToDevice));
    EXPECT_CODE(POSE(0, P, D, M, d_shs, NULL, d_sc, d_rot, NULL, wb, pb, NULL, NULL, gC), GSR_OK, "campos alone");
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h2, d_out, sizeof h2, hipMemcpyDeviceToHost));
    if (memcmp(h2 + 37, first + 37, 12)) { printf("campos alone differs\n"); return 1; }
    for (int i = 0; i < 37; i++) if (!isnan(h2[i])) { printf("a NULL output was written (%d)\n", i); return 1; }

    /* P = 0 and R = 0: zeros, no workspace read */
    EXPECT_CODE(gsr_pose_backward(NULL, 0, 0, D, M, W, H, 0, NULL, NULL, NULL, NULL, NULL, mod, NULL, NULL, NULL, NULL, NULL, tanx, tany, NULL, 0, NULL, 0, NULL, 0,
                             gV, gP, gC), GSR_OK, "P = 0");
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h2, d_out, sizeof h2, hipMemcpyDeviceToHost));
    for (int i = 1; i < 40; i++) if (i != 17 && i != 18 && i != 35 && i != 36 && (h2[i] != 0.f || signbit(h2[i]))) { printf("P = 0: output %d is not +0\n", i); return 1; }
    CK(hipMemcpy(d_out, first, sizeof first, hipMemcpyHostToDevice));
    EXPECT_CODE(gsr_pose_backward(NULL, 2, P, D, M, W, H, 0, NULL, NULL, NULL, NULL, NULL, mod, NULL, NULL, NULL, NULL, NULL, tanx, tany, NULL, 0, NULL, 0, NULL, 0,
                             gV, NULL, gC), GSR_OK, "R = 0");
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h2, d_out, sizeof h2, hipMemcpyDeviceToHost));
    for (int i = 1; i < 17; i++) if (h2[i] != 0.f) { printf("R = 0: viewmatrix %d not zero\n", i); return 1; }
    if (memcmp(h2 + 19, first + 19, 64)) { printf("R = 0: the NULL output was written\n"); return 1; }
    printf("pose C client ok\n");
    return 0;
}
