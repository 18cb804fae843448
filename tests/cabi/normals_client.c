/* Plain-C client of the surface-normal calls of libgsr_hip.so (include/gsr_normals.h): no torch, no C++ types.
 * Built and run by tests/test_gpu_normals_cabi.py on the GPU box:
 *   gcc normals_client.c -I<repo>/include -I/opt/rocm/include -L<pkg> -lgsr_hip -L/opt/rocm/lib -lamdhip64
 *   normals_client <problem file> <result file>
 *   normals_client --refusals            the refusals alone, on made-up addresses that are never followed: needs no device
 * The problem file is written by the Python side: int32 P H W, float32 tanfovx tanfovy alpha_min, then float32 means3D [P,3],
 * scales [P,3], rotations [P,4], viewmatrix [16], dL_dnormals [P,3], depth [H,W], alpha [H,W], normals [3,H,W].  The client makes every
 * refusal of the five calls on outputs that hold a pattern -- each must come with its code and its text and leave the outputs as they
 * were -- then the calls with nothing to do, then the five calls themselves.  It writes normals [P,3], axis [P] int32, dL_drots [P,4],
 * out2 [2], out_surf [3,H,W], dL_ddepth [H,W], dL_dalpha [H,W], dL_dnormals [3,H,W] of the unscaled backward call, and dL_ddepth [H,W] of
 * a call with grad_loss = 0.25 and the other two outputs NULL.  The Python side judges the numbers. */
#include "gsr_normals.h"
#include "client_common.h"

struct bufs {
    int32_t P, H, W;
    float tx, ty, amin;
    const float *means, *scales, *rots, *view, *gN, *depth, *alpha, *normals;
    float *out_n, *g_rots, *out2, *surf, *gd, *ga, *gn;
    int32_t *axis;
    void *ws;
    size_t wb;
};

/* Every refusal, in the header's order, and the calls with nothing to do.  None of them follows a pointer. */
static int refusals(const struct bufs *b) {
    const int32_t P = b->P, H = b->H, W = b->W;
    size_t n = 0;
#define GF "gsr_gaussian_normals_forward: "
#define GB "gsr_gaussian_normals_backward: "
#define LW "gsr_normal_loss_workspace: "
#define LF "gsr_normal_loss_forward: "
#define LB "gsr_normal_loss_backward: "
#define AMIN "alpha_min must be positive (D = depth / alpha is formed where alpha >= alpha_min)"
#define INV GSR_ERR_INVALID_ARGUMENT
    EXPECT_TEXT(gsr_gaussian_normals_forward(NULL, -1, b->means, b->scales, b->rots, b->view, b->out_n, b->axis), INV, GF "bad sizes");
    EXPECT_TEXT(gsr_gaussian_normals_forward(NULL, P, NULL, b->scales, b->rots, b->view, b->out_n, b->axis), INV, GF "missing input or output buffer");
    EXPECT_TEXT(gsr_gaussian_normals_forward(NULL, P, b->means, NULL, b->rots, b->view, b->out_n, b->axis), INV, GF "missing input or output buffer");
    EXPECT_TEXT(gsr_gaussian_normals_forward(NULL, P, b->means, b->scales, NULL, b->view, b->out_n, b->axis), INV, GF "missing input or output buffer");
    EXPECT_TEXT(gsr_gaussian_normals_forward(NULL, P, b->means, b->scales, b->rots, NULL, b->out_n, b->axis), INV, GF "missing input or output buffer");
    EXPECT_TEXT(gsr_gaussian_normals_forward(NULL, P, b->means, b->scales, b->rots, b->view, NULL, b->axis), INV, GF "missing input or output buffer");
    EXPECT_TEXT(gsr_gaussian_normals_forward(NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL), GSR_OK, "");
    EXPECT_TEXT(gsr_gaussian_normals_backward(NULL, -1, b->rots, b->view, b->axis, b->gN, b->g_rots), INV, GB "bad sizes");
    EXPECT_TEXT(gsr_gaussian_normals_backward(NULL, P, NULL, b->view, b->axis, b->gN, b->g_rots), INV, GB "missing input or output buffer");
    EXPECT_TEXT(gsr_gaussian_normals_backward(NULL, P, b->rots, NULL, b->axis, b->gN, b->g_rots), INV, GB "missing input or output buffer");
    EXPECT_TEXT(gsr_gaussian_normals_backward(NULL, P, b->rots, b->view, NULL, b->gN, b->g_rots), INV, GB "missing input or output buffer");
    EXPECT_TEXT(gsr_gaussian_normals_backward(NULL, P, b->rots, b->view, b->axis, NULL, b->g_rots), INV, GB "missing input or output buffer");
    EXPECT_TEXT(gsr_gaussian_normals_backward(NULL, P, b->rots, b->view, b->axis, b->gN, NULL), INV, GB "missing input or output buffer");
    EXPECT_TEXT(gsr_gaussian_normals_backward(NULL, 0, NULL, NULL, NULL, NULL, NULL), GSR_OK, "");
    EXPECT_TEXT(gsr_normal_loss_workspace(0, W, &n), INV, LW "bad sizes");
    EXPECT_TEXT(gsr_normal_loss_workspace(H, 0, &n), INV, LW "bad sizes");
    EXPECT_TEXT(gsr_normal_loss_workspace(H, W, NULL), INV, LW "bad argument");
    EXPECT_TEXT(gsr_normal_loss_workspace(8 * 65535 + 1, W, &n), INV, LW "image too large");
#define FWD(H_, W_, am_, d_, a_, n_, o2_, ws_, wb_) gsr_normal_loss_forward(NULL, H_, W_, b->tx, b->ty, am_, d_, a_, n_, o2_, b->surf, ws_, wb_)
    EXPECT_TEXT(FWD(0, W, b->amin, b->depth, b->alpha, b->normals, b->out2, b->ws, b->wb), INV, LF "bad sizes");
    EXPECT_TEXT(FWD(H, -3, b->amin, b->depth, b->alpha, b->normals, b->out2, b->ws, b->wb), INV, LF "bad sizes");
    EXPECT_TEXT(FWD(H, (1 << 20) + 1, b->amin, b->depth, b->alpha, b->normals, b->out2, b->ws, b->wb), INV, LF "image too large");
    EXPECT_TEXT(FWD(H, W, 0.f, b->depth, b->alpha, b->normals, b->out2, b->ws, b->wb), INV, LF AMIN);
    EXPECT_TEXT(FWD(H, W, -1.f, b->depth, b->alpha, b->normals, b->out2, b->ws, b->wb), INV, LF AMIN);
    EXPECT_TEXT(FWD(H, W, b->amin, NULL, b->alpha, b->normals, b->out2, b->ws, b->wb), INV, LF "missing input, output or workspace");
    EXPECT_TEXT(FWD(H, W, b->amin, b->depth, NULL, b->normals, b->out2, b->ws, b->wb), INV, LF "missing input, output or workspace");
    EXPECT_TEXT(FWD(H, W, b->amin, b->depth, b->alpha, NULL, b->out2, b->ws, b->wb), INV, LF "missing input, output or workspace");
    EXPECT_TEXT(FWD(H, W, b->amin, b->depth, b->alpha, b->normals, NULL, b->ws, b->wb), INV, LF "missing input, output or workspace");
    EXPECT_TEXT(FWD(H, W, b->amin, b->depth, b->alpha, b->normals, b->out2, NULL, b->wb), INV, LF "missing input, output or workspace");
    {
        char text[128];
        snprintf(text, sizeof text, LF "workspace %zu < %zu", b->wb - 1, b->wb);
        EXPECT_TEXT(FWD(H, W, b->amin, b->depth, b->alpha, b->normals, b->out2, b->ws, b->wb - 1), GSR_ERR_WORKSPACE, text);
    }
    /* the order: sizes, alpha_min, pointers, the workspace's size */
    EXPECT_TEXT(FWD(0, W, 0.f, NULL, b->alpha, b->normals, b->out2, b->ws, 0), INV, LF "bad sizes");
    EXPECT_TEXT(FWD(H, W, 0.f, NULL, b->alpha, b->normals, b->out2, b->ws, 0), INV, LF AMIN);
    EXPECT_TEXT(FWD(H, W, b->amin, NULL, b->alpha, b->normals, b->out2, b->ws, 0), INV, LF "missing input, output or workspace");
#define BWD(H_, W_, am_, d_, a_, n_, gd_, ga_, gn_) gsr_normal_loss_backward(NULL, H_, W_, b->tx, b->ty, am_, d_, a_, n_, NULL, gd_, ga_, gn_)
    EXPECT_TEXT(BWD(H, 0, b->amin, b->depth, b->alpha, b->normals, b->gd, b->ga, b->gn), INV, LB "bad sizes");
    EXPECT_TEXT(BWD(-1, W, b->amin, b->depth, b->alpha, b->normals, b->gd, b->ga, b->gn), INV, LB "bad sizes");
    EXPECT_TEXT(BWD(H, W, 0.f, b->depth, b->alpha, b->normals, b->gd, b->ga, b->gn), INV, LB AMIN);
    EXPECT_TEXT(BWD(H, W, b->amin, NULL, b->alpha, b->normals, b->gd, b->ga, b->gn), INV, LB "missing input");
    EXPECT_TEXT(BWD(H, W, b->amin, b->depth, NULL, b->normals, b->gd, b->ga, b->gn), INV, LB "missing input");
    EXPECT_TEXT(BWD(H, W, b->amin, b->depth, b->alpha, NULL, b->gd, b->ga, b->gn), INV, LB "missing input");
    EXPECT_TEXT(BWD(H, W, b->amin, b->depth, b->alpha, b->normals, NULL, NULL, NULL), GSR_OK, "");        /* no output wanted: nothing runs */
    return 0;
}

int main(int argc, char **argv) {
    if (gsr_abi_version() != GSR_ABI_VERSION) { printf("ABI version mismatch\n"); return 1; }
    if (argc == 2 && strcmp(argv[1], "--refusals") == 0) {
        static float stand_in[8];                       /* addresses only: no refused call follows a pointer */
        struct bufs b = {10, 16, 40, 0.5f, 0.5f, 0.05f, stand_in, stand_in, stand_in, stand_in, stand_in, stand_in, stand_in, stand_in,
                         stand_in, stand_in, stand_in, stand_in, stand_in, stand_in, stand_in, (int32_t *)stand_in, stand_in, 0};
        if (gsr_normal_loss_workspace(b.H, b.W, &b.wb) != GSR_OK || b.wb != 256) { printf("workspace size: %s\n", gsr_last_error()); return 1; }
        const int rc = refusals(&b);
        if (rc == 0) printf("normals C client: refusals ok\n");
        return rc;
    }
    if (argc < 3) { printf("usage: normals_client <problem file> <result file> | --refusals\n"); return 3; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 3; }
    int32_t hdr[3];
    float par[3];
    rd_into(f, hdr, sizeof hdr); rd_into(f, par, sizeof par);
    struct bufs b;
    memset(&b, 0, sizeof b);
    b.P = hdr[0]; b.H = hdr[1]; b.W = hdr[2]; b.tx = par[0]; b.ty = par[1]; b.amin = par[2];
    if (b.P < 1 || b.H < 1 || b.W < 1) { printf("bad problem header\n"); return 3; }
    const size_t n = (size_t)b.P, px = (size_t)b.H * b.W * 4;
    b.means = dev_copy(rd(f, n * 12), n * 12); b.scales = dev_copy(rd(f, n * 12), n * 12); b.rots = dev_copy(rd(f, n * 16), n * 16);
    b.view = dev_copy(rd(f, 64), 64); b.gN = dev_copy(rd(f, n * 12), n * 12);
    b.depth = dev_copy(rd(f, px), px); b.alpha = dev_copy(rd(f, px), px); b.normals = dev_copy(rd(f, 3 * px), 3 * px);
    fclose(f);
    if (!b.means || !b.scales || !b.rots || !b.view || !b.gN || !b.depth || !b.alpha || !b.normals) { printf("hipMalloc failed\n"); return 2; }
    if (gsr_normal_loss_workspace(b.H, b.W, &b.wb) != GSR_OK || b.wb == 0) { printf("workspace size: %s\n", gsr_last_error()); return 1; }
    CK(hipMalloc(&b.ws, b.wb));
    b.out_n = (float *)dev_out(n * 12); b.axis = (int32_t *)dev_out(n * 4); b.g_rots = (float *)dev_out(n * 16); b.out2 = (float *)dev_out(8);
    b.surf = (float *)dev_out(3 * px); b.gd = (float *)dev_out(px); b.ga = (float *)dev_out(px); b.gn = (float *)dev_out(3 * px);
    if (!b.out_n || !b.axis || !b.g_rots || !b.out2 || !b.surf || !b.gd || !b.ga || !b.gn) { printf("hipMalloc failed\n"); return 2; }

    const int rc = refusals(&b);
    if (rc) return rc;

    FILE *res = fopen(argv[2], "wb");
    if (!res) { printf("cannot write %s\n", argv[2]); return 3; }
    if (gsr_gaussian_normals_forward(NULL, b.P, b.means, b.scales, b.rots, b.view, b.out_n, b.axis) != GSR_OK ||
        gsr_gaussian_normals_backward(NULL, b.P, b.rots, b.view, b.axis, b.gN, b.g_rots) != GSR_OK) { printf("gaussian normals: %s\n", gsr_last_error()); return 1; }
    if (gsr_normal_loss_forward(NULL, b.H, b.W, b.tx, b.ty, b.amin, b.depth, b.alpha, b.normals, b.out2, b.surf, b.ws, b.wb) != GSR_OK ||
        gsr_normal_loss_backward(NULL, b.H, b.W, b.tx, b.ty, b.amin, b.depth, b.alpha, b.normals, NULL, b.gd, b.ga, b.gn) != GSR_OK) {
        printf("normal loss: %s\n", gsr_last_error()); return 1;
    }
    CK(hipDeviceSynchronize());
    int bad = dump(res, b.out_n, n * 12) | dump(res, b.axis, n * 4) | dump(res, b.g_rots, n * 16) | dump(res, b.out2, 8) | dump(res, b.surf, 3 * px) |
              dump(res, b.gd, px) | dump(res, b.ga, px) | dump(res, b.gn, 3 * px);
    /* grad_loss = 0.25 from the device, depth alone: the other two outputs keep what they hold */
    const float quarter = 0.25f;
    float *gl = dev_copy(&quarter, 4);
    if (!gl) { printf("hipMalloc failed\n"); return 2; }
    CK(hipMemset(b.ga, PATTERN, px)); CK(hipMemset(b.gn, PATTERN, 3 * px));
    if (gsr_normal_loss_backward(NULL, b.H, b.W, b.tx, b.ty, b.amin, b.depth, b.alpha, b.normals, gl, b.gd, NULL, NULL) != GSR_OK) {
        printf("normal loss backward: %s\n", gsr_last_error()); return 1;
    }
    CK(hipDeviceSynchronize());
    bad |= dump(res, b.gd, px);
    if (buf_changed(b.ga, px) || buf_changed(b.gn, 3 * px)) { printf("a NULL output's neighbour was written\n"); return 1; }
    if (fclose(res) || bad) { printf("could not write the results\n"); return 3; }
    printf("normals C client ok\n");
    return 0;
}
