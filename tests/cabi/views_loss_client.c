/* Plain-C client of the multi-view loss entry points of libgsr_hip.so (include/gsr_loss.h): no torch, no C++ types.
 * Built and run by tests/test_gpu_views_loss_cabi.py on the GPU box:
 *   gcc views_loss_client.c -I<repo>/include -I/opt/rocm/include -L<pkg> -lgsr_hip -L/opt/rocm/lib -lamdhip64
 *   views_loss_client <problem file> <gradient file>
 * The problem file is written by the Python side: int32 B H W sanitize, float32 w_l1 w_ssim, then float32 images [B,3,H,W] and
 * targets [B,3,H,W].  Prints "out3" and "terms" as the bit patterns of the floats (and readably), writes the B gradient images. */
#include "gsr_loss.h"
#include "client_common.h"

#define MAXB 64

static int expect_invalid(const char *what, int rc) {
    if (rc == GSR_ERR_INVALID_ARGUMENT && strlen(gsr_last_error()) > 0) return 1;
    printf("%s: expected INVALID_ARGUMENT with a message, got %d\n", what, rc);
    return 0;
}
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main(int argc, char **argv) {
    if (argc < 3) { printf("usage: views_loss_client <problem file> <gradient file>\n"); return 3; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 3; }
    int32_t hdr[4]; float w[2];
    rd_into(f, hdr, sizeof hdr); rd_into(f, w, sizeof w);
    const int32_t B = hdr[0], H = hdr[1], W = hdr[2], sanitize = hdr[3];
    if (B < 1 || B > MAXB) return 3;
    const size_t view = (size_t)3 * H * W, n = view * B;
    float *h_img = rd(f, n * 4), *h_gt = rd(f, n * 4), *h_grad = malloc(n * 4);
    if (!h_grad) return 3;
    fclose(f);

    if (gsr_abi_version() != GSR_ABI_VERSION) { printf("ABI version mismatch\n"); return 1; }
    /* every view in an allocation of its own: the library is handed B pointers, not one batch */
    const float *imgs[MAXB], *gts[MAXB]; float *grads[MAXB];
    for (int b = 0; b < B; b++) {
        float *a, *c, *g;
        CK(hipMalloc((void **)&a, view * 4)); CK(hipMalloc((void **)&c, view * 4)); CK(hipMalloc((void **)&g, view * 4));
        CK(hipMemcpy(a, h_img + b * view, view * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(c, h_gt + b * view, view * 4, hipMemcpyHostToDevice));
        CK(hipMemset(g, 0x7f, view * 4));
        imgs[b] = a; gts[b] = c; grads[b] = g;
    }
    size_t wb = 0;
    if (gsr_views_loss_workspace(B, H, W, &wb) != GSR_OK || wb < (size_t)36 * B * H * W) { printf("workspace: %zu (%s)\n", wb, gsr_last_error()); return 1; }
    void *ws; float *out3, *terms;
    CK(hipMalloc(&ws, wb)); CK(hipMalloc((void **)&out3, 12)); CK(hipMalloc((void **)&terms, (size_t)B * 12));

    /* error paths first: codes, not aborts, nothing launched, and the device stays usable */
    size_t dummy;
    if (!expect_invalid("workspace B = 0", gsr_views_loss_workspace(0, H, W, &dummy))) return 1;
    if (!expect_invalid("workspace H = 0", gsr_views_loss_workspace(B, 0, W, &dummy))) return 1;
    if (!expect_invalid("B = 0", gsr_views_loss_forward(NULL, 0, H, W, imgs, gts, w[0], w[1], sanitize, out3, terms, ws, wb))) return 1;
    if (!expect_invalid("B = -1", gsr_views_loss_forward(NULL, -1, H, W, imgs, gts, w[0], w[1], sanitize, out3, terms, ws, wb))) return 1;
    if (!expect_invalid("H = 0", gsr_views_loss_forward(NULL, B, 0, W, imgs, gts, w[0], w[1], sanitize, out3, terms, ws, wb))) return 1;
    if (!expect_invalid("W = 0", gsr_views_loss_forward(NULL, B, H, 0, imgs, gts, w[0], w[1], sanitize, out3, terms, ws, wb))) return 1;
    if (!expect_invalid("imgs = NULL", gsr_views_loss_forward(NULL, B, H, W, NULL, gts, w[0], w[1], sanitize, out3, terms, ws, wb))) return 1;
    if (!expect_invalid("ws = NULL", gsr_views_loss_forward(NULL, B, H, W, imgs, gts, w[0], w[1], sanitize, out3, terms, NULL, wb))) return 1;
    if (!expect_invalid("small ws", gsr_views_loss_forward(NULL, B, H, W, imgs, gts, w[0], w[1], sanitize, out3, terms, ws, wb - 1))) return 1;
    {
        const float *hole[MAXB];
        memcpy(hole, imgs, sizeof(hole));
        hole[B - 1] = NULL;
        if (!expect_invalid("imgs[B-1] = NULL", gsr_views_loss_forward(NULL, B, H, W, hole, gts, w[0], w[1], sanitize, out3, terms, ws, wb))) return 1;
        if (!expect_invalid("gts[B-1] = NULL", gsr_views_loss_forward(NULL, B, H, W, imgs, hole, w[0], w[1], sanitize, out3, terms, ws, wb))) return 1;
        if (!expect_invalid("backward imgs[B-1] = NULL", gsr_views_loss_backward(NULL, B, H, W, hole, gts, w[0], w[1], sanitize, NULL, ws, wb, grads))) return 1;
    }
    if (!expect_invalid("backward small ws", gsr_views_loss_backward(NULL, B, H, W, imgs, gts, w[0], w[1], sanitize, NULL, ws, wb - 1, grads))) return 1;

    /* the real calls */
    int rc = gsr_views_loss_forward(NULL, B, H, W, imgs, gts, w[0], w[1], sanitize, out3, terms, ws, wb);
    if (rc != GSR_OK) { printf("forward failed: %s\n", gsr_last_error()); return 1; }
    rc = gsr_views_loss_backward(NULL, B, H, W, imgs, gts, w[0], w[1], sanitize, NULL, ws, wb, grads);
    if (rc != GSR_OK) { printf("backward failed: %s\n", gsr_last_error()); return 1; }
    CK(hipDeviceSynchronize());
    float h_out[3], h_terms[3 * MAXB];
    CK(hipMemcpy(h_out, out3, 12, hipMemcpyDeviceToHost)); CK(hipMemcpy(h_terms, terms, (size_t)B * 12, hipMemcpyDeviceToHost));
    for (int b = 0; b < B; b++) CK(hipMemcpy(h_grad + b * view, grads[b], view * 4, hipMemcpyDeviceToHost));
    printf("out3 %08x %08x %08x  loss %.9g L1 %.9g SSIM %.9g\n", bits(h_out[0]), bits(h_out[1]), bits(h_out[2]), h_out[0], h_out[1], h_out[2]);
    printf("terms");
    for (int i = 0; i < 3 * B; i++) printf(" %08x", bits(h_terms[i]));
    printf("\n");

    /* a NULL gradient pointer: that view's image is left alone, the others are written as before */
    if (B > 1) {
        float *some[MAXB];
        memcpy(some, grads, sizeof(some));
        some[0] = NULL;
        CK(hipMemset(grads[0], 0x7f, view * 4)); CK(hipMemset(grads[1], 0, view * 4));
        rc = gsr_views_loss_backward(NULL, B, H, W, imgs, gts, w[0], w[1], sanitize, NULL, ws, wb, some);
        if (rc != GSR_OK) { printf("backward (NULL gradient) failed: %s\n", gsr_last_error()); return 1; }
        float *chk = malloc(view * 4);
        CK(hipMemcpy(chk, grads[0], view * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < view; i++) if (bits(chk[i]) != 0x7f7f7f7fu) { printf("view 0 was written at %zu\n", i); return 1; }
        CK(hipMemcpy(chk, grads[1], view * 4, hipMemcpyDeviceToHost));
        if (memcmp(chk, h_grad + view, view * 4)) { printf("view 1 differs when view 0 wants no gradient\n"); return 1; }
        free(chk);
    }
    f = fopen(argv[2], "wb");
    if (!f || fwrite(h_grad, 4, n, f) != n) { printf("cannot write %s\n", argv[2]); return 3; }
    fclose(f);
    printf("views loss C client ok\n");
    return 0;
}
