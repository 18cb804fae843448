/* Plain-C client of the Chamfer entry points of libgsr_hip.so (include/gsr_chamfer.h): no torch, no C++ types.
 * Built and run by tests/test_gpu_chamfer_cabi.py on the GPU box:
 *   gcc chamfer_client.c -I<repo>/include -I/opt/rocm/include -L<pkg> -lgsr_hip -L/opt/rocm/lib -lamdhip64
 *   chamfer_client <problem file>
 * The problem file is written by the Python side: int32 B N M D, then float32 x1 x2 g1 g2, the expected float32 dist1 dist2,
 * int32 idx1 idx2, float32 dx1 dx2 (float64 reference, rounded), and the float32 tolerances of dist1 dist2 dx1 dx2. */
#include <math.h>
#include "gsr_chamfer.h"
#include "client_common.h"

static int close_f(const char *what, const float *got, const float *want, const float *tol, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!(fabs((double)got[i] - (double)want[i]) <= (double)tol[i])) {
            printf("%s[%zu] = %.9g, expected %.9g +- %.3g\n", what, i, got[i], want[i], tol[i]);
            return 0;
        }
    return 1;
}

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: chamfer_client <problem file>\n"); return 3; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 3; }
    int32_t hdr[4];
    rd_into(f, hdr, sizeof hdr);
    const int32_t B = hdr[0], N = hdr[1], M = hdr[2], D = hdr[3];
    const size_t n1 = (size_t)B * N, n2 = (size_t)B * M, e1 = n1 * D, e2 = n2 * D;
    float *x1 = rd(f, e1 * 4), *x2 = rd(f, e2 * 4), *g1 = rd(f, n1 * 4), *g2 = rd(f, n2 * 4);
    float *w_d1 = rd(f, n1 * 4), *w_d2 = rd(f, n2 * 4);
    int32_t *w_i1 = rd(f, n1 * 4), *w_i2 = rd(f, n2 * 4);
    float *w_dx1 = rd(f, e1 * 4), *w_dx2 = rd(f, e2 * 4);
    float *t_d1 = rd(f, n1 * 4), *t_d2 = rd(f, n2 * 4), *t_dx1 = rd(f, e1 * 4), *t_dx2 = rd(f, e2 * 4);
    fclose(f);

    if (gsr_abi_version() != GSR_ABI_VERSION) { printf("ABI version mismatch\n"); return 1; }
    float *d_x1 = dev_copy(x1, e1 * 4), *d_x2 = dev_copy(x2, e2 * 4), *d_g1 = dev_copy(g1, n1 * 4), *d_g2 = dev_copy(g2, n2 * 4);
    float *d_d1, *d_d2, *d_dx1, *d_dx2; int32_t *d_i1, *d_i2; void *ws;
    CK(hipMalloc((void **)&d_d1, n1 * 4)); CK(hipMalloc((void **)&d_d2, n2 * 4)); CK(hipMalloc((void **)&d_i1, n1 * 4)); CK(hipMalloc((void **)&d_i2, n2 * 4));
    CK(hipMalloc((void **)&d_dx1, e1 * 4)); CK(hipMalloc((void **)&d_dx2, e2 * 4));
    size_t wb = 0;
    if (gsr_chamfer_workspace(B, N, M, &wb) != GSR_OK || wb != 8 * (n1 + n2)) { printf("workspace: %zu (%s)\n", wb, gsr_last_error()); return 1; }
    CK(hipMalloc(&ws, wb));

    /* error paths first: codes, not aborts, and the device stays usable */
    int rc = gsr_chamfer_forward(NULL, B, N, M, D, d_x1, d_x2, d_d1, d_d2, d_i1, d_i2, ws, wb - 1);
    if (rc != GSR_ERR_WORKSPACE || strlen(gsr_last_error()) == 0) { printf("expected WORKSPACE with a message, got %d\n", rc); return 1; }
    rc = gsr_chamfer_forward(NULL, B, 0, M, D, d_x1, d_x2, d_d1, d_d2, d_i1, d_i2, ws, wb);
    if (rc != GSR_ERR_INVALID_ARGUMENT) { printf("expected INVALID_ARGUMENT for N = 0, got %d\n", rc); return 1; }
    rc = gsr_chamfer_forward(NULL, B, N, 0, D, d_x1, d_x2, d_d1, d_d2, d_i1, d_i2, ws, wb);
    if (rc != GSR_ERR_INVALID_ARGUMENT) { printf("expected INVALID_ARGUMENT for M = 0, got %d\n", rc); return 1; }
    rc = gsr_chamfer_forward(NULL, B, N, M, 65, d_x1, d_x2, d_d1, d_d2, d_i1, d_i2, ws, wb);
    if (rc != GSR_ERR_INVALID_ARGUMENT) { printf("expected INVALID_ARGUMENT for D = 65, got %d\n", rc); return 1; }
    rc = gsr_chamfer_forward(NULL, B, N, M, 0, d_x1, d_x2, d_d1, d_d2, d_i1, d_i2, ws, wb);
    if (rc != GSR_ERR_INVALID_ARGUMENT) { printf("expected INVALID_ARGUMENT for D = 0, got %d\n", rc); return 1; }
    rc = gsr_chamfer_forward(NULL, B, N, M, D, d_x1, NULL, d_d1, d_d2, d_i1, d_i2, ws, wb);
    if (rc != GSR_ERR_INVALID_ARGUMENT) { printf("expected INVALID_ARGUMENT for x2 = NULL, got %d\n", rc); return 1; }
    rc = gsr_chamfer_backward(NULL, B, N, 0, D, d_x1, d_x2, d_i1, d_i2, d_g1, d_g2, d_dx1, d_dx2);
    if (rc != GSR_ERR_INVALID_ARGUMENT) { printf("backward: expected INVALID_ARGUMENT for M = 0, got %d\n", rc); return 1; }
    if (gsr_chamfer_forward(NULL, 0, N, M, D, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0) != GSR_OK) { printf("B = 0 must succeed\n"); return 1; }
    if (gsr_chamfer_forward(NULL, B, 0, 0, D, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0) != GSR_OK) { printf("N = M = 0 must succeed\n"); return 1; }

    /* the real calls */
    rc = gsr_chamfer_forward(NULL, B, N, M, D, d_x1, d_x2, d_d1, d_d2, d_i1, d_i2, ws, wb);
    if (rc != GSR_OK) { printf("forward failed: %s\n", gsr_last_error()); return 1; }
    rc = gsr_chamfer_backward(NULL, B, N, M, D, d_x1, d_x2, d_i1, d_i2, d_g1, d_g2, d_dx1, d_dx2);
    if (rc != GSR_OK) { printf("backward failed: %s\n", gsr_last_error()); return 1; }
    CK(hipDeviceSynchronize());
    float *h_d1 = malloc(n1 * 4), *h_d2 = malloc(n2 * 4), *h_dx1 = malloc(e1 * 4), *h_dx2 = malloc(e2 * 4);
    int32_t *h_i1 = malloc(n1 * 4), *h_i2 = malloc(n2 * 4);
    CK(hipMemcpy(h_d1, d_d1, n1 * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(h_d2, d_d2, n2 * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(h_i1, d_i1, n1 * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(h_i2, d_i2, n2 * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(h_dx1, d_dx1, e1 * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(h_dx2, d_dx2, e2 * 4, hipMemcpyDeviceToHost));
    if (memcmp(h_i1, w_i1, n1 * 4) || memcmp(h_i2, w_i2, n2 * 4)) { printf("indices differ from the Python side's\n"); return 1; }
    if (!close_f("dist1", h_d1, w_d1, t_d1, n1) || !close_f("dist2", h_d2, w_d2, t_d2, n2)) return 1;
    if (!close_f("dx1", h_dx1, w_dx1, t_dx1, e1) || !close_f("dx2", h_dx2, w_dx2, t_dx2, e2)) return 1;

    /* g2 = NULL and dx2 = NULL: dx1 is the direct term alone and is fully written; an out-of-range index is skipped */
    int32_t *bad = malloc(n1 * 4); memcpy(bad, h_i1, n1 * 4); bad[0] = M; bad[1] = -1;
    int32_t *d_bad = dev_copy(bad, n1 * 4);
    CK(hipMemset(d_dx1, 0x7f, e1 * 4));
    rc = gsr_chamfer_backward(NULL, B, N, M, D, d_x1, d_x2, d_bad, d_i2, d_g1, NULL, d_dx1, NULL);
    if (rc != GSR_OK) { printf("backward (g2 = NULL) failed: %s\n", gsr_last_error()); return 1; }
    CK(hipMemcpy(h_dx1, d_dx1, e1 * 4, hipMemcpyDeviceToHost));
    for (size_t e = 0; e < e1; e++) {
        const size_t row = e / D; const int k = (int)(e % D);
        const size_t b = row / N;
        const float want = row < 2 ? 0.f : 2.f * g1[row] * (x1[e] - x2[(b * M + (size_t)h_i1[row]) * D + k]);
        if (!(fabsf(h_dx1[e] - want) <= 4.f * 5.9604645e-8f * fabsf(want))) { printf("direct term dx1[%zu] = %.9g, expected %.9g\n", e, h_dx1[e], want); return 1; }
    }
    printf("chamfer C client ok\n");
    return 0;
}
