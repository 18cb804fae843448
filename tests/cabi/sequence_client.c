/* Plain-C client of the sequence entry points of libgsr_hip.so (include/gsr_sequence.h): no torch, no C++ types.
 * Built and run by tests/test_gpu_sequence_cabi.py on the GPU box:
 *   gcc sequence_client.c -I<repo>/include -I/opt/rocm/include -L<pkg> -lgsr_hip -L/opt/rocm/lib -lamdhip64
 *   sequence_client <problem file>
 * The problem file is written by the Python side: int32 P D xyz_col n Q B, then float32 rows [P,D], the expected float32
 * out_rows [P,D], int32 perm [P], int32 count; then float32 means [Q,3] scales [Q,3] rotations [Q,4] view [B,16] proj [B,16]
 * tanfovx [B] tanfovy [B], int32 widths [B] heights [B], and the expected int32 radii [B,Q] (float32 CPU oracle). */
#include "gsr_sequence.h"
#include "client_common.h"

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: sequence_client <problem file>\n"); return 3; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 3; }
    int32_t hdr[6];
    rd_into(f, hdr, sizeof hdr);
    const int32_t P = hdr[0], D = hdr[1], col = hdr[2], n = hdr[3], Q = hdr[4], B = hdr[5];
    const size_t e = (size_t)P * D;
    float *rows = rd(f, e * 4), *w_rows = rd(f, e * 4);
    int32_t *w_perm = rd(f, (size_t)P * 4), *w_count = rd(f, 4);
    float *means = rd(f, (size_t)Q * 12), *scales = rd(f, (size_t)Q * 12), *rots = rd(f, (size_t)Q * 16);
    float *view = rd(f, (size_t)B * 64), *proj = rd(f, (size_t)B * 64), *tfx = rd(f, (size_t)B * 4), *tfy = rd(f, (size_t)B * 4);
    int32_t *ws_ = rd(f, (size_t)B * 4), *hs_ = rd(f, (size_t)B * 4), *w_radii = rd(f, (size_t)B * Q * 4);
    fclose(f);
    if (gsr_abi_version() != GSR_ABI_VERSION) { printf("ABI version mismatch\n"); return 1; }

    /* ---- box sort ---- */
    float *d_rows = dev_copy(rows, e * 4), *d_out; int32_t *d_perm, *d_count; void *ws;
    CK(hipMalloc((void **)&d_out, e * 4)); CK(hipMalloc((void **)&d_perm, (size_t)P * 4)); CK(hipMalloc((void **)&d_count, 4));
    size_t wb = 0;
    EXPECT_CODE(gsr_box_sort_workspace(P, n, &wb), GSR_OK, "workspace");
    if (wb < 12 * (size_t)P) { printf("workspace %zu < 12 P\n", wb); return 1; }
    CK(hipMalloc(&ws, wb));
    EXPECT_CODE(gsr_box_sort_workspace(P, 129, &wb), GSR_ERR_INVALID_ARGUMENT, "workspace n = 129");
    EXPECT_CODE(gsr_box_sort_workspace(P, n, &wb), GSR_OK, "workspace");
    EXPECT_CODE(gsr_box_sort(NULL, P, D, d_rows, col, n, d_out, d_perm, d_count, ws, wb - 1), GSR_ERR_WORKSPACE, "small workspace");
    EXPECT_CODE(gsr_box_sort(NULL, P, D, d_rows, col, n, d_rows, d_perm, d_count, ws, wb), GSR_ERR_INVALID_ARGUMENT, "rows == out_rows");
    EXPECT_CODE(gsr_box_sort(NULL, P, D, d_rows, col, 0, d_out, d_perm, d_count, ws, wb), GSR_ERR_INVALID_ARGUMENT, "n = 0");
    EXPECT_CODE(gsr_box_sort(NULL, P, 2, d_rows, 0, n, d_out, d_perm, d_count, ws, wb), GSR_ERR_INVALID_ARGUMENT, "D = 2");
    EXPECT_CODE(gsr_box_sort(NULL, P, D, d_rows, D - 2, n, d_out, d_perm, d_count, ws, wb), GSR_ERR_INVALID_ARGUMENT, "xyz_col = D - 2");
    EXPECT_CODE(gsr_box_sort(NULL, P, D, NULL, col, n, d_out, d_perm, d_count, ws, wb), GSR_ERR_INVALID_ARGUMENT, "rows = NULL");
    int32_t h_count = -5;
    EXPECT_CODE(gsr_box_sort(NULL, 0, D, NULL, col, n, NULL, NULL, d_count, NULL, 0), GSR_OK, "P = 0");
    CK(hipMemcpy(&h_count, d_count, 4, hipMemcpyDeviceToHost));
    if (h_count != 0) { printf("P = 0: count %d\n", h_count); return 1; }
    EXPECT_CODE(gsr_box_sort(NULL, P, D, d_rows, col, n, d_out, d_perm, d_count, ws, wb), GSR_OK, "box sort");
    CK(hipDeviceSynchronize());
    float *h_out = malloc(e * 4); int32_t *h_perm = malloc((size_t)P * 4);
    CK(hipMemcpy(h_out, d_out, e * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(h_perm, d_perm, (size_t)P * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(&h_count, d_count, 4, hipMemcpyDeviceToHost));
    if (h_count != w_count[0]) { printf("count %d, expected %d\n", h_count, w_count[0]); return 1; }
    if (memcmp(h_perm, w_perm, (size_t)P * 4)) { printf("perm differs from the Python side's\n"); return 1; }
    if (memcmp(h_out, w_rows, e * 4)) { printf("rows differ from the Python side's\n"); return 1; }

    /* ---- visibility ---- */
    float *d_means = dev_copy(means, (size_t)Q * 12), *d_scales = dev_copy(scales, (size_t)Q * 12), *d_rots = dev_copy(rots, (size_t)Q * 16);
    float *d_view = dev_copy(view, (size_t)B * 64), *d_proj = dev_copy(proj, (size_t)B * 64);
    int32_t *d_radii, *d_counts; uint8_t *d_vis;
    CK(hipMalloc((void **)&d_radii, (size_t)B * Q * 4)); CK(hipMalloc((void **)&d_counts, (size_t)B * 4)); CK(hipMalloc((void **)&d_vis, Q));
#define VIS(P_, B_, sc_, cov_, raw_, r_, v_, c_) gsr_visible_union(NULL, P_, B_, d_means, sc_, 1.0f, d_rots, cov_, raw_, d_view, d_proj, tfx, tfy, ws_, hs_, r_, v_, c_)
    EXPECT_CODE(VIS(Q, 0, d_scales, NULL, 0, d_radii, d_vis, d_counts), GSR_ERR_INVALID_ARGUMENT, "B = 0");
    EXPECT_CODE(VIS(Q, 65, d_scales, NULL, 0, d_radii, d_vis, d_counts), GSR_ERR_INVALID_ARGUMENT, "B = 65");
    EXPECT_CODE(VIS(Q, B, NULL, NULL, 0, d_radii, d_vis, d_counts), GSR_ERR_INVALID_ARGUMENT, "no covariance source");
    EXPECT_CODE(VIS(Q, B, d_scales, d_means, 0, d_radii, d_vis, d_counts), GSR_ERR_INVALID_ARGUMENT, "two covariance sources");
    EXPECT_CODE(VIS(Q, B, NULL, d_means, 1, d_radii, d_vis, d_counts), GSR_ERR_INVALID_ARGUMENT, "raw_params with cov3D_precomp");
    EXPECT_CODE(VIS(Q, B, d_scales, NULL, 0, NULL, NULL, NULL), GSR_OK, "all outputs NULL");
    EXPECT_CODE(VIS(Q, B, d_scales, NULL, 0, d_radii, d_vis, d_counts), GSR_OK, "visible union");
    CK(hipDeviceSynchronize());
    int32_t *h_radii = malloc((size_t)B * Q * 4), *h_counts = malloc((size_t)B * 4); uint8_t *h_vis = malloc(Q);
    CK(hipMemcpy(h_radii, d_radii, (size_t)B * Q * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(h_counts, d_counts, (size_t)B * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(h_vis, d_vis, Q, hipMemcpyDeviceToHost));
    if (memcmp(h_radii, w_radii, (size_t)B * Q * 4)) { printf("radii differ from the float32 CPU oracle's\n"); return 1; }
    for (int b = 0; b < B; b++) {
        int c = 0;
        for (int i = 0; i < Q; i++) c += w_radii[(size_t)b * Q + i] > 0;
        if (c != h_counts[b]) { printf("counts[%d] = %d, expected %d\n", b, h_counts[b], c); return 1; }
    }
    for (int i = 0; i < Q; i++) {
        int any = 0;
        for (int b = 0; b < B; b++) any |= w_radii[(size_t)b * Q + i] > 0;
        if (h_vis[i] != any) { printf("visible[%d] = %d, expected %d\n", i, h_vis[i], any); return 1; }
    }
    printf("sequence C client ok\n");
    return 0;
}
