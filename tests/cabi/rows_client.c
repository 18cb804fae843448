/* Plain-C client of the row entry points of libgsr_hip.so (include/gsr_rows.h): no torch, no C++ types.
 * Built and run by tests/test_gpu_rows_cabi.py on the GPU box:
 *   gcc rows_client.c -I<repo>/include -I/opt/rocm/include -L<pkg> -lgsr_hip -L/opt/rocm/lib -lamdhip64
 *   rows_client <problem file>
 * The problem file is written by the Python side: int32 P D B, then float32 rows [P,D], the expected xyz [P,3], f_dc [P,3],
 * f_rest [P,3(K-1)], opacity [P], scaling [P,3], rotation [P,4] (tests/rows_ref.py unpack_ref), B arenas of P (3 K + 11) floats
 * each, and the expected grad_rows [P,D] (pack_ref).  Everything is compared bit for bit. */
#include "gsr_rows.h"
#include "client_common.h"

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: rows_client <problem file>\n"); return 3; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 3; }
    int32_t hdr[3];
    rd_into(f, hdr, sizeof hdr);
    const int32_t P = hdr[0], D = hdr[1], B = hdr[2];
    const int32_t K = (D - 14) / 3;
    if (B < 1 || B > GSR_ROWS_MAX_B || K < 2) { printf("bad problem header\n"); return 3; }
    const size_t e = (size_t)P * D, n = (size_t)P * (3 * K + 11);
    const size_t w[6] = {3, 3, 3 * (size_t)(K - 1), 1, 3, 4};
    const char *names[6] = {"xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"};
    float *rows = rd(f, e * 4), *want[6], *arenas[GSR_ROWS_MAX_B];
    for (int k = 0; k < 6; k++) want[k] = rd(f, (size_t)P * w[k] * 4);
    for (int b = 0; b < B; b++) arenas[b] = rd(f, n * 4);
    float *want_grad = rd(f, e * 4);
    fclose(f);
    if (gsr_abi_version() != GSR_ABI_VERSION) { printf("ABI version mismatch\n"); return 1; }

    /* ---- unpack ---- */
    float *d_rows = dev_copy(rows, e * 4), *d_out[6];
    for (int k = 0; k < 6; k++) CK(hipMalloc((void **)&d_out[k], (size_t)P * w[k] * 4 + 16));
    EXPECT_CODE(gsr_rows_unpack(NULL, P, 18, d_rows, d_out[0], d_out[1], d_out[2], d_out[3], d_out[4], d_out[5]), GSR_ERR_INVALID_ARGUMENT, "D = 18");
    EXPECT_CODE(gsr_rows_unpack(NULL, P, D, d_rows, d_out[0], d_out[1], d_out[2], d_out[3], d_out[4], d_out[5] + 1), GSR_ERR_INVALID_ARGUMENT,
           "misaligned rotation");
    EXPECT_CODE(gsr_rows_unpack(NULL, 0, D, NULL, NULL, NULL, d_out[2], NULL, NULL, NULL), GSR_OK, "P = 0");
    EXPECT_CODE(gsr_rows_unpack(NULL, P, D, d_rows, d_out[0], d_out[1], d_out[2], d_out[3], d_out[4], d_out[5]), GSR_OK, "unpack");
    CK(hipDeviceSynchronize());
    for (int k = 0; k < 6; k++) {
        const size_t bytes = (size_t)P * w[k] * 4;
        float *h = malloc(bytes);
        CK(hipMemcpy(h, d_out[k], bytes, hipMemcpyDeviceToHost));
        if (memcmp(h, want[k], bytes)) { printf("%s differs from the Python side's\n", names[k]); return 1; }
        free(h);
    }

    /* ---- gradient pack ---- */
    const float *d_arenas[GSR_ROWS_MAX_B + 1];
    for (int b = 0; b < B; b++) d_arenas[b] = dev_copy(arenas[b], n * 4);
    for (int b = B; b <= GSR_ROWS_MAX_B; b++) d_arenas[b] = d_arenas[0];
    float *d_grad;
    CK(hipMalloc((void **)&d_grad, e * 4));
    EXPECT_CODE(gsr_rows_grad_pack(NULL, P, D, GSR_ROWS_MAX_B + 1, d_arenas, d_grad), GSR_ERR_INVALID_ARGUMENT, "B = 65");
    EXPECT_CODE(gsr_rows_grad_pack(NULL, P, D, 0, d_arenas, d_grad), GSR_ERR_INVALID_ARGUMENT, "B = 0");
    EXPECT_CODE(gsr_rows_grad_pack(NULL, P, D, B, d_arenas, (float *)d_arenas[B - 1] + 1), GSR_ERR_INVALID_ARGUMENT, "grad_rows inside an arena");
    EXPECT_CODE(gsr_rows_grad_pack(NULL, P, D, B, d_arenas, d_grad), GSR_OK, "grad pack");
    CK(hipDeviceSynchronize());
    float *h_grad = malloc(e * 4);
    CK(hipMemcpy(h_grad, d_grad, e * 4, hipMemcpyDeviceToHost));
    if (memcmp(h_grad, want_grad, e * 4)) { printf("grad_rows differs from the Python side's\n"); return 1; }
    printf("rows C client ok\n");
    return 0;
}
