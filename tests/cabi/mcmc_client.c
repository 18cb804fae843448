/* Plain-C client of the MCMC density-control entry points of libgsr_hip.so (include/gsr_mcmc.h): no torch, no C++ types.
 * Built and run by tests/test_gpu_mcmc_cabi.py on the GPU box:
 *   gcc mcmc_client.c -I<repo>/include -I/opt/rocm/include -L<pkg> -lgsr_hip -L/opt/rocm/lib -lamdhip64
 *   mcmc_client <problem file> <result file>
 * The problem file is written by the Python side: int32 P, six int32 widths (xyz, f_dc, f_rest, opacity, scaling, rotation), float32 L,
 * float64 min_opacity, float32 gate_k gate_t scale, then float32 u [P], noise [P,3], and per group the parameter [P,w], exp_avg [P,w],
 * exp_avg_sq [P,w].  The client relocates in place (plan + apply), then adds the noise, and writes: uint32 counts[4], per group the
 * parameter and both moments after the relocation, and xyz [P,3] after the noise.  The Python side judges the numbers. */
#include "gsr_mcmc.h"
#include "client_common.h"

int main(int argc, char **argv) {
    if (argc < 3) { printf("usage: mcmc_client <problem file> <result file>\n"); return 3; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 3; }
    int32_t hdr[7];
    float L, gate[3];
    double m;
    rd_into(f, hdr, sizeof hdr); rd_into(f, &L, 4); rd_into(f, &m, 8); rd_into(f, gate, sizeof gate);
    const int32_t P = hdr[0], *w = hdr + 1;
    const int32_t role[6] = {GSR_MCMC_COPY, GSR_MCMC_COPY, GSR_MCMC_COPY, GSR_MCMC_OPACITY, GSR_MCMC_SCALING, GSR_MCMC_COPY};
    if (P < 1 || w[0] != 3 || w[3] != 1 || w[4] != 3 || w[5] != 4) { printf("bad problem header\n"); return 3; }
    float *u = dev_copy(rd(f, (size_t)P * 4), (size_t)P * 4), *noise = dev_copy(rd(f, (size_t)P * 12), (size_t)P * 12);
    float *par[6], *m1[6], *m2[6];
    for (int k = 0; k < 6; k++) {
        const size_t bytes = (size_t)P * w[k] * 4;
        par[k] = dev_copy(rd(f, bytes), bytes); m1[k] = dev_copy(rd(f, bytes), bytes); m2[k] = dev_copy(rd(f, bytes), bytes);
        if (!par[k] || !m1[k] || !m2[k]) { printf("hipMalloc failed\n"); return 2; }
    }
    fclose(f);
    if (gsr_abi_version() != GSR_ABI_VERSION) { printf("ABI version mismatch\n"); return 1; }

    size_t need = 0;
    EXPECT_CODE(gsr_mcmc_plan_workspace(P, 0, &need), GSR_OK, "workspace size");
    void *ws;
    uint32_t *counts;
    CK(hipMalloc(&ws, need));
    CK(hipHostMalloc((void **)&counts, 16, 0));
    EXPECT_CODE(gsr_mcmc_plan(NULL, GSR_MCMC_RELOCATE, P, par[3], par[4], L, m, 0, 0, u, counts, ws, need), GSR_ERR_INVALID_ARGUMENT, "n_max = 0");
    EXPECT_CODE(gsr_mcmc_plan(NULL, GSR_MCMC_RELOCATE, P, par[3], par[4], L, m, GSR_MCMC_N_MAX, 0, u, counts, ws, need - 1), GSR_ERR_WORKSPACE, "short workspace");
    EXPECT_CODE(gsr_mcmc_plan(NULL, GSR_MCMC_RELOCATE, P, par[3], par[4], L, m, GSR_MCMC_N_MAX, 0, u, counts, ws, need), GSR_OK, "plan");
    gsr_mcmc_group_t g[6];
    for (int k = 0; k < 6; k++) {
        g[k].src = par[k]; g[k].src_exp_avg = m1[k]; g[k].src_exp_avg_sq = m2[k];
        g[k].dst = par[k]; g[k].dst_exp_avg = m1[k]; g[k].dst_exp_avg_sq = m2[k];
        g[k].width_floats = w[k]; g[k].role = role[k];
    }
    EXPECT_CODE(gsr_mcmc_apply(NULL, GSR_MCMC_RELOCATE, P, 0, GSR_MCMC_MAX_GROUPS + 1, g, ws, need), GSR_ERR_INVALID_ARGUMENT, "17 groups");
    EXPECT_CODE(gsr_mcmc_apply(NULL, GSR_MCMC_RELOCATE, P, 0, 6, g, ws, need), GSR_OK, "apply");
    CK(hipDeviceSynchronize());

    FILE *out = fopen(argv[2], "wb");
    if (!out) { printf("cannot write %s\n", argv[2]); return 3; }
    int bad = fwrite(counts, 4, 4, out) != 4;
    for (int k = 0; k < 6; k++) {
        const size_t bytes = (size_t)P * w[k] * 4;
        bad |= dump(out, par[k], bytes) | dump(out, m1[k], bytes) | dump(out, m2[k], bytes);
    }
    EXPECT_CODE(gsr_mcmc_noise(NULL, P, par[3], par[4], par[5] + 1, noise, par[0], gate[0], gate[1], gate[2]), GSR_ERR_INVALID_ARGUMENT, "misaligned rotation");
    EXPECT_CODE(gsr_mcmc_noise(NULL, P, par[3], par[4], par[5], noise, par[0], gate[0], gate[1], gate[2]), GSR_OK, "noise");
    CK(hipDeviceSynchronize());
    bad |= dump(out, par[0], (size_t)P * 12);
    if (fclose(out) || bad) { printf("could not write the results\n"); return 3; }
    printf("mcmc C client ok\n");
    return 0;
}
