/* client_common.h held against host stand-ins of the HIP calls it makes: no GPU, no libamdhip64, no libgsr_hip.so.
 * Built and run by tests/test_cabi_common_host.py:
 *   gcc common_selftest.c -I<repo>/include -I/opt/rocm/include
 *   common_selftest                                 the refusal macros: each passes on a call that matches and returns 1 on one that does not
 *   common_selftest <problem file> <result file>    reads the scene block with cabi_scene_read() and writes every field back, in the
 *                                                   file's order, through dump(): the Python side compares the bytes with what it wrote */
#include "client_common.h"

hipError_t hipMalloc(void **p, size_t bytes) { *p = malloc(bytes); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void *p) { free(p); return hipSuccess; }
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) { (void)kind; memcpy(dst, src, bytes); return hipSuccess; }
hipError_t hipMemset(void *dst, int value, size_t bytes) { memset(dst, value, bytes); return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }

/* a library call that answers `rc`, says `text` and, where `poke` is given, writes one byte of an output */
static const char *g_said = "";
const char *gsr_last_error(void) { return g_said; }
static int fake(int rc, const char *text, unsigned char *poke) {
    g_said = text;
    if (poke) *poke ^= 1;
    return rc;
}

#define INV GSR_ERR_INVALID_ARGUMENT
static unsigned char *g_out;            /* a registered output of 24 bytes */
/* one function per case: the macros return from the function they stand in */
#define CASE(name, check) static int name(void) { check; return 0; }
CASE(text_matches, EXPECT_TEXT(fake(INV, "f: bad sizes", NULL), INV, "f: bad sizes"))
CASE(text_ok_call, EXPECT_TEXT(fake(GSR_OK, "", NULL), GSR_OK, ""))
CASE(text_wrong_code, EXPECT_TEXT(fake(GSR_ERR_WORKSPACE, "f: bad sizes", NULL), INV, "f: bad sizes"))
CASE(text_ok_wanted, EXPECT_TEXT(fake(INV, "", NULL), GSR_OK, ""))
CASE(text_longer, EXPECT_TEXT(fake(INV, "f: bad sizes, and more", NULL), INV, "f: bad sizes"))
CASE(text_output_written, EXPECT_TEXT(fake(INV, "f: bad sizes", g_out + 23), INV, "f: bad sizes"))
CASE(text_ok_output_written, EXPECT_TEXT(fake(GSR_OK, "", g_out), GSR_OK, ""))
CASE(prefix_matches, EXPECT_PREFIX(fake(GSR_ERR_WORKSPACE, "geom workspace 0 < 4096", NULL), GSR_ERR_WORKSPACE, "geom workspace 0 < "))
CASE(prefix_wrong_code, EXPECT_PREFIX(fake(INV, "geom workspace 0 < 4096", NULL), GSR_ERR_WORKSPACE, "geom workspace 0 < "))
CASE(prefix_wrong_text, EXPECT_PREFIX(fake(GSR_ERR_WORKSPACE, "image workspace 0 < 4096", NULL), GSR_ERR_WORKSPACE, "geom workspace 0 < "))
CASE(prefix_shorter, EXPECT_PREFIX(fake(GSR_ERR_WORKSPACE, "geom workspace", NULL), GSR_ERR_WORKSPACE, "geom workspace 0 < "))
CASE(prefix_output_written, EXPECT_PREFIX(fake(GSR_ERR_WORKSPACE, "geom workspace 0 < 4096", g_out + 7), GSR_ERR_WORKSPACE, "geom workspace 0 < "))
CASE(code_matches, EXPECT_CODE(fake(INV, "anything", NULL), INV, "a refusal"))
CASE(code_ok_call, EXPECT_CODE(fake(GSR_OK, "", NULL), GSR_OK, "a call"))
CASE(code_wrong_code, EXPECT_CODE(fake(GSR_ERR_WORKSPACE, "anything", NULL), INV, "a refusal"))
CASE(code_ok_wanted, EXPECT_CODE(fake(INV, "anything", NULL), GSR_OK, "a call"))
CASE(code_no_message, EXPECT_CODE(fake(INV, "", NULL), INV, "a refusal"))

static int macros(void) {
    static const struct { const char *name; int (*run)(void); int want; } cases[] = {
        {"text_matches", text_matches, 0}, {"text_ok_call", text_ok_call, 0}, {"text_wrong_code", text_wrong_code, 1}, {"text_ok_wanted", text_ok_wanted, 1},
        {"text_longer", text_longer, 1}, {"text_output_written", text_output_written, 1}, {"text_ok_output_written", text_ok_output_written, 1},
        {"prefix_matches", prefix_matches, 0}, {"prefix_wrong_code", prefix_wrong_code, 1}, {"prefix_wrong_text", prefix_wrong_text, 1},
        {"prefix_shorter", prefix_shorter, 1}, {"prefix_output_written", prefix_output_written, 1},
        {"code_matches", code_matches, 0}, {"code_ok_call", code_ok_call, 0}, {"code_wrong_code", code_wrong_code, 1}, {"code_ok_wanted", code_ok_wanted, 1},
        {"code_no_message", code_no_message, 1},
    };
    unsigned char *other = (unsigned char *)dev_out(5);
    g_out = (unsigned char *)dev_out(24);
    if (!other || !g_out || n_outs != 2 || changed()) { printf("dev_out: the outputs do not hold the pattern\n"); return 1; }
    for (size_t k = 0; k < sizeof cases / sizeof cases[0]; k++) {
        const int got = cases[k].run();
        if (got != cases[k].want) { printf("%s: returned %d, expected %d\n", cases[k].name, got, cases[k].want); return 1; }
        CK(outs_fill());
        if (changed()) { printf("%s: outs_fill left an output off the pattern\n", cases[k].name); return 1; }
    }
    other[4] = 0;                       /* the last byte of the first registered output: every buffer is walked, to its end */
    if (!changed() || !buf_changed(other, 5) || buf_changed(other, 4) || buf_changed(g_out, 24)) { printf("changed() misses a byte\n"); return 1; }
    hipFree(other); hipFree(g_out);
    printf("common selftest ok\n");
    return 0;
}

static int scene(const char *problem, const char *result) {
    FILE *f = fopen(problem, "rb");
    if (!f) { printf("cannot open %s\n", problem); return 3; }
    struct cabi_scene s = {0};
    const int rc = cabi_scene_read(f, &s);
    if (rc) return rc;
    if (fgetc(f) != EOF) { printf("bytes after the scene block\n"); return 3; }
    fclose(f);
    FILE *res = fopen(result, "wb");
    if (!res) { printf("cannot write %s\n", result); return 3; }
    const int32_t hdr[5] = {s.P, s.D, s.M, s.W, s.H};
    const float par[3] = {s.tanfovx, s.tanfovy, s.scale_modifier};
    const size_t n = (size_t)s.P;
    float *arrays[9] = {s.bg, s.means3D, s.shs, s.opacities, s.scales, s.rotations, s.viewmatrix, s.projmatrix, s.campos};
    const size_t bytes[9] = {12, n * 12, n * s.M * 12, n * 4, n * 12, n * 16, 64, 64, 12};
    int bad = fwrite(hdr, 4, 5, res) != 5 || fwrite(par, 4, 3, res) != 3;
    for (int k = 0; k < 9; k++) { bad |= dump(res, arrays[k], bytes[k]); hipFree(arrays[k]); }
    if (fclose(res) || bad) { printf("could not write the results\n"); return 3; }
    printf("common selftest: scene ok\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 1) return macros();
    if (argc == 3) return scene(argv[1], argv[2]);
    printf("usage: common_selftest [<problem file> <result file>]\n");
    return 3;
}
