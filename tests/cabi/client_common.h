/* What the plain-C clients of libgsr_hip.so under tests/cabi/ share: plain C11, <hip/hip_runtime_api.h>, libc and the public gsr.h.
 * Header-only (static inline, so a client takes what it needs without a warning for the rest).  tests/cabi_client.py is the Python side:
 * it builds and runs the clients and writes the scene block that cabi_scene_read() reads; tests/cabi/common_selftest.c holds this file
 * against host stand-ins of the HIP calls, without a GPU.
 * Exit codes of every client: 1 a failed expectation, 2 a HIP error, 3 usage or a bad problem file. */
#ifndef GSR_TESTS_CABI_CLIENT_COMMON_H
#define GSR_TESTS_CABI_CLIENT_COMMON_H
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gsr.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %d at line %d\n", (int)e_, __LINE__); return 2; } } while (0)
#define PATTERN 0xA5

/* ---- files and device buffers ---- */
static inline void rd_into(FILE *f, void *dst, size_t bytes) {
    if (fread(dst, 1, bytes, f) != bytes) { printf("short problem file\n"); exit(3); }
}
static inline void *rd(FILE *f, size_t bytes) {
    void *p = malloc(bytes ? bytes : 1);
    if (!p) { printf("short problem file\n"); exit(3); }
    rd_into(f, p, bytes);
    return p;
}
/* `bytes` of the host's in an allocation of bytes + spare */
static inline void *dev_copy_spare(const void *host, size_t bytes, size_t spare) {
    void *d;
    if (hipMalloc(&d, bytes + spare ? bytes + spare : 1) != hipSuccess) return NULL;
    hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
    return d;
}
static inline void *dev_copy(const void *host, size_t bytes) { return dev_copy_spare(host, bytes, 0); }
static inline int dump(FILE *f, const void *d, size_t bytes) {
    void *h = malloc(bytes ? bytes : 1);
    if (hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost) != hipSuccess) { free(h); return 1; }
    const int bad = fwrite(h, 1, bytes, f) != bytes;
    free(h);
    return bad;
}

/* ---- the output check: every output buffer of the run holds PATTERN, so that a refusal can be shown to have written none of them
 * (none registered: nothing to look at) ---- */
static struct { void *p; size_t bytes; } outs[16];
static int n_outs;
static inline void *dev_out(size_t bytes) {
    void *d;
    if (n_outs == (int)(sizeof outs / sizeof outs[0])) return NULL;
    if (hipMalloc(&d, bytes) != hipSuccess || hipMemset(d, PATTERN, bytes) != hipSuccess) return NULL;
    outs[n_outs].p = d; outs[n_outs].bytes = bytes; n_outs++;
    return d;
}
/* the pattern again in every registered output, between the phases of a client */
static inline hipError_t outs_fill(void) {
    for (int k = 0; k < n_outs; k++) {
        const hipError_t e = hipMemset(outs[k].p, PATTERN, outs[k].bytes);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
static inline int buf_changed(const void *d, size_t bytes) {
    unsigned char *h = (unsigned char *)malloc(bytes ? bytes : 1);
    int bad = hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost) != hipSuccess;      /* blocking: this is what orders the check behind the null-stream call */
    for (size_t i = 0; i < bytes && !bad; i++) bad = h[i] != PATTERN;
    free(h);
    return bad;
}
static inline int changed(void) {
    for (int k = 0; k < n_outs; k++)
        if (buf_changed(outs[k].p, outs[k].bytes)) return 1;
    return 0;
}

/* ---- the three refusal checks, named for what they pin; each returns 1 from the function it stands in ---- */
#define EXPECT_SAID_(call, code, text, differs) do { const int rc_ = (call); const char *said_ = gsr_last_error(); \
    if (rc_ != (code) || ((code) != GSR_OK && (differs))) { \
        printf("line %d: expected %d \"%s\", got %d \"%s\"\n", __LINE__, (int)(code), text, rc_, said_); return 1; } \
    if (changed()) { printf("line %d: an output was written\n", __LINE__); return 1; } } while (0)
/* the call returns `code`; a refusal's text is `text` exactly, and every registered output still holds the pattern */
#define EXPECT_TEXT(call, code, text) EXPECT_SAID_(call, code, text, strcmp(said_, text) != 0)
/* the call returns `code`; a refusal's text starts with `text`, and every registered output still holds the pattern */
#define EXPECT_PREFIX(call, code, text) EXPECT_SAID_(call, code, text, strncmp(said_, text, strlen(text)) != 0)
/* the call returns `code`, and a refusal comes with some text: neither the text nor the outputs are looked at */
#define EXPECT_CODE(call, code, what) do { int rc_ = (call); if (rc_ != (code) || ((code) != GSR_OK && strlen(gsr_last_error()) == 0)) { \
    printf("%s: expected %d with a message, got %d (%s)\n", what, (int)(code), rc_, gsr_last_error()); return 1; } } while (0)

/* ---- the binning allocator handed to gsr_forward: the last allocation and its size; g_fail_alloc makes it refuse ---- */
static void *g_bin;
static size_t g_bin_bytes;
static int g_fail_alloc;
static inline void *alloc_binning(void *user, size_t bytes) {
    (void)user;
    if (g_fail_alloc || hipMalloc(&g_bin, bytes ? bytes : 1) != hipSuccess) return NULL;
    g_bin_bytes = bytes;
    return g_bin;
}

/* ---- the scene block of a problem file, as tests/cabi_client.py write_scene() writes it: int32 P D M W H, float32 tanfovx tanfovy
 * scale_modifier, then float32 bg [3], means3D [P,3], shs [P,M,3], opacities [P], scales [P,3], rotations [P,4], viewmatrix [16],
 * projmatrix [16], campos [3].  What follows the block in a file is the client's own. ---- */
struct cabi_scene {
    size_t spare;                   /* set before reading: bytes to allocate past the end of each array */
    int32_t P, D, M, W, H;
    float tanfovx, tanfovy, scale_modifier;
    float *bg, *means3D, *shs, *opacities, *scales, *rotations, *viewmatrix, *projmatrix, *campos;     /* on the device */
};
static inline float *cabi_scene_array_(FILE *f, size_t bytes, size_t spare) {
    void *h = rd(f, bytes);
    float *d = (float *)dev_copy_spare(h, bytes, spare);
    free(h);
    return d;
}
/* 0, or the exit code (a short file exits at once) */
static inline int cabi_scene_read(FILE *f, struct cabi_scene *s) {
    int32_t hdr[5];
    float par[3];
    rd_into(f, hdr, sizeof hdr); rd_into(f, par, sizeof par);
    s->P = hdr[0]; s->D = hdr[1]; s->M = hdr[2]; s->W = hdr[3]; s->H = hdr[4];
    s->tanfovx = par[0]; s->tanfovy = par[1]; s->scale_modifier = par[2];
    if (s->P < 1 || s->M < 1 || s->W < 1 || s->H < 1) { printf("bad problem header\n"); return 3; }
    const size_t n = (size_t)s->P, sp = s->spare;
    s->bg = cabi_scene_array_(f, 12, sp); s->means3D = cabi_scene_array_(f, n * 12, sp); s->shs = cabi_scene_array_(f, n * s->M * 12, sp);
    s->opacities = cabi_scene_array_(f, n * 4, sp); s->scales = cabi_scene_array_(f, n * 12, sp); s->rotations = cabi_scene_array_(f, n * 16, sp);
    s->viewmatrix = cabi_scene_array_(f, 64, sp); s->projmatrix = cabi_scene_array_(f, 64, sp); s->campos = cabi_scene_array_(f, 12, sp);
    if (!s->bg || !s->means3D || !s->shs || !s->opacities || !s->scales || !s->rotations || !s->viewmatrix || !s->projmatrix || !s->campos) {
        printf("hipMalloc failed\n"); return 2;
    }
    return 0;
}

/* ---- one gsr_forward of a scene into workspaces of exactly the sizes gsr_workspace_sizes names ---- */
struct cabi_render {
    size_t gb, ib, bb;              /* geometry, image and reverse-pass workspace bytes, as asked for */
    void *geom, *img, *binning;     /* binning: what alloc_binning handed out */
    size_t binning_bytes;
    float *color;                   /* [3,H,W] */
    int32_t *radii;                 /* [P] */
    int64_t R;                      /* num_rendered */
};
/* 0, or the exit code */
static inline int cabi_render(const struct cabi_scene *s, struct cabi_render *r) {
    memset(r, 0, sizeof *r);
    if (gsr_workspace_sizes(s->P, s->W, s->H, &r->gb, &r->ib, &r->bb) != GSR_OK) { printf("workspace sizes: %s\n", gsr_last_error()); return 1; }
    CK(hipMalloc(&r->geom, r->gb)); CK(hipMalloc(&r->img, r->ib));
    CK(hipMalloc((void **)&r->color, (size_t)3 * s->W * s->H * 4)); CK(hipMalloc((void **)&r->radii, (size_t)s->P * 4));
    g_bin = NULL; g_bin_bytes = 0;
    if (gsr_forward(NULL, s->P, s->D, s->M, s->W, s->H, s->bg, s->means3D, s->shs, NULL, s->opacities, s->scales, s->scale_modifier, s->rotations, NULL,
                    s->viewmatrix, s->projmatrix, s->campos, s->tanfovx, s->tanfovy, 0, 0, r->color, r->radii, r->geom, r->gb, alloc_binning, NULL,
                    r->img, r->ib, &r->R, NULL, 0) != GSR_OK) { printf("gsr_forward: %s\n", gsr_last_error()); return 1; }
    r->binning = g_bin; r->binning_bytes = g_bin_bytes;
    if (r->R < 1 || !r->binning) { printf("nothing was rendered\n"); return 3; }
    return 0;
}
#endif
