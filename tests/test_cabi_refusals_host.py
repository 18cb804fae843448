"""What the C entry points refuse, and what they accept without launching, pinned to the letter: return code and the exact text of
gsr_last_error().  No device is needed and none is used: every device pointer below is a made-up address that is only compared, never
followed, and every call returns before it asks the HIP runtime for any work (a refusal, or an accepted case with nothing to do).  The
one exception is harmless: gsr_forward and gsr_backward_prefill look the current device up before their checks, and without a device
that lookup fails quietly (device 0 is assumed) and leaves the message alone.  With a device every case ends the same way.

One case per `fail(...)` site that can be reached that way, in gsr.h (the rasterizer: gsr_forward, gsr_backward, gsr_backward_prefill,
the size queries, gsr_mark_visible, gsr_composited_mask and the debug readers), gsr_loss.h (gsr_l1_ssim_*, gsr_views_loss_*), gsr_optim.h
(gsr_adam_step, gsr_adam_step_masked), gsr_density.h, gsr_knn.h, gsr_chamfer.h, gsr_sequence.h and gsr_rows.h, among them the two-step
refusals where a nested check leaves the text and the caller returns the bare code, and for gsr.h a handful of calls that break two
checks at once, to pin which refusal wins.  Before every call the message buffer holds a sentinel, so an accepted call is also seen to
leave it alone.

NOT covered, because they lie behind a call into the HIP runtime (a workspace size asked of rocPRIM, a memset or a launch):
  - gsr_forward with P = 0 (a memset of out_color), and everything from its workspace checks on ("scan temp query", "geom workspace %zu
    < %zu", "image workspace %zu < %zu", the allocator's refusal, every launch); gsr_backward likewise from "scan temp query" on
    ("binning workspace too small", "P too large for the 28-bit accumulator row index", "backward workspace %zu < %zu", "deterministic_bwd: ...")
  - gsr_workspace_sizes beyond its argument checks and gsr_binning_bytes for large N (rocPRIM's size queries want a device; the sizes
    themselves are pinned by tests/test_gpu_cabi.py), gsr_composited_mask's "geom workspace %zu < %zu", gsr_mark_visible's launch
  - gsr_debug_read_wave_trace: its argument check comes after a device synchronisation, which fails first without a device
  - gsr_densify_plan_workspace, gsr_knn_workspace, gsr_box_sort_workspace: the size itself ("densify workspace size", "knn temp query",
    "box sort workspace size")
  - gsr_densify_plan: "densify workspace %zu < %zu", "densify plan launch"
  - gsr_densify_apply: "densify workspace %zu < %zu", every per-group refusal ("group %d: width", "P_new * width", "src / dst NULL or
    equal", "the four moment pointers", "role %d", "needs width 3", "the xyz role needs scaling, rotation and noise"), "densify apply launch"
  - gsr_knn_mean_dist2: "knn workspace %zu < %zu", "knn launch"
  - gsr_box_sort: P = 0 ("box sort: clear count"), "box sort workspace %zu < %zu", "box sort launch"
  - gsr_visible_union with counts_out given ("visible union: clear counts"), "visible union launch"
  - every other GSR_ERR_HIP path: "l1+ssim forward launch", "l1+ssim backward launch", "views loss forward launch", "views loss backward
    launch", "adam launch", "masked adam launch", "density record launch", "chamfer forward launch", "chamfer backward launch",
    "rows unpack launch", "rows grad pack launch"
"""
import ctypes as C

import pytest

from gaussian_transformer_amd import _lib

OK, INVALID, WORKSPACE = 0, 1, 4
SENTINEL = "gsr_set_option: unknown option 'sentinel'"
BIG = 1 << 40                      # "large enough" for every workspace size below
A = 1 << 20                        # made-up device addresses: A * k, 16-byte aligned and far apart
NAN = float("nan")


def ptrs(*v):
    return (C.c_void_p * len(v))(*v)


def size():
    return C.byref(C.c_size_t())


def adam_groups(*g):               # (param, grad, exp_avg, exp_avg_sq, n, step)
    return (_lib.AdamGroup * len(g))(*[_lib.AdamGroup(p, gr, m, v, n, 0.01, step) for p, gr, m, v, n, step in g])


def density_groups(n):
    return (_lib.DensityGroup * n)()


V3, HOLE = ptrs(256, 512, 768), ptrs(256, None, 768)
G_OK = (A, 2 * A, 3 * A, 4 * A, 40, 1)
G_EMPTY = (None, None, None, None, 0, 1)
ARENAS = ptrs(*[16 * A + 4096 * b for b in range(65)])
F2, I2 = (C.c_float * 2)(0.5, 0.5), (C.c_int32 * 2)(64, 48)


def l1f(C_, H, W, img=A, gt=2 * A, out=3 * A, ws=4 * A, n=BIG):
    return lambda L: L.gsr_l1_ssim_forward(None, C_, H, W, img, gt, 0.2, out, ws, n)


def l1b(C_, H, W, img=A, gt=2 * A, ws=4 * A, n=BIG, grad=5 * A):
    return lambda L: L.gsr_l1_ssim_backward(None, C_, H, W, img, gt, 0.2, None, ws, n, grad)


def vf(B, H, W, imgs=V3, gts=V3, ws=4096, n=BIG, out3=1024, terms=2048):
    return lambda L: L.gsr_views_loss_forward(None, B, H, W, imgs, gts, 0.5, 0.5, 1, out3, terms, ws, n)


def vb(B, H, W, imgs=V3, gts=V3, ws=4096, n=BIG, grads=V3):
    return lambda L: L.gsr_views_loss_backward(None, B, H, W, imgs, gts, 0.5, 0.5, 1, None, ws, n, grads)


def adam(n, groups, b1=0.9, b2=0.999):
    return lambda L: L.gsr_adam_step(None, n, groups, b1, b2, 1e-8)


def madam(n, groups, P=10, mask=A, kind=_lib.ADAM_MASK_BYTES, b1=0.9, b2=0.999):
    return lambda L: L.gsr_adam_step_masked(None, n, groups, b1, b2, 1e-8, P, mask, kind)


def record(P, stride=2, grad=A, radii=2 * A, accum=3 * A, denom=4 * A, maxr=5 * A):
    return lambda L: L.gsr_density_record(None, P, grad, stride, radii, None, accum, denom, maxr)


def plan(P, N, counts=A, thr=0.0002, opacity=A, ws=5 * A):
    return lambda L: L.gsr_densify_plan(None, P, opacity, 2 * A, 3 * A, 4 * A, thr, 0.005, 0.01, 0.1, N, counts, ws, BIG)


def apply_(P, N, n_split, P_new, n_groups, groups, ws=A):
    return lambda L: L.gsr_densify_apply(None, P, N, n_split, P_new, n_groups, groups, 2 * A, 3 * A, 4 * A, ws, BIG)


def chf(B, N, M, D, x1=A, ws=7 * A, n=BIG):
    return lambda L: L.gsr_chamfer_forward(None, B, N, M, D, x1, 2 * A, 3 * A, 4 * A, 5 * A, 6 * A, ws, n)


def chb(B, N, M, D, idx1=3 * A):
    return lambda L: L.gsr_chamfer_backward(None, B, N, M, D, A, 2 * A, idx1, 4 * A, None, None, 5 * A, 6 * A)


def box(P, D, xyz_col, n, rows=A, out_rows=8 * A, perm=2 * A, count=3 * A, ws=4 * A):
    return lambda L: L.gsr_box_sort(None, P, D, rows, xyz_col, n, out_rows, perm, count, ws, BIG)


def vis(P, B, means=A, scales=2 * A, rots=3 * A, cov=None, raw=0, vm=4 * A, pm=5 * A, tx=F2, ty=F2, w=I2, h=I2):
    return lambda L: L.gsr_visible_union(None, P, B, means, scales, 1.0, rots, cov, raw, vm, pm, tx, ty, w, h, 6 * A, 7 * A, None)


def unpack(P, D, rows=A, xyz=2 * A, dc=3 * A, rest=4 * A, op=5 * A, sc=6 * A, rot=7 * A):
    return lambda L: L.gsr_rows_unpack(None, P, D, rows, xyz, dc, rest, op, sc, rot)


def gpack(P, D, B, arenas=ARENAS, grad=8 * A):
    return lambda L: L.gsr_rows_grad_pack(None, P, D, B, arenas, grad)


ALLOC = _lib.ALLOC_FN(lambda user, n: None)        # never called: every case returns before the allocator is needed


def fwd(**kw):
    """gsr_forward with arguments that pass every check, except the ones given; num_rendered must come back zeroed."""
    a = dict(P=10, D=1, M=4, W=32, H=32, bg=A, means3D=2 * A, shs=3 * A, colors=None, opac=4 * A, scales=5 * A, rots=6 * A, cov=None,
             view=7 * A, proj=8 * A, campos=9 * A, debug=0, out=10 * A, radii=11 * A, geom=12 * A, alloc=ALLOC, img=13 * A, rest=None, raw=0)
    a.update(kw)

    def call(L):
        n = C.c_int64(77)
        rc = L.gsr_forward(None, a["P"], a["D"], a["M"], a["W"], a["H"], a["bg"], a["means3D"], a["shs"], a["colors"], a["opac"],
                           a["scales"], 1.0, a["rots"], a["cov"], a["view"], a["proj"], a["campos"], 0.5, 0.5, 0, a["debug"], a["out"],
                           a["radii"], a["geom"], BIG, a["alloc"], None, a["img"], BIG, C.byref(n), a["rest"], a["raw"])
        assert n.value == 0
        return rc
    return call


def bwd(**kw):
    """gsr_backward likewise (the eight gradient outputs are g0 .. g7 in the order of the signature, g8 is dL_dsh_rest)."""
    a = dict(P=10, D=1, M=4, R=100, W=32, H=32, bg=A, means3D=2 * A, radii=3 * A, shs=4 * A, colors=None, scales=5 * A, rots=6 * A,
             cov=None, view=7 * A, proj=8 * A, campos=9 * A, dpix=10 * A, geom=11 * A, binning=12 * A, img=13 * A, ws=14 * A,
             g0=15 * A, g1=16 * A, g2=None, g3=17 * A, g4=None, g5=18 * A, g6=19 * A, g7=20 * A, debug=0, rest=None, raw=0, g8=None)
    a.update(kw)
    return lambda L: L.gsr_backward(None, a["P"], a["D"], a["M"], a["R"], a["W"], a["H"], a["bg"], a["means3D"], a["radii"], a["shs"],
                                    a["colors"], a["scales"], 1.0, a["rots"], a["cov"], a["view"], a["proj"], a["campos"], 0.5, 0.5,
                                    a["dpix"], a["geom"], BIG, a["binning"], BIG, a["img"], BIG, a["ws"], BIG, a["g0"], a["g1"], a["g2"],
                                    a["g3"], a["g4"], a["g5"], a["g6"], a["g7"], a["debug"], a["rest"], a["raw"], a["g8"])


def prefill(P, M):
    return lambda L: L.gsr_backward_prefill(P, M, A, 2 * A, None, 3 * A, None, 4 * A, 5 * A, 6 * A, None)


FWD, BWD = "gsr_forward: ", "gsr_backward: "
F_SIZES = FWD + "bad sizes or missing bg/matrices/out_color"
F_MISSING = FWD + "missing means3D/opacities/radii/workspaces/allocator"
F_COLOUR, B_COLOUR = FWD + "exactly one of shs / colors_precomp must be given", BWD + "exactly one of shs / colors_precomp must be given"
F_COV = FWD + "exactly one of (scales, rotations) / cov3D_precomp must be given"
B_COV = BWD + "exactly one of (scales, rotations) / cov3D_precomp must be given"
F_REST = FWD + "shs_rest needs shs (= features_dc) and M >= 2"
B_MISSING = BWD + "missing input, workspace or gradient buffer"
B_PRECOMP = BWD + "dL_dcolors / dL_dcov3D required with colors_precomp / cov3D_precomp"
B_SH, B_REST = BWD + "SH inputs inconsistent", BWD + "shs_rest needs shs, dL_dsh_rest and M >= 2"
PRECOLOUR = dict(shs=None, colors=3 * A)           # colours instead of SH coefficients
TOO_WIDE = 65535 * 16 + 1

VF, VB = "gsr_views_loss_forward", "gsr_views_loss_backward"
MA = "gsr_adam_step_masked"
ALIGN16 = "gsr_rows_unpack: rotation must be 16-byte aligned (gsr_forward reads a quaternion as one 16-byte load)"

# (call, return code, text of gsr_last_error() afterwards)
CASES = [
    # ---- gsr_loss.h: single image ----
    (lambda L: L.gsr_l1_ssim_workspace(0, 37, 29, size()), INVALID, "gsr_l1_ssim_workspace: bad argument"),
    (lambda L: L.gsr_l1_ssim_workspace(3, 37, -1, size()), INVALID, "gsr_l1_ssim_workspace: bad argument"),
    (lambda L: L.gsr_l1_ssim_workspace(3, 37, 29, None), INVALID, "gsr_l1_ssim_workspace: bad argument"),
    (l1f(0, 37, 29), INVALID, "gsr_l1_ssim_workspace: bad argument"),                      # two steps: the nested check's text
    (l1f(3, 37, 29, img=None), INVALID, "gsr_l1_ssim_forward: null pointer"),
    (l1f(3, 37, 29, ws=None), INVALID, "gsr_l1_ssim_forward: null pointer"),
    (l1f(3, 37, 29, n=38911), WORKSPACE, "loss workspace 38911 < 38912"),
    (l1b(3, 0, 29), INVALID, "gsr_l1_ssim_workspace: bad argument"),
    (l1b(3, 37, 29, grad=None), INVALID, "gsr_l1_ssim_backward: null pointer"),
    (l1b(3, 37, 29, n=0), WORKSPACE, "loss workspace 0 < 38912"),
    # ---- gsr_loss.h: B views ----
    (lambda L: L.gsr_views_loss_workspace(0, 37, 29, size()), INVALID, "gsr_views_loss_workspace: bad argument (B=0 H=37 W=29)"),
    (lambda L: L.gsr_views_loss_workspace(3, 37, 29, None), INVALID, "gsr_views_loss_workspace: bad argument (B=3 H=37 W=29)"),
    (lambda L: L.gsr_views_loss_workspace(1, 1048576, 1, size()), INVALID, "gsr_views_loss_workspace: image 1 x 1048576 too large"),
    (lambda L: L.gsr_views_loss_workspace(1, 1048560, 174753, size()), INVALID, "gsr_views_loss_workspace: image 174753 x 1048560 too large"),
    (vf(0, 37, 29), INVALID, "gsr_views_loss_workspace: bad argument (B=0 H=37 W=29)"),   # two steps
    (vf(3, 37, 29, imgs=None), INVALID, VF + ": null pointer (imgs, gts or workspace)"),
    (vf(3, 37, 29, ws=None), INVALID, VF + ": null pointer (imgs, gts or workspace)"),
    (vf(3, 37, 29, imgs=HOLE), INVALID, VF + ": view 1: null image pointer"),
    (vf(3, 37, 29, gts=HOLE), INVALID, VF + ": view 1: null target pointer"),
    (vf(3, 37, 29, n=100), INVALID, VF + ": workspace 100 < 117248"),
    (vf(3, 37, 29, out3=None), INVALID, VF + ": null pointer (out3 or terms)"),
    (vf(3, 37, 29, terms=None), INVALID, VF + ": null pointer (out3 or terms)"),
    (vb(3, 37, 0), INVALID, "gsr_views_loss_workspace: bad argument (B=3 H=37 W=0)"),
    (vb(3, 37, 29, gts=None), INVALID, VB + ": null pointer (imgs, gts or workspace)"),
    (vb(3, 37, 29, gts=HOLE), INVALID, VB + ": view 1: null target pointer"),
    (vb(3, 37, 29, n=117247), INVALID, VB + ": workspace 117247 < 117248"),
    (vb(3, 37, 29, grads=None), INVALID, VB + ": null pointer (grad_imgs)"),
    # ---- gsr_optim.h ----
    (adam(-1, adam_groups(G_OK)), INVALID, "gsr_adam_step: -1 groups (at most 16)"),
    (adam(17, adam_groups(*[G_OK] * 17)), INVALID, "gsr_adam_step: 17 groups (at most 16)"),
    (adam(2, None), INVALID, "gsr_adam_step: 2 groups (at most 16)"),
    (adam(2, adam_groups(G_OK, (A, 2 * A, 3 * A, 4 * A, -5, 1))), INVALID, "gsr_adam_step: group 1: n=-5 step=1 or a NULL buffer"),
    (adam(1, adam_groups((A, None, 3 * A, 4 * A, 40, 1))), INVALID, "gsr_adam_step: group 0: n=40 step=1 or a NULL buffer"),
    (adam(1, adam_groups((A, 2 * A, 3 * A, 4 * A, 40, 0))), INVALID, "gsr_adam_step: group 0: n=40 step=0 or a NULL buffer"),
    (adam(1, adam_groups(G_OK), b1=1.0), INVALID, "gsr_adam_step: betas"),
    (adam(1, adam_groups(G_OK), b2=NAN), INVALID, "gsr_adam_step: betas"),
    (adam(0, None), OK, SENTINEL),
    (adam(2, adam_groups(G_EMPTY, G_EMPTY)), OK, SENTINEL),                                # no element: nothing is launched
    (madam(0, adam_groups(G_OK)), INVALID, MA + ": 0 groups (1 to 16)"),
    (madam(17, adam_groups(*[G_OK] * 17)), INVALID, MA + ": 17 groups (1 to 16)"),
    (madam(1, None), INVALID, MA + ": 1 groups (1 to 16)"),
    (madam(1, adam_groups(G_OK), P=-3), INVALID, MA + ": P=-3 is negative"),
    (madam(1, adam_groups(G_OK), kind=2), INVALID, MA + ": unknown mask_kind 2"),
    (madam(1, adam_groups(G_OK), mask=None), INVALID, MA + ": mask is NULL with P=10"),
    (madam(1, adam_groups(G_OK), mask=A + 2, kind=_lib.ADAM_MASK_RADII), INVALID, MA + ": an int32 mask must be 4-byte aligned"),
    (madam(1, adam_groups((A, 2 * A, 3 * A, 4 * A, -1, 1))), INVALID, MA + ": group 0: n=-1 not in 0..2^31-1"),
    (madam(1, adam_groups((A, 2 * A, 3 * A, 4 * A, 1 << 31, 1))), INVALID, MA + ": group 0: n=2147483648 not in 0..2^31-1"),
    (madam(2, adam_groups(G_OK, (A, 2 * A, 3 * A, 4 * A, 41, 1))), INVALID, MA + ": group 1: n=41 is not a multiple of P=10"),
    (madam(1, adam_groups(G_OK), P=0, mask=None), INVALID, MA + ": group 0: n=40 is not a multiple of P=0"),
    (madam(1, adam_groups((A, 2 * A, None, 4 * A, 40, 1))), INVALID, MA + ": group 0: a NULL buffer with n=40"),
    (madam(1, adam_groups((A, 2 * A, 3 * A, 4 * A, 40, 0))), INVALID, MA + ": group 0: step=0"),
    (madam(1, adam_groups(G_OK), b1=-0.1), INVALID, MA + ": betas"),
    (madam(1, adam_groups(G_OK), b2=1.0), INVALID, MA + ": betas"),
    (madam(2, adam_groups(G_EMPTY, G_EMPTY)), OK, SENTINEL),
    (madam(1, adam_groups(G_EMPTY), P=0, mask=None), OK, SENTINEL),
    # ---- gsr_density.h ----
    (record(-1), INVALID, "gsr_density_record: P=-1 is negative"),
    (record(0, stride=0, grad=None, radii=None, accum=None, denom=None, maxr=None), OK, SENTINEL),      # P = 0: nothing else is looked at
    (record(10, stride=1), INVALID, "gsr_density_record: grad_stride_floats=1, at least 2"),
    (record(10, radii=None), INVALID, "gsr_density_record: null pointer"),
    (record(10, maxr=None), INVALID, "gsr_density_record: null pointer"),
    (lambda L: L.gsr_densify_plan_workspace(10, 2, None), INVALID, "gsr_densify_plan_workspace: bytes is NULL"),
    (lambda L: L.gsr_densify_plan_workspace(-1, 2, size()), INVALID, "gsr_densify_plan_workspace: P=-1 is negative"),
    (lambda L: L.gsr_densify_plan_workspace(10, 0, size()), INVALID, "gsr_densify_plan_workspace: N=0, at least 1"),
    (lambda L: L.gsr_densify_plan_workspace(1 << 30, 1, size()), INVALID,
     "gsr_densify_plan_workspace: P * (N + 1) = 2147483648, must stay below 2^31"),
    (plan(-2, 2), INVALID, "gsr_densify_plan: P=-2 is negative"),                         # two steps
    (plan(10, -1), INVALID, "gsr_densify_plan: N=-1, at least 1"),
    (plan(1 << 29, 3), INVALID, "gsr_densify_plan: P * (N + 1) = 2147483648, must stay below 2^31"),
    (plan(10, 2, counts=None), INVALID, "gsr_densify_plan: counts_host is NULL"),
    (plan(10, 2, thr=0.0), INVALID, "gsr_densify_plan: grad_threshold=0, must be > 0"),
    (plan(10, 2, thr=-1.5), INVALID, "gsr_densify_plan: grad_threshold=-1.5, must be > 0"),
    (plan(10, 2, thr=NAN), INVALID, "gsr_densify_plan: grad_threshold=nan, must be > 0"),
    (plan(10, 2, opacity=None), INVALID, "gsr_densify_plan: null pointer"),
    (plan(10, 2, ws=None), INVALID, "gsr_densify_plan: null pointer"),
    (apply_(-1, 2, 0, 0, 0, None), INVALID, "gsr_densify_apply: P=-1 is negative"),       # two steps
    (apply_(10, 0, 0, 0, 0, None), INVALID, "gsr_densify_apply: N=0, at least 1"),
    (apply_(10, 2, 3, 13, -1, None), INVALID, "gsr_densify_apply: -1 groups (at most 16)"),
    (apply_(10, 2, 3, 13, 17, density_groups(17)), INVALID, "gsr_densify_apply: 17 groups (at most 16)"),
    (apply_(10, 2, 3, 13, 2, None), INVALID, "gsr_densify_apply: 2 groups (at most 16)"),
    (apply_(10, 2, -1, 5, 0, None), INVALID, "gsr_densify_apply: n_split=-1 P_new=5 do not belong to a plan of P=10 N=2"),
    (apply_(10, 2, 11, 5, 0, None), INVALID, "gsr_densify_apply: n_split=11 P_new=5 do not belong to a plan of P=10 N=2"),
    (apply_(10, 2, 3, -1, 0, None), INVALID, "gsr_densify_apply: n_split=3 P_new=-1 do not belong to a plan of P=10 N=2"),
    (apply_(10, 2, 3, 31, 0, None), INVALID, "gsr_densify_apply: n_split=3 P_new=31 do not belong to a plan of P=10 N=2"),
    (apply_(0, 2, 0, 0, 1, density_groups(1), ws=None), OK, SENTINEL),
    (apply_(10, 2, 0, 0, 1, density_groups(1), ws=None), OK, SENTINEL),                    # P_new = 0: an empty new state
    (apply_(10, 2, 3, 13, 1, density_groups(1), ws=None), INVALID, "gsr_densify_apply: null pointer (ws)"),
    # ---- gsr_knn.h ----
    (lambda L: L.gsr_knn_workspace(-1, size()), INVALID, "gsr_knn_workspace: bad argument"),
    (lambda L: L.gsr_knn_workspace(100, None), INVALID, "gsr_knn_workspace: bad argument"),
    (lambda L: L.gsr_knn_mean_dist2(None, -1, A, 2 * A, 3 * A, BIG), INVALID, "gsr_knn_mean_dist2: bad argument"),
    (lambda L: L.gsr_knn_mean_dist2(None, 100, None, 2 * A, 3 * A, BIG), INVALID, "gsr_knn_mean_dist2: bad argument"),
    (lambda L: L.gsr_knn_mean_dist2(None, 100, A, None, 3 * A, BIG), INVALID, "gsr_knn_mean_dist2: bad argument"),
    (lambda L: L.gsr_knn_mean_dist2(None, 100, A, 2 * A, None, BIG), INVALID, "gsr_knn_mean_dist2: bad argument"),
    # ---- gsr_chamfer.h ----
    (lambda L: L.gsr_chamfer_workspace(-1, 3, 5, size()), INVALID, "gsr_chamfer_workspace: bad argument"),
    (lambda L: L.gsr_chamfer_workspace(2, 3, -5, size()), INVALID, "gsr_chamfer_workspace: bad argument"),
    (lambda L: L.gsr_chamfer_workspace(2, 3, 5, None), INVALID, "gsr_chamfer_workspace: bad argument"),
    (chf(-1, 3, 5, 3), INVALID, "gsr_chamfer_forward: negative size (B=-1 N=3 M=5)"),
    (chf(2, 3, -5, 3), INVALID, "gsr_chamfer_forward: negative size (B=2 N=3 M=-5)"),
    (chf(2, 3, 5, 0), INVALID, "gsr_chamfer_forward: D=0 not in 1..64"),
    (chf(2, 3, 5, 65), INVALID, "gsr_chamfer_forward: D=65 not in 1..64"),
    (chf(0, 3, 5, 3, x1=None, ws=None, n=0), OK, SENTINEL),                               # B = 0: nothing to do, no pointer is looked at
    (chf(2, 0, 0, 3, x1=None, ws=None, n=0), OK, SENTINEL),                               # N = M = 0 likewise
    (chf(2, 0, 5, 3), INVALID, "gsr_chamfer_forward: N=0, M=5: an empty set has no nearest neighbour"),
    (chf(2, 3, 0, 3), INVALID, "gsr_chamfer_forward: N=3, M=0: an empty set has no nearest neighbour"),
    (chf(512, 2 ** 31 - 1, 1, 3), INVALID, "gsr_chamfer_forward: B * max(N, M) too large"),
    (chf(2, 3, 5, 3, x1=None), INVALID, "gsr_chamfer_forward: null pointer"),
    (chf(2, 3, 5, 3, ws=None), INVALID, "gsr_chamfer_forward: null pointer"),
    (chf(2, 3, 5, 3, n=127), WORKSPACE, "chamfer workspace 127 < 128"),
    (chb(2, -3, 5, 3), INVALID, "gsr_chamfer_backward: negative size (B=2 N=-3 M=5)"),
    (chb(2, 3, 5, 100), INVALID, "gsr_chamfer_backward: D=100 not in 1..64"),
    (chb(0, 3, 5, 3, idx1=None), OK, SENTINEL),
    (chb(2, 0, 0, 3, idx1=None), OK, SENTINEL),
    (chb(2, 0, 5, 3), INVALID, "gsr_chamfer_backward: N=0, M=5: an empty set has no nearest neighbour"),
    (chb(512, 1, 2 ** 31 - 1, 3), INVALID, "gsr_chamfer_backward: B * max(N, M) too large"),
    (chb(2, 3, 5, 3, idx1=None), INVALID, "gsr_chamfer_backward: null pointer"),
    # ---- gsr_sequence.h ----
    (lambda L: L.gsr_box_sort_workspace(10, 4, None), INVALID, "gsr_box_sort_workspace: bytes is NULL"),
    (lambda L: L.gsr_box_sort_workspace(-1, 4, size()), INVALID, "gsr_box_sort_workspace: P=-1 is negative"),
    (lambda L: L.gsr_box_sort_workspace(10, 0, size()), INVALID, "gsr_box_sort_workspace: n=0 not in 1..128"),
    (lambda L: L.gsr_box_sort_workspace(10, 129, size()), INVALID, "gsr_box_sort_workspace: n=129 not in 1..128"),
    (box(-1, 26, 17, 4), INVALID, "gsr_box_sort: P=-1 is negative"),                      # two steps
    (box(10, 26, 17, 129), INVALID, "gsr_box_sort: n=129 not in 1..128"),
    (box(10, 2, 0, 4), INVALID, "gsr_box_sort: D=2 not in 3..64"),
    (box(10, 65, 0, 4), INVALID, "gsr_box_sort: D=65 not in 3..64"),
    (box(10, 26, -1, 4), INVALID, "gsr_box_sort: xyz_col=-1 not in 0..D-3=23"),
    (box(10, 26, 24, 4), INVALID, "gsr_box_sort: xyz_col=24 not in 0..D-3=23"),
    (box(2 ** 31 - 1, 3, 0, 4), INVALID, "gsr_box_sort: P * D = 6442450941 too large"),
    (box(10, 26, 17, 4, count=None), INVALID, "gsr_box_sort: out_count is NULL"),
    (box(10, 26, 17, 4, rows=None), INVALID, "gsr_box_sort: null pointer"),
    (box(10, 26, 17, 4, ws=None), INVALID, "gsr_box_sort: null pointer"),
    (box(10, 26, 17, 4, out_rows=A), INVALID, "gsr_box_sort: rows and out_rows must not overlap (same pointer)"),
    (box(10, 26, 17, 4, out_rows=A + 4 * 259), INVALID,
     "gsr_box_sort: rows and out_rows must not overlap (the ranges of P * D floats intersect)"),
    (box(10, 26, 17, 4, out_rows=A - 4 * 259), INVALID,
     "gsr_box_sort: rows and out_rows must not overlap (the ranges of P * D floats intersect)"),
    (vis(-1, 2), INVALID, "gsr_visible_union: P=-1 is negative"),
    (vis(10, 0), INVALID, "gsr_visible_union: B=0 not in 1..64"),
    (vis(10, 65), INVALID, "gsr_visible_union: B=65 not in 1..64"),
    (vis(10, 2, tx=None), INVALID, "gsr_visible_union: tanfovx/tanfovy/widths/heights (host) required"),
    (vis(10, 2, h=None), INVALID, "gsr_visible_union: tanfovx/tanfovy/widths/heights (host) required"),
    (vis(10, 2, w=(C.c_int32 * 2)(64, 0)), INVALID, "gsr_visible_union: camera 1: image size 0 x 48"),
    (vis(10, 2, h=(C.c_int32 * 2)(65535 * 16 + 1, 48)), INVALID, "gsr_visible_union: camera 0: image size 64 x 1048561"),
    (vis(0, 2, means=None, vm=None, pm=None), OK, SENTINEL),                              # P = 0 and no counts to clear
    (vis(10, 2, means=None), INVALID, "gsr_visible_union: missing means3D or matrices"),
    (vis(10, 2, pm=None), INVALID, "gsr_visible_union: missing means3D or matrices"),
    (vis(10, 2, cov=8 * A), INVALID, "gsr_visible_union: exactly one of (scales, rotations) / cov3D_precomp must be given"),
    (vis(10, 2, scales=None, rots=None), INVALID, "gsr_visible_union: exactly one of (scales, rotations) / cov3D_precomp must be given"),
    (vis(10, 2, rots=None), INVALID, "gsr_visible_union: exactly one of (scales, rotations) / cov3D_precomp must be given"),
    (vis(10, 2, scales=None, rots=None, cov=8 * A, raw=1), INVALID, "gsr_visible_union: raw_params needs scales/rotations, not cov3D_precomp"),
    # ---- gsr_rows.h ----
    (unpack(-1, 26), INVALID, "gsr_rows_unpack: P=-1 is negative"),                       # two steps
    (unpack(10, 18), INVALID, "gsr_rows_unpack: D=18 is not 3 K + 14 for K in 1..16 SH coefficients"),
    (unpack(10, 65), INVALID, "gsr_rows_unpack: D=65 is not 3 K + 14 for K in 1..16 SH coefficients"),
    (unpack(2 ** 31 - 1, 26), INVALID, "gsr_rows_unpack: P * D = 55834574822 too large"),
    (unpack(0, 26, rows=None, xyz=None, dc=None, rest=None, op=None, sc=None, rot=None), OK, SENTINEL),
    (unpack(10, 26, rest=None), INVALID, "gsr_rows_unpack: f_rest must be NULL if and only if K = 1 (D=26 holds K=4)"),
    (unpack(10, 17), INVALID, "gsr_rows_unpack: f_rest must be NULL if and only if K = 1 (D=17 holds K=1)"),
    (unpack(10, 26, xyz=None), INVALID, "gsr_rows_unpack: null pointer"),
    (unpack(10, 26, rot=7 * A + 4), INVALID, ALIGN16),
    (unpack(10, 26, op=A + 4 * 259), INVALID, "gsr_rows_unpack: opacity overlaps rows"),
    (unpack(10, 26, rest=A - 4 * 89), INVALID, "gsr_rows_unpack: f_rest overlaps rows"),
    (gpack(-1, 26, 1), INVALID, "gsr_rows_grad_pack: P=-1 is negative"),
    (gpack(10, 18, 1), INVALID, "gsr_rows_grad_pack: D=18 is not 3 K + 14 for K in 1..16 SH coefficients"),
    (gpack(2 ** 31 - 1, 17, 1), INVALID, "gsr_rows_grad_pack: P * D = 36507221999 too large"),
    (gpack(10, 26, 0), INVALID, "gsr_rows_grad_pack: B=0 not in 1..64"),
    (gpack(0, 26, 65, arenas=None, grad=None), INVALID, "gsr_rows_grad_pack: B=65 not in 1..64"),
    (gpack(0, 26, 64, grad=None), OK, SENTINEL),
    (gpack(10, 26, 1, arenas=None), INVALID, "gsr_rows_grad_pack: arenas (host array) required"),
    (gpack(10, 26, 1, grad=None), INVALID, "gsr_rows_grad_pack: grad_rows is NULL"),
    (gpack(10, 26, 2, arenas=ptrs(A, None)), INVALID, "gsr_rows_grad_pack: arenas[1] is NULL"),
    (gpack(10, 26, 1, arenas=ptrs(A + 2)), INVALID, "gsr_rows_grad_pack: arenas[0] is not 4-byte aligned"),
    (gpack(10, 26, 3, grad=16 * A + 2 * 4096 + 4 * 229), INVALID, "gsr_rows_grad_pack: grad_rows overlaps arenas[2]"),
    (gpack(10, 26, 3, grad=16 * A + 4096 - 4 * 259), INVALID, "gsr_rows_grad_pack: grad_rows overlaps arenas[1]"),
    # (the cases above keep their numbers: new ones are added below)
    # ---- gsr.h: gsr_forward, in the order of its checks ----
    (fwd(P=-1), INVALID, F_SIZES),
    (fwd(W=0), INVALID, F_SIZES),
    (fwd(H=-5), INVALID, F_SIZES),
    (fwd(out=None), INVALID, F_SIZES),
    (fwd(bg=None), INVALID, F_SIZES),
    (fwd(view=None), INVALID, F_SIZES),
    (fwd(proj=None), INVALID, F_SIZES),
    (fwd(W=TOO_WIDE), INVALID, "image too large"),
    (fwd(H=TOO_WIDE), INVALID, "image too large"),
    (fwd(means3D=None), INVALID, F_MISSING),
    (fwd(opac=None), INVALID, F_MISSING),
    (fwd(radii=None), INVALID, F_MISSING),
    (fwd(geom=None), INVALID, F_MISSING),
    (fwd(img=None), INVALID, F_MISSING),
    (fwd(alloc=_lib.ALLOC_FN(0)), INVALID, F_MISSING),                                       # a NULL function pointer
    (fwd(colors=14 * A), INVALID, F_COLOUR),
    (fwd(shs=None), INVALID, F_COLOUR),
    (fwd(cov=14 * A), INVALID, F_COV),
    (fwd(scales=None, rots=None), INVALID, F_COV),
    (fwd(rots=None), INVALID, F_COV),
    (fwd(scales=None, cov=14 * A), INVALID, F_COV),
    (fwd(rest=14 * A, M=1, D=0), INVALID, F_REST),
    (fwd(rest=14 * A, **PRECOLOUR), INVALID, F_REST),
    (fwd(raw=1, scales=None, rots=None, cov=14 * A), INVALID, FWD + "raw_params needs scales/rotations, not cov3D_precomp"),
    (fwd(D=-1), INVALID, FWD + "SH degree -1 not in 0..3"),
    (fwd(D=4, M=25), INVALID, FWD + "SH degree 4 not in 0..3"),
    (fwd(D=2, M=8), INVALID, FWD + "M=8 < (D+1)^2=9"),
    (fwd(campos=None), INVALID, FWD + "campos required with shs"),
    # two checks broken at once: the earlier one answers
    (fwd(P=-1, W=TOO_WIDE), INVALID, F_SIZES),
    (fwd(W=TOO_WIDE, means3D=None), INVALID, "image too large"),
    (fwd(means3D=None, colors=14 * A), INVALID, F_MISSING),
    (fwd(colors=14 * A, cov=14 * A), INVALID, F_COLOUR),
    (fwd(rots=None, rest=14 * A, M=1, D=0), INVALID, F_COV),
    (fwd(rest=14 * A, M=1, D=4), INVALID, F_REST),
    (fwd(D=4, M=25, campos=None), INVALID, FWD + "SH degree 4 not in 0..3"),
    (fwd(D=3, M=4, campos=None), INVALID, FWD + "M=4 < (D+1)^2=16"),
    # ---- gsr.h: gsr_backward, in the order of its checks ----
    (bwd(P=-1), INVALID, BWD + "bad sizes"),
    (bwd(W=0), INVALID, BWD + "bad sizes"),
    (bwd(H=0), INVALID, BWD + "bad sizes"),
    (bwd(R=-1), INVALID, BWD + "bad sizes"),
    (bwd(P=0, bg=None, means3D=None, geom=None, ws=None, g0=None), OK, SENTINEL),          # P = 0: nothing else is looked at
    (bwd(bg=None), INVALID, B_MISSING),
    (bwd(means3D=None), INVALID, B_MISSING),
    (bwd(radii=None), INVALID, B_MISSING),
    (bwd(view=None), INVALID, B_MISSING),
    (bwd(proj=None), INVALID, B_MISSING),
    (bwd(dpix=None), INVALID, B_MISSING),
    (bwd(geom=None), INVALID, B_MISSING),
    (bwd(img=None), INVALID, B_MISSING),
    (bwd(ws=None), INVALID, B_MISSING),
    (bwd(g0=None), INVALID, B_MISSING),
    (bwd(g1=None), INVALID, B_MISSING),
    (bwd(g3=None), INVALID, B_MISSING),
    (bwd(shs=None, colors=21 * A), INVALID, B_PRECOMP),
    (bwd(scales=None, rots=None, cov=21 * A), INVALID, B_PRECOMP),
    (bwd(colors=21 * A, g2=22 * A), INVALID, B_COLOUR),
    (bwd(shs=None), INVALID, B_COLOUR),
    (bwd(cov=21 * A, g4=22 * A), INVALID, B_COV),
    (bwd(scales=None, rots=None), INVALID, B_COV),
    (bwd(scales=None), INVALID, B_COV),
    (bwd(g5=None), INVALID, B_SH),
    (bwd(campos=None), INVALID, B_SH),
    (bwd(D=-1), INVALID, B_SH),
    (bwd(D=4, M=25), INVALID, B_SH),
    (bwd(D=1, M=3), INVALID, B_SH),
    (bwd(g6=None), INVALID, BWD + "dL_dscales/dL_drots required"),
    (bwd(g7=None), INVALID, BWD + "dL_dscales/dL_drots required"),
    (bwd(rest=21 * A), INVALID, B_REST),                                                   # no dL_dsh_rest
    (bwd(rest=21 * A, g8=22 * A, M=1, D=0), INVALID, B_REST),
    (bwd(raw=1, scales=None, rots=None, cov=21 * A, g4=22 * A), INVALID, BWD + "raw_params needs scales/rotations"),
    (bwd(binning=None), INVALID, BWD + "binning workspace missing"),
    # two checks broken at once
    (bwd(P=0, W=0), INVALID, BWD + "bad sizes"),
    (bwd(R=-1, bg=None), INVALID, BWD + "bad sizes"),
    (bwd(bg=None, shs=None), INVALID, B_MISSING),
    (bwd(shs=None, colors=21 * A, cov=21 * A, g4=22 * A), INVALID, B_PRECOMP),
    (bwd(shs=None, cov=21 * A, g4=22 * A), INVALID, B_COLOUR),
    (bwd(cov=21 * A, g4=22 * A, g5=None), INVALID, B_COV),
    (bwd(g5=None, g6=None), INVALID, B_SH),
    (bwd(g6=None, rest=21 * A), INVALID, BWD + "dL_dscales/dL_drots required"),
    (bwd(rest=21 * A, binning=None), INVALID, B_REST),
    # ---- gsr.h: announcements, size queries, visibility, debug readers ----
    (prefill(10, -1), INVALID, "gsr_backward_prefill: M < 0"),
    (prefill(0, -1), OK, SENTINEL),                                                        # P <= 0 withdraws: M is not looked at
    (prefill(-3, 16), OK, SENTINEL),
    (lambda L: L.gsr_workspace_sizes(-1, 32, 32, size(), size(), size()), INVALID, "gsr_workspace_sizes: P=-1 W=32 H=32"),
    (lambda L: L.gsr_workspace_sizes(10, 0, 32, size(), size(), size()), INVALID, "gsr_workspace_sizes: P=10 W=0 H=32"),
    (lambda L: L.gsr_workspace_sizes(10, 32, -2, None, None, None), INVALID, "gsr_workspace_sizes: P=10 W=32 H=-2"),
    (lambda L: L.gsr_workspace_sizes(10, TOO_WIDE, 32, size(), size(), size()), INVALID, "image too large"),
    (lambda L: L.gsr_workspace_sizes(10, 32, TOO_WIDE, size(), size(), size()), INVALID, "image too large"),
    (lambda L: L.gsr_workspace_sizes(-1, TOO_WIDE, 32, size(), size(), size()), INVALID, "gsr_workspace_sizes: P=-1 W=1048561 H=32"),
    (lambda L: L.gsr_backward_workspace_bytes(-1, 5, size()), INVALID, "gsr_backward_workspace_bytes: bad argument"),
    (lambda L: L.gsr_backward_workspace_bytes(10, -5, size()), INVALID, "gsr_backward_workspace_bytes: bad argument"),
    (lambda L: L.gsr_backward_workspace_bytes(10, 5, None), INVALID, "gsr_backward_workspace_bytes: bad argument"),
    (lambda L: L.gsr_binning_bytes(-1, 32, 32, size()), INVALID, "gsr_binning_bytes: bad argument"),
    (lambda L: L.gsr_binning_bytes(10, 0, 32, size()), INVALID, "gsr_binning_bytes: bad argument"),
    (lambda L: L.gsr_binning_bytes(10, 32, -1, size()), INVALID, "gsr_binning_bytes: bad argument"),
    (lambda L: L.gsr_binning_bytes(10, 32, 32, None), INVALID, "gsr_binning_bytes: bad argument"),
    (lambda L: L.gsr_mark_visible(None, -1, A, 2 * A, 3 * A, 4 * A), INVALID, "gsr_mark_visible: bad argument"),
    (lambda L: L.gsr_mark_visible(None, 10, None, 2 * A, 3 * A, 4 * A), INVALID, "gsr_mark_visible: bad argument"),
    (lambda L: L.gsr_mark_visible(None, 10, A, None, 3 * A, 4 * A), INVALID, "gsr_mark_visible: bad argument"),
    (lambda L: L.gsr_mark_visible(None, 10, A, 2 * A, 3 * A, None), INVALID, "gsr_mark_visible: bad argument"),
    (lambda L: L.gsr_composited_mask(None, -1, A, BIG, 2 * A), INVALID, "gsr_composited_mask: bad argument"),
    (lambda L: L.gsr_composited_mask(None, 10, None, BIG, 2 * A), INVALID, "gsr_composited_mask: bad argument"),
    (lambda L: L.gsr_composited_mask(None, 10, A, BIG, None), INVALID, "gsr_composited_mask: bad argument"),
    (lambda L: L.gsr_composited_mask(None, 0, None, 0, None), OK, SENTINEL),               # P = 0: nothing to do
    (lambda L: L.gsr_debug_read_segments(None, 32, 32, None, A), INVALID, "gsr_debug_read_segments: bad argument"),
    (lambda L: L.gsr_debug_read_segments(None, 32, 32, A, None), INVALID, "gsr_debug_read_segments: bad argument"),
    (lambda L: L.gsr_debug_read_segments(None, 0, 32, A, 2 * A), INVALID, "gsr_debug_read_segments: bad argument"),
    (lambda L: L.gsr_debug_read_segments(None, 32, -1, A, 2 * A), INVALID, "gsr_debug_read_segments: bad argument"),
    (lambda L: L.gsr_debug_read_bound_errors(None, 10, A, 32, 32, 2 * A, None), INVALID, "gsr_debug_read_bound_errors: bad argument"),
]


@pytest.mark.parametrize("k", range(len(CASES)), ids=[f"{k:03d}-{'ok' if c[1] == OK else c[2][:48]}" for k, c in enumerate(CASES)])
def test_return_code_and_message(k):
    call, rc, text = CASES[k]
    lib = _lib.load()
    assert lib.gsr_set_option(b"sentinel", 0) == INVALID and lib.gsr_last_error().decode() == SENTINEL
    got = call(lib)
    assert (got, lib.gsr_last_error().decode()) == (rc, text)


def test_sizes_that_need_no_runtime_are_what_they_were():
    lib = _lib.load()
    n = C.c_size_t(0)
    assert lib.gsr_l1_ssim_workspace(3, 37, 29, C.byref(n)) == OK and n.value == 38912
    assert lib.gsr_views_loss_workspace(3, 37, 29, C.byref(n)) == OK and n.value == 117248
    assert lib.gsr_views_loss_workspace(1, 1048560, 174752, C.byref(n)) == OK         # the largest image: 3 * 65535 * 10922 blocks < 2^31
    assert lib.gsr_chamfer_workspace(2, 3, 5, C.byref(n)) == OK and n.value == 128
    assert lib.gsr_chamfer_workspace(0, 3, 5, C.byref(n)) == OK and n.value == 0


def test_backward_workspace_bytes_are_what_they_were():
    """gsr_backward_workspace_bytes needs no device: accumulator rows + the deterministic mode's slots (2 * 64 bytes per rendered pair at the
    default two blocks per wave, only under deterministic_bwd) + the dense per-Gaussian stage's list and records.  The numbers were
    recorded from the library before gsr_api.hip was restructured around a per-call options snapshot."""
    lib = _lib.load()
    sizes, pairs = (0, 1, 1023, 1024, 500000), (0, 1, 1023, 1024, 500000)
    plain = {0: 66048, 1: 81664, 1023: 383232, 1024: 383232, 500000: 66523392}
    slots = {0: 0, 1: 256, 1023: 131072, 1024: 131072, 500000: 64000000}
    n = C.c_size_t(0)
    assert _lib.get_option("deterministic_bwd") == 0 and _lib.get_option("bwd_blocks_per_wave") == 2
    try:
        for det in (0, 1):
            _lib.set_option("deterministic_bwd", det)
            for P in sizes:
                for R in pairs:
                    assert lib.gsr_backward_workspace_bytes(P, R, C.byref(n)) == OK
                    assert n.value == plain[P] + det * slots[R], (det, P, R)
    finally:
        _lib.set_option("deterministic_bwd", 0)


def test_densify_plan_of_nothing_writes_four_zeros_and_launches_nothing():
    lib = _lib.load()
    counts = (C.c_uint32 * 4)(7, 7, 7, 7)
    assert lib.gsr_set_option(b"sentinel", 0) == INVALID
    rc = lib.gsr_densify_plan(None, 0, None, None, None, None, 0.0002, 0.005, 0.01, 0.1, 2, counts, None, 0)
    assert rc == OK and list(counts) == [0, 0, 0, 0] and lib.gsr_last_error().decode() == SENTINEL
    # the checks in front of P == 0 still hold for an empty cloud
    counts = (C.c_uint32 * 4)(7, 7, 7, 7)
    rc = lib.gsr_densify_plan(None, 0, None, None, None, None, 0.0, 0.005, 0.01, 0.1, 2, counts, None, 0)
    assert rc == INVALID and list(counts) == [7, 7, 7, 7]
    assert lib.gsr_last_error().decode() == "gsr_densify_plan: grad_threshold=0, must be > 0"


def test_a_refusal_replaces_the_previous_text_whichever_file_wrote_it():
    """One buffer per thread for every entry point: a refusal from one header's functions is replaced by the next one from another's."""
    lib = _lib.load()
    seq = [(unpack(-1, 26), "gsr_rows_unpack: P=-1 is negative"), (madam(0, None), MA + ": 0 groups (1 to 16)"),
           (record(-1), "gsr_density_record: P=-1 is negative"), (chb(2, 3, 5, 0), "gsr_chamfer_backward: D=0 not in 1..64"),
           (lambda L: L.gsr_set_option(b"tile_lists", 3), "tile_lists must be 0, 1 or 2")]
    for call, text in seq:
        assert call(lib) == INVALID and lib.gsr_last_error().decode() == text
