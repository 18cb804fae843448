"""-m gpu: camera gradients (include/gsr_pose.h) through the public API -- GaussianRasterizer with camera tensors that require grad ->
_RasterizeGaussiansPose -> ctypes -> C ABI -> csrc/pose_grad.hip -- against tests/pose_ref.py in float64.

Gate.  Each output tensor is judged relative to the largest absolute entry of the float64 reference.  e32 is the error of the same
reference evaluated with the float32 oracle (float32 torch on the float32 oracle's per-Gaussian gradients) on the same scene; the
kernel is held to 2 e32 + 1e-6: twice the float32 formulation's own error.  Both figures are printed per scene.  The translation
identity ties the camera gradient to the same call's dL/dmeans3D (summed in float64): its residual, relative to the largest entry of
the float64 oracle's sum, is held to twice the float32 reference's own residual + 1e-6.
"""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib, camera, synth
from gaussian_transformer_amd.rasterizer import (GaussianRasterizationSettings, GaussianRasterizer, arena_floats, get_backend,
                                                 gradient_arena)
from tests import grad_outputs_ref as gr
from tests import pose_ref
from tests.helpers import oracle_scene
from tests.test_gpu_grad_outputs import options

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("viewmatrix", "projmatrix", "campos")


# ---- the device side ----
def tensors(S, cam_grad=(True, True, True), gauss_grad=True):
    P = int(np.asarray(S.means3D).shape[0])

    def t(a, g=False):
        return None if a is None else torch.tensor(np.asarray(a, dtype=np.float32), device=DEV).requires_grad_(g)
    gg = gauss_grad
    inp = dict(means3D=t(np.asarray(S.means3D).reshape(P, 3), gg), opacities=t(np.asarray(S.opacities).reshape(P, 1), gg), shs=t(S.shs, gg),
               colors_precomp=t(S.colors_precomp, gg), scales=t(S.scales, gg), rotations=t(S.rotations, gg), cov3D_precomp=t(S.cov3D_precomp, gg))
    inp["means2D"] = torch.zeros((P, 3), dtype=torch.float32, device=DEV, requires_grad=gg)
    rs = GaussianRasterizationSettings(
        image_height=S.H, image_width=S.W, tanfovx=S.tanfovx, tanfovy=S.tanfovy, bg=t(S.bg), scale_modifier=S.scale_modifier,
        viewmatrix=t(np.asarray(S.viewmatrix).reshape(4, 4), cam_grad[0]), projmatrix=t(np.asarray(S.projmatrix).reshape(4, 4), cam_grad[1]),
        sh_degree=S.sh_degree, campos=t(S.campos, cam_grad[2]), prefiltered=False, debug=False)
    return rs, inp


def cam_of(rs):
    return {k: (None if x.grad is None else x.grad.detach().cpu().numpy().astype(np.float64).reshape(-1))
            for k, x in zip(KEYS, (rs.viewmatrix, rs.projmatrix, rs.campos))}


def hip(S, gC=None, mode=None, gD=None, gA=None, **kw):
    """One render through the public API and the backward of <gC, color> + <gD, depth> + <gA, alpha>.  Returns the camera gradients
    (float64 numpy, flat) and "means3D" = the same call's dL/dmeans3D."""
    rs, inp = tensors(S, **kw)
    d = lambda a: None if a is None else torch.tensor(np.asarray(a, np.float32), device=DEV)
    out = GaussianRasterizer(rs)(depth=mode, **inp)
    assert out[0].grad_fn.__class__.__name__.startswith("_RasterizeGaussiansPoseBackward")
    terms = [] if gC is None else [(out[0] * d(gC)).sum()]
    if gD is not None:
        terms.append((out[2][0] * d(gD)).sum())
    if gA is not None:
        terms.append((out[3][0] * d(gA)).sum())
    sum(terms).backward()
    res = cam_of(rs)
    res["means3D"] = None if inp["means3D"].grad is None else inp["means3D"].grad.detach().cpu().numpy().astype(np.float64)
    res["rs"], res["inp"] = rs, inp
    return res


def check_zeros(h):
    """The structural zeros are exactly +0.0."""
    for k, idx in (("viewmatrix", [3, 7, 11, 15]), ("projmatrix", [2, 6, 10, 14])):
        if h.get(k) is not None:
            z = h[k][idx]
            assert not z.any() and not np.signbit(z).any(), (k, z)


def gate(tag, h, g64, g32, S=None, keys=KEYS):
    check_zeros(h)
    for k in keys:
        e32, e = pose_ref.rel_err(g32[k], g64[k]), pose_ref.rel_err(h[k], g64[k])
        print(f"POSE {tag} {k}: e32 {e32:.3e} kernel {e:.3e} max|ref| {np.abs(g64[k]).max():.3e}")
        assert np.isfinite(h[k]).all()
        assert e <= 2 * e32 + 1e-6, (tag, k, e, e32, h[k], g64[k])
    if S is not None and h.get("means3D") is not None and all(h.get(k) is not None for k in KEYS):
        lhs64, _ = pose_ref.translation_identity(S, g64, g64["oracle"]["dL_dmeans3D"])
        lhs32, rhs32 = pose_ref.translation_identity(S, g32, g32["oracle"]["dL_dmeans3D"])
        lhs, rhs = pose_ref.translation_identity(S, h, h["means3D"])
        s = max(np.abs(lhs64).max(), 1e-30)
        r32, r = np.abs(lhs32 - rhs32).max() / s, np.abs(lhs - rhs).max() / s
        print(f"POSE {tag} identity: residual32 {r32:.3e} kernel {r:.3e} max|sum| {s:.3e}")
        assert r <= 2 * r32 + 1e-6, (tag, r, r32, lhs, rhs)


# ---- scenes and their references (computed once, shared, left alone) ----
EDGE_S0 = {1: 0.3, 63: 0.3, 64: 0.3, 65: 0.3, 256: 0.15, 257: 0.15, 4000: 0.05, 66000: 0.012}


def _colours(P, seed):
    return np.random.default_rng(seed + 7).uniform(0.0, 1.0, (P, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene(name):
    """(oracle Scene, dL [3,H,W] float64)."""
    kind, _, arg = name.partition(":")
    if kind in ("edge", "edgec"):                     # reduction edges: P Gaussians at 64 x 64, SH degree 3 or colors_precomp
        P = int(arg)
        sc = synth.make_scene(P=P, width=64, height=64, sh_degree=3, s0=EDGE_S0[P], seed=P % 97)
        S = oracle_scene(sc)
        if kind == "edgec":
            S = dataclasses.replace(S, shs=None, sh_degree=0, colors_precomp=_colours(P, 1))
    elif kind == "replica":                           # tests/test_gpu_depth.py's: the first Gaussian covers all 272 tiles
        sc = synth.make_scene(P=201, width=272, height=256, sh_degree=1, s0=0.05, seed=0)
        sc.scales[0] = np.array([8.0, 8.0, 8.0], np.float32)
        sc.opacities[0] = 0.6
        S = oracle_scene(sc)
    elif kind == "fov":                               # Gaussians beyond 1.3 tanfov that still reach into the image
        sc = synth.make_scene(P=300, width=80, height=48, sh_degree=2, s0=0.08, seed=7)
        m, s = pose_ref.beyond_clamp(sc)
        S = oracle_scene(sc, means3D=m.astype(np.float32), scales=s.astype(np.float32))
    elif kind == "colclamp":                          # colours clamped at 0
        sc = synth.make_scene(P=300, width=80, height=48, sh_degree=1, s0=0.08, seed=5)
        shs = np.array(sc.shs, np.float32, copy=True)
        shs[::2, 0, :2] = -3.0
        S = oracle_scene(sc, shs=shs)
    elif kind == "mod":                               # scale_modifier 0.5
        sc = synth.make_scene(P=300, width=80, height=48, sh_degree=3, s0=0.15, seed=9)
        S = oracle_scene(sc, scale_modifier=0.5)
    elif kind == "cov":                               # cov3D_precomp
        sc = synth.make_scene(P=300, width=80, height=48, sh_degree=3, s0=0.08, seed=11)
        S = dataclasses.replace(oracle_scene(sc), scales=None, rotations=None, cov3D_precomp=gr.cov6_of(sc.scales, sc.rotations))
    elif kind == "deg":                               # SH degree 0..3 (M = (degree + 1)^2)
        d = int(arg)
        sc = synth.make_scene(P=300, width=80, height=48, sh_degree=d, s0=0.08, seed=20 + d)
        S = oracle_scene(sc)
    else:
        raise KeyError(name)
    dL = np.random.default_rng(5).normal(size=(3, S.H, S.W))
    return S, dL


@functools.lru_cache(maxsize=None)
def reference(name):
    S, dL = scene(name)
    return pose_ref.colour_grads(S, dL, "f64"), pose_ref.colour_grads(S, dL, "f32")


@functools.lru_cache(maxsize=None)
def gr_reference(name):
    """Camera gradients of a tests/grad_outputs_ref.py scene from its shared oracle runs."""
    S, _ = gr.scene(name)
    f32, g32, f64, g64 = gr.oracles(name)
    out = []
    for f, g, prec in ((f64, g64, "f64"), (f32, g32, "f32")):
        c = pose_ref.surrogate_grads(S, f["radii"], g["dL_dmeans2D"], g["dL_dconic"], g["dL_dcolors"], f["state"].geom()["clamped"], precision=prec)
        c["oracle"] = g
        out.append(c)
    return tuple(out)


def map_upstream(S, seed=11):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(S.H, S.W)), rng.normal(size=(S.H, S.W))


@functools.lru_cache(maxsize=None)
def map_reference(name, mode):
    S, _ = scene(name)
    gD, gA = map_upstream(S)
    return pose_ref.map_grads(S, mode, gD, gA, "f64"), pose_ref.map_grads(S, mode, gD, gA, "f32")


# ---- reduction edges ----
@pytest.mark.parametrize("P", sorted(EDGE_S0))
@pytest.mark.parametrize("kind", ("edge", "edgec"))
def test_reduction_edges(kind, P):
    name = f"{kind}:{P}"
    S, dL = scene(name)
    g64, g32 = reference(name)
    h = hip(S, dL)
    gate(name, h, g64, g32, S)
    if kind == "edgec":
        assert not h["campos"].any() and not np.signbit(h["campos"]).any()       # colors_precomp: exactly 0
    else:
        assert np.abs(g64["campos"]).max() > 0
    if P == 66000:                                                               # more block rows than the final kernel has lanes
        n = _lib.C.c_size_t()
        _lib.check(_lib.load().gsr_pose_workspace_bytes(P, _lib.C.byref(n)), "size")
        assert n.value // 256 > 256


def test_replica_rows():
    S, dL = scene("replica")
    g64, g32 = reference("replica")
    h = hip(S, dL)
    gate("replica", h, g64, g32, S)
    geom = None
    rs, inp = tensors(S, gauss_grad=False)
    out = GaussianRasterizer(rs)(**inp)
    geom = out[0].grad_fn.saved_tensors[7]
    tiles = np.zeros(201, np.uint32)
    _lib.check(_lib.load().gsr_debug_read_geom(torch.cuda.current_stream().cuda_stream, 201, geom.data_ptr(), None, None, None, None, tiles.ctypes.data, None), "read geom")
    assert tiles[0] >= 256                                                       # the scene does drive replica rows
    for mode in ("expected", "inverse"):
        gD, gA = map_upstream(S)
        m64, m32 = map_reference("replica", mode)
        gate(f"replica {mode}", hip(S, None, mode, gD, gA), m64, m32, S)


@pytest.mark.parametrize("name", ("fov", "colclamp", "mod", "cov", "deg:0", "deg:1", "deg:2", "deg:3"))
def test_clamps_and_input_forms(name):
    S, dL = scene(name)
    g64, g32 = reference(name)
    if name == "fov":
        p = np.c_[np.asarray(S.means3D, np.float64), np.ones(len(S.means3D))] @ np.asarray(S.viewmatrix, np.float64).reshape(4, 4)
        vis = np.asarray(g64["oracle"]["dL_dconic"]).any(1)
        assert (vis & (np.abs(p[:, 0] / p[:, 2]) > 1.3 * S.tanfovx)).sum() >= 2 and (vis & (np.abs(p[:, 1] / p[:, 2]) > 1.3 * S.tanfovy)).sum() >= 2
        bad = pose_ref.colour_grads(S, dL, "f64", fault="no_masks")
        assert pose_ref.rel_err(bad["viewmatrix"], g64["viewmatrix"]) > 1e-3      # the scene tells the mask apart
    if name == "colclamp":
        bad = pose_ref.colour_grads(S, dL, "f64", fault="no_masks")
        assert pose_ref.rel_err(bad["campos"], g64["campos"]) > 1e-3
    gate(name, hip(S, dL), g64, g32, S)


# ---- maps ----
@pytest.mark.parametrize("mode", ("expected", "inverse"))
def test_maps_alone_and_in_one_graph_with_the_colour(mode):
    name = "deg:1"
    S, dL = scene(name)
    gD, gA = map_upstream(S)
    c64, c32 = reference(name)
    m64, m32 = map_reference(name, mode)
    alone = hip(S, None, mode, gD, gA)
    gate(f"maps {mode}", alone, m64, m32, S)
    assert not alone["campos"].any()
    colour = hip(S, dL, mode)                                                    # the colour of the 4-tuple alone
    gate(f"colour of 4-tuple {mode}", colour, c64, c32, S)
    s64, s32 = pose_ref.add(c64, m64), pose_ref.add(c32, m32)
    s64["oracle"] = {"dL_dmeans3D": np.asarray(c64["oracle"]["dL_dmeans3D"]) + np.asarray(m64["oracle"]["dL_dmeans3D"])}
    s32["oracle"] = {"dL_dmeans3D": np.asarray(c32["oracle"]["dL_dmeans3D"], np.float64) + np.asarray(m32["oracle"]["dL_dmeans3D"], np.float64)}
    both = hip(S, dL, mode, gD, gA)
    gate(f"colour + maps {mode}", both, s64, s32, S)
    # ... and equals the sum of the separate graphs at the same gate
    parts = pose_ref.add(colour, alone)
    for k in KEYS:
        assert pose_ref.rel_err(both[k], parts[k]) <= 2 * pose_ref.rel_err(s32[k], s64[k]) + 1e-6, k
    # with a gradient arena around forward and backward
    P = int(np.asarray(S.means3D).shape[0])
    flat = torch.zeros(arena_floats(P, int(np.asarray(S.shs).shape[1])), device=DEV)
    with gradient_arena(flat):
        arena = hip(S, dL, mode, gD, gA)
    gate(f"colour + maps {mode}, arena", arena, s64, s32, S)
    with gradient_arena(flat):
        arena_maps = hip(S, None, mode, gD, gA)                                  # the maps alone while an announced fill is in flight
    gate(f"maps {mode}, arena", arena_maps, m64, m32, S)


# ---- bit identity ----
def test_deterministic_bwd_is_bitwise_reproducible():
    S, dL = gr.scene("main")
    with options("stream_det"):
        a, b = hip(S, dL), hip(S, dL)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    g64, g32 = gr_reference("main")
    gate("main stream_det", a, g64, g32, S)


def test_two_calls_on_one_untouched_workspace_are_bit_identical():
    S, dL = scene("edge:4000")
    be = get_backend()
    rs, inp = tensors(S, cam_grad=(False, False, False), gauss_grad=False)
    e = torch.empty(0, device=DEV)
    a = [inp["means3D"], inp["shs"], e, inp["opacities"], inp["scales"], inp["rotations"], e]
    n, color, radii, geom, binning, img = be.forward(rs, *a)
    res = be.backward(rs, n, torch.tensor(dL, dtype=torch.float32, device=DEV), a[0], radii, a[1], a[2], a[4], a[5], a[6], geom, binning, img,
                      return_ws=True)
    assert len(res) == 9 and res[8].dtype == torch.uint8
    assert len(be.backward(rs, n, torch.tensor(dL, dtype=torch.float32, device=DEV), a[0], radii, a[1], a[2], a[4], a[5], a[6], geom, binning, img)) == 8
    ws = res[8]
    keep = ws.clone()
    one = be.pose_backward(rs, 0, n, a[0], radii, a[1], a[2], a[4], a[5], a[6], geom, ws)
    two = be.pose_backward(rs, 0, n, a[0], radii, a[1], a[2], a[4], a[5], a[6], geom, ws)
    assert all(torch.equal(x, y) for x, y in zip(one, two))
    assert torch.equal(ws, keep)                                                 # the accumulator workspace is only read
    only = be.pose_backward(rs, 0, n, a[0], radii, a[1], a[2], a[4], a[5], a[6], geom, ws, want=(False, True, False))
    assert only[0] is None and only[2] is None and torch.equal(only[1], one[1])  # NULL outputs
    g64, g32 = reference("edge:4000")
    h = {k: x.cpu().numpy().astype(np.float64).reshape(-1) for k, x in zip(KEYS, one)}
    gate("edge:4000 direct", h, g64, g32)


# ---- routes ----
@pytest.mark.parametrize("route", ("persistent", "persistent_c", "classic", "dense_late", "dense_early", "dense_det", "fill"))
def test_reverse_routes_small_image(route):
    S, dL = gr.scene("main")
    g64, g32 = gr_reference("main")
    with options(route):
        h = hip(S, dL)
        path = _lib.get_option("pergauss_path")
    assert bool(path & 1) == route.startswith("dense")
    gate(f"main {route}", h, g64, g32, S)


def test_length_ordered_route_large_image():
    S, dL = gr.scene("large")
    g64, g32 = gr_reference("large")
    with options("lpt"):
        h = hip(S, dL)
    gate("large lpt", h, g64, g32, S)


# ---- edge cases ----
def test_p0_nothing_in_view_and_no_grad():
    S, dL = scene("deg:1")
    empty = dataclasses.replace(S, means3D=np.zeros((0, 3), np.float32), opacities=np.zeros((0, 1), np.float32), shs=np.zeros((0, 4, 3), np.float32),
                                scales=np.zeros((0, 3), np.float32), rotations=np.zeros((0, 4), np.float32))
    h = hip(empty, dL)
    for k in KEYS:
        assert h[k] is not None and not h[k].any(), k
    S0, dL0 = gr.scene("r0")                                                      # every Gaussian behind the camera
    h = hip(S0, dL0)
    for k in KEYS:
        assert not h[k].any() and not np.signbit(h[k]).any(), k
    rs, inp = tensors(S)
    with torch.no_grad():
        out = GaussianRasterizer(rs)(**inp)
    assert out[0].grad_fn is None and len(out) == 2
    plain_rs, plain_inp = tensors(S, cam_grad=(False, False, False))
    assert torch.equal(GaussianRasterizer(plain_rs)(**plain_inp)[0], out[0])      # the same image either way


def test_only_campos_and_gaussians_without_grad():
    S, dL = scene("deg:2")
    g64, g32 = reference("deg:2")
    h = hip(S, dL, cam_grad=(False, False, True), gauss_grad=False)
    assert h["viewmatrix"] is None and h["projmatrix"] is None and h["means3D"] is None
    gate("deg:2 campos only", h, g64, g32, keys=("campos",))
    h = hip(S, dL, cam_grad=(True, True, False))
    assert h["campos"] is None
    gate("deg:2 matrices only", h, g64, g32, keys=("viewmatrix", "projmatrix"))


def test_side_stream_and_two_renders_in_flight():
    (S1, dL1), (S2, dL2) = scene("deg:1"), scene("deg:3")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        h = hip(S1, dL1)
    torch.cuda.current_stream().wait_stream(side)
    gate("deg:1 side stream", h, *reference("deg:1"), S1)
    # two renders in flight before their backward passes, backward in the other order
    rs1, in1 = tensors(S1); rs2, in2 = tensors(S2)
    c1 = GaussianRasterizer(rs1)(**in1)[0]
    c2 = GaussianRasterizer(rs2)(**in2)[0]
    (c2 * torch.tensor(dL2, dtype=torch.float32, device=DEV)).sum().backward()
    (c1 * torch.tensor(dL1, dtype=torch.float32, device=DEV)).sum().backward()
    gate("deg:1 in flight", cam_of(rs1), *reference("deg:1"))
    gate("deg:3 in flight", cam_of(rs2), *reference("deg:3"))


# ---- pose refinement ----
def test_pose_refinement_reduces_loss_and_pose_error():
    """A camera perturbed by a small rotation and translation, optimised with Adam on L1 against the unperturbed render of a fixed
    synthetic scene for a fixed number of steps: final loss and final pose error are both below their initial values."""
    from gaussian_transformer_amd.render import PipelineParams, render
    sc = synth.make_scene(P=2000, width=128, height=96, sh_degree=1, s0=0.12, seed=2)
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=DEV)

    class PC:
        get_xyz = t(sc.means3D); get_opacity = t(sc.opacities).reshape(-1, 1); get_scaling = t(sc.scales); get_rotation = t(sc.rotations)
        get_features = t(sc.shs); active_sh_degree = 1; max_sh_degree = 1
    bg, pipe = torch.zeros(3, device=DEV), PipelineParams()
    fovx, fovy = sc.camera.FoVx, sc.camera.FoVy
    with torch.no_grad():
        target = render(camera.torch_camera(torch.eye(4, device=DEV), fovx, fovy, 128, 96), PC(), pipe, bg)["render"]
    rot = torch.zeros(3, device=DEV).add_(torch.tensor([0.02, -0.015, 0.01], device=DEV)).requires_grad_(True)    # axis-angle, radians
    trans = torch.tensor([0.05, -0.04, 0.03], device=DEV, requires_grad=True)

    def w2c():
        x, y, z = rot
        o = torch.zeros((), device=DEV)
        K = torch.stack([torch.stack([o, -z, y]), torch.stack([z, o, -x]), torch.stack([-y, x, o])])
        R = torch.linalg.matrix_exp(K)
        top = torch.cat([R, trans[:, None]], 1)
        return torch.cat([top, torch.tensor([[0.0, 0.0, 0.0, 1.0]], device=DEV)], 0)

    def pose_error():
        return float(rot.detach().norm() + trans.detach().norm())
    opt = torch.optim.Adam([rot, trans], lr=2e-3)
    first = last = None
    e0 = pose_error()
    for step in range(60):
        opt.zero_grad()
        loss = (render(camera.torch_camera(w2c(), fovx, fovy, 128, 96), PC(), pipe, bg)["render"] - target).abs().mean()
        loss.backward()
        assert rot.grad is not None and trans.grad is not None and torch.isfinite(rot.grad).all() and torch.isfinite(trans.grad).all()
        opt.step()
        first = float(loss) if first is None else first
        last = float(loss)
    print(f"POSE refinement: loss {first:.5e} -> {last:.5e}, pose error {e0:.5e} -> {pose_error():.5e} (60 Adam steps)")
    assert last < first and pose_error() < e0
