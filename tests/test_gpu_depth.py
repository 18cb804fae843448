"""-m gpu: the depth and alpha maps (include/gsr_depth.h) through the public API -- GaussianRasterizer.forward(depth=...) -> ctypes ->
C ABI -> csrc/depth_maps.hip -- against the oracle used through the colour trick (tests/depth_ref.py).

The reference render S' carries the colour (v / vmax, 1, 0), vmax = max(1, max |v| over radii > 0): channel 0 of the oracle's image is the
depth map divided by that constant, so [D / vmax, A, 0] is compared with the project's image helpers at their absolute RGB tolerance and
the gradients -- of the same loss, with dL = (gD vmax, gA, 0) -- go through helpers.build_report / assert_parity with the gates unchanged.

Scenes: the five of tests/depth_ref.py (one Gaussian in one tile; odd image sizes that are no multiple of the tile; several tiles; lists
longer than one 64-entry batch; pixels that stop in front of the end of their lists) and one with replica accumulator rows: 272 x 256
pixels (17 x 16 tiles), 200 Gaussians and one that covers all 272 tiles (>= GSR_HOT_MIN_TILES = 256).  Seed 0 of that scene, float32
against float64 oracle on the CPU, both modes: 0 pixels over tolerance.
"""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib, synth
from gaussian_transformer_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer, arena_floats, gradient_arena
from tests import depth_ref as dr
from tests.helpers import (F32_P99_MAX, GRAD_RTOL, MAX_CERTIFIED_FRAC, assert_image_certified, assert_parity, build_report, grad_rows,
                           oracle_scene)

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPLICA = "replica"
CONFIGS = dr.SCENES + (REPLICA,)
IDS = [f"P{c[0]}" for c in dr.SCENES] + [REPLICA]
GRAD_NAMES = (("means3D", "dL_dmeans3D"), ("means2D", "dL_dmeans2D"), ("opacities", "dL_dopacity"), ("scales", "dL_dscales"),
              ("rotations", "dL_drots"), ("cov3D_precomp", "dL_dcov3D"))


@functools.lru_cache(maxsize=None)
def scene(cfg, cov=False):
    if cfg == REPLICA:
        sc = synth.make_scene(P=201, width=272, height=256, sh_degree=1, s0=0.05, seed=0)
        sc.scales[0] = np.array([8.0, 8.0, 8.0], np.float32)
        sc.opacities[0] = 0.6
    else:
        P, W, H, s0, seed = cfg
        sc = synth.make_scene(P=P, width=W, height=H, sh_degree=1, s0=s0, seed=seed)
    S = oracle_scene(sc)
    if cov:             # the same Gaussians given as packed 3D covariances (xx xy xz yy yz zz) of R S S^T R^T
        q = np.asarray(S.rotations, np.float64); s = np.asarray(S.scales, np.float64)
        r, x, y, z = q.T
        R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                      2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
        Mm = R * s[:, None, :]
        Sg = Mm @ Mm.transpose(0, 2, 1)
        cov6 = np.stack([Sg[:, 0, 0], Sg[:, 0, 1], Sg[:, 0, 2], Sg[:, 1, 1], Sg[:, 1, 2], Sg[:, 2, 2]], 1).astype(np.float32)
        S = dataclasses.replace(S, scales=None, rotations=None, cov3D_precomp=cov6)
    return S


def map_grads(S, which, seed=11):
    """Random upstream gradients of scale 1 / (H W) for the maps named in `which` ('D', 'A' or 'DA'); None for the others."""
    rng = np.random.default_rng(seed)
    gD = (rng.normal(size=(S.H, S.W)) / (S.H * S.W)).astype(np.float32)
    gA = (rng.normal(size=(S.H, S.W)) / (S.H * S.W)).astype(np.float32)
    return (gD if "D" in which else None), (gA if "A" in which else None)


@functools.lru_cache(maxsize=None)
def reference(cfg, mode, cov=False):
    """The oracle's side, computed once per (scene, mode) and shared: S' forward in float32 and float64 (same colours: the float32
    run's depths and vmax), and the gradients of the three losses."""
    S = scene(cfg, cov)
    t32 = dr.trick_forward(S, mode, "f32", scale="vmax")
    Sp = t32["scene"]
    r64 = dr.ref.get("f64")
    f64 = r64.forward(Sp, nthreads=r64.max_threads())
    t64 = dict(t32, fwd=f64)
    grads = {}
    for which in ("D", "A", "DA"):
        gD, gA = map_grads(S, which)
        grads[which] = (dr.trick_backward(t32, S, mode, gD, gA, "f32"), dr.trick_backward(t64, S, mode, gD, gA, "f64"))
    return dict(S=S, Sp=Sp, t32=t32, f64=f64, grads=grads)


def tensors(S, grad=True):
    P = int(np.asarray(S.means3D).shape[0])

    def t(a, g=grad):
        return None if a is None else torch.tensor(np.asarray(a, dtype=np.float32), device=DEV).requires_grad_(g)
    inp = dict(means3D=t(np.asarray(S.means3D).reshape(P, 3)), opacities=t(np.asarray(S.opacities).reshape(P, 1)), shs=t(S.shs),
               colors_precomp=t(S.colors_precomp), scales=t(S.scales), rotations=t(S.rotations), cov3D_precomp=t(S.cov3D_precomp))
    inp["means2D"] = torch.zeros((P, 3), dtype=torch.float32, device=DEV, requires_grad=grad)
    rs = GaussianRasterizationSettings(
        image_height=S.H, image_width=S.W, tanfovx=S.tanfovx, tanfovy=S.tanfovy, bg=t(S.bg, False), scale_modifier=S.scale_modifier,
        viewmatrix=t(np.asarray(S.viewmatrix).reshape(4, 4), False), projmatrix=t(np.asarray(S.projmatrix).reshape(4, 4), False),
        sh_degree=S.sh_degree, campos=t(S.campos, False), prefiltered=False, debug=False)
    return rs, inp


def dev(a):
    return None if a is None else torch.tensor(a, device=DEV)


def loss_of(out, gC=None, gD=None, gA=None):
    color, _radii, depth, alpha = out
    terms = []
    if gC is not None:
        terms.append((color * gC).sum())
    if gD is not None:
        terms.append((depth[0] * gD).sum())
    if gA is not None:
        terms.append((alpha[0] * gA).sum())
    return sum(terms)


def grads_of(inp):
    return {k: (None if v is None or v.grad is None else v.grad.detach().cpu().numpy().astype(np.float64)) for k, v in inp.items()}


def render_maps(S, mode, gC=None, gD=None, gA=None):
    """One render with the maps through the public API; backward of <gC, color> + <gD, depth> + <gA, alpha> if any is given."""
    rs, inp = tensors(S)
    out = GaussianRasterizer(rs)(depth=mode, **inp)
    res = dict(color=out[0].detach().cpu().numpy(), radii=out[1].cpu().numpy(), depth=out[2].detach().cpu().numpy(), alpha=out[3].detach().cpu().numpy(),
               out=out, inp=inp, rs=rs)
    if gC is not None or gD is not None or gA is not None:
        loss_of(out, dev(gC), dev(gD), dev(gA)).backward()
        res["grads"] = grads_of(inp)
    return res


def final_T_of(out, S):
    """1 - final_T as gsr_debug_read_image_state reads it from the image workspace of the render that produced `out`."""
    img = out[2].grad_fn.saved_tensors[9]
    fT = np.zeros((S.H, S.W), np.float32); nc = np.zeros((S.H, S.W), np.uint32)
    lib = _lib.load()
    _lib.check(lib.gsr_debug_read_image_state(torch.cuda.current_stream().cuda_stream, S.W, S.H, img.data_ptr(), fT.ctypes.data, nc.ctypes.data), "read image")
    return fT


# ---- images ----
@pytest.mark.parametrize("mode", ["expected", "inverse"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_maps_against_the_oracle(cfg, mode):
    R = reference(cfg, mode)
    S, t32 = R["S"], R["t32"]
    h = render_maps(S, mode)
    np.testing.assert_array_equal(h["radii"], t32["radii"])
    img = np.stack([h["depth"][0] / t32["vmax"], h["alpha"][0], np.zeros((S.H, S.W), np.float32)])
    st = assert_image_certified(img, t32["fwd"]["color"], t32["fwd"]["state"].decision_margin())
    print(cfg, mode, "vmax", t32["vmax"], st)
    assert st["over"] <= max(3, MAX_CERTIFIED_FRAC * st["pixels"]), st
    # alpha is 1 - final_T of the colour pass, bit for bit
    np.testing.assert_array_equal(h["alpha"][0], np.float32(1.0) - final_T_of(h["out"], S))
    # colour and radii of the 4-tuple are those of a plain render of the same inputs
    rs, inp = tensors(S, grad=False)
    color, radii = GaussianRasterizer(rs)(**inp)
    assert torch.equal(color, h["out"][0]) and torch.equal(radii, h["out"][1])
    if cfg == REPLICA:      # the scene does drive replica rows: the giant emits pairs for >= 256 tiles on the device too
        P = radii.shape[0]
        geom = h["out"][2].grad_fn.saved_tensors[7]
        tiles = np.zeros(P, np.uint32)
        _lib.check(_lib.load().gsr_debug_read_geom(torch.cuda.current_stream().cuda_stream, P, geom.data_ptr(), None, None, None, None, tiles.ctypes.data, None), "read geom")
        assert tiles[0] >= 256


# ---- gradients ----
def check_grads(R, h, which):
    S, Sp, t32 = R["S"], R["Sp"], R["t32"]
    g32, g64 = R["grads"][which]
    H, G32, G64 = {}, {}, {}
    for hk, rk in GRAD_NAMES:
        if h["grads"].get(hk) is None or g32.get(rk) is None:
            continue
        H[hk] = h["grads"][hk]
        G32[hk] = np.asarray(g32[rk], np.float64).reshape(H[hk].shape); G64[hk] = np.asarray(g64[rk], np.float64).reshape(H[hk].shape)
    assert {"means3D", "means2D", "opacities"} <= set(H) and ({"scales", "rotations"} <= set(H) or "cov3D_precomp" in H)
    img = np.stack([h["depth"][0] / t32["vmax"], h["alpha"][0], np.zeros((S.H, S.W), np.float32)])
    rep = build_report(Sp, t32["fwd"], R["f64"], img, H, G32, G64, radii_equal=bool(np.array_equal(h["radii"], t32["radii"])))
    print(which, {k: (rep["grads_vs_f32"][k]["p99"], rep["grads_vs_f32"][k]["fail_frac"], rep["grads"][k]["p99"], rep["grads_f32_oracle"][k]["p99"]) for k in H})
    assert_parity(rep)
    # the maps give the SH coefficients no gradient: None or zero
    sh = h["inp"]["shs"].grad
    assert sh is None or not bool(sh.any())


@pytest.mark.parametrize("which", ["D", "A", "DA"])
@pytest.mark.parametrize("mode", ["expected", "inverse"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_gradients_against_the_oracle(cfg, mode, which):
    R = reference(cfg, mode)
    gD, gA = map_grads(R["S"], which)
    check_grads(R, render_maps(R["S"], mode, gD=gD, gA=gA), which)


def test_gradients_with_precomputed_covariance():
    R = reference(dr.SCENES[2], "expected", True)
    gD, gA = map_grads(R["S"], "DA")
    h = render_maps(R["S"], "expected", gD=gD, gA=gA)
    assert h["grads"]["cov3D_precomp"] is not None and h["grads"]["scales"] is None
    check_grads(R, h, "DA")


# ---- colour, depth and alpha losses in one graph ----
def assert_sums_agree(got, want):
    """Float atomics land in another order from run to run, and the combined pass adds two float32 results: close, not bit-equal."""
    for k, a in got.items():
        if a is None:
            assert want[k] is None, k
            continue
        st = grad_rows(a, want[k])
        assert st["p99"] <= F32_P99_MAX and st["max"] <= GRAD_RTOL, (k, st)


@pytest.mark.parametrize("arena", [False, True], ids=["tensors", "arena"])
@pytest.mark.parametrize("cfg,mode", [(dr.SCENES[3], "expected"), (REPLICA, "inverse")], ids=["P3000", REPLICA])
def test_combined_losses_equal_the_sum_of_separate_graphs(cfg, mode, arena):
    S = scene(cfg)
    gD, gA = map_grads(S, "DA")
    gC = (np.random.default_rng(3).normal(size=(3, S.H, S.W)) / (S.H * S.W)).astype(np.float32)
    colour = render_maps(S, mode, gC=gC)["grads"]
    maps = render_maps(S, mode, gD=gD, gA=gA)["grads"]
    want = {k: (None if colour[k] is None and maps[k] is None else (0 if colour[k] is None else colour[k]) + (0 if maps[k] is None else maps[k])) for k in colour}
    if not arena:
        assert_sums_agree(render_maps(S, mode, gC=gC, gD=gD, gA=gA)["grads"], want)
        return
    P, M = int(S.means3D.shape[0]), int(S.shs.shape[1])
    flat = torch.full((arena_floats(P, M, True),), float("nan"), device=DEV)
    with gradient_arena(flat):
        h = render_maps(S, mode, gC=gC, gD=gD, gA=gA)
    assert_sums_agree(h["grads"], want)
    assert not bool(torch.isnan(flat).any()) and torch.equal(flat[:3 * P].view(P, 3), h["inp"]["means3D"].grad)      # the arena holds the combined gradients
    # the maps alone: an arena around forward and backward (the colour pass runs with a zero gradient first: only it joins the
    # library's fill of the announced slices), and around the backward call only (the map pass carves the arena itself)
    for around_forward in (True, False):
        flat.fill_(float("nan"))
        if around_forward:
            with gradient_arena(flat):
                h = render_maps(S, mode, gD=gD, gA=gA)
        else:
            h = render_maps(S, mode)
            with gradient_arena(flat):
                loss_of(h["out"], None, dev(gD), dev(gA)).backward()
            h["grads"] = grads_of(h["inp"])
        assert h["grads"]["shs"] is None
        assert_sums_agree({k: v for k, v in h["grads"].items() if k != "shs"}, {k: v for k, v in maps.items() if k != "shs"})
        assert not bool(torch.isnan(flat).any()) and not bool(flat[3 * P:3 * P + 3 * M * P].any()), around_forward      # the SH slice reads zero
        assert torch.equal(flat[:3 * P].view(P, 3), h["inp"]["means3D"].grad)


# ---- robustness ----
def test_list_builders_give_identical_maps():
    S = scene(dr.SCENES[3])
    outs = []
    try:
        for tl in (0, 2):
            _lib.set_option("tile_lists", tl)
            h = render_maps(S, "expected")
            outs.append((h["depth"], h["alpha"]))
    finally:
        _lib.set_option("tile_lists", 2)
    np.testing.assert_array_equal(outs[0][0], outs[1][0])
    np.testing.assert_array_equal(outs[0][1], outs[1][1])


def test_no_gaussians_and_a_camera_that_sees_nothing():
    S = scene(dr.SCENES[1])
    empty = dataclasses.replace(S, means3D=np.zeros((0, 3), np.float32), opacities=np.zeros((0, 1), np.float32), shs=np.zeros((0, 4, 3), np.float32),
                                scales=np.zeros((0, 3), np.float32), rotations=np.zeros((0, 4), np.float32))
    m = np.asarray(S.viewmatrix, np.float64).reshape(16)
    behind = dataclasses.replace(S, means3D=(np.asarray(S.means3D, np.float64) - 1000.0 * np.array([m[2], m[6], m[10]])).astype(np.float32))
    gD, gA = map_grads(S, "DA")
    for name, Sx in (("P = 0", empty), ("nothing in view", behind)):
        h = render_maps(Sx, "inverse", gD=gD, gA=gA)
        assert not h["depth"].any() and not h["alpha"].any() and h["depth"].shape == (1, S.H, S.W), name
        assert not (h["radii"] > 0).any(), name
        # (an empty scales tensor reads as "not given", as in the plain call: no gradient for it with P = 0)
        for k in ("means3D", "means2D", "opacities") + (("scales", "rotations") if Sx.means3D.shape[0] else ()):
            g = h["grads"][k]
            assert g is not None and g.shape[0] == Sx.means3D.shape[0] and not g.any(), (name, k)


def test_no_grad_gives_the_same_maps():
    S = scene(dr.SCENES[2])
    h = render_maps(S, "expected")
    rs, inp = tensors(S)
    with torch.no_grad():
        out = GaussianRasterizer(rs)(depth="expected", **inp)
    assert all(o.grad_fn is None for o in out)
    for a, b in zip(out, h["out"]):
        assert torch.equal(a, b)


def test_strided_non_leaf_inputs():
    """Every input a slice of one [P,26] row tensor: non-contiguous, no leaf.  The gradients reach the rows."""
    S = scene(dr.SCENES[2])
    gD, gA = map_grads(S, "DA")
    want = render_maps(S, "expected", gD=gD, gA=gA)
    P = int(S.means3D.shape[0])
    rows = torch.zeros((P, 26), device=DEV)
    rs, inp = tensors(S, grad=False)
    rows[:, 0:3] = inp["means3D"]; rows[:, 3:15] = inp["shs"].reshape(P, 12); rows[:, 15:16] = inp["opacities"]
    rows[:, 16:19] = inp["scales"]; rows[:, 19:23] = inp["rotations"]
    rows.requires_grad_(True)
    means2D = torch.zeros((P, 3), device=DEV, requires_grad=True)
    out = GaussianRasterizer(rs)(means3D=rows[:, 0:3], means2D=means2D, shs=rows[:, 3:15].reshape(P, 4, 3), opacities=rows[:, 15:16],
                                 scales=rows[:, 16:19], rotations=rows[:, 19:23], depth="expected")
    assert not rows[:, 16:19].is_contiguous()
    assert torch.equal(out[2], want["out"][2]) and torch.equal(out[3], want["out"][3])
    loss_of(out, None, dev(gD), dev(gA)).backward()
    g = rows.grad.cpu().numpy().astype(np.float64)
    got = dict(means3D=g[:, 0:3], opacities=g[:, 15:16], scales=g[:, 16:19], rotations=g[:, 19:23], means2D=means2D.grad.cpu().numpy().astype(np.float64))
    assert_sums_agree(got, {k: want["grads"][k] for k in got})
    assert not g[:, 3:15].any() and not g[:, 23:].any()


def test_on_a_side_stream():
    S = scene(dr.SCENES[2])
    gD, gA = map_grads(S, "DA")
    want = render_maps(S, "inverse", gD=gD, gA=gA)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        h = render_maps(S, "inverse", gD=gD, gA=gA)
    s.synchronize()
    np.testing.assert_array_equal(h["depth"], want["depth"]); np.testing.assert_array_equal(h["alpha"], want["alpha"])
    assert_sums_agree(h["grads"], want["grads"])


def test_two_renders_in_flight_then_both_backwards():
    Sa, Sb = scene(dr.SCENES[2]), scene(dr.SCENES[3])
    ga, gb = map_grads(Sa, "DA"), map_grads(Sb, "DA", seed=12)
    wa, wb = render_maps(Sa, "expected", gD=ga[0], gA=ga[1]), render_maps(Sb, "inverse", gD=gb[0], gA=gb[1])
    (rsa, ia), (rsb, ib) = tensors(Sa), tensors(Sb)
    oa = GaussianRasterizer(rsa)(depth="expected", **ia)
    ob = GaussianRasterizer(rsb)(depth="inverse", **ib)
    assert torch.equal(oa[2], wa["out"][2]) and torch.equal(ob[2], wb["out"][2])
    loss_of(oa, None, dev(ga[0]), dev(ga[1])).backward()
    loss_of(ob, None, dev(gb[0]), dev(gb[1])).backward()
    assert_sums_agree(grads_of(ia), wa["grads"])
    assert_sums_agree(grads_of(ib), wb["grads"])


def test_deterministic_bwd_is_refused_and_the_device_stays_usable():
    S = scene(dr.SCENES[1])
    gD, gA = map_grads(S, "DA")
    rs, inp = tensors(S)
    try:
        _lib.set_option("deterministic_bwd", 1)
        out = GaussianRasterizer(rs)(depth="expected", **inp)          # the forward walk does not care
        with pytest.raises(_lib.GsrError, match="deterministic_bwd is on"):
            loss_of(out, None, dev(gD), dev(gA)).backward()
    finally:
        _lib.set_option("deterministic_bwd", 0)
    rs, inp = tensors(S)
    color, radii = GaussianRasterizer(rs)(**{k: v for k, v in inp.items()})
    color.sum().backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(color).all()) and inp["means3D"].grad is not None
    h = render_maps(S, "expected", gD=gD, gA=gA)                      # and the maps work again
    assert h["grads"]["means3D"] is not None and np.isfinite(h["grads"]["means3D"]).all()
