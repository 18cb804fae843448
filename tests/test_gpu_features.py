"""-m gpu: the N-channel feature maps (include/gsr_features.h) through the public API -- GaussianRasterizer.forward(features=...) ->
ctypes -> C ABI -> csrc/feature_maps.hip -- against the oracle used through the colour trick (tests/features_ref.py).

The reference renders carry the colours F[:, 3k:3k+3] / fmax, fmax = max(1, max |F|) over radii > 0: a triple of the oracle's image is
three channels of the map divided by that constant, compared with the project's image helpers at their absolute RGB tolerance, and
the gradients -- of the same loss, the triples' added, dL/dF held as dL_dcolors is -- go through helpers.build_report / assert_parity with
the gates unchanged.  The oracle's side is computed once per (scene, triple) and shared (features_ref.reference).

Scenes: the five of tests/depth_ref.py (one Gaussian in one tile; odd image sizes that are no multiple of the tile; several tiles; lists
longer than one 64-entry batch; pixels that stop in front of the end of their lists) and tests/test_gpu_depth.py's replica scene.
Channel counts: features_ref.EDGE_CHANNELS holds chunk - 1, chunk and chunk + 1 of the kernels' chunks (4, 8, 16) and the same around
32 and 64, where the number of 16-channel chunks changes.
"""
import dataclasses

import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib
from gaussian_transformer_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
from gaussian_transformer_amd.render import PipelineParams, render, render_fused
from gaussian_transformer_amd.rows import render_rows
from tests import depth_ref as dr
from tests import features_ref as fr
from tests.helpers import F32_P99_MAX, GRAD_RTOL, RGB_ATOL, grad_rows

pytestmark = pytest.mark.gpu
DEV = "cuda"


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


def grads_of(inp):
    return {k: (None if v is None or v.grad is None else v.grad.detach().cpu().numpy().astype(np.float64)) for k, v in inp.items()}


def render_features(S, F, gF=None, gC=None, gD=None, gA=None, depth=None, feat_grad=True):
    """One render with the feature map through the public API; backward of <gF, feat> + <gC, color> + <gD, depth> + <gA, alpha> for
    those given."""
    rs, inp = tensors(S)
    inp["features"] = torch.tensor(F, device=DEV).requires_grad_(feat_grad)
    extra = {} if depth is None else {"depth": depth}
    out = GaussianRasterizer(rs)(**inp, **extra)
    res = dict(color=out[0].detach().cpu().numpy(), radii=out[1].cpu().numpy(), feat=out[-1].detach().cpu().numpy(), out=out, inp=inp, rs=rs)
    terms = [(o * dev(g)).sum() for o, g in ((out[-1], gF), (out[0], gC)) if g is not None]
    if depth is not None:
        terms += [(o[0] * dev(g)).sum() for o, g in ((out[2], gD), (out[3], gA)) if g is not None]
    if terms:
        sum(terms).backward()
        res["grads"] = grads_of(inp)
    return res


def check(R, C, h):
    assert h["feat"].shape == (C, R.S.H, R.S.W)
    np.testing.assert_array_equal(h["radii"], R.radii)
    print(C, fr.check_against(R, C, h["feat"], h.get("grads"), h["radii"]))


# ---- channel counts: around every chunk size, on sizes that are no multiple of the tile ----
@pytest.mark.parametrize("C", fr.EDGE_CHANNELS)
def test_channel_edges(C):
    R = fr.reference(dr.SCENES[1])
    o = R.of(C)
    check(R, C, render_features(R.S, o["F"], gF=o["G"]))


# ---- scenes ----
@pytest.mark.parametrize("C", fr.SCENE_CHANNELS)
@pytest.mark.parametrize("cfg", fr.CONFIGS, ids=fr.IDS)
def test_scenes_against_the_oracle(cfg, C):
    R = fr.reference(cfg)
    o = R.of(C)
    h = render_features(R.S, o["F"], gF=o["G"])
    check(R, C, h)
    if cfg == fr.REPLICA:      # the scene does drive replica rows: the giant emits pairs for >= 256 tiles on the device too
        P = h["radii"].shape[0]
        fresh = render_features(R.S, o["F"])                           # (a render of its own: the backward above freed h's workspaces)
        geom = fresh["out"][2].grad_fn.saved_tensors[7]
        tiles = np.zeros(P, np.uint32)
        _lib.check(_lib.load().gsr_debug_read_geom(torch.cuda.current_stream().cuda_stream, P, geom.data_ptr(), None, None, None, None, tiles.ctypes.data, None), "read geom")
        assert tiles[0] >= 256


@pytest.mark.parametrize("C", fr.SCENE_CHANNELS)
def test_precomputed_covariance(C):
    R = fr.reference(dr.SCENES[2], True)
    o = R.of(C)
    h = render_features(R.S, o["F"], gF=o["G"])
    assert h["grads"]["cov3D_precomp"] is not None and h["grads"]["scales"] is None
    check(R, C, h)


def test_sixty_four_channels():
    R = fr.reference(dr.SCENES[3])
    o = R.of(64)
    check(R, 64, render_features(R.S, o["F"], gF=o["G"]))


# ---- colour, depth, alpha and features in one graph ----
def assert_sums_agree(got, want):
    """Float atomics land in another order from run to run, and a combined pass adds float32 results: close, not bit-equal."""
    for k, a in got.items():
        if a is None:
            assert want[k] is None, k
            continue
        st = grad_rows(a, want[k])
        assert st["p99"] <= F32_P99_MAX and st["max"] <= GRAD_RTOL, (k, st)


def map_losses(S, seed=3):
    rng = np.random.default_rng(seed)
    n = S.H * S.W
    return ((rng.normal(size=(3, S.H, S.W)) / n).astype(np.float32), (rng.normal(size=(S.H, S.W)) / n).astype(np.float32),
            (rng.normal(size=(S.H, S.W)) / n).astype(np.float32))


@pytest.mark.parametrize("cfg", [dr.SCENES[3], fr.REPLICA], ids=["P3000", fr.REPLICA])
def test_one_graph_equals_the_sum_of_the_oracles_gradients(cfg):
    """<gC, color> + <gD, depth> + <gA, alpha> + <gF, feat> in one graph (the colour pass, then the depth pass and the feature pass with
    accumulate = 1) against the oracle: colour by its own run, depth and alpha through tests/depth_ref.py, features through the trick."""
    C, mode = 5, "expected"
    R = fr.reference(cfg)
    S, o = R.S, R.of(C)
    gC, gD, gA = map_losses(S)
    h = render_features(S, o["F"], gF=o["G"], gC=gC, gD=gD, gA=gA, depth=mode)
    assert len(h["out"]) == 5 and h["out"][2].shape == (1, S.H, S.W) and h["out"][4].shape == (C, S.H, S.W)
    want32, want64 = {}, {}
    for prec, want in (("f32", want32), ("f64", want64)):
        r = dr.ref.get(prec)
        f = r.forward(S, nthreads=r.max_threads())
        gc = r.backward(f, gC.astype(np.float64), nthreads=r.max_threads())
        t = dr.trick_forward(S, mode, prec, scale="vmax")
        gm = dr.trick_backward(t, S, mode, gD, gA, prec)
        gf = o["g32" if prec == "f32" else "g64"]
        for hk, rk in fr.GRAD_NAMES[:5]:
            want[hk] = np.asarray(gc[rk], np.float64).reshape(len(R.radii), -1) + np.asarray(gm[rk], np.float64).reshape(len(R.radii), -1) + \
                gf[rk].reshape(len(R.radii), -1)
        want["features"] = gf["dL_dfeatures"]
        want["shs"] = np.asarray(gc["dL_dsh"], np.float64)
    for k, w64 in want64.items():
        got = h["grads"][k].reshape(w64.shape)
        st, base, v32 = grad_rows(got, w64), grad_rows(want32[k], w64), grad_rows(got, want32[k])
        print(k, st["p99"], base["p99"], v32["p99"], v32["fail_frac"])
        assert st["fail_frac"] <= 2.0 * base["fail_frac"] + 1e-3 and st["p99"] <= max(GRAD_RTOL, 2.0 * base["p99"]), (k, st, base)
        assert v32["fail_frac"] <= 2e-3 and v32["p99"] <= F32_P99_MAX, (k, v32)
    # the same graph piece by piece: features alone (accumulate = 0) and colour + features (accumulate = 1) add up to colour + features
    alone_h = render_features(S, o["F"], gF=o["G"])
    alone = alone_h["grads"]
    colour = render_features(S, o["F"], gC=gC)["grads"]
    assert colour["features"] is None and alone["shs"] is None
    both = render_features(S, o["F"], gF=o["G"], gC=gC)["grads"]
    want = {k: (None if colour[k] is None and alone[k] is None else (0 if colour[k] is None else colour[k]) + (0 if alone[k] is None else alone[k])) for k in both}
    assert_sums_agree(both, want)
    check(R, C, alone_h)


# ---- consistency with what exists ----
def test_the_colours_as_features_give_the_colour_image_and_ones_give_the_alpha_map():
    S0 = fr.scene(dr.SCENES[3])
    P = S0.means3D.shape[0]
    col = np.random.default_rng(5).uniform(0.0, 1.0, size=(P, 3)).astype(np.float32)
    S = dataclasses.replace(S0, shs=None, colors_precomp=col, bg=np.zeros(3, np.float32), sh_degree=0)
    F = np.concatenate([col, np.ones((P, 1), np.float32)], axis=1)
    rs, inp = tensors(S, grad=False)
    color, _radii, _depth, alpha, feat = GaussianRasterizer(rs)(depth="expected", features=torch.tensor(F, device=DEV), **inp)
    assert float((feat[:3] - color).abs().max()) <= RGB_ATOL
    assert float((feat[3] - alpha[0]).abs().max()) <= RGB_ATOL
    again = GaussianRasterizer(rs)(features=torch.tensor(F, device=DEV), **inp)
    assert len(again) == 3 and torch.equal(again[2], feat) and torch.equal(again[0], color)      # bit-identical from run to run


# ---- glue ----
def test_a_strided_non_leaf_view_receives_its_gradient():
    R = fr.reference(dr.SCENES[2])
    C, a = 6, 23
    o = R.of(C)
    want = render_features(R.S, o["F"], gF=o["G"])
    P = R.S.means3D.shape[0]
    rows = torch.zeros((P, 40), device=DEV)
    rows[:, a:a + C] = torch.tensor(o["F"], device=DEV)
    rows.requires_grad_(True)
    rs, inp = tensors(R.S)
    scaled = rows * 1.0                                            # no leaf
    view = scaled[:, a:a + C]
    assert not view.is_contiguous() and view.grad_fn is not None
    out = GaussianRasterizer(rs)(features=view, **inp)
    assert torch.equal(out[2], want["out"][2])
    (out[2] * dev(o["G"])).sum().backward()
    g = rows.grad.cpu().numpy().astype(np.float64)
    assert_sums_agree({"features": g[:, a:a + C]}, {"features": want["grads"]["features"]})
    assert not g[:, :a].any() and not g[:, a + C:].any()
    assert_sums_agree({k: v for k, v in grads_of(inp).items() if k != "features"}, {k: v for k, v in want["grads"].items() if k != "features"})


def test_features_that_need_no_gradient():
    R = fr.reference(dr.SCENES[3])
    C = 17
    o = R.of(C)
    want = render_features(R.S, o["F"], gF=o["G"])
    h = render_features(R.S, o["F"], gF=o["G"], feat_grad=False)
    assert h["grads"]["features"] is None and h["inp"]["features"].grad is None
    assert_sums_agree({k: v for k, v in h["grads"].items() if k != "features"}, {k: v for k, v in want["grads"].items() if k != "features"})
    check(R, C, dict(h, grads={k: v for k, v in h["grads"].items() if k != "features"}))


def test_without_the_keyword_the_call_is_the_plain_one():
    S = fr.scene(dr.SCENES[2])
    rs, inp = tensors(S, grad=False)
    plain = GaussianRasterizer(rs)(**inp)
    none = GaussianRasterizer(rs)(features=None, **inp)
    assert len(plain) == len(none) == 2 and torch.equal(plain[0], none[0]) and torch.equal(plain[1], none[1])
    F = torch.tensor(fr.reference(dr.SCENES[2]).F[:, :3].copy(), device=DEV)
    with_f = GaussianRasterizer(rs)(features=F, **inp)
    assert torch.equal(with_f[0], plain[0]) and torch.equal(with_f[1], plain[1])
    with torch.no_grad():
        rs2, inp2 = tensors(S)
        out = GaussianRasterizer(rs2)(features=F, **inp2)
    assert all(o.grad_fn is None for o in out) and torch.equal(out[2], with_f[2])


def test_two_renders_in_flight_then_both_backwards():
    Ra, Rb = fr.reference(dr.SCENES[2]), fr.reference(dr.SCENES[3])
    oa, ob = Ra.of(4), Rb.of(17)
    wa, wb = render_features(Ra.S, oa["F"], gF=oa["G"]), render_features(Rb.S, ob["F"], gF=ob["G"])
    (rsa, ia), (rsb, ib) = tensors(Ra.S), tensors(Rb.S)
    ia["features"] = torch.tensor(oa["F"], device=DEV).requires_grad_(True)
    ib["features"] = torch.tensor(ob["F"], device=DEV).requires_grad_(True)
    xa = GaussianRasterizer(rsa)(**ia)
    xb = GaussianRasterizer(rsb)(**ib)
    assert torch.equal(xa[2], wa["out"][2]) and torch.equal(xb[2], wb["out"][2])
    (xa[2] * dev(oa["G"])).sum().backward()
    (xb[2] * dev(ob["G"])).sum().backward()
    assert_sums_agree(grads_of(ia), wa["grads"])
    assert_sums_agree(grads_of(ib), wb["grads"])


def test_render_adds_the_features_to_its_dict():
    from gaussian_transformer_amd import synth
    from gaussian_transformer_amd.model import GaussianParams
    from gaussian_transformer_amd.render import TorchCamera
    sc = synth.make_scene(P=300, width=48, height=40, sh_degree=1, s0=0.05, seed=2)
    pc = GaussianParams.from_synthetic(sc, DEV)
    cam = TorchCamera(sc.camera, DEV)
    F = torch.rand((300, 5), device=DEV)
    d = render(cam, pc, PipelineParams(), torch.zeros(3, device=DEV), features=F)
    assert d["features"].shape == (5, 40, 48) and "depth" not in d
    d2 = render(cam, pc, PipelineParams(), torch.zeros(3, device=DEV), features=F, depth="inverse")
    assert torch.equal(d2["features"], d["features"]) and d2["depth"].shape == (1, 40, 48) and d2["alpha"].shape == (1, 40, 48)


def test_the_stated_limits_raise():
    S = fr.scene(dr.SCENES[1])
    R = fr.reference(dr.SCENES[1])
    F = torch.tensor(R.F[:, :4].copy(), device=DEV, requires_grad=True)
    rs, inp = tensors(S)
    with pytest.raises(_lib.GsrError, match="no camera gradient of the feature map"):
        GaussianRasterizer(rs._replace(viewmatrix=rs.viewmatrix.clone().requires_grad_(True)))(features=F, **inp)
    with pytest.raises(_lib.GsrError, match="render_fused: no feature maps on the raw-parameter path"):
        render_fused(None, None, PipelineParams(), None, features=F)
    with pytest.raises(_lib.GsrError, match="render_rows: no feature maps on the raw-parameter path"):
        render_rows([], None, PipelineParams(), None, features=F)
    for bad in (F[:, :0], torch.zeros((F.shape[0], 65), device=DEV), F[:-1], F.double()):
        with pytest.raises(_lib.GsrError, match="features must"):
            GaussianRasterizer(rs)(features=bad, **inp)
    try:
        _lib.set_option("deterministic_bwd", 1)
        out = GaussianRasterizer(rs)(features=F, **inp)                # the forward walk does not care
        with pytest.raises(_lib.GsrError, match="deterministic_bwd is on"):
            out[2].sum().backward()
    finally:
        _lib.set_option("deterministic_bwd", 0)
    rs, inp = tensors(S)                                               # and the device stays usable
    out = GaussianRasterizer(rs)(features=F, **inp)
    out[2].sum().backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(inp["means3D"].grad).all()) and F.grad is not None
