"""The reference of the depth and alpha maps (tests/depth_ref.py) checked against itself on the CPU: the colour trick on the oracle
against an independent per-pixel re-composition from the oracle's lists, and three planted faults told from the correct result."""
import dataclasses

import numpy as np
import pytest

from gaussian_transformer_amd import synth
from tests import depth_ref as dr
from tests.helpers import oracle_scene


def scene(P, W, H, s0, seed):
    return oracle_scene(synth.make_scene(P=P, width=W, height=H, sh_degree=1, s0=s0, seed=seed))


@pytest.mark.parametrize("mode", ["expected", "inverse"])
@pytest.mark.parametrize("cfg", dr.SCENES[:3], ids=lambda c: f"P{c[0]}")
def test_trick_agrees_with_the_per_pixel_recomposition(cfg, mode):
    S = scene(*cfg)
    t = dr.trick_forward(S, mode)
    D, A, vmax = dr.depth_alpha_pixels(S, mode)
    assert vmax == t["vmax"]
    print("max |dD| / vmax", np.abs(D - t["depth"]).max() / vmax, "max |dA|", np.abs(A - t["alpha"]).max())
    assert np.abs(D - t["depth"]).max() <= 1e-6 * vmax
    assert np.abs(A - t["alpha"]).max() <= 1e-6
    # the oracle's alpha channel is 1 - final_T (issue: to 5e-7)
    fT = t["fwd"]["state"].image_state()["final_T"]
    assert np.abs(t["alpha"] - (1.0 - fT.astype(np.float64))).max() <= 5e-7


def test_trick_scale_is_only_a_constant():
    S = scene(*dr.SCENES[1])
    a, b = dr.trick_forward(S, "expected"), dr.trick_forward(S, "expected", scale="vmax")
    assert b["scale"] == b["vmax"] > 1.0
    assert np.abs(a["depth"] - b["depth"]).max() <= 1e-6 * a["vmax"] and np.array_equal(a["alpha"], b["alpha"])
    rng = np.random.default_rng(0)
    gD, gA = rng.normal(size=(S.H, S.W)) / (S.H * S.W), rng.normal(size=(S.H, S.W)) / (S.H * S.W)
    ga, gb = dr.trick_backward(a, S, "expected", gD, gA), dr.trick_backward(b, S, "expected", gD, gA)
    for k in ("dL_dmeans3D", "dL_dopacity", "dL_dscales", "dL_drots", "dL_dv"):
        scale = np.abs(ga[k]).max()
        assert scale > 0 and np.abs(ga[k] - gb[k]).max() <= 1e-4 * scale, k


def test_the_mean_gradient_includes_the_depth_term():
    """Finite differences in float64: moving a Gaussian along the view axis changes the depth map through v as well as through the splat."""
    S = scene(*dr.SCENES[1])
    for mode in ("expected", "inverse"):
        t = dr.trick_forward(S, mode, precision="f64")
        rng = np.random.default_rng(5)
        gD = rng.normal(size=(S.H, S.W)) / (S.H * S.W)
        g = dr.trick_backward(t, S, mode, gD, None, precision="f64")
        i = int(np.abs(g["dL_dv"]).argmax())
        for ax in range(3):
            vals = []
            for h in (1e-5, -1e-5):
                m = np.array(S.means3D, np.float64); m[i, ax] += h
                vals.append(float((gD * dr.trick_forward(dataclasses.replace(S, means3D=m), mode, precision="f64")["depth"]).sum()))
            fd = (vals[0] - vals[1]) / 2e-5
            assert abs(fd - g["dL_dmeans3D"][i, ax]) <= 1e-4 * max(abs(fd), np.abs(g["dL_dmeans3D"][i]).max()), (mode, ax, fd, g["dL_dmeans3D"][i])


# a scene dense enough that pixels stop (T < 1e-4) in front of the end of their lists: only there can the first two faults show
DENSE = (4000, 32, 32, 0.2, 7)


@pytest.mark.parametrize("fault", ["blend_stop", "alpha_whole_list", "normalised"])
def test_planted_faults_are_told_from_the_correct_result(fault):
    S = scene(*(dr.SCENES[2] if fault == "normalised" else DENSE))      # (dividing by alpha shows where alpha is far from 1: a sparse scene)
    t = dr.trick_forward(S, "expected")
    vmax = t["vmax"]
    step = 3
    ys, xs = np.arange(0, S.H, step), np.arange(0, S.W, step)
    sub = lambda a: a[np.ix_(ys, xs)]
    D0, A0, _ = dr.depth_alpha_pixels(S, "expected", step=step)
    assert np.abs(sub(D0) - sub(t["depth"])).max() <= 1e-6 * vmax and np.abs(sub(A0) - sub(t["alpha"])).max() <= 1e-6
    D, A, _ = dr.depth_alpha_pixels(S, "expected", fault=fault, step=step)
    dD, dA = np.abs(sub(D) - sub(t["depth"])) / vmax, np.abs(sub(A) - sub(t["alpha"]))
    print(fault, "pixels over 1e-4:", int((dD > 1e-4).sum()), int((dA > 1e-4).sum()), "max", dD.max(), dA.max())
    # the check the GPU test applies (helpers.RGB_ATOL = 1e-4 on [D / vmax, A]) must see the fault on far more than a handful of pixels
    over = ((dD > 1e-4) | (dA > 1e-4)).sum()
    assert over > 10, (fault, over)
    if fault == "alpha_whole_list":
        assert (dD <= 1e-6).all()          # this fault lives in the alpha map alone
    if fault == "normalised":
        assert (dA <= 1e-6).all()


@pytest.mark.parametrize("mode", ["expected", "inverse"])
def test_the_large_scene_certifies_itself(mode):
    """depth_ref.LARGE, the reference alone: the float64 oracle's [D / vmax, A, 0] against the float32 oracle's through the certificate
    the GPU tests apply, and the float32 oracle's gradients in the place of a device's through assert_parity.  Measured, both modes:
    6363 tiles, 5 empty, 67452 pairs, longest list 23; 2 pixels over tolerance, 0 uncertified, cap max(3, 1e-5 * 1628928) = 16."""
    from oracle import ref
    from tests.helpers import MAX_CERTIFIED_FRAC, assert_image_certified, assert_parity, build_report
    S = oracle_scene(synth.make_scene(**dr.LARGE))
    t32 = dr.trick_forward(S, mode, "f32", scale="vmax")
    r64 = ref.get("f64")
    f64 = r64.forward(t32["scene"], nthreads=r64.max_threads())
    ranges = np.asarray(t32["base_fwd"]["state"].binning()["ranges"], np.int64)
    lengths = ranges[:, 1] - ranges[:, 0]
    st = assert_image_certified(f64["color"], t32["fwd"]["color"], t32["fwd"]["state"].decision_margin())
    cap = max(3, MAX_CERTIFIED_FRAC * st["pixels"])
    print(mode, st, "tiles", len(lengths), "empty", int((lengths == 0).sum()), "pairs", int(lengths.sum()), "longest", int(lengths.max()), "cap", cap)
    assert st["over"] <= cap / 4, (st, cap)                   # the reference alone uses at most a quarter of what a device is allowed
    assert (lengths == 0).any()                               # some tile is empty
    assert len(lengths) == ((S.W + 15) // 16) * ((S.H + 15) // 16) > 6144      # past the persistent kernels' image size
    rng = np.random.default_rng(11)
    gD, gA = rng.normal(size=(S.H, S.W)) / (S.H * S.W), rng.normal(size=(S.H, S.W)) / (S.H * S.W)
    g32 = dr.trick_backward(t32, S, mode, gD, gA, "f32")
    g64 = dr.trick_backward(dict(t32, fwd=f64), S, mode, gD, gA, "f64")
    names = (("means3D", "dL_dmeans3D"), ("means2D", "dL_dmeans2D"), ("opacities", "dL_dopacity"), ("scales", "dL_dscales"), ("rotations", "dL_drots"))
    G32 = {k: np.asarray(g32[r], np.float64).reshape(S.means3D.shape[0], -1) for k, r in names}
    G64 = {k: np.asarray(g64[r], np.float64).reshape(G32[k].shape) for k, r in names}
    assert_parity(build_report(t32["scene"], t32["fwd"], f64, t32["fwd"]["color"], G32, G32, G64, radii_equal=True))
