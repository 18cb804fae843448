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
