"""The reference of the feature maps (tests/features_ref.py) checked against itself on the CPU: the colour trick on the oracle against
an independent per-pixel re-composition from the oracle's lists, three planted faults told from the correct result, and every scene
and channel count tests/test_gpu_features.py uses certifying itself: the float64 oracle's triples against the float32 oracle's
through the certificate and the gradient gates the GPU tests apply."""
import numpy as np
import pytest

from tests import depth_ref as dr
from tests import features_ref as fr
from tests.helpers import F32_FAIL_FRAC_MAX, F32_P99_MAX, GRAD_RTOL, RGB_ATOL, grad_rows


@pytest.mark.parametrize("C", [1, 4, 7])
@pytest.mark.parametrize("cfg", dr.SCENES[:3], ids=lambda c: f"P{c[0]}")
def test_trick_agrees_with_the_per_pixel_recomposition(cfg, C):
    S = fr.scene(cfg)
    R = fr.reference(cfg)
    F = R.F[:, :C]
    t = fr.trick_forward(S, F)
    assert t["fmax"] == fr.fmax_of(F, t["radii"]) == (fr.FMAX if (t["radii"] > 0).any() else 1.0)
    assert (F < 0).any() or S.means3D.shape[0] == 1                # negative features are part of the test
    step = 1 if S.W * S.H <= 1024 else 3
    M = fr.feature_pixels(S, F, step=step)
    seen = ~np.isnan(M)
    d = np.abs(M[seen] - t["map"][seen]).max()
    print("max |d map| / fmax", d / t["fmax"])
    assert d <= 1e-6 * t["fmax"]
    # ... and the shared per-triple runs compose to the same map
    o = R.of(C)
    for lo, hi, tr in o["triples"]:
        np.testing.assert_array_equal(np.asarray(tr["f32"]["color"], np.float64)[:hi - lo] * o["fmax"], t["map"][lo:hi])


def test_the_trick_gradient_is_the_gradient_of_the_map():
    """Finite differences in float64 on a feature and on an opacity: the summed triples differentiate <G, map>."""
    S = fr.scene(dr.SCENES[1])
    R = fr.reference(dr.SCENES[1])
    C = 5
    F, G = R.F[:, :C].astype(np.float64), R.G[:C].astype(np.float64)
    g = fr.trick_backward(fr.trick_forward(S, F, "f64"), G, "f64")
    i = int(np.abs(g["dL_dfeatures"]).max(axis=1).argmax())
    for c in (0, 4):
        vals = []
        for h in (1e-4, -1e-4):
            Fp = F.copy(); Fp[i, c] += h
            vals.append(float((G * fr.trick_forward(S, Fp, "f64")["map"]).sum()))
        fd = (vals[0] - vals[1]) / 2e-4
        assert abs(fd - g["dL_dfeatures"][i, c]) <= 1e-6 * max(abs(fd), np.abs(g["dL_dfeatures"][i]).max()), (c, fd, g["dL_dfeatures"][i])
    import dataclasses
    vals = []
    for h in (1e-5, -1e-5):
        op = np.array(S.opacities, np.float64); op.reshape(-1)[i] += h
        vals.append(float((G * fr.trick_forward(dataclasses.replace(S, opacities=op), F, "f64")["map"]).sum()))
    fd = (vals[0] - vals[1]) / 2e-5
    assert abs(fd - g["dL_dopacity"].reshape(-1)[i]) <= 1e-4 * max(abs(fd), np.abs(g["dL_dopacity"]).max())


# a scene dense enough that pixels stop (T < 1e-4) in front of the end of their lists
DENSE = (4000, 32, 32, 0.2, 7)


@pytest.mark.parametrize("fault", ["background", "normalised", "missed_last"])
def test_planted_faults_are_told_from_the_correct_result(fault):
    cfg = DENSE if fault == "missed_last" else dr.SCENES[2]        # (a background term and a division by alpha show where alpha is far from 1)
    S = fr.scene(cfg)
    R = fr.reference(cfg)
    C = 4
    F = R.F[:, :C]
    t = fr.trick_forward(S, F)
    step = 3
    ys, xs = np.arange(0, S.H, step), np.arange(0, S.W, step)
    sub = lambda a: a[:, ys][:, :, xs]
    M0 = fr.feature_pixels(S, F, step=step)
    assert np.abs(sub(M0) - sub(t["map"])).max() <= 1e-6 * t["fmax"]
    M = fr.feature_pixels(S, F, fault=fault, step=step)
    d = np.abs(sub(M) - sub(t["map"])).max(axis=0) / t["fmax"]
    over = int((d > RGB_ATOL).sum())
    print(fault, "pixels over", RGB_ATOL, ":", over, "of", d.size, "max", d.max())
    # the check the GPU test applies (RGB_ATOL on map / fmax) must see the fault on far more than a handful of pixels
    assert over > 10, (fault, over)


CASES = [(cfg, False, C) for cfg in fr.CONFIGS for C in fr.SCENE_CHANNELS] + [(dr.SCENES[2], True, C) for C in fr.SCENE_CHANNELS] + \
        [(dr.SCENES[3], False, 64)]


@pytest.mark.parametrize("cfg,cov,C", CASES, ids=[f"{fr.IDS[fr.CONFIGS.index(c)]}{'-cov' if v else ''}-C{n}" for c, v, n in CASES])
def test_every_gpu_scene_certifies_itself(cfg, cov, C):
    """The reference alone: the float64 oracle's map in the place of a device's against the float32 oracle's, triple by triple, within
    the cap; the float32 oracle's summed gradients in the place of a device's inside assert_parity's gates."""
    R = fr.reference(cfg, cov)
    o = R.of(C)
    f64map = np.concatenate([np.asarray(t["f64"]["color"], np.float64)[:hi - lo] for lo, hi, t in o["triples"]]) * o["fmax"]
    grads = {hk: o["g32"][rk] for hk, rk in fr.GRAD_NAMES}
    counts = fr.check_against(R, C, f64map, grads)
    rows = int((R.radii > 0).sum())
    if rows * F32_FAIL_FRAC_MAX < 1:           # one row beyond GRAD_RTOL would be more than the gates' failing fraction: none may come near
        for hk, rk in fr.GRAD_NAMES:
            if S_has(R.S, hk):
                st = grad_rows(o["g32"][rk].reshape(len(R.radii), -1), o["g64"][rk].reshape(len(R.radii), -1))
                assert st["max"] <= GRAD_RTOL / 2, (hk, st)
    print(cfg, cov, C, "pixels over / uncertified per triple:", counts)


def S_has(S, name):
    """Whether a render of S gives the input `name` a gradient (the oracle fills dL_dcov3D either way)."""
    return name != "cov3D_precomp" or S.cov3D_precomp is not None


def test_the_channel_edge_scene_certifies_itself_at_every_channel_count():
    R = fr.reference(dr.SCENES[1])
    total = [0, 0]
    P = len(R.radii)
    for C in fr.EDGE_CHANNELS:
        o = R.of(C)
        # 63 gradient rows: p99 is the worst row.  The reference's own float32 evaluation uses at most half of the gate a device is held
        # to against it, the other half is left to a device's different rounding (features_ref.map_grad)
        for hk, rk in fr.GRAD_NAMES:
            if S_has(R.S, hk):
                st = grad_rows(o["g32"][rk].reshape(P, -1), o["g64"][rk].reshape(P, -1))
                assert st["p99"] <= F32_P99_MAX / 2, (C, hk, st)
        f64map = np.concatenate([np.asarray(t["f64"]["color"], np.float64)[:hi - lo] for lo, hi, t in o["triples"]]) * o["fmax"]
        for over, unc in fr.check_against(R, C, f64map, {hk: o["g32"][rk] for hk, rk in fr.GRAD_NAMES}):
            total[0] += over; total[1] += unc
    print("pixels over / uncertified, all channel counts:", total)
