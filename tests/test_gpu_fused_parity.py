"""-m gpu: the fused raw-parameter path (opacity logits, log-scales, un-normalised quaternions, features_dc / features_rest; the RAW /
SPLIT instantiations of preprocess_fwd_kernel, pergauss_bwd_kernel and pergauss_bwd_dense_kernel) against the float64 oracle with the
activations and their Jacobians restated in float64 (tests/fused_ref.py), under the per-Gaussian row bars of helpers.assert_parity;
the instantiations no public entry point reaches, bit for bit against the ones that are; the edges of the activations."""
import dataclasses

import numpy as np
import pytest
import torch

from tests import fused_ref as fr
from tests.helpers import assert_parity, grad_err

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


def _t(a, grad=False):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV).requires_grad_(grad)


def _settings(raw):
    from gaussian_transformer_amd.rasterizer import GaussianRasterizationSettings
    sc, cam = raw.sc, raw.sc.camera
    return GaussianRasterizationSettings(cam.image_height, cam.image_width, cam.tanfovx, cam.tanfovy, _t(sc.bg), raw.scale_modifier,
                                         _t(cam.world_view_transform), _t(cam.full_proj_transform), sc.sh_degree, _t(cam.camera_center),
                                         False, False)


def _hip_fused(raw, dL, arena=None):
    """rasterize_gaussians_fused, called directly; gradients keyed by fused_ref.RAW_KEYS."""
    from gaussian_transformer_amd.rasterizer import gradient_arena, rasterize_gaussians_fused
    sc, P = raw.sc, raw.P
    p = dict(means3D=_t(sc.means3D, True), f_dc=_t(sc.shs[:, :1], True), f_rest=_t(sc.shs[:, 1:], True), opacity=_t(raw.logits, True),
             scaling=_t(raw.log_scales, True), rotation=_t(raw.quats, True))
    m2 = torch.zeros((P, 3), dtype=torch.float32, device=DEV, requires_grad=True)
    color, radii = rasterize_gaussians_fused(p["means3D"], m2, p["f_dc"], p["f_rest"], p["opacity"], p["scaling"], p["rotation"], _settings(raw))
    if arena is not None:
        with gradient_arena(arena):
            color.backward(_t(dL))
    else:
        color.backward(_t(dL))
    g = {k: v.grad.cpu().numpy() for k, v in p.items()}
    g["means2D"] = m2.grad.cpu().numpy()
    return dict(color=color.detach().cpu().numpy(), radii=radii.cpu().numpy(), grads=g)


def _backend_run(raw, dL, shs, split, raw_params, aligned=True):
    """HipBackend.forward / backward with shs_rest and raw_params set independently (what the C ABI offers and no autograd entry
    point combines freely); backward writes into a gradient arena pre-filled with NaN, so an element nobody wrote shows.
    The SH gradient sits 3 P floats into the arena; the LDS tile for its rows and the dense per-Gaussian stage both need it 16-byte
    aligned (as separately allocated outputs are), so the arena starts (-3 P) mod 4 floats into its allocation -- or, `aligned` =
    False, one float further.  `path`: the library's "pergauss_path" after the call (bit 0 dense kernel, bit 1 LDS tile)."""
    from gaussian_transformer_amd import _lib
    from gaussian_transformer_amd.rasterizer import arena_floats, get_backend, gradient_arena
    be = get_backend()
    rs = _settings(raw)
    P, M = int(shs.shape[0]), int(shs.shape[1])
    e = torch.empty(0, device=DEV)
    means = _t(raw.sc.means3D)
    if raw_params:
        opac, scales, rots = _t(raw.logits), _t(raw.log_scales), _t(raw.quats)
    else:
        o, s, qh, _ = fr.activate(raw.logits, raw.log_scales, raw.quats)
        opac, scales, rots = _t(o.reshape(P, 1)), _t(s), _t(qh)
    sh = _t(shs)
    a_sh, rest = (sh[:, :1].contiguous(), sh[:, 1:].contiguous()) if split else (sh, None)
    n, color, radii, geom, binning, img = be.forward(rs, means, a_sh, e, opac, scales, rots, e, shs_rest=rest, raw_params=raw_params)
    pad = (-3 * P) % 4 + (0 if aligned else 1)
    store = torch.full((arena_floats(P, M) + 8,), NAN, device=DEV)
    assert store.data_ptr() % 16 == 0
    flat = store[pad:pad + arena_floats(P, M)]
    with gradient_arena(flat):
        g = be.backward(rs, n, _t(dL), means, radii, a_sh, e, scales, rots, e, geom, binning, img, shs_rest=rest, raw_params=raw_params)
    torch.cuda.synchronize()
    path = _lib.get_option("pergauss_path")
    assert not bool(torch.isnan(flat).any()), "an element of the gradient arena was never written"
    assert bool(torch.isnan(store[:pad]).all()) and bool(torch.isnan(store[pad + flat.numel():]).all()), "written outside the arena"
    assert (g[2].data_ptr() % 16 == 0) == aligned
    for x in (g[0], g[2], g[4], g[5], g[6]):
        assert flat.data_ptr() <= x.data_ptr() < flat.data_ptr() + 4 * flat.numel()
    g_sh = torch.cat([g[2], g[8]], dim=1) if split else g[2]
    assert g_sh.shape == (P, M, 3)
    grads = dict(means3D=g[0], means2D=g[1], sh=g_sh, opacity=g[4], scaling=g[5], rotation=g[6])
    return dict(n=n, path=path, color=color.cpu().numpy(), radii=radii.cpu().numpy(), grads={k: v.cpu().numpy() for k, v in grads.items()})


def _raw_keys(h):
    """A _backend_run result in the shape fused_parity_report takes."""
    g = dict(h["grads"])
    sh = g.pop("sh")
    return dict(color=h["color"], radii=h["radii"], grads=dict(g, f_dc=sh[:, :1], f_rest=sh[:, 1:]))


def _assert_bit_equal(a, b, what):
    assert a["n"] == b["n"] and a["n"] > 0, what
    assert np.array_equal(a["color"], b["color"]), (what, "image")
    assert np.array_equal(a["radii"], b["radii"]), (what, "radii")
    for k, v in a["grads"].items():
        assert np.array_equal(v, b["grads"][k]), (what, k, float(np.abs(v - b["grads"][k]).max()))
    assert max(float(np.abs(v).max()) for k, v in a["grads"].items() if k != "means2D") > 0


def _print_table(tag, rep):
    print(f"\n[{tag}] radii: hip != f64 in {rep['radii']['hip_vs_f64_rows']} rows, f32 != f64 in {rep['radii']['f32_vs_f64_rows']} rows, "
          f"max |diff| {rep['radii']['max_abs']}")
    for k in rep["grads"]:
        g, b = rep["grads"][k], rep["grads_f32_oracle"][k]
        print(f"[{tag}] {k:9s} hip vs f64: fail_frac {g['fail_frac']:.2e} p99 {g['p99']:.2e} | f32 oracle vs f64: fail_frac {b['fail_frac']:.2e} "
              f"p99 {b['p99']:.2e} | hip vs f32: fail_frac {rep['grads_vs_f32'][k]['fail_frac']:.2e} p99 {rep['grads_vs_f32'][k]['p99']:.2e}")


def _check_parity(tag, orc, hip):
    rep = fr.fused_parity_report(orc, hip)
    _print_table(tag, rep)
    assert rep["radii"]["ok"], rep["radii"]
    assert_parity(rep)
    return rep


# ---- A: the public fused path against float64 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("deg,max_deg", [(3, 3), (2, 3), (1, 3), (0, 3), (2, 2), (1, 1)])
def test_fused_path_against_float64(deg, max_deg):
    """rasterize_gaussians_fused (RAW && SPLIT, D = 0..3) on P = 3001 (not a multiple of 64 or 256), 128 x 80, logits U[-6, 8],
    quaternion norms log-uniform in [0.3, 3], scale_modifier 0.9, non-zero background: every gradient under assert_parity's row bars
    against the float64 chain; below the maximum degree the tail of features_rest's gradient is exactly 0."""
    raw = fr.make_raw_scene(P=3001, width=128, height=80, deg=deg, max_deg=max_deg, s0=0.04, seed=51 + deg + 10 * (3 - max_deg))
    dL = fr.seeded_dL(raw, 151 + deg)
    orc = fr.FusedOracles(raw, dL)
    hip = _hip_fused(raw, dL)
    rep = _check_parity(f"A deg={deg} max_deg={max_deg}", orc, hip)
    assert rep["grads"]["f_dc"]["rows"] > 1000 and rep["grads"]["opacity"]["rows"] > 1000
    K = (deg + 1) ** 2
    rest = hip["grads"]["f_rest"]
    assert rest.shape == (raw.P, (max_deg + 1) ** 2 - 1, 3)
    assert np.all(rest[:, K - 1:] == 0), "features_rest gradient beyond the active degree"
    if K > 1:
        assert np.abs(rest[:, :K - 1]).max() > 0
    assert np.all(hip["grads"]["means2D"][:, 2] == 0)


# ---- B: the instantiations nobody reaches ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg,M", [(0, 16), (0, 2), (1, 16), (1, 4), (2, 16), (2, 9), (3, 16)])     # M = 16 and M = (D+1)^2 (>= 2: split)
def test_unreached_instantiations_bit_equal(deg, M):
    """!RAW && SPLIT against the plain path on cat(dc, rest); RAW && !SPLIT against RAW && SPLIT: the same arithmetic (the
    translation units are built with -ffp-contract=off), only the loads and stores differ, so with the deterministic reverse pass
    image, radii and every gradient must agree bit for bit -- and every element of a NaN-filled arena must have been written.
    Unsplit M = 16 rows leave through the LDS tile when dL/dshs is 16-byte aligned and by direct stores when it is not: both run,
    and the library must report which one it took."""
    from gaussian_transformer_amd import _lib
    raw = fr.make_raw_scene(P=1501, width=96, height=64, deg=deg, max_deg=3, s0=0.05, seed=61 + deg)
    shs = raw.sc.shs[:, :M]
    dL = fr.seeded_dL(raw, 161 + deg)
    _lib.set_option("deterministic_bwd", 1)
    try:
        plain = _backend_run(raw, dL, shs, split=False, raw_params=False)
        split = _backend_run(raw, dL, shs, split=True, raw_params=False)
        raw_unsplit = _backend_run(raw, dL, shs, split=False, raw_params=True)
        raw_split = _backend_run(raw, dL, shs, split=True, raw_params=True)
        raw_direct = _backend_run(raw, dL, shs, split=False, raw_params=True, aligned=False) if M == 16 else None
    finally:
        _lib.set_option("deterministic_bwd", 0)
    _assert_bit_equal(split, plain, "!RAW SPLIT vs plain")
    _assert_bit_equal(raw_unsplit, raw_split, "RAW !SPLIT vs RAW SPLIT")
    tile = 2 if M == 16 else 0
    assert (plain["path"], split["path"], raw_unsplit["path"], raw_split["path"]) == (tile, 0, tile, 0)
    if raw_direct is not None:
        assert raw_direct["path"] == 0
        _assert_bit_equal(raw_direct, raw_unsplit, "RAW !SPLIT direct stores vs LDS tile")
    K = (deg + 1) ** 2
    for h in (split, raw_unsplit):
        assert np.all(h["grads"]["sh"][:, K:] == 0)
    # the raw pair did go through the activations: same image up to rounding, another opacity gradient than the activated pair
    assert np.abs(raw_split["color"] - plain["color"]).max() < 1e-3
    assert grad_err(raw_split["grads"]["opacity"], plain["grads"]["opacity"]) > 1e-2


# ---- C: the dense per-Gaussian stage with raw parameters ----------------------------------------------------------------------------
@pytest.mark.parametrize("deg", [3, 1])
def test_dense_per_gaussian_stage_with_raw_parameters(deg):
    """pergauss_bwd_dense_kernel<D, true>: raw, unsplit, M = 16, `dense_pergauss` = 1, on the dense test's scene (P = 20001).  Bit-equal
    to the streaming kernel under the deterministic reverse pass; D = 3 also under assert_parity's bars against float64."""
    from gaussian_transformer_amd import _lib
    raw = fr.make_raw_scene(P=20001, width=250, height=131, deg=deg, max_deg=3, s0=0.05, seed=7)
    dL = fr.seeded_dL(raw, 107)
    _lib.set_option("deterministic_bwd", 1)
    try:
        _lib.set_option("dense_pergauss", 0)
        a = _backend_run(raw, dL, raw.sc.shs, split=False, raw_params=True)
        _lib.set_option("dense_pergauss", 1)
        b = _backend_run(raw, dL, raw.sc.shs, split=False, raw_params=True)
    finally:
        _lib.set_option("deterministic_bwd", 0)
        _lib.set_option("dense_pergauss", 2)
    assert a["path"] == 2, a["path"]                          # streaming kernel, LDS tile
    assert b["path"] == 3, b["path"]                          # the dense kernel did run (no quiet fall-back to the streaming one)
    _assert_bit_equal(b, a, "dense vs streaming, raw")
    if deg == 3:
        _check_parity("C deg=3 dense raw", fr.FusedOracles(raw, dL), _raw_keys(b))


# ---- D: edges of the activations ----------------------------------------------------------------------------------------------------
EDGE = dict(P=2000, width=96, height=64, deg=1, max_deg=1, s0=0.05)


def _without(rep, key):
    return dict(rep, **{n: {k: v for k, v in rep[n].items() if k != key}
                        for n in ("grads", "grads_f32_oracle", "grads_vs_f32", "grads_maxnorm_vs_f32", "grads_maxnorm_where")})


def test_saturated_logits():
    """Logits U[8, 16] plus single rows at +30 and -30.  Once o is rounded to float32, 1 - o carries an absolute error of up to 2^-24
    (half an ulp of o below 1, twice that with the last-place error of expf and the division): relative to 1 - o that is
    2 * 2^-24 / (1 - o64), on top of the 1e-3 of every other row -- derived, not measured.  torch's sigmoid backward has the same
    form, so this loss is documented, not fixed.  The row bound is the issue's; as everywhere in helpers.assert_parity
    it is a bound on rows that a plain float32 evaluation keeps itself: borderline alpha tests and cancelling sums put ~0.2 % of
    the rows of ANY float32 evaluation outside 1e-3 of float64 (the float32 oracle with the float32 Jacobian is measured under
    the same row bound, and the share allowed is assert_parity's 2 * base + 1e-3; on the CPU that model has one row of 1998 over
    the bound, by 1.28x).  The worst row is capped too: twice the float32 model's own worst ratio to the bound."""
    raw = fr.make_raw_scene(seed=71, logits=(8.0, 16.0), **EDGE)
    hi, lo = 5, 11
    raw.logits[hi] = 30.0; raw.logits[lo] = -30.0
    dL = fr.seeded_dL(raw, 171)
    orc = fr.FusedOracles(raw, dL)
    hip = _hip_fused(raw, dL)
    rep = fr.fused_parity_report(orc, hip)
    _print_table("D saturated", rep)
    assert rep["radii"]["ok"], rep["radii"]
    assert_parity(_without(rep, "opacity"))
    for k, v in hip["grads"].items():
        assert np.isfinite(v).all(), k
    got = hip["grads"]["opacity"].astype(np.float64).reshape(-1)
    want = orc.raw64["opacity"].reshape(-1)
    one = orc.o32 == np.float32(1.0)
    assert one[hi] and one.sum() == 1                          # U[8, 16] stays below 16.64, where 1 + exp(-x) first rounds to 1
    assert np.all(got[one] == 0.0)
    assert abs(want[hi]) > 0                                    # ... while the float64 gradient of that row is not 0
    mx = grad_err(got, want)
    print(f"[D saturated] opacity max-norm vs f64 {mx:.3e}")
    assert mx < 1e-3
    # derived row bar, each row relative to its own float64 magnitude (grad_rows' floor: 1e-3 of the median magnitude)
    mag = np.abs(want)
    floor = 1e-3 * float(np.median(mag[mag > 0]))
    bar = 1e-3 + 2.0 * 2.0 ** -24 / (1.0 - orc.o)
    live = (mag > 0) | (got != 0)
    e_hip = np.abs(got - want) / np.maximum(mag, floor)
    e_f32 = np.abs(orc.raw32["opacity"].reshape(-1) - want) / np.maximum(mag, floor)
    fail_hip, fail_f32 = float((e_hip > bar)[live].mean()), float((e_f32 > bar)[live].mean())
    plain_hip = float((e_hip > 1e-3)[live].mean())
    print(f"[D saturated] rows {int(live.sum())}: over the derived bar hip {fail_hip:.2e}, f32 model {fail_f32:.2e}; over plain 1e-3 hip {plain_hip:.2e}, "
          f"p99 hip {np.quantile(e_hip[live], 0.99):.2e}; worst hip e/bar {float((e_hip / bar)[live].max()):.2f}")
    assert live.sum() > 300
    assert fail_hip <= 2.0 * fail_f32 + 1e-3, (fail_hip, fail_f32)
    # no row far over its bar, however small its gradient: at most twice what the float32 model's own worst row shows (or the bar itself)
    worst_hip, worst_f32 = float((e_hip / bar)[live].max()), float((e_f32 / bar)[live].max())
    assert worst_hip <= 2.0 * max(worst_f32, 1.0), (worst_hip, worst_f32)
    # logit -30: opacity 9e-14 never blends -- every gradient of the row exactly 0, radius the oracle's
    for k, v in hip["grads"].items():
        assert np.all(v[lo] == 0), k
    assert orc.f64["radii"][lo] > 0 and hip["radii"][lo] == orc.f64["radii"][lo]


def test_quaternion_norms_over_six_decades_and_zero_quaternions():
    """|q| log-uniform in [1e-3, 1e3]: rotation rows within assert_parity's row bars (which are relative to each row's own magnitude:
    the 1 / |q| factor spans six decades across rows).  Plus four exactly-zero quaternions in view (act_normalize4: q_hat = 0, R = I):
    dL/dq_hat is linear in q_hat, so it is 0 there and the 1e12 Jacobian of the clamp multiplies 0 -- what these rows check is R = I
    (image, radii, the other gradients of the row), finiteness, and a rotation gradient of exactly 0."""
    raw = fr.make_raw_scene(seed=72, qnorm=(1e-3, 1e3), **EDGE)
    zero = np.array([3, 64, 700, 1999])
    raw.quats[zero] = 0.0
    raw.logits[zero] = 2.0                                     # opaque enough to blend
    dL = fr.seeded_dL(raw, 172)
    orc = fr.FusedOracles(raw, dL)
    hip = _hip_fused(raw, dL)
    _check_parity("D quaternion norms", orc, hip)
    assert np.all(hip["radii"][zero] > 0)
    assert np.abs(hip["grads"]["scaling"][zero]).max() > 0     # they do receive gradients ...
    assert np.isfinite(hip["grads"]["rotation"]).all()
    assert np.all(hip["grads"]["rotation"][zero] == 0) and np.all(orc.raw64["rotation"][zero] == 0)
    n = np.linalg.norm(raw.quats.astype(np.float64), axis=1)
    small = (n > 0) & (n < 1e-2)
    assert small.sum() > 50 and np.abs(hip["grads"]["rotation"][small]).max() > 0


def _head(raw, n):
    sc = raw.sc
    sc = dataclasses.replace(sc, means3D=sc.means3D[:n], scales=sc.scales[:n], rotations=sc.rotations[:n], opacities=sc.opacities[:n],
                             shs=sc.shs[:n])
    return fr.RawScene(sc, raw.logits[:n].copy(), raw.log_scales[:n].copy(), raw.quats[:n].copy(), raw.scale_modifier)


@pytest.mark.parametrize("P", [1, 63, 65])
def test_single_partial_wave_and_no_full_wave(P):
    """The first P Gaussians of the edge scene alone: one partial wave (1, 63), one full wave plus one lane (65), under A's bars."""
    raw = _head(fr.make_raw_scene(seed=73, logits=(0.0, 8.0), **EDGE), P)
    dL = fr.seeded_dL(raw, 173)
    orc = fr.FusedOracles(raw, dL)
    hip = _hip_fused(raw, dL)
    rep = _check_parity(f"D P={P}", orc, hip)
    assert rep["grads"]["means3D"]["rows"] >= min(P, 32)        # (almost) every one of them blends somewhere
    for k in fr.RAW_KEYS:
        assert hip["grads"][k].shape[0] == P


def test_every_gaussian_behind_the_camera_raw_path():
    """Nothing in front of the near plane: the image is the background, a NaN-filled arena ends up all zeros, means2D.grad is 0."""
    from gaussian_transformer_amd.rasterizer import arena_floats
    raw = _head(fr.make_raw_scene(seed=74, **EDGE), 300)
    raw.sc.means3D[:, 2] *= -1.0
    dL = fr.seeded_dL(raw, 174)
    arena = torch.full((arena_floats(raw.P, int(raw.sc.shs.shape[1])),), NAN, device=DEV)
    hip = _hip_fused(raw, dL, arena=arena)
    assert np.all(hip["radii"] == 0)
    bg = np.asarray(raw.sc.bg, np.float32)
    assert np.array_equal(hip["color"], np.broadcast_to(bg[:, None, None], hip["color"].shape))
    assert bool((arena == 0).all())
    assert np.all(hip["grads"]["means2D"] == 0)
    for k in fr.RAW_KEYS:
        assert np.all(hip["grads"][k] == 0), k
