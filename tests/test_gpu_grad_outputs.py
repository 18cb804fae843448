"""-m gpu: every route by which gsr_backward keeps its promise that each element of each gradient output is written exactly once --
zeros for the Gaussians the frame culled or never composited -- run on outputs that hold NaN beforehand and sit between NaN guard zones.

Three mechanisms write the zeros (csrc/gsr_api.hip: make_plan, bwd_plan, bwd_dense_setup, bwd_take_prefill, bwd_fork_and_clear):
  streaming  pergauss_bwd_kernel writes them itself (skip_unmarked = 0);
  dense      fill_zero_kernel on the second stream, gather_visible_kernel, pergauss_bwd_dense_kernel ("pergauss_path" bit 0);
  fill       the persistent compositing kernel's fill units (composite_bwd.hip::fill_unit), pergauss_bwd_kernel with skip_unmarked = 1.
The outputs are the test's own: carved from one NaN-filled tensor, at least 64 floats of it left before and after each, and handed to
HipBackend.backward as an announcement the library was never told of (no gsr_backward_prefill), so nothing but gsr_backward itself can
have written them.  The scenes (tests/grad_outputs_ref.py, certified by tests/test_grad_outputs_host.py) hold culled Gaussians,
Gaussians in view that nothing composited, and Gaussians with a gradient.

Routes.  Every route sets every option below; which kernels then run follows from the plan (P < 500 000 everywhere, 2 blocks per wave):
  classic       persistent_bwd 0: make_plan's pk is false and a small image has no lpt_span -> launch_composite_bwd; streaming zeros
  persistent    persistent_bwd 2, image <= 6144 tiles -> Plan::persistent_bwd, R > 0 -> composite_bwd_pk_walk_kernel; fill_chunk 0 -> streaming zeros
  persistent_c  the same with asm_walk 0 -> bwd_asm 0 -> composite_bwd_pk_kernel<0, false> (and the C++ forward walk); streaming zeros
  fill          persistent and fill_in_tail -> fill_chunk 256, skip_unmarked 1 (R > 0); launch_composite_bwd_persistent takes
                composite_bwd_pk_kernel<0, false> because fill.chunk > 0; the fill units write the zeros
  fill_det      the same under deterministic_bwd: composite_bwd_pk_kernel<0, true> + det_reduce_kernel; the fill units write the zeros
  dense_late    dense_pergauss 1, dense_fork 1: bwd_fork after launch_zero_marked_rows; fill_zero_kernel writes the zeros (bit 0 read back)
  dense_early   dense_fork 0: bwd_fork first (bit 0 read back)
  dense_det     dense under deterministic_bwd (bit 0 read back)
  stream_det    dense_pergauss 0 under deterministic_bwd: persistent DET kernel, streaming zeros (bit 0 read back clear)
  lpt           the defaults on > 6144 tiles: not small_image -> not persistent, lpt_span 512, bwd_asm 1, no counters, wpb 1 ->
                composite_bwd_lpt_kernel; streaming zeros
  lpt_fill      the same with fill_in_tail 1: not persistent -> fill_chunk 0, no fill units, skip_unmarked 0 -> streaming zeros
A dense route falls back to the streaming kernel where pergauss_dense_eligible() says no (colours / covariances given, M != 16, dL_dsh
not 16-byte aligned) or R == 0: "pergauss_path" bit 0 must then read clear.  Bit 1 (LDS tile for the dL/dshs rows) is set exactly when
M = 16 SH rows are written to a 16-byte-aligned dL_dsh.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib
from tests import grad_outputs_ref as gr
from tests.helpers import assert_image_close, assert_parity, grad_err, parity_report

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
GUARD = 64

DEFAULTS = dict(persistent_bwd=2, dense_pergauss=2, fill_in_tail=0, deterministic_bwd=0, dense_fork=2, asm_walk=1, bwd_lpt=1,
                bwd_blocks_per_wave=2, fwd_blocks_per_wave=2, composite_waves_per_block=1, segment_entries=256, prefill_at=1)
ROUTES = {
    "classic": dict(persistent_bwd=0, dense_pergauss=0),
    "persistent": dict(persistent_bwd=2, dense_pergauss=0),
    "persistent_c": dict(persistent_bwd=2, dense_pergauss=0, asm_walk=0),
    "fill": dict(persistent_bwd=2, fill_in_tail=1),
    "fill_det": dict(persistent_bwd=2, fill_in_tail=1, deterministic_bwd=1),
    "dense_late": dict(dense_pergauss=1, dense_fork=1),
    "dense_early": dict(dense_pergauss=1, dense_fork=0),
    "dense_det": dict(dense_pergauss=1, deterministic_bwd=1),
    "stream_det": dict(dense_pergauss=0, deterministic_bwd=1),
    "lpt": dict(),
    "lpt_fill": dict(fill_in_tail=1),
}
DENSE = ("dense_late", "dense_early", "dense_det")
API_KEYS = dict(means3D="means3D", means2D="means2D", sh="shs", colors="colors_precomp", opacity="opacities", scales="scales",
                rots="rotations", cov3D="cov3D_precomp")


@contextlib.contextmanager
def options(route):
    """Every option a route depends on, set explicitly; all of them, and the device's adaptive depth map, restored afterwards."""
    kw = dict(DEFAULTS, **ROUTES[route])
    saved = {k: _lib.get_option(k) for k in set(kw) | {"depth_log_map"}}
    try:
        for k, v in kw.items():
            _lib.set_option(k, v)
        yield
    finally:
        for k, v in saved.items():
            _lib.set_option(k, v)


def _t(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def _carve(shapes, offsets):
    """One NaN-filled tensor and a view per entry of `shapes` (name -> shape or None): each view starts offsets.get(name, 0) floats past
    a 16-byte boundary and has at least GUARD floats that belong to no view before and after it.  Returns (store, views, is_output)."""
    spans, at = {}, 0
    for name, shape in shapes.items():
        if shape is None:
            continue
        n = int(np.prod(shape))
        start = (at + GUARD + 3) // 4 * 4 + offsets.get(name, 0)
        spans[name] = (start, n, shape)
        at = start + n
    store = torch.full((at + GUARD + 4,), NAN, dtype=torch.float32, device=DEV)
    assert store.data_ptr() % 16 == 0
    inside = np.zeros(store.numel(), bool)
    views = {}
    for name, (start, n, shape) in spans.items():
        assert not inside[start - GUARD:start + n + GUARD].any()
        inside[start:start + n] = True
        views[name] = store[start:start + n].view(shape)
        assert views[name].data_ptr() % 16 == 4 * offsets.get(name, 0)
    return store, views, inside


@functools.lru_cache(maxsize=None)
def _inputs(name):
    from gaussian_transformer_amd.rasterizer import GaussianRasterizationSettings
    S, dL = gr.scene(name)
    P = int(np.asarray(S.means3D).shape[0])
    e = torch.empty(0, device=DEV)
    opt = lambda a: e if a is None else _t(a)
    rs = GaussianRasterizationSettings(S.H, S.W, S.tanfovx, S.tanfovy, _t(S.bg), S.scale_modifier, _t(np.asarray(S.viewmatrix).reshape(4, 4)),
                                       _t(np.asarray(S.projmatrix).reshape(4, 4)), S.sh_degree, _t(S.campos), False, False)
    args = (_t(np.asarray(S.means3D).reshape(P, 3)), opt(S.shs), opt(S.colors_precomp), _t(np.asarray(S.opacities).reshape(P, 1)), opt(S.scales),
            opt(S.rotations), opt(S.cov3D_precomp))
    return S, P, rs, args, _t(dL)


@functools.lru_cache(maxsize=None)
def run(name, route, off_sh=0, off_others=0):
    """Forward and backward of scene `name` through HipBackend under `route`, the gradient outputs carved from a NaN tensor (dL_dsh
    off_sh floats, every other output off_others floats past a 16-byte boundary).  Asserts (a) no NaN in any output, (b) every guard
    float still NaN, (c) exact zeros in every output for every Gaussian with radii <= 0 or outside composited_mask, (f) the per-Gaussian
    variant the library reports.  Returns color, radii, mask and the gradients (API names) as numpy, and the path bits."""
    from gaussian_transformer_amd.rasterizer import get_backend
    be = get_backend()
    S, P, rs, a, dL = _inputs(name)
    means3D, shs, colors, opac, scales, rots, cov = a
    M = int(shs.shape[1]) if shs.numel() else 0
    has_sr = scales.numel() > 0
    shapes = dict(means3D=(P, 3), means2D=(P, 3), sh=(P, M, 3) if M else None, colors=(P, 3) if colors.numel() else None, opacity=(P, 1),
                  scales=(P, 3) if has_sr else None, rots=(P, 4) if has_sr else None, cov3D=(P, 6) if cov.numel() else None)
    offsets = {k: (off_sh if k == "sh" else off_others) for k in shapes}
    store, v, inside = _carve(shapes, offsets)
    e = torch.empty(0, device=DEV)
    grads = (v["means3D"], v["means2D"], v.get("sh", e), v.get("colors"), v["opacity"], v.get("scales", e), v.get("rots", e), v.get("cov3D"), None)
    dev = means3D.device
    with options(route):
        try:
            n, color, radii, geom, binning, img = be.forward(rs, means3D, shs, colors, opac, scales, rots, cov)
            mask = be.composited_mask(geom, P)
            be._announced[dev.index] = (geom.data_ptr(), P, M, grads, None)      # never announced to the library: it knows nothing of them
            got = be.backward(rs, n, dL, means3D, radii, shs, colors, scales, rots, cov, geom, binning, img)
            path = _lib.get_option("pergauss_path")
            torch.cuda.synchronize()
        finally:
            be._announced.clear()
    for g, w in zip(got, grads[:8]):
        assert (g is None and w is None) or g.data_ptr() == w.data_ptr(), "backward did not write the test's outputs"
    host = store.cpu().numpy()
    nan = np.isnan(host)
    tag = (name, route, off_sh, off_others)
    assert not nan[inside].any(), (tag, "never written", {k: int(np.isnan(x.cpu().numpy()).sum()) for k, x in v.items()})       # (a)
    assert nan[~inside].all(), (tag, "written outside an output", np.nonzero(~nan & ~inside)[0][:8])                              # (b)
    radii_h, mask_h = radii.cpu().numpy(), mask.cpu().numpy().astype(bool)
    out = {API_KEYS[k]: x.cpu().numpy() for k, x in v.items()}
    idle = (radii_h <= 0) | ~mask_h
    for k, x in out.items():
        assert not np.any(x[idle]), (tag, k, "non-zero row of a Gaussian without a gradient")                                      # (c)
    aligned_rows = M == 16 and off_sh == 0
    dense = route in DENSE and aligned_rows and has_sr and n > 0
    assert path == (1 if dense else 0) | (2 if aligned_rows else 0), (tag, path)                                                   # (f)
    return dict(n=n, path=path, color=color.cpu().numpy(), radii=radii_h, mask=mask_h, grads=out)


def check(name, route, off_sh=0, off_others=0):
    """run() and (d) every row with a float32-oracle gradient lies in the composited mask, (e) image and gradients under
    helpers.assert_parity against the float32 and float64 oracles of the scene."""
    h = run(name, route, off_sh, off_others)
    S, dL = gr.scene(name)
    orc = gr.oracles(name)
    has = gr.rows_with_gradient(orc[1])
    assert not (has & ~h["mask"]).any(), (name, route, "a Gaussian with a gradient outside composited_mask")
    assert_parity(parity_report(S, dL, hip=h, oracles=orc))
    return h


SMALL_ROUTES = [r for r in ROUTES if not r.startswith("lpt")]
THREE = ("persistent", "fill", "dense_late")


@pytest.mark.parametrize("route", SMALL_ROUTES)
def test_every_small_image_route_on_the_main_scene(route):
    """P = 1501, 250 x 131, M = 16: 374 culled, 706 in view without a gradient, 421 with one."""
    h = check("main", route)
    assert h["n"] > 0 and (h["radii"] <= 0).sum() >= 1501 // 16 and ((h["radii"] > 0) & ~h["mask"]).sum() >= 1


@pytest.mark.parametrize("route", ["classic", "persistent", "fill", "dense_late"])
def test_colours_and_covariances_given(route):
    """colors_precomp + cov3D_precomp: the only form in which dL_dcolors and dL_dcov3D exist (fill_unit's colour and covariance stores);
    not the dense variant's layout, so dense_late must report the streaming kernel."""
    h = check("main_cc", route)
    assert h["path"] == 0 and set(h["grads"]) == {"means3D", "means2D", "colors_precomp", "opacities", "cov3D_precomp"}


@pytest.mark.parametrize("route", THREE)
@pytest.mark.parametrize("name", ["m4", "m9", "m16_deg2"])
def test_sh_layouts(name, route):
    """M = 4 and M = 9 (fill_rows' generic branch; never dense, no LDS tile), M = 16 with active degree 2 (the rows' tail is zero)."""
    h = check(name, route)
    if name == "m16_deg2":
        assert not np.any(h["grads"]["shs"][:, 9:]) and np.any(h["grads"]["shs"][:, :9])


@pytest.mark.parametrize("route", THREE)
@pytest.mark.parametrize("name", ["p1", "p63", "p64", "p65", "p257", "p4099"])
def test_edges_of_p(name, route):
    """One Gaussian; one short of, exactly, and one past a wave; one past a fill chunk and a workgroup; 17 chunks with a ragged last."""
    check(name, route)


def test_fill_units_several_per_band_with_a_ragged_last_band():
    """P = 16411: 65 fill chunks of 256 over 32 unit lists -- three per band, two in band 21, none behind it, the last one 27 Gaussians."""
    check("p16411", "fill")


@pytest.mark.parametrize("route", ["dense_late", "fill"])
@pytest.mark.parametrize("off", [1, 2, 3])
def test_outputs_off_the_16_byte_grid(off, route):
    """Every output but dL_dsh starts `off` floats past a 16-byte boundary: still dense-eligible (fill_zero_kernel's head and tail
    stores; the float4 stores of dL_drots land on 4-byte-aligned addresses); fill_unit's dword stores."""
    check("main", route, 0, off)


@pytest.mark.parametrize("route", THREE)
def test_sh_gradient_off_the_16_byte_grid(route):
    """dL_dsh one float past a 16-byte boundary: no dense variant, no LDS tile (path bits 0, asserted in run()), fill_rows' dword branch."""
    assert check("main", route, 1, 0)["path"] == 0


@pytest.mark.parametrize("route", ["fill", "dense_late"])
def test_nothing_rendered(route):
    """R == 0 (every mean 1000 units behind the camera): neither persistent nor dense (both need R > 0), so no fill units and
    skip_unmarked = 0 -- the streaming kernel writes every zero."""
    h = check("r0", route)
    assert h["n"] == 0 and not (h["path"] & 1)        # (composited_mask may still name Gaussians: GeomView::touched is never cleared, and a
                                                     # stale byte of a reused workspace can equal this frame's mark; their rows are zero like the rest)
    for k, x in h["grads"].items():
        assert not np.any(x), k


@pytest.mark.parametrize("route", ["lpt", "lpt_fill"])
def test_large_image(route):
    """1552 x 1040 = 6305 tiles: the length-ordered kernel; fill_in_tail changes nothing there, the streaming kernel writes the zeros."""
    check("large", route)


# ---- route against route -----------------------------------------------------------------------------------------------------------
def test_deterministic_routes_agree_bit_for_bit():
    """stream_det, dense_det and fill_det: all three run composite_bwd_pk_kernel<0, true> (bwd_plan: deterministic_bwd turns bwd_asm off;
    make_plan: no checkpoints under deterministic_bwd, so the forward passes are the same too) and det_reduce_kernel, whose order of
    addition is a function of the scene; the per-Gaussian chain is the same arithmetic in the streaming and the dense kernel
    (-ffp-contract=off).  Only who writes the zeros differs: every gradient tensor must be identical."""
    a = run("main", "stream_det")
    for other in ("dense_det", "fill_det"):
        b = run("main", other)
        assert np.array_equal(a["color"], b["color"])        # (not the masks: a stale byte that equals the frame's mark adds a Gaussian with a zero row)
        for k, x in a["grads"].items():
            assert np.array_equal(x, b["grads"][k]), (other, k, float(np.abs(x - b["grads"][k]).max()))
    assert max(float(np.abs(x).max()) for x in a["grads"].values()) > 0


@pytest.mark.parametrize("route", ["persistent", "persistent_c", "fill", "dense_late", "dense_early"])
def test_atomic_routes_agree_with_the_classic_kernel(route):
    """Float atomics in another order: the bound tests/test_gpu_parity.py uses between its kernels."""
    a, b = run("main", "classic"), run("main", route)
    errs = {k: grad_err(b["grads"][k], x) for k, x in a["grads"].items()}
    print(f"\n[{route} vs classic] " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e <= 2e-4, (route, k, e)


# ---- split SH through the fused entry point -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["persistent", "fill"])
def test_split_sh_through_render_fused(route):
    """render_fused (raw parameters, dL_dsh as dc + rest: fill_rows(sh, 3) and fill_rows(sh_rest, 45)), degree 1 of max 3, into a
    NaN-filled gradient arena with 64 spare floats behind it: every arena float written, none behind it, exact zeros in the rows of
    every Gaussian outside composited_mask, and the gradients of render() through torch's activations, within
    test_fused_raw_parameter_path_matches_activation_graph's bounds (max norm: the scene is one in which no decision of the compositing
    walk lies within reach of the activations' rounding, tests/grad_outputs_ref.py::SPLIT)."""
    from gaussian_transformer_amd.model import GaussianParams
    from gaussian_transformer_amd.rasterizer import arena_floats, composited_mask, gradient_arena
    from gaussian_transformer_amd.render import PipelineParams, TorchCamera, render, render_fused
    sc = gr.planted_synth(*gr.SPLIT)
    P, M = sc.P, sc.shs.shape[1]
    assert M == 16 and sc.sh_degree == 1
    cam = TorchCamera(sc.camera, DEV)
    bg = _t(sc.bg)
    dL = _t(sc.dL_dimage)
    n = arena_floats(P, M)
    store = torch.full((n + GUARD,), NAN, device=DEV)
    out = []
    with options(route):
        for fn in (render, render_fused):
            pc = GaussianParams.from_synthetic(sc, DEV)
            pc._rotation.data *= 1.7
            with gradient_arena(store[:n]) if fn is render_fused else contextlib.nullcontext():
                pkg = fn(cam, pc, PipelineParams(), bg, gr.SPLIT_SCALE_MODIFIER)
                mask = composited_mask(pkg["render"]).cpu().numpy().astype(bool)
                (pkg["render"] * dL).sum().backward()
            torch.cuda.synchronize()
            out.append((pkg["render"].detach().cpu().numpy(), pkg["radii"].cpu().numpy(), pkg["viewspace_points"].grad.cpu().numpy(),
                        [p.grad.cpu().numpy() for p in pc.parameters()], mask))
    host = store.cpu().numpy()
    assert not np.isnan(host[:n]).any(), "an element of the gradient arena was never written"
    assert np.isnan(host[n:]).all(), "written behind the arena"
    (img0, rad0, v0, g0, _), (img1, rad1, v1, g1, mask) = out
    idle = (rad1 <= 0) | ~mask
    assert (rad1 <= 0).sum() >= P // 16 and ((rad1 > 0) & ~mask).sum() >= 1 and mask.sum() >= P // 8
    at = 0
    for name, fl in (("xyz", 3), ("f_dc", 3), ("f_rest", 3 * (M - 1)), ("opacity", 1), ("scaling", 3), ("rotation", 4)):
        rows = host[at:at + P * fl].reshape(P, fl)
        assert not np.any(rows[idle]), (name, "non-zero row of a Gaussian without a gradient")
        assert np.any(rows[~idle]) or name == "f_rest" and M == 1
        at += P * fl
    assert at == n and not np.any(v1[idle])
    np.testing.assert_array_equal(rad0, rad1)
    # where the two renders part: pixels whose colour differs by more than rounding (a discrete decision of the compositing walk taken
    # the other way), and the Gaussian whose screen-space gradient differs most, with its distance from the nearest such pixel
    d = np.abs(img1.astype(np.float64) - img0).max(axis=0)
    ys, xs = np.nonzero(d > 2e-6)
    w = int(np.abs(v1 - v0).max(axis=1).argmax())
    px = (sc.means3D[w, 0] / sc.means3D[w, 2] / sc.camera.tanfovx + 1.0) * 0.5 * sc.camera.image_width - 0.5
    py = (sc.means3D[w, 1] / sc.means3D[w, 2] / sc.camera.tanfovy + 1.0) * 0.5 * sc.camera.image_height - 0.5
    near = float(np.hypot(xs - px, ys - py).min()) if len(ys) else float("inf")
    print(f"\n[split {route}] pixels over 2e-6: {len(ys)} (max {d.max():.3e}) at {list(zip(xs.tolist(), ys.tolist()))[:6]}; viewspace gradient: "
          f"grad_err {grad_err(v1, v0):.3e}, worst Gaussian {w} at pixel ({px:.1f}, {py:.1f}) radius {rad1[w]} scale {sc.scales[w]} opacity "
          f"{sc.opacities[w]}, fused {v1[w]} activation graph {v0[w]}, largest |v| {np.abs(v0).max():.3e}, nearest differing pixel {near:.1f} px; "
          + " ".join(f"{nm} {grad_err(a, b):.2e}" for a, b, nm in zip(g1, g0, ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"))))
    assert_image_close(img1, img0, atol=2e-6, outlier_frac=1e-4, outlier_max=6e-3)
    assert grad_err(v1, v0) < 1e-4
    for a, b, name in zip(g1, g0, ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")):
        assert a.shape == b.shape
        assert grad_err(a, b) < 2e-4, name
