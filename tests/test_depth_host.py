"""include/gsr_depth.h without a device: the header against the ctypes table, the workspace size, every refusal that is decided before
the HIP runtime is asked for anything (return code and the exact text of gsr_last_error(), as tests/test_cabi_refusals_host.py pins
the other headers), and the Python side's routing: depth=None is today's call through _RasterizeGaussians."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib, rasterizer, synth
from gaussian_transformer_amd.render import PipelineParams, render
from tests.oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, WORKSPACE = 0, 1, 4
SENTINEL = "gsr_set_option: unknown option 'sentinel'"
BIG = 1 << 40
A = 1 << 20                        # made-up device addresses, only compared, never followed


def test_header_declares_exactly_what_the_ctypes_stub_binds():
    header = open(os.path.join(ROOT, "include", "gsr_depth.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decls = dict(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", code, flags=re.S))
    assert set(decls) == {"gsr_depth_workspace_bytes", "gsr_depth_forward", "gsr_depth_backward"} == set(_lib.DEPTH_SIGNATURES)
    for name, args in decls.items():
        assert len(_lib.DEPTH_SIGNATURES[name][1]) == len(args.split(",")), name
    others = (_lib.SIGNATURES, _lib.CHAMFER_SIGNATURES, _lib.SEQUENCE_SIGNATURES, _lib.ROWS_SIGNATURES, _lib.DENSITY_SIGNATURES)
    assert not any(set(_lib.DEPTH_SIGNATURES) & set(t) for t in others)
    assert not any(n.startswith("gsr_depth") for n in _lib.SIGNATURES)                    # SIGNATURES stays gsr.h + loss + knn + optim
    assert "#define GSR_ABI_VERSION 2" in open(os.path.join(ROOT, "include", "gsr.h")).read()   # purely additive
    low = header.lower()
    assert "raw_params" in low and "split sh" in low and "deterministic_bwd" in low and "not normalised" in low
    from gaussian_transformer_amd import build
    assert build.SOURCES["depth_maps.hip"] == build.SOURCES["composite_bwd.hip"]
    lib = _lib.load()
    for name in decls:
        assert hasattr(lib, name)
    assert (_lib.DEPTH_EXPECTED, _lib.DEPTH_INVERSE) == (0, 1) == tuple(rasterizer.DEPTH_MODES[k] for k in ("expected", "inverse"))


def test_workspace_bytes_need_no_device():
    """acc_rows(P) = P + P / 32 + 1024 rows (P taken as 1 when 0) of 64 bytes, rounded up to 256, + 80 P bytes rounded up to 256."""
    lib = _lib.load()
    n = C.c_size_t(0)
    up = lambda x: (x + 255) // 256 * 256
    for P, want in ((0, 65792), (1, 66048), (1023, 215040), (1024, 215040), (500000, 73065728)):
        q = max(P, 1)
        assert want == up((q + q // 32 + 1024) * 64) + up(80 * P)
        assert lib.gsr_depth_workspace_bytes(P, C.byref(n)) == OK and n.value == want, P


def fwd(**kw):
    a = dict(P=10, W=32, H=32, R=100, mode=0, geom=A, binning=2 * A, img=3 * A, depth=4 * A, alpha=5 * A)
    a.update(kw)
    return lambda L: L.gsr_depth_forward(None, a["P"], a["W"], a["H"], a["R"], a["mode"], a["geom"], BIG, a["binning"], BIG, a["img"], BIG,
                                         a["depth"], a["alpha"])


def bwd(**kw):
    a = dict(P=10, W=32, H=32, R=100, mode=0, means3D=A, radii=2 * A, scales=3 * A, rots=4 * A, cov=None, view=5 * A, proj=6 * A, campos=7 * A,
             gD=8 * A, gA=9 * A, geom=10 * A, binning=11 * A, img=12 * A, ws=13 * A, n=BIG, acc=0, g2=14 * A, gop=15 * A, g3=16 * A, gcov=None,
             gsc=17 * A, grot=18 * A)
    a.update(kw)
    return lambda L: L.gsr_depth_backward(None, a["P"], a["W"], a["H"], a["R"], a["mode"], a["means3D"], a["radii"], a["scales"], 1.0, a["rots"],
                                          a["cov"], a["view"], a["proj"], a["campos"], 0.5, 0.5, a["gD"], a["gA"], a["geom"], BIG, a["binning"], BIG,
                                          a["img"], BIG, a["ws"], a["n"], a["acc"], a["g2"], a["gop"], a["g3"], a["gcov"], a["gsc"], a["grot"])


F, B = "gsr_depth_forward: ", "gsr_depth_backward: "
B_MISSING = B + "missing input, workspace or gradient buffer"
B_COV = B + "exactly one of (scales, rotations) / cov3D_precomp must be given"
B_OUT = B + "dL_dcov3D required with cov3D_precomp, dL_dscales and dL_drots with scales and rotations"
TOO_WIDE = 65535 * 16 + 1
COV = dict(scales=None, rots=None, cov=19 * A, gcov=20 * A)

CASES = [
    (lambda L: L.gsr_depth_workspace_bytes(-1, C.byref(C.c_size_t())), INVALID, "gsr_depth_workspace_bytes: bad argument"),
    (lambda L: L.gsr_depth_workspace_bytes(10, None), INVALID, "gsr_depth_workspace_bytes: bad argument"),
    (fwd(P=-1), INVALID, F + "bad sizes"),
    (fwd(W=0), INVALID, F + "bad sizes"),
    (fwd(H=-3), INVALID, F + "bad sizes"),
    (fwd(R=-1), INVALID, F + "bad sizes"),
    (fwd(W=TOO_WIDE), INVALID, "image too large"),
    (fwd(mode=2), INVALID, F + "mode 2 is neither 0 (expected depth) nor 1 (inverse depth)"),
    (fwd(mode=-1), INVALID, F + "mode -1 is neither 0 (expected depth) nor 1 (inverse depth)"),
    (fwd(depth=None, alpha=None, geom=None), OK, SENTINEL),                                # no output asked for: nothing to do
    (fwd(geom=None), INVALID, F + "missing workspace"),
    (fwd(binning=None), INVALID, F + "missing workspace"),
    (fwd(img=None), INVALID, F + "missing workspace"),
    (bwd(P=-1), INVALID, B + "bad sizes"),
    (bwd(H=0), INVALID, B + "bad sizes"),
    (bwd(R=-5), INVALID, B + "bad sizes"),
    (bwd(H=TOO_WIDE), INVALID, "image too large"),
    (bwd(mode=7), INVALID, B + "mode 7 is neither 0 (expected depth) nor 1 (inverse depth)"),
    (bwd(gD=None, gA=None), INVALID, B + "dL_ddepth and dL_dalpha are both NULL"),
    (bwd(P=0, means3D=None, geom=None, ws=None, g2=None), OK, SENTINEL),                   # P = 0: nothing else is looked at
    (bwd(P=0, gD=None, gA=None), INVALID, B + "dL_ddepth and dL_dalpha are both NULL"),    # ... but the checks in front of it hold
    (bwd(means3D=None), INVALID, B_MISSING),
    (bwd(radii=None), INVALID, B_MISSING),
    (bwd(view=None), INVALID, B_MISSING),
    (bwd(proj=None), INVALID, B_MISSING),
    (bwd(geom=None), INVALID, B_MISSING),
    (bwd(img=None), INVALID, B_MISSING),
    (bwd(ws=None), INVALID, B_MISSING),
    (bwd(g2=None), INVALID, B_MISSING),
    (bwd(gop=None), INVALID, B_MISSING),
    (bwd(g3=None), INVALID, B_MISSING),
    (bwd(cov=19 * A, gcov=20 * A), INVALID, B_COV),
    (bwd(scales=None, rots=None), INVALID, B_COV),
    (bwd(rots=None), INVALID, B_COV),
    (bwd(scales=None, cov=19 * A, gcov=20 * A), INVALID, B_COV),
    (bwd(gsc=None), INVALID, B_OUT),
    (bwd(grot=None), INVALID, B_OUT),
    (bwd(**{**COV, "gcov": None}), INVALID, B_OUT),
    (bwd(binning=None), INVALID, B + "binning workspace missing"),
    (bwd(n=67327), WORKSPACE, "depth workspace 67327 < 67328"),
    (bwd(n=0, **COV), WORKSPACE, "depth workspace 0 < 67328"),
    (bwd(gA=None, n=100), WORKSPACE, "depth workspace 100 < 67328"),
    # two checks broken at once: the earlier one answers
    (bwd(P=-1, mode=5), INVALID, B + "bad sizes"),
    (bwd(mode=5, gD=None, gA=None), INVALID, B + "mode 5 is neither 0 (expected depth) nor 1 (inverse depth)"),
    (bwd(means3D=None, rots=None), INVALID, B_MISSING),
    (bwd(rots=None, n=0), INVALID, B_COV),
    (bwd(binning=None, n=0), INVALID, B + "binning workspace missing"),
]


@pytest.mark.parametrize("k", range(len(CASES)), ids=[f"{k:02d}-{'ok' if c[1] == OK else c[2][:48]}" for k, c in enumerate(CASES)])
def test_return_code_and_message(k):
    call, rc, text = CASES[k]
    lib = _lib.load()
    assert lib.gsr_set_option(b"sentinel", 0) == INVALID and lib.gsr_last_error().decode() == SENTINEL
    got = call(lib)
    assert (got, lib.gsr_last_error().decode()) == (rc, text)


def test_deterministic_bwd_is_refused_with_a_text_that_says_so():
    lib = _lib.load()
    assert _lib.get_option("deterministic_bwd") == 0
    try:
        _lib.set_option("deterministic_bwd", 1)
        for call in (bwd(), bwd(n=0), bwd(acc=1, **COV)):                                  # before the workspace is even measured
            assert call(lib) == INVALID
            msg = lib.gsr_last_error().decode()
            assert msg.startswith(B + "not available while the option deterministic_bwd is on") and "float atomics" in msg and "no slot form" in msg
        assert fwd(geom=None)(lib) == INVALID and lib.gsr_last_error().decode() == F + "missing workspace"   # the forward walk does not care
    finally:
        _lib.set_option("deterministic_bwd", 0)
    assert bwd(n=0)(lib) == WORKSPACE


# ---- Python side ----
def _inputs(P=50, W=32, H=32):
    sc = synth.make_scene(P=P, width=W, height=H, sh_degree=1, s0=0.1, seed=3)
    cam = sc.camera
    t = lambda a: torch.tensor(np.asarray(a, np.float32))
    rs = rasterizer.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=t(sc.bg), scale_modifier=1.0,
        viewmatrix=t(cam.world_view_transform), projmatrix=t(cam.full_proj_transform), sh_degree=1, campos=t(cam.camera_center),
        prefiltered=False, debug=False)
    kw = dict(means3D=t(sc.means3D).requires_grad_(True), means2D=torch.zeros(P, 3, requires_grad=True), opacities=t(sc.opacities).reshape(P, 1),
              shs=t(sc.shs), scales=t(sc.scales), rotations=t(sc.rotations))
    return rs, kw


def test_depth_none_is_todays_call_through_rasterize_gaussians(monkeypatch):
    rs, kw = _inputs()
    seen = []
    real = rasterizer._RasterizeGaussians.apply

    def spy(*a):
        seen.append(len(a))
        return real(*a)
    monkeypatch.setattr(rasterizer._RasterizeGaussians, "apply", staticmethod(spy))
    monkeypatch.setattr(rasterizer._RasterizeGaussiansDepth, "apply", staticmethod(lambda *a: pytest.fail("the depth function was reached")))
    prev = rasterizer._set_backend_for_tests(OracleBackend())
    try:
        out = rasterizer.GaussianRasterizer(rs)(**kw)
        out_kw = rasterizer.GaussianRasterizer(rs)(depth=None, **kw)
        out[0].sum().backward()                                                        # and its backward is the plain one
    finally:
        rasterizer._set_backend_for_tests(prev)
    assert seen == [9, 9] and len(out) == 2 and len(out_kw) == 2
    assert torch.equal(out[0], out_kw[0]) and torch.equal(out[1], out_kw[1])
    assert kw["means3D"].grad is not None and out[0].grad_fn.__class__.__name__.startswith("_RasterizeGaussiansBackward")


def test_depth_keyword_is_validated_and_needs_a_backend_that_has_the_maps():
    rs, kw = _inputs()
    with pytest.raises(_lib.GsrError, match="depth must be None, 'expected' or 'inverse', got 'median'"):
        rasterizer.GaussianRasterizer(rs)(depth="median", **kw)
    prev = rasterizer._set_backend_for_tests(OracleBackend())
    try:
        with pytest.raises(_lib.GsrError, match="renders no depth or alpha map"):      # no quiet fall-back to two renders
            rasterizer.GaussianRasterizer(rs)(depth="expected", **kw)
    finally:
        rasterizer._set_backend_for_tests(prev)


def test_render_adds_the_maps_only_when_asked(monkeypatch):
    """render(depth=...) passes the keyword on and adds "depth" and "alpha"; without it the dict is the reference's."""
    calls = []

    class FakeRasterizer:
        def __init__(self, raster_settings):
            pass

        def __call__(self, **kw):
            calls.append(kw.get("depth", "absent"))
            P = kw["means3D"].shape[0]
            base = (torch.zeros(3, 4, 4), torch.ones(P, dtype=torch.int32))
            return base + (torch.zeros(1, 4, 4), torch.ones(1, 4, 4)) if kw.get("depth") else base
    from gaussian_transformer_amd import render as render_mod
    monkeypatch.setattr(render_mod, "GaussianRasterizer", FakeRasterizer)

    class PC:
        get_xyz = torch.zeros(5, 3); get_opacity = torch.zeros(5, 1); get_scaling = torch.ones(5, 3); get_rotation = torch.zeros(5, 4)
        get_features = torch.zeros(5, 4, 3); active_sh_degree = 1; max_sh_degree = 1

    class Cam:
        image_height = image_width = 4; FoVx = FoVy = 1.0
        world_view_transform = full_proj_transform = torch.eye(4); camera_center = torch.zeros(3)
    plain = render(Cam(), PC(), PipelineParams(), torch.zeros(3))
    assert set(plain) == {"render", "viewspace_points", "visibility_filter", "radii"}
    maps = render(Cam(), PC(), PipelineParams(), torch.zeros(3), depth="inverse")
    assert set(maps) == set(plain) | {"depth", "alpha"} and maps["depth"].shape == (1, 4, 4)
    assert calls == ["absent", "inverse"]
