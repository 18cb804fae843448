"""include/gsr_features.h without a device: the header against the ctypes table, the build flags, the workspace formula, every refusal
that is decided before the HIP runtime is asked for anything (return code and the exact text of gsr_last_error()), and the Python side's
glue through stand-in backends: the texts of the stated limits and the shape of the returned tuple."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib, build, rasterizer, synth
from gaussian_transformer_amd.render import PipelineParams, render, render_fused
from gaussian_transformer_amd.rows import render_rows
from tests.oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, WORKSPACE = 0, 1, 4
SENTINEL = "gsr_set_option: unknown option 'sentinel'"
BIG = 1 << 40
A = 1 << 20                        # made-up device addresses, only compared, never followed
NAMES = {"gsr_features_workspace_bytes", "gsr_features_forward", "gsr_features_backward"}


def test_header_declares_exactly_what_the_ctypes_stub_binds():
    header = open(os.path.join(ROOT, "include", "gsr_features.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decls = dict(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", code, flags=re.S))
    assert set(decls) == NAMES == set(_lib.FEATURES_SIGNATURES)
    for name, args in decls.items():
        assert len(_lib.FEATURES_SIGNATURES[name][1]) == len(args.split(",")), name
    others = (_lib.SIGNATURES, _lib.CHAMFER_SIGNATURES, _lib.SEQUENCE_SIGNATURES, _lib.ROWS_SIGNATURES, _lib.DENSITY_SIGNATURES,
              _lib.DEPTH_SIGNATURES, _lib.POSE_SIGNATURES)
    assert not any(NAMES & set(t) for t in others)
    assert "#define GSR_ABI_VERSION 2" in open(os.path.join(ROOT, "include", "gsr.h")).read()   # purely additive
    assert f"#define GSR_FEATURES_MAX_C {_lib.FEATURES_MAX_C}" in header and _lib.FEATURES_MAX_C == 64
    low = header.lower()
    assert "raw_params" in low and "split sh" in low and "deterministic_bwd" in low and "not normalised" in low
    assert build.SOURCES["feature_maps.hip"] == build.SOURCES["composite_bwd.hip"]
    lib = _lib.load()
    for name in decls:
        assert hasattr(lib, name)


@pytest.mark.parametrize("Cn", [1, 3, 64])
@pytest.mark.parametrize("P", [0, 1, 31, 32, 33, 4000])
def test_workspace_formula(P, Cn):
    """gsr_depth_workspace_bytes(P) + acc_rows(P) rows of 4 C bytes, rounded up to 256; acc_rows(P) = P + P / 32 + 1024, P taken as 1 when 0."""
    lib = _lib.load()
    n, d = C.c_size_t(0), C.c_size_t(0)
    up = lambda x: (x + 255) // 256 * 256
    q = max(P, 1)
    rows = q + q // 32 + 1024
    assert lib.gsr_depth_workspace_bytes(P, C.byref(d)) == OK and d.value == up(rows * 64) + up(80 * P)
    assert lib.gsr_features_workspace_bytes(P, Cn, C.byref(n)) == OK and n.value == d.value + up(rows * 4 * Cn), (P, Cn)


def fwd(**kw):
    a = dict(P=10, C=4, W=32, H=32, R=100, feat=6 * A, geom=A, binning=2 * A, img=3 * A, out=4 * A)
    a.update(kw)
    return lambda L: L.gsr_features_forward(None, a["P"], a["C"], a["W"], a["H"], a["R"], a["feat"], a["geom"], BIG, a["binning"], BIG, a["img"], BIG,
                                            a["out"])


def bwd(**kw):
    a = dict(P=10, C=4, W=32, H=32, R=100, means3D=A, radii=2 * A, scales=3 * A, rots=4 * A, cov=None, view=5 * A, proj=6 * A, campos=7 * A,
             feat=8 * A, gF=9 * A, geom=10 * A, binning=11 * A, img=12 * A, ws=13 * A, n=BIG, acc=0, g2=14 * A, gop=15 * A, g3=16 * A, gcov=None,
             gsc=17 * A, grot=18 * A, gfeat=21 * A)
    a.update(kw)
    return lambda L: L.gsr_features_backward(None, a["P"], a["C"], a["W"], a["H"], a["R"], a["means3D"], a["radii"], a["scales"], 1.0, a["rots"],
                                             a["cov"], a["view"], a["proj"], a["campos"], 0.5, 0.5, a["feat"], a["gF"], a["geom"], BIG, a["binning"],
                                             BIG, a["img"], BIG, a["ws"], a["n"], a["acc"], a["g2"], a["gop"], a["g3"], a["gcov"], a["gsc"],
                                             a["grot"], a["gfeat"])


W_, F, B = "gsr_features_workspace_bytes: bad argument", "gsr_features_forward: ", "gsr_features_backward: "
B_MISSING = B + "missing input, workspace or gradient buffer"
B_COV = B + "exactly one of (scales, rotations) / cov3D_precomp must be given"
B_OUT = B + "dL_dcov3D required with cov3D_precomp, dL_dscales and dL_drots with scales and rotations"
TOO_WIDE = 65535 * 16 + 1
COV = dict(scales=None, rots=None, cov=19 * A, gcov=20 * A)
WS10 = 67328 + (1034 * 16 + 255) // 256 * 256                      # P = 10, C = 4: the depth workspace + 1034 rows of 16 bytes, rounded up

CASES = [
    (lambda L: L.gsr_features_workspace_bytes(-1, 4, C.byref(C.c_size_t())), INVALID, W_),
    (lambda L: L.gsr_features_workspace_bytes(10, 0, C.byref(C.c_size_t())), INVALID, W_),
    (lambda L: L.gsr_features_workspace_bytes(10, 65, C.byref(C.c_size_t())), INVALID, W_),
    (lambda L: L.gsr_features_workspace_bytes(10, 4, None), INVALID, W_),
    (fwd(P=-1), INVALID, F + "bad sizes"),
    (fwd(W=0), INVALID, F + "bad sizes"),
    (fwd(H=-3), INVALID, F + "bad sizes"),
    (fwd(R=-1), INVALID, F + "bad sizes"),
    (fwd(W=TOO_WIDE), INVALID, "image too large"),
    (fwd(C=0), INVALID, F + "C = 0 channels, must be 1 .. 64"),
    (fwd(C=65), INVALID, F + "C = 65 channels, must be 1 .. 64"),
    (fwd(C=-2), INVALID, F + "C = -2 channels, must be 1 .. 64"),
    (fwd(out=None), INVALID, F + "out is NULL"),
    (fwd(feat=None), INVALID, F + "missing features or workspace"),
    (fwd(geom=None), INVALID, F + "missing features or workspace"),
    (fwd(binning=None), INVALID, F + "missing features or workspace"),
    (fwd(img=None), INVALID, F + "missing features or workspace"),
    (bwd(P=-1), INVALID, B + "bad sizes"),
    (bwd(H=0), INVALID, B + "bad sizes"),
    (bwd(R=-5), INVALID, B + "bad sizes"),
    (bwd(H=TOO_WIDE), INVALID, "image too large"),
    (bwd(C=0), INVALID, B + "C = 0 channels, must be 1 .. 64"),
    (bwd(C=65), INVALID, B + "C = 65 channels, must be 1 .. 64"),
    (bwd(gF=None), INVALID, B + "dL_dout is NULL"),
    (bwd(P=0, means3D=None, geom=None, ws=None, g2=None, feat=None, gfeat=None), OK, SENTINEL),     # P = 0: nothing else is looked at
    (bwd(P=0, gF=None), INVALID, B + "dL_dout is NULL"),                                            # ... but the checks in front of it hold
    (bwd(means3D=None), INVALID, B_MISSING),
    (bwd(radii=None), INVALID, B_MISSING),
    (bwd(view=None), INVALID, B_MISSING),
    (bwd(proj=None), INVALID, B_MISSING),
    (bwd(feat=None), INVALID, B_MISSING),
    (bwd(geom=None), INVALID, B_MISSING),
    (bwd(img=None), INVALID, B_MISSING),
    (bwd(ws=None), INVALID, B_MISSING),
    (bwd(g2=None), INVALID, B_MISSING),
    (bwd(gop=None), INVALID, B_MISSING),
    (bwd(g3=None), INVALID, B_MISSING),
    (bwd(cov=19 * A, gcov=20 * A), INVALID, B_COV),                                                 # both forms
    (bwd(scales=None, rots=None), INVALID, B_COV),                                                  # neither
    (bwd(rots=None), INVALID, B_COV),
    (bwd(scales=None, cov=19 * A, gcov=20 * A), INVALID, B_COV),
    (bwd(gsc=None), INVALID, B_OUT),
    (bwd(grot=None), INVALID, B_OUT),
    (bwd(**{**COV, "gcov": None}), INVALID, B_OUT),
    (bwd(binning=None), INVALID, B + "binning workspace missing"),
    (bwd(n=WS10 - 1), WORKSPACE, f"features workspace {WS10 - 1} < {WS10}"),
    (bwd(n=0, **COV), WORKSPACE, f"features workspace 0 < {WS10}"),
    (bwd(gfeat=None, n=100), WORKSPACE, f"features workspace 100 < {WS10}"),                        # the dL/dF rows are part of it either way
    (bwd(C=64, n=WS10), WORKSPACE, f"features workspace {WS10} < {67328 + 1034 * 256}"),
    # two checks broken at once: the earlier one answers
    (bwd(P=-1, C=0), INVALID, B + "bad sizes"),
    (bwd(C=0, gF=None), INVALID, B + "C = 0 channels, must be 1 .. 64"),
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
        assert fwd(geom=None)(lib) == INVALID and lib.gsr_last_error().decode() == F + "missing features or workspace"   # the forward walk does not care
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


class MapsBackend(OracleBackend):
    """The CPU backend with stand-ins for the two map walks (zeros of the right shapes): the glue's routing is what is looked at."""
    name = "oracle+maps"

    def depth_forward(self, rs, P, num_rendered, mode, geom, binning, img):
        z = torch.zeros((int(rs.image_height), int(rs.image_width)))
        return z, z.clone()

    def features_forward(self, rs, P, num_rendered, features, geom, binning, img):
        assert features.is_contiguous() and features.dtype == torch.float32
        return torch.zeros((int(features.shape[1]), int(rs.image_height), int(rs.image_width)))


def test_the_four_keyword_combinations_return_their_tuples():
    rs, kw = _inputs()
    P, H, W = 50, 32, 32
    F = torch.rand(P, 40)[:, 3:8]                                    # a strided view
    prev = rasterizer._set_backend_for_tests(MapsBackend())
    try:
        R = rasterizer.GaussianRasterizer(rs)
        shapes = lambda out: [tuple(o.shape) for o in out]
        assert shapes(R(**kw)) == [(3, H, W), (P,)] == shapes(R(depth=None, features=None, **kw))
        assert shapes(R(depth="inverse", **kw)) == [(3, H, W), (P,), (1, H, W), (1, H, W)]
        assert shapes(R(features=F, **kw)) == [(3, H, W), (P,), (5, H, W)]
        assert shapes(R(depth="expected", features=F, **kw)) == [(3, H, W), (P,), (1, H, W), (1, H, W), (5, H, W)]
        with torch.no_grad():
            out = R(features=F, **kw)
        assert shapes(out) == [(3, H, W), (P,), (5, H, W)] and all(o.grad_fn is None for o in out)
        # a map whose gradient is None costs no reverse pass: the colour loss alone runs the colour pass only (the stand-in has no
        # features_backward to call)
        F2 = F.clone().requires_grad_(True)
        out = R(features=F2, **kw)
        out[0].sum().backward()
        assert kw["means3D"].grad is not None and F2.grad is None
    finally:
        rasterizer._set_backend_for_tests(prev)


def test_without_the_keyword_the_call_goes_where_it_went(monkeypatch):
    rs, kw = _inputs()
    monkeypatch.setattr(rasterizer._RasterizeGaussiansFeatures, "apply", staticmethod(lambda *a: pytest.fail("the feature function was reached")))
    prev = rasterizer._set_backend_for_tests(OracleBackend())
    try:
        out = rasterizer.GaussianRasterizer(rs)(**kw)
        out_kw = rasterizer.GaussianRasterizer(rs)(features=None, **kw)
    finally:
        rasterizer._set_backend_for_tests(prev)
    assert len(out) == len(out_kw) == 2 and torch.equal(out[0], out_kw[0]) and torch.equal(out[1], out_kw[1])
    assert out[0].grad_fn.__class__.__name__.startswith("_RasterizeGaussiansBackward")


def test_the_stated_limits_raise_with_their_texts():
    rs, kw = _inputs()
    P = 50
    F = torch.rand(P, 4)
    R = rasterizer.GaussianRasterizer(rs)
    prev = rasterizer._set_backend_for_tests(OracleBackend())
    try:
        with pytest.raises(_lib.GsrError, match="the oracle backend renders no feature map"):      # no quiet fall-back to extra renders
            R(features=F, **kw)
        with pytest.raises(_lib.GsrError, match="the oracle backend renders no feature map"):
            R(features=F, depth="expected", **kw)
        cam = rs._replace(campos=rs.campos.clone().requires_grad_(True))
        with pytest.raises(_lib.GsrError, match="features together with camera tensors that require grad: no camera gradient of the feature map"):
            rasterizer.GaussianRasterizer(cam)(features=F, **kw)
    finally:
        rasterizer._set_backend_for_tests(prev)
    for bad, text in ((torch.rand(P, 0), r"features must have dimensions \(num_points, C\) with 1 <= C <= 64, got \(50, 0\) for 50 points"),
                      (torch.rand(P, 65), r"got \(50, 65\) for 50 points"), (torch.rand(P - 1, 4), r"got \(49, 4\) for 50 points"),
                      (torch.rand(P), r"got \(50,\) for 50 points"), (torch.rand(P, 4).double(), "GaussianRasterizer: features must be float32, got float64"),
                      (np.zeros((P, 4), np.float32), "GaussianRasterizer: features must be a torch.Tensor, got ndarray")):
        with pytest.raises(_lib.GsrError, match=text):
            R(features=bad, **kw)
    with pytest.raises(_lib.GsrError, match=r"render_fused: no feature maps on the raw-parameter path \(include/gsr_features.h has no raw_params form\)"):
        render_fused(None, None, PipelineParams(), None, features=F)
    with pytest.raises(_lib.GsrError, match=r"render_rows: no feature maps on the raw-parameter path \(include/gsr_features.h has no raw_params form\)"):
        render_rows([], None, PipelineParams(), None, features=F)


def test_render_adds_the_features_only_when_asked(monkeypatch):
    calls = []

    class FakeRasterizer:
        def __init__(self, raster_settings):
            pass

        def __call__(self, **kw):
            calls.append((kw.get("depth", "absent"), "features" in kw))
            P = kw["means3D"].shape[0]
            out = (torch.zeros(3, 4, 4), torch.ones(P, dtype=torch.int32))
            if kw.get("depth"):
                out += (torch.zeros(1, 4, 4), torch.ones(1, 4, 4))
            if kw.get("features") is not None:
                out += (torch.full((kw["features"].shape[1], 4, 4), 2.0),)
            return out
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
    feat = render(Cam(), PC(), PipelineParams(), torch.zeros(3), features=torch.zeros(5, 7))
    assert set(feat) == set(plain) | {"features"} and feat["features"].shape == (7, 4, 4)
    both = render(Cam(), PC(), PipelineParams(), torch.zeros(3), features=torch.zeros(5, 7), depth="inverse")
    assert set(both) == set(plain) | {"features", "depth", "alpha"} and both["depth"].shape == (1, 4, 4) and float(both["features"].max()) == 2.0
    assert calls == [("absent", False), ("absent", True), ("inverse", True)]
