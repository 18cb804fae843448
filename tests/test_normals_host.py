"""include/gsr_normals.h without a device: the header against the ctypes table, the refusals that are decided before the HIP runtime is
asked for anything, the workspace formula, the Python-side refusals with their texts, and the route of render(normals=True) -- through
the feature path with C + 3 channels -- on a recording backend that computes the normals with tests/normals_ref.py and no map at all."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib, loss, rasterizer
from gaussian_transformer_amd.render import PipelineParams, render, render_fused
from tests import normals_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, WORKSPACE = 0, 1, 4
SENTINEL = "gsr_set_option: unknown option 'sentinel'"
BIG = 1 << 40
A = 1 << 20                        # made-up device addresses, only compared, never followed
NAMES = {"gsr_gaussian_normals_forward", "gsr_gaussian_normals_backward", "gsr_normal_loss_workspace", "gsr_normal_loss_forward",
         "gsr_normal_loss_backward"}


def test_header_declares_exactly_what_the_ctypes_stub_binds():
    header = open(os.path.join(ROOT, "include", "gsr_normals.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decls = dict(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", code, flags=re.S))
    assert set(decls) == NAMES == set(_lib.NORMALS_SIGNATURES)
    for name, args in decls.items():
        assert len(_lib.NORMALS_SIGNATURES[name][1]) == len(args.split(",")), name
    others = (_lib.SIGNATURES, _lib.CHAMFER_SIGNATURES, _lib.SEQUENCE_SIGNATURES, _lib.ROWS_SIGNATURES, _lib.DENSITY_SIGNATURES,
              _lib.MCMC_SIGNATURES, _lib.DEPTH_SIGNATURES, _lib.FEATURES_SIGNATURES, _lib.POSE_SIGNATURES, _lib.CONTRIB_SIGNATURES,
              _lib.ABSGRAD_SIGNATURES)
    assert not any(set(_lib.NORMALS_SIGNATURES) & set(t) for t in others)
    assert "#define GSR_ABI_VERSION 2" in open(os.path.join(ROOT, "include", "gsr.h")).read()   # purely additive
    low = header.lower()
    assert "no gradient goes to scales or means" in low and "no normalisation" in low and "taken as a constant" in low
    assert f"#define GSR_NORMAL_TILE_X {_lib.NORMAL_TILE_X}\n" in header and f"#define GSR_NORMAL_TILE_Y {_lib.NORMAL_TILE_Y}\n" in header
    from gaussian_transformer_amd import build
    assert build.SOURCES["normals.hip"] == build.SOURCES["pergauss_bwd.hip"] == ["-ffp-contract=off", "-fno-slp-vectorize"]
    lib = _lib.load()
    for name in decls:
        assert hasattr(lib, name)


@pytest.mark.parametrize("hw", [(1, 1), (2, 2), (8, 32), (9, 33), (96, 160), (800, 800), (1080, 1920), (3, 100000)])
def test_workspace_bytes(hw):
    H, W = hw
    tiles = ((W + 31) // 32) * ((H + 7) // 8)
    assert _lib.workspace_bytes("gsr_normal_loss_workspace", H, W) == (16 * tiles + 255) // 256 * 256


def gfwd(**kw):
    a = dict(P=10, means=A, scales=2 * A, rots=3 * A, view=4 * A, out=5 * A, axis=6 * A)
    a.update(kw)
    return lambda L: L.gsr_gaussian_normals_forward(None, a["P"], a["means"], a["scales"], a["rots"], a["view"], a["out"], a["axis"])


def gbwd(**kw):
    a = dict(P=10, rots=A, view=2 * A, axis=3 * A, g=4 * A, out=5 * A)
    a.update(kw)
    return lambda L: L.gsr_gaussian_normals_backward(None, a["P"], a["rots"], a["view"], a["axis"], a["g"], a["out"])


def lfwd(**kw):
    a = dict(H=16, W=40, tx=0.5, ty=0.5, amin=0.05, depth=A, alpha=2 * A, normals=3 * A, out2=4 * A, surf=None, ws=5 * A, ws_n=BIG)
    a.update(kw)
    return lambda L: L.gsr_normal_loss_forward(None, a["H"], a["W"], a["tx"], a["ty"], a["amin"], a["depth"], a["alpha"], a["normals"],
                                               a["out2"], a["surf"], a["ws"], a["ws_n"])


def lbwd(**kw):
    a = dict(H=16, W=40, tx=0.5, ty=0.5, amin=0.05, depth=A, alpha=2 * A, normals=3 * A, g=None, gd=4 * A, ga=5 * A, gn=6 * A)
    a.update(kw)
    return lambda L: L.gsr_normal_loss_backward(None, a["H"], a["W"], a["tx"], a["ty"], a["amin"], a["depth"], a["alpha"], a["normals"],
                                                a["g"], a["gd"], a["ga"], a["gn"])


def wsz(H, W, null=False):
    def call(L):
        n = C.c_size_t(0)
        return L.gsr_normal_loss_workspace(H, W, None if null else C.byref(n))
    return call


GF, GB, LW, LF, LB = (n + ": " for n in ("gsr_gaussian_normals_forward", "gsr_gaussian_normals_backward", "gsr_normal_loss_workspace",
                                          "gsr_normal_loss_forward", "gsr_normal_loss_backward"))
AMIN = "alpha_min must be positive (D = depth / alpha is formed where alpha >= alpha_min)"
CASES = [
    (gfwd(P=-1), INVALID, GF + "bad sizes"),
    (gfwd(P=0, means=None, out=None), OK, SENTINEL),                            # nothing to do: nothing is looked at
    (gfwd(means=None), INVALID, GF + "missing input or output buffer"),
    (gfwd(scales=None), INVALID, GF + "missing input or output buffer"),
    (gfwd(rots=None), INVALID, GF + "missing input or output buffer"),
    (gfwd(view=None), INVALID, GF + "missing input or output buffer"),
    (gfwd(out=None), INVALID, GF + "missing input or output buffer"),
    (gbwd(P=-5), INVALID, GB + "bad sizes"),
    (gbwd(P=0, rots=None, out=None), OK, SENTINEL),
    (gbwd(rots=None), INVALID, GB + "missing input or output buffer"),
    (gbwd(view=None), INVALID, GB + "missing input or output buffer"),
    (gbwd(axis=None), INVALID, GB + "missing input or output buffer"),
    (gbwd(g=None), INVALID, GB + "missing input or output buffer"),
    (gbwd(out=None), INVALID, GB + "missing input or output buffer"),
    (wsz(0, 5), INVALID, LW + "bad sizes"),
    (wsz(5, -1), INVALID, LW + "bad sizes"),
    (wsz(5, 5, null=True), INVALID, LW + "bad argument"),
    (wsz(8 * 65535 + 1, 5), INVALID, LW + "image too large"),
    (wsz(5, (1 << 20) + 1), INVALID, LW + "image too large"),
    (lfwd(H=0), INVALID, LF + "bad sizes"),
    (lfwd(W=0), INVALID, LF + "bad sizes"),
    (lfwd(W=-7), INVALID, LF + "bad sizes"),
    (lfwd(amin=0.0), INVALID, LF + AMIN),
    (lfwd(amin=-0.1), INVALID, LF + AMIN),
    (lfwd(amin=float("nan")), INVALID, LF + AMIN),
    (lfwd(depth=None), INVALID, LF + "missing input, output or workspace"),
    (lfwd(alpha=None), INVALID, LF + "missing input, output or workspace"),
    (lfwd(normals=None), INVALID, LF + "missing input, output or workspace"),
    (lfwd(out2=None), INVALID, LF + "missing input, output or workspace"),
    (lfwd(ws=None), INVALID, LF + "missing input, output or workspace"),
    (lfwd(ws_n=255), WORKSPACE, LF + "workspace 255 < 256"),                    # 2 x 2 tiles of 16 bytes, rounded up to 256
    (lfwd(H=1080, W=1920, ws_n=129535), WORKSPACE, LF + "workspace 129535 < 129792"),
    # the order: sizes, alpha_min, pointers, the workspace's size
    (lfwd(H=0, amin=0.0, depth=None, ws_n=0), INVALID, LF + "bad sizes"),
    (lfwd(amin=0.0, depth=None, ws_n=0), INVALID, LF + AMIN),
    (lfwd(depth=None, ws_n=0), INVALID, LF + "missing input, output or workspace"),
    (lbwd(H=0), INVALID, LB + "bad sizes"),
    (lbwd(W=0), INVALID, LB + "bad sizes"),
    (lbwd(amin=0.0), INVALID, LB + AMIN),
    (lbwd(depth=None), INVALID, LB + "missing input"),
    (lbwd(alpha=None), INVALID, LB + "missing input"),
    (lbwd(normals=None), INVALID, LB + "missing input"),
    (lbwd(gd=None, ga=None, gn=None), OK, SENTINEL),                            # no output wanted: nothing runs
    (lbwd(H=0, amin=0.0, depth=None), INVALID, LB + "bad sizes"),
    (lbwd(amin=0.0, depth=None), INVALID, LB + AMIN),
]


@pytest.mark.parametrize("k", range(len(CASES)), ids=[f"{k:02d}" for k in range(len(CASES))])
def test_return_code_and_message(k):
    call, rc, text = CASES[k]
    lib = _lib.load()
    assert lib.gsr_set_option(b"sentinel", 0) == INVALID and lib.gsr_last_error().decode() == SENTINEL
    got, said = call(lib), lib.gsr_last_error().decode()
    assert got == rc and said == text, said


# ---- Python-side refusals ----
class PC:
    get_xyz = torch.zeros(5, 3); get_opacity = torch.zeros(5, 1); get_scaling = torch.ones(5, 3); get_rotation = torch.zeros(5, 4)
    get_features = torch.zeros(5, 4, 3); active_sh_degree = 1; max_sh_degree = 1

    def get_covariance(self, _mod):
        return torch.zeros(5, 6)


class Cam:
    image_height = image_width = 4; FoVx = FoVy = 1.0
    world_view_transform = full_proj_transform = torch.eye(4); camera_center = torch.zeros(3)


def test_render_refuses_what_the_normals_cannot_go_with():
    with pytest.raises(_lib.GsrError, match="render: normals=True with pipe.compute_cov3D_python: the normals are formed from scales and rotations"):
        render(Cam(), PC(), PipelineParams(compute_cov3D_python=True), torch.zeros(3), normals=True)
    with pytest.raises(_lib.GsrError, match=r"render_fused: no normal map on the raw-parameter path \(the normals travel as feature channels"):
        render_fused(None, None, PipelineParams(), None, normals=True)
    with pytest.raises(_lib.GsrError, match="render: normals=True takes 3 of the 64 feature channels: features may have at most 61 columns beside it, got 62"):
        render(Cam(), PC(), PipelineParams(), torch.zeros(3), features=torch.zeros(5, 62), normals=True)
    with pytest.raises(_lib.GsrError, match=r"render: features must be a \[P,C\] tensor to travel with normals=True, got ndarray"):
        render(Cam(), PC(), PipelineParams(), torch.zeros(3), features=np.zeros((5, 2), np.float32), normals=True)


def test_gaussian_normals_refuses_with_the_argument_named():
    rs = rasterizer.GaussianRasterizationSettings(4, 4, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False, False)
    m, s, q = torch.zeros(5, 3), torch.ones(5, 3), torch.zeros(5, 4)
    for args, text in (((m, s[:4], q), r"gaussian_normals: scales must have dimensions \(num_points, 3\), got \(4, 3\) for 5 points"),
                       ((m, s, q[:, :3]), r"gaussian_normals: rotations must have dimensions \(num_points, 4\), got \(5, 3\)"),
                       ((m[:, :2], s, q), r"gaussian_normals: means3D must have dimensions \(num_points, 3\), got \(5, 2\)"),
                       ((m, s.double(), q), "gaussian_normals: scales must be float32, got float64"),
                       ((m, s, None), "gaussian_normals: rotations must be a torch.Tensor, got NoneType")):
        with pytest.raises(_lib.GsrError, match=text):
            rasterizer.gaussian_normals(*args, rs)
    with pytest.raises(_lib.GsrError, match=r"gaussian_normals: viewmatrix must hold 16 values, got shape \(3, 3\)"):
        rasterizer.gaussian_normals(m, s, q, rs._replace(viewmatrix=torch.eye(3)))
    from tests.oracle_backend import OracleBackend
    prev = rasterizer._set_backend_for_tests(OracleBackend())
    try:
        with pytest.raises(_lib.GsrError, match="the oracle backend computes no Gaussian normals"):       # no quiet fall-back to torch
            rasterizer.gaussian_normals(m, s, q, rs)
    finally:
        rasterizer._set_backend_for_tests(prev)


def test_the_loss_refuses_with_the_argument_named():
    d, a, n = torch.ones(6, 7), torch.ones(6, 7), torch.zeros(3, 6, 7)
    f = loss.normal_consistency_loss
    for args, kw, text in (((d, a, n), {}, r"normal_consistency_loss: depth must be on a HIP device, got cpu \(no CPU fallback\)"),
                           ((d[None], a[None], n), {}, "normal_consistency_loss: depth must be on a HIP device"),
                           ((d, a[:5], n), {}, r"normal_consistency_loss: alpha must have depth's shape \(6, 7\) \(or a leading 1\), got \(5, 7\)"),
                           ((d, a, n[:2]), {}, r"normal_consistency_loss: normals must have shape \(3, 6, 7\), got \(2, 6, 7\)"),
                           ((d[0], a[0], n), {}, r"normal_consistency_loss: depth must have shape \[H,W\] or \[1,H,W\], got \(7,\)"),
                           ((d.double(), a, n), {}, "normal_consistency_loss: depth must be float32, got float64"),
                           ((d, a, None), {}, "normal_consistency_loss: normals must be a torch.Tensor, got NoneType"),
                           ((d, a, n), dict(alpha_min=0.0), r"normal_consistency_loss: alpha_min must be positive \(D = depth / alpha is formed where alpha >= alpha_min\), got 0.0")):
        with pytest.raises(_lib.GsrError, match=text):
            f(*args, 0.5, 0.5, **kw)
    with pytest.raises(_lib.GsrError, match="surface_normals: alpha must be on a HIP device|surface_normals: depth must be on a HIP device"):
        loss.surface_normals(d, a, 0.5, 0.5)
    with pytest.raises(_lib.GsrError, match="surface_normals: alpha_min must be positive"):
        loss.surface_normals(d, a, 0.5, 0.5, alpha_min=-1.0)


# ---- the route of render(normals=True) ----
class Recorder:
    """Records what the glue asks of a backend; the normals come from tests/normals_ref.py in float32, the maps are the channel index."""
    name = "recorder"
    H = W = 4

    def __init__(self):
        self.calls = []

    def forward(self, rs, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, **kw):
        self.calls.append(("forward",))
        P = means3D.shape[0]
        return (11, torch.zeros(3, self.H, self.W), torch.ones(P, dtype=torch.int32), torch.zeros(5, dtype=torch.uint8),
                torch.zeros(2, dtype=torch.uint8), torch.zeros(3, dtype=torch.uint8))

    def depth_forward(self, rs, P, num_rendered, mode, geom, binning, img):
        self.calls.append(("depth_forward", mode))
        return torch.zeros(self.H, self.W), torch.ones(self.H, self.W)

    def gaussian_normals_forward(self, viewmatrix, means3D, scales, rotations):
        assert not viewmatrix.requires_grad and all(t.is_contiguous() and t.dtype == torch.float32 for t in (means3D, scales, rotations))
        self.calls.append(("gaussian_normals_forward", tuple(means3D.shape)))
        g = nr.gaussian_normals(means3D, scales, rotations, viewmatrix, torch.float32)
        return g["normals"].detach(), torch.tensor(g["axis"])

    def gaussian_normals_backward(self, viewmatrix, rotations, axis, dL_dnormals):
        self.calls.append(("gaussian_normals_backward", tuple(dL_dnormals.shape)))
        return torch.full((rotations.shape[0], 4), 3.0)

    def features_forward(self, rs, P, num_rendered, features, geom, binning, img):
        self.calls.append(("features_forward", tuple(features.shape)))
        self.features = features.clone()
        C_ = features.shape[1]
        return torch.arange(float(C_))[:, None, None].expand(C_, self.H, self.W).contiguous()

    def features_backward(self, rs, num_rendered, features, dL_dout, means3D, radii, scales, rotations, cov3D_precomp, geom, binning, img,
                          into=None, sh_floats=0, want_features_grad=True):
        self.calls.append(("features_backward", tuple(dL_dout.shape), want_features_grad))
        P = means3D.shape[0]
        return (torch.zeros(P, 3), torch.zeros(P, 3), torch.zeros(P, 1), torch.zeros(P, 3), torch.ones(P, 4), None,
                torch.full(tuple(features.shape), 2.0) if want_features_grad else None)


@pytest.fixture
def recorder():
    be = Recorder()
    prev = rasterizer._set_backend_for_tests(be)
    yield be
    rasterizer._set_backend_for_tests(prev)


def scene_pc(P=5):
    means, scales, q, V = nr.rows(P)

    class Scene(PC):
        get_xyz = torch.tensor(means); get_opacity = torch.full((P, 1), 0.5); get_scaling = torch.tensor(scales)
        get_rotation = torch.tensor(q).requires_grad_(True); get_features = torch.zeros(P, 4, 3)

    class View(Cam):
        world_view_transform = torch.tensor(V)
    return Scene(), View()


@pytest.mark.parametrize("C_user", [0, 1, 61])
def test_normals_travel_as_three_more_feature_channels(recorder, C_user):
    pc, cam = scene_pc()
    P = 5
    F = None if C_user == 0 else torch.rand(P, C_user, requires_grad=True)
    out = render(cam, pc, PipelineParams(), torch.zeros(3), features=F, normals=True)
    assert recorder.calls == [("gaussian_normals_forward", (P, 3)), ("forward",), ("features_forward", (P, C_user + 3))]
    want = nr.gaussian_normals(pc.get_xyz, pc.get_scaling, pc.get_rotation, cam.world_view_transform, torch.float32)["normals"]
    assert torch.equal(recorder.features[:, C_user:], want.detach())
    assert C_user == 0 or torch.equal(recorder.features[:, :C_user], F.detach())
    # the split: the last three planes are the normals, the others the caller's
    assert out["normals"].shape == (3, 4, 4) and [float(out["normals"].detach()[c, 0, 0]) for c in range(3)] == [C_user, C_user + 1.0, C_user + 2.0]
    assert ("features" in out) == (C_user > 0) and (C_user == 0 or out["features"].shape == (C_user, 4, 4))
    assert "depth" not in out
    del recorder.calls[:]
    out["normals"].sum().backward()
    assert recorder.calls == [("features_backward", (C_user + 3, 4, 4), True), ("gaussian_normals_backward", (P, 3))]
    # rotations: the feature pass's own gradient (1) plus the normals' (3); the caller's features get theirs
    assert torch.equal(pc.get_rotation.grad, torch.full((P, 4), 4.0))
    assert C_user == 0 or torch.equal(F.grad, torch.full((P, C_user), 2.0))


def test_normals_with_depth_and_without(recorder):
    pc, cam = scene_pc()
    out = render(cam, pc, PipelineParams(), torch.zeros(3), depth="expected", normals=True)
    assert set(out) == {"render", "viewspace_points", "visibility_filter", "radii", "normals", "depth", "alpha"}
    assert [c[0] for c in recorder.calls] == ["gaussian_normals_forward", "forward", "features_forward", "depth_forward"]
    del recorder.calls[:]
    plain = render(cam, pc, PipelineParams(), torch.zeros(3))
    assert set(plain) == {"render", "viewspace_points", "visibility_filter", "radii"} and recorder.calls == [("forward",)]
    again = render(cam, pc, PipelineParams(), torch.zeros(3), normals=False, features=torch.zeros(5, 2))
    assert "normals" not in again and again["features"].shape == (2, 4, 4)


def test_camera_tensors_that_require_grad_are_refused_by_the_feature_route(recorder):
    pc, cam = scene_pc()

    class GradCam(type(cam)):
        world_view_transform = cam.world_view_transform.clone().requires_grad_(True)
    with pytest.raises(_lib.GsrError, match="features together with camera tensors that require grad: no camera gradient of the feature map"):
        render(GradCam(), pc, PipelineParams(), torch.zeros(3), normals=True)
    # GaussianRasterizer.forward keeps its signature: a caller at that level passes features=gaussian_normals(...)
    import inspect
    assert list(inspect.signature(rasterizer.GaussianRasterizer.forward).parameters) == [
        "self", "means3D", "means2D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp", "depth", "features"]
