"""include/gsr_pose.h without a device: the header against the ctypes table, the workspace size, every refusal that is decided before the
HIP runtime is asked for anything (return code and exact text, as tests/test_cabi_refusals_host.py pins the other headers),
camera.torch_camera against make_camera, and the autograd plumbing of _RasterizeGaussiansPose on an oracle-backed stand-in."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib, camera, rasterizer, synth
from gaussian_transformer_amd.render import PipelineParams, render
from tests import pose_ref
from tests.helpers import oracle_scene
from tests.pose_backend import PoseOracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, WORKSPACE = 0, 1, 4
SENTINEL = "gsr_set_option: unknown option 'sentinel'"
BIG = 1 << 40
A = 1 << 20                        # made-up device addresses, only compared, never followed


def test_header_declares_exactly_what_the_ctypes_stub_binds():
    header = open(os.path.join(ROOT, "include", "gsr_pose.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decls = dict(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", code, flags=re.S))
    assert set(decls) == {"gsr_pose_workspace_bytes", "gsr_pose_backward"} == set(_lib.POSE_SIGNATURES)
    for name, args in decls.items():
        assert len(_lib.POSE_SIGNATURES[name][1]) == len(args.split(",")), name
    others = (_lib.SIGNATURES, _lib.CHAMFER_SIGNATURES, _lib.SEQUENCE_SIGNATURES, _lib.ROWS_SIGNATURES, _lib.DENSITY_SIGNATURES,
              _lib.DEPTH_SIGNATURES)
    assert not any(set(_lib.POSE_SIGNATURES) & set(t) for t in others)
    assert not any(n.startswith("gsr_pose") for n in _lib.SIGNATURES)                     # SIGNATURES stays as it is
    assert "#define GSR_ABI_VERSION 2" in open(os.path.join(ROOT, "include", "gsr.h")).read()   # purely additive
    low = header.lower()
    assert "raw_params" in low and "split sh" in low and "unmodified" in low and "same stream" in low
    from gaussian_transformer_amd import build
    assert build.SOURCES["pose_grad.hip"] == build.SOURCES["pergauss_bwd.hip"]
    lib = _lib.load()
    for name in decls:
        assert hasattr(lib, name)
    assert (_lib.POSE_COLOR, _lib.POSE_DEPTH_EXPECTED, _lib.POSE_DEPTH_INVERSE) == (0, 1, 2)


def test_workspace_bytes_need_no_device():
    """ceil(P / 256) rows of 32 doubles, at least one."""
    lib = _lib.load()
    n = C.c_size_t(0)
    for P, want in ((0, 256), (1, 256), (256, 256), (257, 512), (66000, 258 * 256), (1000000, 3907 * 256)):
        assert lib.gsr_pose_workspace_bytes(P, C.byref(n)) == OK and n.value == want, P


def pose(**kw):
    a = dict(kind=0, P=10, D=1, M=4, W=32, H=32, R=100, means3D=A, radii=2 * A, shs=3 * A, colors=None, scales=4 * A, rots=5 * A, cov=None,
             view=6 * A, proj=7 * A, campos=8 * A, geom=9 * A, acc=10 * A, acc_n=BIG, ws=11 * A, ws_n=BIG, gV=12 * A, gP=13 * A, gC=14 * A)
    a.update(kw)
    return lambda L: L.gsr_pose_backward(None, a["kind"], a["P"], a["D"], a["M"], a["W"], a["H"], a["R"], a["means3D"], a["radii"], a["shs"],
                                         a["colors"], a["scales"], 1.0, a["rots"], a["cov"], a["view"], a["proj"], a["campos"], 0.5, 0.5,
                                         a["geom"], BIG, a["acc"], a["acc_n"], a["ws"], a["ws_n"], a["gV"], a["gP"], a["gC"])


B = "gsr_pose_backward: "
MISSING = B + "missing input or workspace"
COVT = B + "exactly one of (scales, rotations) / cov3D_precomp must be given"
COLT = B + "exactly one of shs / colors_precomp must be given with kind 0"
SHT = B + "SH inputs inconsistent"
ALLNULL = B + "dL_dviewmatrix, dL_dprojmatrix and dL_dcampos are all NULL"
KIND = B + "kind %d is none of 0 (colour), 1 (expected depth), 2 (inverse depth)"
ACC10 = (10 + 1024) * 64                                  # acc_rows(10) rows of 64 bytes

CASES = [
    (lambda L: L.gsr_pose_workspace_bytes(-1, C.byref(C.c_size_t())), INVALID, "gsr_pose_workspace_bytes: bad argument"),
    (lambda L: L.gsr_pose_workspace_bytes(10, None), INVALID, "gsr_pose_workspace_bytes: bad argument"),
    (pose(kind=3), INVALID, KIND % 3),
    (pose(kind=-1), INVALID, KIND % -1),
    (pose(P=-1), INVALID, B + "bad sizes"),
    (pose(W=0), INVALID, B + "bad sizes"),
    (pose(H=-2), INVALID, B + "bad sizes"),
    (pose(R=-1), INVALID, B + "bad sizes"),
    (pose(gV=None, gP=None, gC=None), INVALID, ALLNULL),
    (pose(P=0, gV=None, gP=None, gC=None), INVALID, ALLNULL),
    (pose(means3D=None), INVALID, MISSING),
    (pose(radii=None), INVALID, MISSING),
    (pose(view=None), INVALID, MISSING),
    (pose(proj=None), INVALID, MISSING),
    (pose(geom=None), INVALID, MISSING),
    (pose(acc=None), INVALID, MISSING),
    (pose(ws=None), INVALID, MISSING),
    (pose(cov=15 * A), INVALID, COVT),
    (pose(scales=None, rots=None), INVALID, COVT),
    (pose(rots=None), INVALID, COVT),
    (pose(scales=None, cov=15 * A), INVALID, COVT),
    (pose(colors=16 * A), INVALID, COLT),
    (pose(shs=None), INVALID, COLT),
    (pose(D=4, M=25), INVALID, SHT),
    (pose(D=-1), INVALID, SHT),
    (pose(D=2, M=8), INVALID, SHT),
    (pose(campos=None), INVALID, SHT),
    (pose(ws=11 * A + 8), INVALID, B + "workspaces must be 16-byte aligned"),
    (pose(acc=10 * A + 4), INVALID, B + "workspaces must be 16-byte aligned"),
    (pose(acc_n=ACC10 - 1), WORKSPACE, f"accumulator workspace {ACC10 - 1} < {ACC10}"),
    (pose(kind=1, shs=None, acc_n=0), WORKSPACE, f"accumulator workspace 0 < {ACC10}"),        # the maps read no colour input
    (pose(kind=2, shs=None, colors=None, campos=None, ws_n=255), WORKSPACE, "pose workspace 255 < 256"),
    (pose(P=257, ws_n=511), WORKSPACE, "pose workspace 511 < 512"),
    (pose(gV=None, gC=None, ws_n=0), WORKSPACE, "pose workspace 0 < 256"),                     # one output is enough
    # two checks broken at once: the earlier one answers
    (pose(kind=5, P=-1), INVALID, KIND % 5),
    (pose(W=0, gV=None, gP=None, gC=None), INVALID, B + "bad sizes"),
    (pose(means3D=None, rots=None), INVALID, MISSING),
    (pose(rots=None, shs=None), INVALID, COVT),
    (pose(colors=16 * A, acc_n=0), INVALID, COLT),
    (pose(D=7, ws_n=0), INVALID, SHT),
    (pose(acc_n=0, ws_n=0), WORKSPACE, f"accumulator workspace 0 < {ACC10}"),
]


@pytest.mark.parametrize("k", range(len(CASES)), ids=[f"{k:02d}-{'ok' if c[1] == OK else c[2][:48]}" for k, c in enumerate(CASES)])
def test_return_code_and_message(k):
    call, rc, text = CASES[k]
    lib = _lib.load()
    assert lib.gsr_set_option(b"sentinel", 0) == INVALID and lib.gsr_last_error().decode() == SENTINEL
    got = call(lib)
    assert (got, lib.gsr_last_error().decode()) == (rc, text)


# ---- camera.torch_camera ----
def _pose(seed=0):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    r, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                  [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                  [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]])
    return R, rng.normal(size=3)


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_torch_camera_reproduces_make_camera(seed):
    R, t = _pose(seed)
    fovx, fovy = 1.1, 0.8
    ref_cam = camera.make_camera(R, t, fovx, fovy, 64, 48)
    w2c = camera.world_to_view(R, t)
    for pose_in in (w2c, torch.tensor(w2c)):
        cam = camera.torch_camera(pose_in, fovx, fovy, 64, 48)
        assert (cam.image_width, cam.image_height, cam.FoVx, cam.FoVy) == (64, 48, fovx, fovy)
        assert cam.world_view_transform.dtype == torch.float32
        assert np.array_equal(cam.world_view_transform.numpy(), ref_cam.world_view_transform)
        # float32 products of the same float32 factors; the centre in closed form against make_camera's float32 inverse
        np.testing.assert_allclose(cam.full_proj_transform.numpy(), ref_cam.full_proj_transform, rtol=0, atol=4e-7 * np.abs(ref_cam.full_proj_transform).max())
        np.testing.assert_allclose(cam.camera_center.numpy(), ref_cam.camera_center, rtol=0, atol=2e-6 * max(1.0, np.abs(ref_cam.camera_center).max()))
    with pytest.raises(ValueError, match=r"w2c must be \[4,4\]"):
        camera.torch_camera(np.eye(3), fovx, fovy, 64, 48)


def test_torch_camera_is_differentiable_in_the_pose():
    R, t = _pose(3)
    w2c = torch.tensor(camera.world_to_view(R, t), dtype=torch.float64, requires_grad=True)
    cam = camera.torch_camera(w2c, 1.0, 0.9, 32, 32)
    assert cam.world_view_transform.requires_grad and cam.full_proj_transform.requires_grad and cam.camera_center.requires_grad
    torch.autograd.gradcheck(lambda m: camera.torch_camera(m, 1.0, 0.9, 32, 32).full_proj_transform, (w2c,))
    torch.autograd.gradcheck(lambda m: camera.torch_camera(m, 1.0, 0.9, 32, 32).camera_center, (w2c,))
    # the centre is the camera's position: it maps to the origin of the camera frame (the rotation is orthonormal to float32)
    c = cam.camera_center.detach()
    assert torch.allclose(w2c.detach()[:3, :3] @ c + w2c.detach()[:3, 3], torch.zeros(3, dtype=torch.float64), atol=1e-6)


# ---- the autograd plumbing, on the oracle-backed stand-in ----
P_, W_, H_ = 40, 32, 32


def _scene():
    return synth.make_scene(P=P_, width=W_, height=H_, sh_degree=1, s0=0.15, seed=3)


def _inputs(sc, cam_grad=(True, True, True), gauss_grad=True, cam=None):
    cam = sc.camera if cam is None else cam
    t = lambda a: a if isinstance(a, torch.Tensor) else torch.tensor(np.asarray(a, np.float32))
    tensors = [t(cam.world_view_transform), t(cam.full_proj_transform), t(cam.camera_center)]
    for x, g in zip(tensors, cam_grad):
        if g and not x.requires_grad:
            x.requires_grad_(True)
    rs = rasterizer.GaussianRasterizationSettings(
        image_height=H_, image_width=W_, tanfovx=cam.tanfovx if hasattr(cam, "tanfovx") else math.tan(cam.FoVx * 0.5),
        tanfovy=cam.tanfovy if hasattr(cam, "tanfovy") else math.tan(cam.FoVy * 0.5), bg=t(sc.bg), scale_modifier=1.0,
        viewmatrix=tensors[0], projmatrix=tensors[1], sh_degree=1, campos=tensors[2], prefiltered=False, debug=False)
    kw = dict(means3D=t(sc.means3D).requires_grad_(gauss_grad), means2D=torch.zeros(P_, 3, requires_grad=gauss_grad),
              opacities=t(sc.opacities).reshape(P_, 1), shs=t(sc.shs).requires_grad_(gauss_grad), scales=t(sc.scales), rotations=t(sc.rotations))
    return rs, kw


@pytest.fixture
def backend():
    be = PoseOracleBackend("f32")
    prev = rasterizer._set_backend_for_tests(be)
    yield be
    rasterizer._set_backend_for_tests(prev)


@pytest.fixture(scope="module")
def reference():
    sc = _scene()
    dL = np.asarray(sc.dL_dimage, np.float64) * 3 * W_ * H_
    return sc, dL, pose_ref.colour_grads(oracle_scene(sc), dL, "f64")


def test_gradients_arrive_on_the_three_camera_tensors(backend, reference):
    sc, dL, want = reference
    rs, kw = _inputs(sc)
    color, radii = rasterizer.GaussianRasterizer(rs)(**kw)
    assert color.grad_fn.__class__.__name__.startswith("_RasterizeGaussiansPoseBackward")
    (color * torch.tensor(dL, dtype=torch.float32)).sum().backward()
    assert backend.calls == ["forward", "backward", "pose_backward"]
    for x, k in ((rs.viewmatrix, "viewmatrix"), (rs.projmatrix, "projmatrix"), (rs.campos, "campos")):
        assert x.grad is not None and x.grad.shape == x.shape and x.grad.dtype == torch.float32, k
        assert pose_ref.rel_err(x.grad.numpy().reshape(-1), want[k]) < 1e-4, k
    assert kw["means3D"].grad is not None and kw["shs"].grad is not None      # the Gaussians' gradients are unchanged company


def test_only_campos_and_gaussians_without_grad(backend, reference):
    sc, dL, want = reference
    rs, kw = _inputs(sc, cam_grad=(False, False, True), gauss_grad=False)
    color, _ = rasterizer.GaussianRasterizer(rs)(**kw)
    (color * torch.tensor(dL, dtype=torch.float32)).sum().backward()
    assert rs.viewmatrix.grad is None and rs.projmatrix.grad is None and kw["means3D"].grad is None
    assert pose_ref.rel_err(rs.campos.grad.numpy(), want["campos"]) < 1e-4


def test_pose_parameter_behind_torch_camera_and_a_transposed_view(backend, reference):
    sc, dL, want = reference
    w2c = torch.eye(4, requires_grad=True)                              # synth's camera: at the origin, looking down +z
    cam = camera.torch_camera(w2c, sc.camera.FoVx, sc.camera.FoVy, W_, H_)
    assert not cam.world_view_transform.is_contiguous()                 # w2c.t(): a strided view reaches the settings
    rs, kw = _inputs(sc, cam_grad=(False, False, False), cam=cam)
    color, _ = rasterizer.GaussianRasterizer(rs)(**kw)
    (color * torch.tensor(dL, dtype=torch.float32)).sum().backward()
    assert w2c.grad is not None and w2c.grad.shape == (4, 4)
    # the chain by hand, float64: viewmatrix = w2c^T, projmatrix = w2c^T P^T, campos = -R^T t
    m = torch.eye(4, dtype=torch.float64, requires_grad=True)
    c64 = camera.torch_camera(m, sc.camera.FoVx, sc.camera.FoVy, W_, H_)
    s = (c64.world_view_transform * torch.tensor(want["viewmatrix"].reshape(4, 4))).sum() + \
        (c64.full_proj_transform * torch.tensor(want["projmatrix"].reshape(4, 4))).sum() + (c64.camera_center * torch.tensor(want["campos"])).sum()
    s.backward()
    assert pose_ref.rel_err(w2c.grad.numpy(), m.grad.numpy()) < 1e-4
    # a non-contiguous view handed in directly
    wv = torch.tensor(np.asarray(sc.camera.world_view_transform, np.float32).T.copy(), requires_grad=True)
    rs2, kw2 = _inputs(sc, cam_grad=(False, True, True))
    rs2 = rs2._replace(viewmatrix=wv.t())
    assert not rs2.viewmatrix.is_contiguous()
    color, _ = rasterizer.GaussianRasterizer(rs2)(**kw2)
    (color * torch.tensor(dL, dtype=torch.float32)).sum().backward()
    assert pose_ref.rel_err(wv.grad.t().numpy().reshape(-1), want["viewmatrix"]) < 1e-4


def test_without_requires_grad_or_under_no_grad_the_old_route_is_taken(backend, reference, monkeypatch):
    sc, dL, _ = reference
    monkeypatch.setattr(rasterizer._RasterizeGaussiansPose, "apply", staticmethod(lambda *a: pytest.fail("the pose function was reached")))
    rs, kw = _inputs(sc, cam_grad=(False, False, False))
    color, _ = rasterizer.GaussianRasterizer(rs)(**kw)
    assert color.grad_fn.__class__.__name__.startswith("_RasterizeGaussiansBackward")
    color.sum().backward()
    assert backend.calls == ["forward", "backward"]
    rs, kw = _inputs(sc)                                                 # cameras with grad, but grad mode off
    with torch.no_grad():
        color, _ = rasterizer.GaussianRasterizer(rs)(**kw)
    assert color.grad_fn is None and backend.calls == ["forward", "backward", "forward"]


def test_render_routes_a_torch_camera_and_the_python_sh_branch_differentiates_the_centre_itself(backend, reference):
    sc, dL, want = reference

    class PC:
        get_xyz = torch.tensor(sc.means3D); get_opacity = torch.tensor(sc.opacities).reshape(P_, 1)
        get_scaling = torch.tensor(sc.scales); get_rotation = torch.tensor(sc.rotations)
        get_features = torch.tensor(sc.shs); active_sh_degree = 1; max_sh_degree = 1
    w2c = torch.eye(4, requires_grad=True)
    out = render(camera.torch_camera(w2c, sc.camera.FoVx, sc.camera.FoVy, W_, H_), PC(), PipelineParams(), torch.tensor(sc.bg))
    (out["render"] * torch.tensor(dL, dtype=torch.float32)).sum().backward()
    g_kernel = w2c.grad.clone()
    assert backend.calls == ["forward", "backward", "pose_backward"] and g_kernel.abs().max() > 0
    # convert_SHs_python: colours are made in torch from camera_center; the kernel's dL/dcampos is zero and torch supplies the rest
    w2c2 = torch.eye(4, requires_grad=True)
    out = render(camera.torch_camera(w2c2, sc.camera.FoVx, sc.camera.FoVy, W_, H_), PC(), PipelineParams(convert_SHs_python=True), torch.tensor(sc.bg))
    (out["render"] * torch.tensor(dL, dtype=torch.float32)).sum().backward()
    assert pose_ref.rel_err(w2c2.grad.numpy(), g_kernel.numpy()) < 2e-3
