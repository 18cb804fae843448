"""Which backend calls the four autograd Functions of rasterizer.py make, with which tensors and keywords: pinned as literal tables on
a recording stand-in that computes nothing (P = 3, a 4 x 4 image, M = 1).  The oracle stand-ins render no maps, so this is the only CPU
test that reaches the map routes of _RasterizeGaussiansDepth.backward and _RasterizeGaussiansPose.backward."""
import pytest
import torch

from gaussian_transformer_amd import _lib, rasterizer
from gaussian_transformer_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer

P, H, W, M = 3, 4, 4, 1
CALLER = torch.arange(1.0, 3 * H * W + 1).reshape(3, H, W)           # the caller's colour gradient
W_DEPTH = torch.arange(1.0, H * W + 1).reshape(1, H, W) * 0.5
W_ALPHA = torch.arange(1.0, H * W + 1).reshape(1, H, W) * 0.25
COLOUR, EXPECTED, INVERSE = _lib.POSE_COLOR, _lib.POSE_DEPTH_EXPECTED, _lib.POSE_DEPTH_INVERSE
# the sentinel values: backward() fills its tensors with these, depth_backward() adds 10 to what it is given (or starts from 10),
# pose_backward() returns (1, 2, 3) times 1 (colour), 10 (expected depth) or 100 (inverse depth)
G = dict(means3D=1.0, means2D=2.0, sh=3.0, colors=4.0, opac=5.0, scales=6.0, rots=7.0, cov=8.0, rest=9.0)
POSE_SCALE = {COLOUR: 1.0, EXPECTED: 10.0, INVERSE: 100.0}


class Recorder:
    """A backend that records its calls.  `announced`: carries the attribute the Functions probe before they pass
    announce_backward.  `fill`: what arena_fill_in_flight answers."""
    name = "recorder"

    def __init__(self, announced=False, fill=False):
        self.calls, self.fill = [], fill
        self.last_backward = self.last_ws = None
        if announced:
            self._announced = {}

    def forward(self, rs, means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, **kw):
        self.rs = rs
        self.forward_args = (means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp)
        self.forward_kw = kw
        self.calls.append(("forward", tuple(sorted(kw))))
        self.geom = torch.full((5,), 7, dtype=torch.uint8)
        return (11, torch.zeros(3, H, W), torch.ones(P, dtype=torch.int32), self.geom, torch.zeros(2, dtype=torch.uint8),
                torch.zeros(3, dtype=torch.uint8))

    def _colour(self, dL):
        if dL.shape == (3, H, W) and not dL.any():
            return "zeros"
        return "caller" if torch.equal(dL, CALLER) else "other"

    def backward(self, rs, num_rendered, dL_dpix, means3D, radii, shs, colors_precomp, scales, rotations, cov3D_precomp,
                 geom, binning, img, **kw):
        assert num_rendered == 11 and geom.data_ptr() == self.geom.data_ptr()
        self.calls.append(("backward", self._colour(dL_dpix), tuple(sorted(kw))))
        full = lambda shape, k: torch.full(shape, G[k])
        out = (full((P, 3), "means3D"), full((P, 3), "means2D"), full((P, M, 3), "sh") if shs.numel() else torch.empty(0),
               full((P, 3), "colors") if colors_precomp.numel() else None, full((P, 1), "opac"), full((P, 3), "scales"),
               full((P, 4), "rots"), None)
        self.last_backward = out
        if kw.get("shs_rest") is not None:
            out = out + (full(tuple(kw["shs_rest"].shape), "rest"),)
        if kw.get("return_ws"):
            self.last_ws = torch.zeros(1, dtype=torch.uint8)
            out = out + (self.last_ws,)
        return out

    def depth_forward(self, rs, n_points, num_rendered, mode, geom, binning, img):
        self.calls.append(("depth_forward", mode))
        return torch.zeros(H, W), torch.zeros(H, W)

    def arena_fill_in_flight(self, geom):
        return self.fill

    def depth_backward(self, rs, num_rendered, mode, dL_ddepth, dL_dalpha, means3D, radii, scales, rotations, cov3D_precomp,
                       geom, binning, img, **kw):
        assert dL_ddepth is None or torch.equal(dL_ddepth, W_DEPTH)
        assert dL_dalpha is None or torch.equal(dL_dalpha, W_ALPHA)
        into = kw.get("into")
        if into is None:
            state = "none"
            out = (torch.full((P, 3), 10.0), torch.full((P, 3), 10.0), torch.full((P, 1), 10.0), torch.full((P, 3), 10.0),
                   torch.full((P, 4), 10.0), None)
        else:
            b = self.last_backward
            state = "previous" if len(into) == 6 and all(x is y for x, y in zip(into, (b[0], b[1], b[4], b[5], b[6], b[7]))) else "other"
            for t in into:
                if t is not None:
                    t += 10.0
            out = tuple(into)
        self.calls.append(("depth_backward", mode, state, kw.get("sh_floats"), (dL_ddepth is not None, dL_dalpha is not None),
                           tuple(sorted(kw))))
        if kw.get("return_ws"):
            self.last_ws = torch.zeros(1, dtype=torch.uint8)
            out = out + (self.last_ws,)
        return out

    def pose_backward(self, rs, kind, num_rendered, means3D, radii, shs, colors_precomp, scales, rotations, cov3D_precomp, geom, acc_ws,
                      **kw):
        want = kw["want"]
        self.calls.append(("pose_backward", kind, tuple(want), acc_ws is self.last_ws, tuple(sorted(kw))))
        s = POSE_SCALE[kind]
        return (torch.full((4, 4), 1.0 * s) if want[0] else None, torch.full((4, 4), 2.0 * s) if want[1] else None,
                torch.full((3,), 3.0 * s) if want[2] else None)

    def composited_mask(self, geom, n_points):
        self.calls.append(("composited_mask", geom.data_ptr() == self.geom.data_ptr(), n_points))
        return torch.ones(n_points, dtype=torch.bool)


@pytest.fixture
def use():
    prev = []

    def install(**kw):
        be = Recorder(**kw)
        prev.append(rasterizer._set_backend_for_tests(be))
        return be
    yield install
    if prev:
        rasterizer._set_backend_for_tests(prev[0])


def _settings(cam_grad=(False, False, False), view=None):
    cam = [torch.eye(4) if view is None else view, torch.eye(4) * 2, torch.arange(3.0)]
    for t, g in zip(cam, cam_grad):
        if g:
            t.requires_grad_(True)
    return GaussianRasterizationSettings(H, W, 1.0, 1.0, torch.zeros(3), 1.0, cam[0], cam[1], 0, cam[2], False, False)


def _inputs(grad=True, precomp=False):
    leaf = lambda *shape: torch.ones(*shape).requires_grad_(grad)
    kw = dict(means3D=leaf(P, 3), means2D=leaf(P, 3), opacities=leaf(P, 1), scales=leaf(P, 3), rotations=leaf(P, 4))
    kw["colors_precomp" if precomp else "shs"] = leaf(P, 3) if precomp else leaf(P, M, 3)
    return kw


def _loss(out, c, depth, alpha):
    parts = ([(out[0] * CALLER).sum()] if c else []) + ([(out[2] * W_DEPTH).sum()] if depth else []) + \
            ([(out[3] * W_ALPHA).sum()] if alpha else [])
    return sum(parts[1:], parts[0])


def _grads(kw):
    return {k: (None if t.grad is None else float(t.grad.reshape(-1)[0])) for k, t in kw.items()}


MAPS = {"depth": (True, False), "alpha": (False, True), "both": (True, True)}
B_PLAIN, B_WS = (), ("return_ws",)
D_PLAIN, D_WS = ("into", "sh_floats"), ("into", "return_ws", "sh_floats")
ONLY_COLOUR = dict(means3D=1.0, means2D=2.0, opacities=5.0, scales=6.0, rotations=7.0, shs=3.0)
ONLY_MAPS = dict(means3D=10.0, means2D=10.0, opacities=10.0, scales=10.0, rotations=10.0, shs=None)
MAPS_ON_ZERO_COLOUR = dict(means3D=11.0, means2D=12.0, opacities=15.0, scales=16.0, rotations=17.0, shs=None)
BOTH = dict(MAPS_ON_ZERO_COLOUR, shs=3.0)


# ---- _RasterizeGaussiansDepth ----
def test_depth_function_without_any_gradient_calls_nothing(use):
    be = use()
    out = GaussianRasterizer(_settings())(depth="expected", **_inputs())
    fn = out[0].grad_fn
    assert type(fn).__name__.startswith("_RasterizeGaussiansDepthBackward")
    n = len(be.calls)
    assert rasterizer._RasterizeGaussiansDepth.backward(fn, None, None, None, None) == (None,) * 10
    assert be.calls[n:] == []


@pytest.mark.parametrize("fill", (False, True))
def test_depth_function_colour_alone(use, fill):
    be = use(fill=fill)
    kw = _inputs()
    out = GaussianRasterizer(_settings())(depth="inverse", **kw)
    n = len(be.calls)
    _loss(out, True, False, False).backward()
    assert be.calls[n:] == [("backward", "caller", B_PLAIN)]
    assert _grads(kw) == ONLY_COLOUR


@pytest.mark.parametrize("maps", MAPS)
@pytest.mark.parametrize("mode", ("expected", "inverse"))
def test_depth_function_maps_alone(use, mode, maps):
    m = rasterizer.DEPTH_MODES[mode]
    be = use(fill=False)
    kw = _inputs()
    out = GaussianRasterizer(_settings())(depth=mode, **kw)
    n = len(be.calls)
    _loss(out, False, *MAPS[maps]).backward()
    assert be.calls[n:] == [("depth_backward", m, "none", 3 * M, MAPS[maps], D_PLAIN)]
    assert _grads(kw) == ONLY_MAPS


@pytest.mark.parametrize("maps", MAPS)
def test_depth_function_maps_alone_while_an_arena_fill_is_in_flight(use, maps):
    be = use(fill=True)
    kw = _inputs()
    out = GaussianRasterizer(_settings())(depth="expected", **kw)
    n = len(be.calls)
    _loss(out, False, *MAPS[maps]).backward()
    assert be.calls[n:] == [("backward", "zeros", B_PLAIN), ("depth_backward", 0, "previous", 3 * M, MAPS[maps], D_PLAIN)]
    assert _grads(kw) == MAPS_ON_ZERO_COLOUR                                   # the colour inputs get None


@pytest.mark.parametrize("fill", (False, True))
@pytest.mark.parametrize("maps", MAPS)
def test_depth_function_colour_and_maps(use, maps, fill):
    be = use(fill=fill)
    kw = _inputs()
    out = GaussianRasterizer(_settings())(depth="expected", **kw)
    n = len(be.calls)
    _loss(out, True, *MAPS[maps]).backward()
    assert be.calls[n:] == [("backward", "caller", B_PLAIN), ("depth_backward", 0, "previous", 3 * M, MAPS[maps], D_PLAIN)]
    assert _grads(kw) == BOTH


def test_depth_function_with_precomputed_colours_has_no_sh_floats(use):
    be = use(fill=True)
    kw = _inputs(precomp=True)
    out = GaussianRasterizer(_settings())(depth="expected", **kw)
    n = len(be.calls)
    _loss(out, False, True, False).backward()
    assert be.calls[n:] == [("backward", "zeros", B_PLAIN), ("depth_backward", 0, "previous", 0, (True, False), D_PLAIN)]
    assert kw["colors_precomp"].grad is None
    kw = _inputs(precomp=True)
    out = GaussianRasterizer(_settings())(depth="expected", **kw)
    _loss(out, True, True, False).backward()
    assert float(kw["colors_precomp"].grad[0, 0]) == G["colors"]


# ---- _RasterizeGaussiansPose, mode None ----
WANTS = {"all": (True, True, True), "campos": (False, False, True), "view-proj": (True, True, False)}


def _cam_grads(rs):
    return [None if t.grad is None else float(t.grad.reshape(-1)[0]) for t in (rs.viewmatrix, rs.projmatrix, rs.campos)]


@pytest.mark.parametrize("want", WANTS)
def test_pose_function_colour_route(use, want):
    be = use(fill=True)
    rs, kw = _settings(WANTS[want]), _inputs()
    out = GaussianRasterizer(rs)(**kw)
    assert len(out) == 2 and type(out[0].grad_fn).__name__.startswith("_RasterizeGaussiansPoseBackward")
    n = len(be.calls)
    _loss(out, True, False, False).backward()
    assert be.calls[n:] == [("backward", "caller", B_WS), ("pose_backward", COLOUR, WANTS[want], True, ("want",))]
    assert _grads(kw) == ONLY_COLOUR
    assert _cam_grads(rs) == [v if w else None for v, w in zip((1.0, 2.0, 3.0), WANTS[want])]


def test_pose_function_without_maps_runs_the_colour_pass_on_a_zero_gradient(use):
    """The colour output unused in mode None: not reachable through autograd (nothing else is differentiable), so backward is
    called on the graph's own context."""
    be = use()
    rs, kw = _settings((True, True, True)), _inputs()
    out = GaussianRasterizer(rs)(**kw)
    n = len(be.calls)
    g = rasterizer._RasterizeGaussiansPose.backward(out[0].grad_fn, None, None)
    assert be.calls[n:] == [("backward", "zeros", B_WS), ("pose_backward", COLOUR, (True, True, True), True, ("want",))]
    assert len(g) == 13 and g[2] is None and g[3] is None and g[11] is None and g[12] is None
    assert [float(x.reshape(-1)[0]) for x in (g[0], g[1], g[4], g[5], g[6])] == [1.0, 2.0, 5.0, 6.0, 7.0] and g[7] is None
    assert [float(x.reshape(-1)[0]) for x in g[8:11]] == [1.0, 2.0, 3.0]


# ---- _RasterizeGaussiansPose, mode expected / inverse ----
KIND = {"expected": EXPECTED, "inverse": INVERSE}


def test_pose_function_with_maps_and_no_gradient_calls_nothing(use):
    be = use()
    out = GaussianRasterizer(_settings((True, True, True)))(depth="expected", **_inputs())
    n = len(be.calls)
    assert rasterizer._RasterizeGaussiansPose.backward(out[0].grad_fn, None, None, None, None) == (None,) * 13
    assert be.calls[n:] == []


@pytest.mark.parametrize("mode", KIND)
def test_pose_function_with_maps_colour_alone(use, mode):
    be = use(fill=True)
    rs, kw = _settings((True, True, True)), _inputs()
    out = GaussianRasterizer(rs)(depth=mode, **kw)
    assert len(out) == 4
    n = len(be.calls)
    _loss(out, True, False, False).backward()
    assert be.calls[n:] == [("backward", "caller", B_WS), ("pose_backward", COLOUR, (True, True, True), True, ("want",))]
    assert _grads(kw) == ONLY_COLOUR and _cam_grads(rs) == [1.0, 2.0, 3.0]


@pytest.mark.parametrize("maps", MAPS)
@pytest.mark.parametrize("mode", KIND)
def test_pose_function_maps_alone(use, mode, maps):
    be = use(fill=False)
    rs, kw = _settings((True, True, True)), _inputs()
    out = GaussianRasterizer(rs)(depth=mode, **kw)
    n = len(be.calls)
    _loss(out, False, *MAPS[maps]).backward()
    assert be.calls[n:] == [("depth_backward", rasterizer.DEPTH_MODES[mode], "none", 3 * M, MAPS[maps], D_WS),
                            ("pose_backward", KIND[mode], (True, True, True), True, ("want",))]
    s = POSE_SCALE[KIND[mode]]
    assert _grads(kw) == ONLY_MAPS and _cam_grads(rs) == [1.0 * s, 2.0 * s, 3.0 * s]


@pytest.mark.parametrize("maps", MAPS)
@pytest.mark.parametrize("mode", KIND)
def test_pose_function_maps_alone_while_an_arena_fill_is_in_flight(use, mode, maps):
    be = use(fill=True)
    rs, kw = _settings((True, True, True)), _inputs()
    out = GaussianRasterizer(rs)(depth=mode, **kw)
    n = len(be.calls)
    _loss(out, False, *MAPS[maps]).backward()
    assert be.calls[n:] == [("backward", "zeros", B_WS),                                       # and no colour pose call
                            ("depth_backward", rasterizer.DEPTH_MODES[mode], "previous", 3 * M, MAPS[maps], D_WS),
                            ("pose_backward", KIND[mode], (True, True, True), True, ("want",))]
    s = POSE_SCALE[KIND[mode]]
    assert _grads(kw) == MAPS_ON_ZERO_COLOUR and _cam_grads(rs) == [1.0 * s, 2.0 * s, 3.0 * s]


@pytest.mark.parametrize("want", WANTS)
@pytest.mark.parametrize("maps", MAPS)
@pytest.mark.parametrize("mode", KIND)
def test_pose_function_colour_and_maps_sums_the_two_camera_parts(use, mode, maps, want):
    be = use(fill=(maps == "both"))
    rs, kw = _settings(WANTS[want]), _inputs()
    out = GaussianRasterizer(rs)(depth=mode, **kw)
    n = len(be.calls)
    _loss(out, True, *MAPS[maps]).backward()
    assert be.calls[n:] == [("backward", "caller", B_WS), ("pose_backward", COLOUR, WANTS[want], True, ("want",)),
                            ("depth_backward", rasterizer.DEPTH_MODES[mode], "previous", 3 * M, MAPS[maps], D_WS),
                            ("pose_backward", KIND[mode], WANTS[want], True, ("want",))]
    s = 1.0 + POSE_SCALE[KIND[mode]]
    assert _grads(kw) == BOTH
    assert _cam_grads(rs) == [v * s if w else None for v, w in zip((1.0, 2.0, 3.0), WANTS[want])]


def test_pose_function_camera_gradient_comes_back_in_the_inputs_shape_dtype_and_device(use):
    """A transposed view and a [1, 3] centre: the backend sees dense float32 copies, the gradients arrive shaped like the inputs.  A
    float64 camera tensor is refused by the forward call ("must be float32", as every other input), so no float64 gradient exists
    to come back."""
    be = use()
    base = torch.arange(16.0).reshape(4, 4).requires_grad_(True)
    rs = _settings((False, False, False), view=base.t())
    rs = rs._replace(campos=torch.arange(3.0).reshape(1, 3).requires_grad_(True))
    assert not rs.viewmatrix.is_contiguous()
    out = GaussianRasterizer(rs)(**_inputs())
    seen = be.rs
    for a, b in ((seen.viewmatrix, rs.viewmatrix), (seen.projmatrix, rs.projmatrix), (seen.campos, rs.campos)):
        assert a is not b and not a.requires_grad and a.is_contiguous() and a.dtype == torch.float32 and torch.equal(a, b.detach())
    assert seen.bg is rs.bg and seen[:4] == rs[:4]
    n = len(be.calls)
    _loss(out, True, False, False).backward()
    assert be.calls[n:][1] == ("pose_backward", COLOUR, (True, False, True), True, ("want",))
    assert base.grad.shape == (4, 4) and base.grad.dtype == torch.float32 and base.grad.device == base.device
    assert torch.equal(base.grad, torch.full((4, 4), 1.0))
    assert rs.campos.grad.shape == (1, 3) and torch.equal(rs.campos.grad, torch.full((1, 3), 3.0))
    rs64 = _settings((False, False, False), view=torch.eye(4, dtype=torch.float64).requires_grad_(True))
    with pytest.raises(_lib.GsrError, match="viewmatrix must be float32, got torch.float64"):
        GaussianRasterizer(rs64)(**_inputs())


# ---- the plain and the fused function: their reverse calls ----
def test_plain_function_backward(use):
    be = use()
    kw = _inputs()
    out = GaussianRasterizer(_settings())(**kw)
    assert type(out[0].grad_fn).__name__.startswith("_RasterizeGaussiansBackward")
    n = len(be.calls)
    g = rasterizer._RasterizeGaussians.backward(out[0].grad_fn, None, None)          # an unused colour output arrives as None
    assert be.calls[n:] == [("backward", "zeros", B_PLAIN)]
    assert len(g) == 9 and float(g[2].reshape(-1)[0]) == G["sh"] and g[3] is None and g[7] is None and g[8] is None
    _loss(out, True, False, False).backward()
    assert be.calls[n + 1:] == [("backward", "caller", B_PLAIN)] and _grads(kw) == ONLY_COLOUR


def _fused_inputs(grad=True):
    leaf = lambda *shape: torch.ones(*shape).requires_grad_(grad)
    return [leaf(P, 3), leaf(P, 3), leaf(P, 1, 3), leaf(P, 2, 3), leaf(P, 1), leaf(P, 3), leaf(P, 4)]


def test_fused_function_forward_and_backward(use):
    be = use(announced=True)
    a = _fused_inputs()
    color, radii = rasterizer.rasterize_gaussians_fused(*a, _settings())
    assert be.calls == [("forward", ("announce_backward", "raw_params", "shs_rest"))]
    assert be.forward_kw["raw_params"] is True and be.forward_kw["announce_backward"] is True
    assert torch.equal(be.forward_kw["shs_rest"], a[3]) and torch.equal(be.forward_args[1], a[2])
    assert be.forward_args[2].numel() == 0 and be.forward_args[6].numel() == 0          # colors_precomp, cov3D_precomp
    fn = color.grad_fn
    assert type(fn).__name__.startswith("_RasterizeGaussiansFusedBackward") and (fn.gsr_geom_index, fn.gsr_means_index) == (6, 0)
    g = rasterizer._RasterizeGaussiansFused.backward(fn, None, None)                 # an unused colour output arrives as None
    assert be.calls[1:] == [("backward", "zeros", ("raw_params", "shs_rest"))] and len(g) == 8 and g[7] is None
    (color * CALLER).sum().backward()
    assert be.calls[2:] == [("backward", "caller", ("raw_params", "shs_rest"))]
    assert [float(t.grad.reshape(-1)[0]) for t in a] == [1.0, 2.0, 3.0, 9.0, 5.0, 6.0, 7.0]
    with pytest.raises(_lib.GsrError, match=r"features_dc must be \[P,1,3\]"):
        rasterizer.rasterize_gaussians_fused(a[0], a[1], a[3], a[3], *a[4:], _settings())
    with pytest.raises(_lib.GsrError, match=r"means3D must have dimensions \(num_points, 3\)"):
        rasterizer.rasterize_gaussians_fused(torch.ones(P, 4), *a[1:], _settings())


# ---- forward, all four functions ----
def _call(which, grad, cam_grad=False):
    rs = _settings((cam_grad,) * 3)
    if which == "fused":
        return rasterizer.rasterize_gaussians_fused(*_fused_inputs(grad), rs)
    return GaussianRasterizer(rs)(depth="expected" if which in ("depth", "pose-maps") else None, **_inputs(grad))


FORWARD_KW = {"plain": (), "depth": (), "pose": (), "pose-maps": (), "fused": ("raw_params", "shs_rest")}
GRAD_FN = {"plain": "_RasterizeGaussiansBackward", "depth": "_RasterizeGaussiansDepthBackward", "pose": "_RasterizeGaussiansPoseBackward",
           "pose-maps": "_RasterizeGaussiansPoseBackward", "fused": "_RasterizeGaussiansFusedBackward"}


@pytest.mark.parametrize("announced", (False, True))
@pytest.mark.parametrize("grad", (False, True))
@pytest.mark.parametrize("which", FORWARD_KW)
def test_announce_backward_is_passed_exactly_when_an_input_needs_grad_and_the_backend_announces(use, which, grad, announced):
    be = use(announced=announced)
    pose = which.startswith("pose")
    out = _call(which, grad, cam_grad=pose)
    needs = grad or pose                                         # the pose function is reached through a camera that needs grad
    kw = tuple(sorted(FORWARD_KW[which] + (("announce_backward",) if needs and announced else ())))
    assert be.calls[0] == ("forward", kw)
    assert be.forward_kw.get("announce_backward", True) is True
    assert be.calls[1:] == ([("depth_forward", 0)] if which in ("depth", "pose-maps") else [])
    assert len(out) == (4 if which in ("depth", "pose-maps") else 2)
    assert not out[1].requires_grad and out[1].grad_fn is None
    if needs:
        fn = out[0].grad_fn
        assert type(fn).__name__.startswith(GRAD_FN[which])
        assert (fn.gsr_geom_index, fn.gsr_means_index) == ((6, 0) if which == "fused" else (7, 1))
        assert fn.saved_tensors[fn.gsr_geom_index].data_ptr() == be.geom.data_ptr()
        assert tuple(fn.saved_tensors[fn.gsr_means_index].shape) == (P, 3)
    else:
        assert out[0].grad_fn is None


@pytest.mark.parametrize("which", FORWARD_KW)
def test_composited_mask_of_an_image_reaches_the_backend_with_the_saved_workspace(use, which):
    be = use()
    out = _call(which, True, cam_grad=which.startswith("pose"))
    n = len(be.calls)
    mask = rasterizer.composited_mask(out[0])
    assert be.calls[n:] == [("composited_mask", True, P)] and mask.shape == (P,)
    assert rasterizer.composited_mask().shape == (P,)                        # the most recent forward pass: the same render
    assert be.calls[n + 1:] == [("composited_mask", True, P)]


@pytest.mark.parametrize("which", ("plain", "depth", "pose"))
def test_inputs_are_checked_before_the_backend_is_called(use, which):
    be = use()
    kw = _inputs()
    kw["means3D"] = torch.ones(P, 4, requires_grad=True)
    call = lambda **k: GaussianRasterizer(_settings((which == "pose",) * 3))(depth="expected" if which == "depth" else None, **k)
    with pytest.raises(_lib.GsrError, match=r"means3D must have dimensions \(num_points, 3\)"):
        call(**kw)
    kw = _inputs()
    kw["scales"] = kw["scales"].double()
    with pytest.raises(_lib.GsrError, match="scales must be float32, got torch.float64"):
        call(**kw)
    assert be.calls == []
