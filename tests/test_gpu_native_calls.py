"""-m gpu: the library boundary.  Every public feature of the package is run once, at the smallest sizes at which its call sites
reach an edge (a NULL pointer for an absent or empty tensor, a chunked call, a skipped call), behind a proxy that forwards each
call to libgsr_hip.so and records (function, arguments).  The recorded list of every case is compared with a literal table.

Only the boundary is observed, so this file passes unchanged on any tree whose Python bindings hand the library the same calls:
the tables below were recorded on the commit before the bindings were moved onto the helpers of _lib.py (call, stream, ptr,
ptr_array, workspace), from the same libgsr_hip.so.

How an argument is written down: an int, a float or bytes as it is (sizes, byte counts and the pair count R included); a pointer as
"NULL", as "ptr", or as "<name>+<byte offset>" when it points into a tensor the case has named (so that pointers that must step
through one tensor are pinned, not only their NULL-ness); a byref as "out"; a callback as "fn"; a ctypes array as ("array",
length, run-length-encoded entries), entries of a pointer array written as pointers, entries of a struct array as tuples of their
fields.  Consecutive repeats of a block of up to three calls are folded into ("repeat", count, block).

Substitutions: none of the cases had to be changed for a validator.  The rasterizer has no unannounced route when a gradient is
wanted (every forward call that will be followed by a backward call announces it), so "with shs" is the announced route."""
import ctypes as C
import types

import pytest
import torch

from gaussian_transformer_amd import _lib, densify, loss, optim, rasterizer, rows as rows_mod, sequence, synth
from gaussian_transformer_amd.chamfer import ChamferDistance
from gaussian_transformer_amd.render import PipelineParams, TorchCamera
from simple_knn._C import distCUDA2
from tests.test_density_host import make_controller

pytestmark = pytest.mark.gpu
DEV = "cuda"
_BYREF = type(C.byref(C.c_int()))


def _rle(seq):
    out = []
    for v in seq:
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return tuple((v, n) for v, n in out)


def _fold(calls):
    """Consecutive repeats of a block of one, two or three calls as ("repeat", count, block)."""
    out, i = [], 0
    while i < len(calls):
        for p in (1, 2, 3):
            n = 1
            while calls[i + n * p:i + (n + 1) * p] == calls[i:i + p]:
                n += 1
            if n > 1:
                out.append(("repeat", n, calls[i:i + p]))
                i += n * p
                break
        else:
            out.append(calls[i])
            i += 1
    return out


class Recorder:
    """Stands in front of the loaded library: every attribute is the library's function, wrapped to note its arguments."""

    def __init__(self, lib):
        self._lib, self._raw, self._named = lib, [], []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def forward(*args):
            assert len(args) == len(fn.argtypes), name
            self._raw.append((name, args, fn.argtypes))
            return fn(*args)
        return forward

    def name(self, label, t):
        """Pointers into the memory of tensor `t` (alive during the calls that take them) are written as label+offset."""
        s = t.untyped_storage()
        self._named.append((label, s.data_ptr(), s.data_ptr() + s.nbytes()))

    def _pointer(self, v):
        if not v:
            return "NULL"
        for label, lo, hi in self._named:
            if lo <= v < hi:
                return f"{label}+{v - lo}"
        return "ptr"

    def _arg(self, a, t):
        if isinstance(a, C.Array):
            if a._type_ is C.c_void_p:
                vals = [self._pointer(v) for v in a]
            elif issubclass(a._type_, C.Structure):
                vals = [tuple(self._arg(getattr(s, f), ft) for f, ft in s._fields_) for s in a]
            else:
                vals = list(a)
            return ("array", len(a), _rle(vals))
        if isinstance(a, _BYREF):
            return "out"
        if isinstance(a, C._CFuncPtr):
            return "fn"
        if t is C.c_void_p:
            return self._pointer(a)
        return a

    def calls(self):
        return _fold([(name, tuple(self._arg(a, t) for a, t in zip(args, types_))) for name, args, types_ in self._raw])


@pytest.fixture
def rec(monkeypatch):
    r = Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: r)
    monkeypatch.setattr(rasterizer, "_backend", rasterizer.HipBackend())       # a fresh one: no binning hint, nothing announced
    return r


# ---------------------------------------------------------------- the cases ----------------------------------------------------------------

def _scene(P=8, W=20, H=18, deg=1, grad=True):
    """A seeded scene of P Gaussians at W x H (not a multiple of the tile) as the rasterizer's tensors, and its settings."""
    sc = synth.make_scene(P=P, width=W, height=H, sh_degree=deg, s0=0.05, seed=3, bg=(0.1, 0.2, 0.3))
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=DEV).requires_grad_(grad)
    inp = dict(means3D=t(sc.means3D), means2D=t(0 * sc.means3D), opacities=t(sc.opacities), shs=t(sc.shs), scales=t(sc.scales),
               rotations=t(sc.rotations))
    cam = TorchCamera(sc.camera, DEV)
    rs = rasterizer.camera_settings(cam, torch.tensor(sc.bg, device=DEV), 1.0, deg, False)
    return sc, cam, rs, inp


def _weights(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def case_raster_shs(rec):
    _, _, rs, inp = _scene()
    color, _radii = rasterizer.GaussianRasterizer(rs)(**inp)
    (color * _weights(color.shape, 1)).sum().backward()


def case_raster_precomputed(rec):
    sc, _, rs, inp = _scene()
    s2 = torch.tensor(sc.scales, device=DEV) ** 2
    z = torch.zeros_like(s2[:, 0])
    cov = torch.stack([s2[:, 0], z, z, s2[:, 1], z, s2[:, 2]], dim=1).requires_grad_(True)
    colors = torch.rand((sc.P, 3), generator=torch.Generator().manual_seed(2)).to(DEV).requires_grad_(True)
    color, _radii = rasterizer.GaussianRasterizer(rs)(means3D=inp["means3D"], means2D=inp["means2D"], opacities=inp["opacities"],
                                                      colors_precomp=colors, cov3D_precomp=cov)
    (color * _weights(color.shape, 1)).sum().backward()


def case_raster_no_gaussians(rec):
    _, _, rs, inp = _scene(P=0)
    color, _radii = rasterizer.GaussianRasterizer(rs)(**inp)
    (color * _weights(color.shape, 1)).sum().backward()


def case_raster_depth_alone(rec):
    _, _, rs, inp = _scene()
    _color, _radii, depth, _alpha = rasterizer.GaussianRasterizer(rs)(depth="expected", **inp)
    (depth * _weights(depth.shape, 3)).sum().backward()


def case_raster_depth_after_colour(rec):
    _, _, rs, inp = _scene()
    color, _radii, depth, alpha = rasterizer.GaussianRasterizer(rs)(depth="inverse", **inp)
    ((color * _weights(color.shape, 1)).sum() + (depth * _weights(depth.shape, 3)).sum() + alpha.sum()).backward()


def case_raster_pose(rec):
    _, _, rs, inp = _scene()
    rs = rs._replace(viewmatrix=rs.viewmatrix.clone().requires_grad_(True), campos=rs.campos.clone().requires_grad_(True))
    color, _radii = rasterizer.GaussianRasterizer(rs)(**inp)
    (color * _weights(color.shape, 1)).sum().backward()
    assert rs.viewmatrix.grad is not None and rs.projmatrix.grad is None and rs.campos.grad is not None


def case_raster_masks(rec):
    _, _, rs, inp = _scene()
    r = rasterizer.GaussianRasterizer(rs)
    color, _radii = r(**inp)
    assert rasterizer.composited_mask(color).shape == (8,)
    assert r.markVisible(inp["means3D"].detach()).shape == (8,)


def case_loss_l1_ssim(rec):
    img = torch.rand((3, 17, 19), generator=torch.Generator().manual_seed(4)).to(DEV).requires_grad_(True)
    gt = torch.rand((3, 17, 19), generator=torch.Generator().manual_seed(5)).to(DEV)
    loss.fused_l1_ssim_loss(img, gt).backward()


def _views(n, shape, seed, grad=()):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(shape, generator=g).to(DEV).requires_grad_(i in grad) for i in range(n)]


def case_loss_views_middle_without_grad(rec):
    imgs, gts = _views(3, (3, 17, 19), 6, grad=(0, 2)), _views(3, (3, 17, 19), 7)
    loss.multi_view_loss(imgs, gts, 0.5 / 3, 0.02 / 3).backward()


def case_loss_views_one_tensor_of_17(rec):
    imgs, gts = _views(1, (17, 3, 16, 16), 8, grad=(0,))[0], _views(1, (17, 3, 16, 16), 9)[0]
    rec.name("images", imgs)
    rec.name("targets", gts)
    loss.multi_view_loss(imgs, gts, 0.5, 0.25, sanitize=False).backward()


def case_loss_view_metrics(rec):
    loss.view_metrics(_views(2, (3, 17, 19), 10), _views(2, (3, 17, 19), 11))


def _clouds(grad2):
    g = torch.Generator().manual_seed(12)
    x1 = torch.randn((2, 5, 26), generator=g).to(DEV).requires_grad_(True)
    x2 = torch.randn((2, 3, 26), generator=g).to(DEV).requires_grad_(grad2)
    return x1, x2


def case_chamfer_dist2_unused(rec):
    d1, _d2, _i1, _i2 = ChamferDistance()(*_clouds(True))
    d1.sum().backward()


def case_chamfer_xyz2_without_grad(rec):
    d1, d2, _i1, _i2 = ChamferDistance()(*_clouds(False))
    (d1.sum() + d2.sum()).backward()


def case_box_sort_no_rows(rec):
    sequence.box_sort_rows(torch.empty((0, 26), device=DEV), 17, 4)


def case_box_sort_seven_rows(rec):
    sequence.box_sort_rows(torch.rand((7, 26), generator=torch.Generator().manual_seed(13)).to(DEV), 17, 4)


def _spy_matrices(rec, monkeypatch):
    """The [B,16] view and projection matrices visible_union_tensors uploads are named, so that the chunks' pointers are pinned."""
    orig = sequence._camera_matrices

    def spy(cameras, dev):
        view, proj = orig(cameras, dev)
        rec.name("view", view)
        rec.name("proj", proj)
        return view, proj
    monkeypatch.setattr(sequence, "_camera_matrices", spy)


def case_visible_union_65_cameras(rec, monkeypatch):
    _, cam, _, inp = _scene(grad=False)
    _spy_matrices(rec, monkeypatch)
    sequence.visible_union_tensors([cam] * 65, inp["means3D"], inp["scales"], inp["rotations"])


def case_visible_union_counts_and_radii(rec, monkeypatch):
    _, cam, _, inp = _scene(grad=False)
    _spy_matrices(rec, monkeypatch)
    _visible, radii, counts = sequence.visible_union_tensors([cam] * 65, inp["means3D"], inp["scales"], inp["rotations"],
                                                            want_radii=True, want_counts=True, want_visible=False)
    rec.name("radii", radii)
    rec.name("counts", counts)


def _rows(K, P=8, grad=False):
    """Flat rows [P, 3 K + 14] of the seeded scene's raw parameters: features, rotation, opacity, xyz, scaling, flags."""
    sc = synth.make_scene(P=P, width=16, height=16, sh_degree=1, s0=0.05, seed=3)
    t = lambda a: torch.tensor(a, dtype=torch.float32)
    op = t(sc.opacities)
    r = torch.cat((t(sc.shs[:, :K, :]).reshape(P, 3 * K), t(sc.rotations), torch.log(op / (1 - op)), t(sc.means3D),
                   torch.log(t(sc.scales)), torch.zeros((P, 3))), dim=1)
    return sc, r.to(DEV).requires_grad_(grad)


def case_rows_unpack_one_coefficient(rec):
    rows_mod.unpack_rows(_rows(1)[1])


def case_rows_unpack_four_coefficients(rec):
    rows_mod.unpack_rows(_rows(4)[1])


def _render_rows_backward(n_cameras, unused):
    sc, r = _rows(4, grad=True)
    cam = TorchCamera(sc.camera, DEV)
    out = rows_mod.render_rows([cam] * n_cameras, r, PipelineParams(), torch.zeros(3, device=DEV))
    w = _weights((3, 16, 16), 14)
    sum((img * w).sum() for b, img in enumerate(out["renders"]) if b not in unused).backward()
    assert r.grad is not None


def case_render_rows_65_cameras_one_unused(rec):
    _render_rows_backward(65, unused=(1,))


def case_render_rows_66_cameras(rec):
    _render_rows_backward(66, unused=())


def _adam_params(n, rows=4):
    g = torch.Generator().manual_seed(15)
    ps = [torch.randn((rows, 1 + i % 3), generator=g).to(DEV).requires_grad_(True) for i in range(n)]
    for p in ps:
        p.grad = torch.ones_like(p)
    return ps


def case_adam_17_tensors_and_one_without_grad(rec):
    ps = _adam_params(18)
    ps[5].grad = None
    optim.HipAdam(ps, lr=1e-3).step()


def case_sparse_adam_both_mask_kinds(rec):
    ps = _adam_params(2)
    opt = optim.HipSparseAdam(ps, lr=1e-3)
    opt.step(visibility=torch.tensor([3, 0, 1, 0], dtype=torch.int32, device=DEV))
    opt.step(visibility=torch.tensor([True, False, False, True], device=DEV))


def _density(P, opacity, scaling, accum):
    """A FusedDensityController over P hand-made Gaussians (f_rest of 3 coefficients) with optimiser state."""
    g = torch.Generator().manual_seed(16)
    n = lambda *s: torch.randn(*s, generator=g).to(DEV)
    par = {"xyz": n(P, 3), "f_dc": n(P, 1, 3), "f_rest": n(P, 3, 3), "opacity": torch.tensor(opacity, device=DEV).reshape(P, 1),
           "scaling": torch.log(torch.tensor(scaling, device=DEV)).reshape(P, 1).repeat(1, 3).contiguous(), "rotation": n(P, 4) + 0.1}
    d = {"par": par, "mom": {k: (0.01 * n(*v.shape), 1e-4 * n(*v.shape).abs()) for k, v in par.items()},
         "accum": torch.tensor(accum, device=DEV).reshape(P, 1), "denom": torch.ones((P, 1), device=DEV), "max_radii": torch.zeros(P, device=DEV)}
    return make_controller(d, cls=densify.FusedDensityController)


def _record(rec, grad_of):
    ctl = _density(6, [1.0] * 6, [0.01] * 6, [0.0] * 6)
    arena = torch.randn((6, 8), generator=torch.Generator().manual_seed(17)).to(DEV)
    rec.name("arena", arena)
    radii = torch.tensor([2, 0, 1, 0, 5, 1], dtype=torch.int32, device=DEV)
    ctl.record(types.SimpleNamespace(grad=grad_of(arena)), None, radii)
    ctl.record(types.SimpleNamespace(grad=grad_of(arena)), radii > 0, radii)


def case_density_record_view_into_arena(rec):
    _record(rec, lambda arena: arena[:, 2:5])                # [P,3], row stride 8, unit column stride: read in place


def case_density_record_copy_needed(rec):
    _record(rec, lambda arena: arena[:, 0:6:2])              # column stride 2: copied to [P,2] first


def case_densify_clone_split_prune(rec):
    """Row 0 is cloned (large gradient, small), row 1 split (large gradient, large), row 2 pruned (transparent)."""
    ctl = _density(6, [1.0, 1.0, -8.0, 1.0, 1.0, 1.0], [0.01, 0.1, 0.01, 0.01, 0.01, 0.01], [0.01, 0.01, 0.0, 0.0, 0.0, 0.0])
    with torch.no_grad():
        out = ctl.densify_and_prune(0.0002, 0.005, 4.0, None, generator=torch.Generator(device=DEV).manual_seed(5))
    assert out == {"cloned": 1, "split": 1, "pruned": 1} and ctl.model._xyz.shape[0] == 7


def case_densify_nothing_survives(rec):
    ctl = _density(3, [-8.0] * 3, [0.01] * 3, [0.0] * 3)
    with torch.no_grad():
        out = ctl.densify_and_prune(0.0002, 0.005, 4.0, None, generator=torch.Generator(device=DEV).manual_seed(5))
    assert out == {"cloned": 0, "split": 0, "pruned": 3} and ctl.model._xyz.shape[0] == 0


def case_knn_no_points_then_five(rec):
    distCUDA2(torch.empty((0, 3), device=DEV))
    distCUDA2(torch.randn((5, 3), generator=torch.Generator().manual_seed(18)).to(DEV))


CASES = {k[len("case_"):]: v for k, v in sorted(globals().items()) if k.startswith("case_")}


# ---------------------------------------------------------------- the tables ----------------------------------------------------------------
# Recorded on the commit before the bindings moved onto the helpers, on an MI355X.  Byte counts and R are the library's.

PTR, NULL, OUT = "ptr", "NULL", "out"
TANX, TANY = 0.5773502691896257, 0.5196152422706631          # 20 x 18 (the 16 x 16 cameras have TANX twice)
TANX32, TANY32 = 0.5773502588272095, 0.5196152329444885      # the same as the c_float entries of gsr_visible_union's host arrays
GEOM, GEOM_P0, IMG, IMG16, BWD_WS, DEPTH_WS = 16952320, 16951808, 1154816, 1153792, 81920, 66816
LR32 = 0.0010000000474974513


def _all(n, v):
    return ("array", n, ((v, n),))


def _steps(label, n, stride):
    return ("array", n, tuple((f"{label}+{b * stride}", 1) for b in range(n)))


def _forward(M, shs, colors, scales_rots, cov, P=8, geom=GEOM):
    g = PTR if P else NULL             # P = 0: every per-Gaussian tensor is empty
    return ("gsr_forward", (NULL, P, 1, M, 20, 18, PTR, g, shs, colors, g, scales_rots, 1.0, scales_rots, cov, PTR, PTR, PTR, TANX, TANY, 0, 0,
                            PTR, g, PTR, geom, "fn", NULL, PTR, IMG, OUT, NULL, 0))


SIZES = ("gsr_workspace_sizes", (8, 20, 18, OUT, OUT, OUT))
PREFILL_SHS = ("gsr_backward_prefill", (8, 4, PTR, PTR, NULL, PTR, NULL, PTR, PTR, PTR, NULL))
FORWARD_SHS = _forward(4, PTR, NULL, PTR, NULL)
BACKWARD_SIZE = ("gsr_backward_workspace_bytes", (8, 9, OUT))
BACKWARD_SHS = ("gsr_backward", (NULL, 8, 1, 4, 9, 20, 18, PTR, PTR, PTR, PTR, NULL, PTR, 1.0, PTR, NULL, PTR, PTR, PTR, TANX, TANY, PTR,
                                 PTR, GEOM, PTR, 512, PTR, IMG, PTR, BWD_WS,
                                 PTR, PTR, NULL, PTR, NULL, PTR, PTR, PTR,          # means2D opacity colors means3D cov3D sh scales rots
                                 0, NULL, 0, NULL))
DEPTH_SIZE = ("gsr_depth_workspace_bytes", (8, OUT))


def _depth_forward(mode):
    return ("gsr_depth_forward", (NULL, 8, 20, 18, 9, mode, PTR, GEOM, PTR, 512, PTR, IMG, PTR, PTR))


def _depth_backward(mode, grad_alpha, accumulate):
    return ("gsr_depth_backward", (NULL, 8, 20, 18, 9, mode, PTR, PTR, PTR, 1.0, PTR, NULL, PTR, PTR, PTR, TANX, TANY, PTR, grad_alpha,
                                   PTR, GEOM, PTR, 512, PTR, IMG, PTR, DEPTH_WS, accumulate, PTR, PTR, PTR, NULL, PTR, PTR))


ROWS_UNPACK = ("gsr_rows_unpack", (NULL, 8, 26, PTR, PTR, PTR, PTR, PTR, PTR, PTR))
ROWS_SIZES = ("gsr_workspace_sizes", (8, 16, 16, OUT, OUT, OUT))
ROWS_FORWARD = ("gsr_forward", (NULL, 8, 1, 4, 16, 16, PTR, PTR, PTR, NULL, PTR, PTR, 1.0, PTR, NULL, PTR, PTR, PTR, TANX, TANX, 0, 0,
                                PTR, PTR, PTR, GEOM, "fn", NULL, PTR, IMG16, OUT, PTR, 1))
ROWS_BACKWARD_SIZE = ("gsr_backward_workspace_bytes", (8, 8, OUT))


def _rows_backward(binning_bytes):
    """512: what the library asked for; 4633: the buffer set aside from the hint of the camera before (512 * 1.05 + 4096)."""
    return ("gsr_backward", (NULL, 8, 1, 4, 8, 16, 16, PTR, PTR, PTR, PTR, NULL, PTR, 1.0, PTR, NULL, PTR, PTR, PTR, TANX, TANX, PTR,
                             PTR, GEOM, PTR, binning_bytes, PTR, IMG16, PTR, BWD_WS, PTR, PTR, NULL, PTR, NULL, PTR, PTR, PTR, 0, PTR, 1, PTR))


def _pack(n):
    return ("gsr_rows_grad_pack", (NULL, 8, 26, n, _all(n, PTR), PTR))


def _union(n, offset, radii, visible, counts):
    return ("gsr_visible_union", (NULL, 8, n, PTR, PTR, 1.0, PTR, NULL, 0, f"view+{offset}", f"proj+{offset}",
                                  _all(n, TANX32), _all(n, TANY32), _all(n, 20), _all(n, 18), radii, visible, counts))


def _adam_groups(numels, step=1):
    return ("array", len(numels), tuple(((PTR, PTR, PTR, PTR, n, LR32, step), 1) for n in numels))


def _views_loss(which, B, H, W, imgs, gts, w_l1, w_ssim, sanitize, ws_bytes, grads=None):
    tail = (PTR, PTR, PTR, ws_bytes) if which == "forward" else (PTR, PTR, ws_bytes, grads)
    return (f"gsr_views_loss_{which}", (NULL, B, H, W, imgs, gts, w_l1, w_ssim, sanitize) + tail)


def _densify_plan(P):
    return ("gsr_densify_plan", (NULL, P, PTR, PTR, PTR, PTR, 0.00019999999494757503, 0.004999999888241291, 0.03999999910593033, -1.0, 2,
                                 PTR, PTR, 4352))


def _density_group(width, role):
    return ((PTR, PTR, PTR, PTR, PTR, PTR, width, role), 1)


IMAGES17, TARGETS17 = _steps("images", 17, 3072), _steps("targets", 17, 3072)         # 3 * 16 * 16 floats apart

EXPECTED = {
    "raster_shs": [SIZES, PREFILL_SHS, FORWARD_SHS, BACKWARD_SIZE, BACKWARD_SHS],
    "raster_precomputed": [
        SIZES,
        ("gsr_backward_prefill", (8, 0, PTR, PTR, PTR, PTR, PTR, NULL, NULL, NULL, NULL)),
        _forward(0, NULL, PTR, NULL, PTR),
        BACKWARD_SIZE,
        ("gsr_backward", (NULL, 8, 1, 0, 9, 20, 18, PTR, PTR, PTR, NULL, PTR, NULL, 1.0, NULL, PTR, PTR, PTR, PTR, TANX, TANY, PTR,
                          PTR, GEOM, PTR, 512, PTR, IMG, PTR, BWD_WS,
                          PTR, PTR, PTR, PTR, PTR, NULL, NULL, NULL,
                          0, NULL, 0, NULL))],
    "raster_no_gaussians": [
        ("gsr_workspace_sizes", (0, 20, 18, OUT, OUT, OUT)),
        _forward(0, NULL, NULL, NULL, NULL, P=0, geom=GEOM_P0),
        ("gsr_backward_workspace_bytes", (0, 0, OUT)),
        ("gsr_backward", (NULL, 0, 1, 0, 0, 20, 18, PTR, NULL, NULL, NULL, NULL, NULL, 1.0, NULL, NULL, PTR, PTR, PTR, TANX, TANY, PTR,
                          PTR, GEOM_P0, NULL, 0, PTR, IMG, PTR, 66048,
                          NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL,
                          0, NULL, 0, NULL))],
    "raster_depth_alone": [SIZES, PREFILL_SHS, FORWARD_SHS, _depth_forward(0), DEPTH_SIZE, _depth_backward(0, NULL, 0)],
    "raster_depth_after_colour": [SIZES, PREFILL_SHS, FORWARD_SHS, _depth_forward(1), BACKWARD_SIZE, BACKWARD_SHS, DEPTH_SIZE,
                                  _depth_backward(1, PTR, 1)],
    "raster_pose": [
        SIZES, PREFILL_SHS, FORWARD_SHS, BACKWARD_SIZE, BACKWARD_SHS,
        ("gsr_pose_workspace_bytes", (8, OUT)),
        ("gsr_pose_backward", (NULL, 0, 8, 1, 4, 20, 18, 9, PTR, PTR, PTR, NULL, PTR, 1.0, PTR, NULL, PTR, PTR, PTR, TANX, TANY,
                               PTR, GEOM, PTR, BWD_WS, PTR, 256, PTR, NULL, PTR))],
    "raster_masks": [SIZES, PREFILL_SHS, FORWARD_SHS,
                     ("gsr_composited_mask", (NULL, 8, PTR, GEOM, PTR)),
                     ("gsr_mark_visible", (NULL, 8, PTR, PTR, PTR, PTR))],
    "loss_l1_ssim": [("gsr_l1_ssim_workspace", (3, 17, 19, OUT)),
                     ("gsr_l1_ssim_forward", (NULL, 3, 17, 19, PTR, PTR, 0.2, PTR, PTR, 12032)),
                     ("gsr_l1_ssim_backward", (NULL, 3, 17, 19, PTR, PTR, 0.2, PTR, PTR, 12032, PTR))],
    "loss_views_middle_without_grad": [
        ("gsr_views_loss_workspace", (3, 17, 19, OUT)),
        _views_loss("forward", 3, 17, 19, _all(3, PTR), _all(3, PTR), 0.16666666666666666, 0.006666666666666667, 1, 36096),
        _views_loss("backward", 3, 17, 19, _all(3, PTR), _all(3, PTR), 0.16666666666666666, 0.006666666666666667, 1, 36096,
                    ("array", 3, ((PTR, 1), (NULL, 1), (PTR, 1))))],
    "loss_views_one_tensor_of_17": [
        ("gsr_views_loss_workspace", (17, 16, 16, OUT)),
        _views_loss("forward", 17, 16, 16, IMAGES17, TARGETS17, 0.5, 0.25, 0, 158208),
        _views_loss("backward", 17, 16, 16, IMAGES17, TARGETS17, 0.5, 0.25, 0, 158208, _all(17, PTR))],
    "loss_view_metrics": [("gsr_views_loss_workspace", (2, 17, 19, OUT)),
                          _views_loss("forward", 2, 17, 19, _all(2, PTR), _all(2, PTR), 0.0, 0.0, 0, 24320)],
    "chamfer_dist2_unused": [
        ("gsr_chamfer_workspace", (2, 5, 3, OUT)),
        ("gsr_chamfer_forward", (NULL, 2, 5, 3, 26, PTR, PTR, PTR, PTR, PTR, PTR, PTR, 128)),
        ("gsr_chamfer_backward", (NULL, 2, 5, 3, 26, PTR, PTR, PTR, PTR, PTR, NULL, PTR, PTR))],
    "chamfer_xyz2_without_grad": [
        ("gsr_chamfer_workspace", (2, 5, 3, OUT)),
        ("gsr_chamfer_forward", (NULL, 2, 5, 3, 26, PTR, PTR, PTR, PTR, PTR, PTR, PTR, 128)),
        ("gsr_chamfer_backward", (NULL, 2, 5, 3, 26, PTR, PTR, PTR, PTR, PTR, PTR, PTR, NULL))],
    "box_sort_no_rows": [("gsr_box_sort_workspace", (0, 4, OUT)),
                         ("gsr_box_sort", (NULL, 0, 26, NULL, 17, 4, NULL, NULL, PTR, PTR, 1024))],
    "box_sort_seven_rows": [("gsr_box_sort_workspace", (7, 4, OUT)),
                            ("gsr_box_sort", (NULL, 7, 26, PTR, 17, 4, PTR, PTR, PTR, PTR, 1024))],
    "visible_union_65_cameras": [_union(64, 0, NULL, PTR, NULL), _union(1, 4096, NULL, PTR, NULL)],          # 64 matrices of 64 bytes
    "visible_union_counts_and_radii": [_union(64, 0, "radii+0", NULL, "counts+0"),
                                       _union(1, 4096, "radii+2048", NULL, "counts+256")],               # 64 * P * 4 and 64 * 4 bytes on
    "rows_unpack_one_coefficient": [("gsr_rows_unpack", (NULL, 8, 17, PTR, PTR, PTR, NULL, PTR, PTR, PTR))],
    "rows_unpack_four_coefficients": [ROWS_UNPACK],
    "render_rows_65_cameras_one_unused": [
        ROWS_UNPACK, ROWS_SIZES, ("repeat", 65, [ROWS_FORWARD]),
        ROWS_BACKWARD_SIZE, _rows_backward(512), ("repeat", 63, [ROWS_BACKWARD_SIZE, _rows_backward(4633)]),
        _pack(64)],
    "render_rows_66_cameras": [
        ROWS_UNPACK, ROWS_SIZES, ("repeat", 66, [ROWS_FORWARD]),
        ROWS_BACKWARD_SIZE, _rows_backward(512), ("repeat", 65, [ROWS_BACKWARD_SIZE, _rows_backward(4633)]),
        _pack(64), _pack(2)],
    "adam_17_tensors_and_one_without_grad": [
        ("gsr_adam_step", (NULL, 16, _adam_groups([4, 8, 12, 4, 8, 4, 8, 12, 4, 8, 12, 4, 8, 12, 4, 8]), 0.9, 0.999, 1e-08)),
        ("gsr_adam_step", (NULL, 1, _adam_groups([12]), 0.9, 0.999, 1e-08))],
    "sparse_adam_both_mask_kinds": [
        ("gsr_adam_step_masked", (NULL, 2, _adam_groups([4, 8]), 0.9, 0.999, 1e-08, 4, PTR, 1)),                # int32: the radii
        ("gsr_adam_step_masked", (NULL, 2, _adam_groups([4, 8], step=2), 0.9, 0.999, 1e-08, 4, PTR, 0))],       # bool: bytes
    "density_record_view_into_arena": [
        ("gsr_density_record", (NULL, 6, "arena+8", 8, PTR, NULL, PTR, PTR, PTR)),
        ("gsr_density_record", (NULL, 6, "arena+8", 8, PTR, PTR, PTR, PTR, PTR))],
    "density_record_copy_needed": [
        ("gsr_density_record", (NULL, 6, PTR, 2, PTR, NULL, PTR, PTR, PTR)),
        ("gsr_density_record", (NULL, 6, PTR, 2, PTR, PTR, PTR, PTR, PTR))],
    "densify_clone_split_prune": [
        ("gsr_densify_plan_workspace", (6, 2, OUT)),
        _densify_plan(6),
        ("gsr_densify_apply", (NULL, 6, 2, 1, 7, 6,
                               ("array", 6, (_density_group(3, 1), _density_group(3, 0), _density_group(9, 0), _density_group(1, 0),
                                             _density_group(3, 2), _density_group(4, 0))),
                               PTR, PTR, PTR, PTR, 4352))],
    "densify_nothing_survives": [("gsr_densify_plan_workspace", (3, 2, OUT)), _densify_plan(3)],
    "knn_no_points_then_five": [
        ("gsr_knn_workspace", (0, OUT)), ("gsr_knn_mean_dist2", (NULL, 0, NULL, NULL, PTR, 1792)),
        ("gsr_knn_workspace", (5, OUT)), ("gsr_knn_mean_dist2", (NULL, 5, PTR, PTR, PTR, 1792))],
}


@pytest.mark.parametrize("name", list(CASES))
def test_the_library_receives_the_recorded_calls(name, rec, monkeypatch):
    case = CASES[name]
    case(rec, monkeypatch) if case.__code__.co_argcount == 2 else case(rec)
    torch.cuda.synchronize()
    assert rec.calls() == EXPECTED[name]
