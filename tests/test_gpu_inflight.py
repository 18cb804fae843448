"""-m gpu: several renders in flight before one backward pass -- the trainer's step (B cameras: prediction with gradients, target
without, clamp(nan_to_num(image)) into a batch tensor, ONE backward) -- against the float64 oracle per render, against each render
done alone bit for bit (deterministic reverse pass), and the shared leaves' .grad against the float64 sum of the lone gradients.
Step builder and expectations: tests/inflight.py (their proof of teeth: tests/test_inflight_host.py).  Cases by letter:
A stock default, B dense stage with live announcements, C backward orders, D a no_grad block in the middle, E rejected calls in the
middle, F the fused path mixed in, G side streams, H segment options, I gradient arenas, J stale composited marks."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib, synth
from gaussian_transformer_amd.camera import look_at_camera
from tests import inflight as fl

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


@contextlib.contextmanager
def options(**kw):
    """Library options for the duration of a case; every one of them, and the device's adaptive depth map, restored afterwards."""
    saved = {k: _lib.get_option(k) for k in set(kw) | {"depth_log_map"}}
    try:
        for k, v in kw.items():
            _lib.set_option(k, v)
        yield
    finally:
        for k, v in saved.items():
            _lib.set_option(k, v)


@pytest.fixture(scope="module")
def fx():
    return fl.Fixture(DEV)


def _poison_allocator(fx):
    """Blocks of the gradient tensors' sizes, filled with NaN and handed back to torch's caching allocator: a zero-fill that was
    skipped, or a gradient written into a freed and reused announced tensor, shows."""
    P = fx.scenes["pred"].P
    blocks = [torch.full((P * n,), NAN, device=DEV) for n in (3, 3, 48, 1, 3, 4) for _ in range(6)]
    torch.cuda.synchronize()
    del blocks


def _det_case(fx, tag, opts, path=None, poison=False, check_step=None, **step_kw):
    """Expectations 1 and 2 on per-render leaf copies, 3 on shared leaves, under the deterministic reverse pass and `opts`."""
    with options(deterministic_bwd=1, **opts):
        lones = [fx.lone("pred", i) for i in range(fl.B)]
        if poison:
            _poison_allocator(fx)
        step = fl.run_step(fx, shared=False, **step_kw)
        torch.cuda.synchronize()
        if path is not None:
            assert _lib.get_option("pergauss_path") == path, (tag, _lib.get_option("pergauss_path"))
        if poison:
            _poison_allocator(fx)
        shared = fl.run_step(fx, shared=True, **step_kw)
    fl.expect_step_parity(fx, step, tag)
    for i in range(fl.B):
        fl.expect_bit_equal(lones[i], step["renders"][i], f"{tag} render {i}")
    if step["again"] is not None:
        fl.expect_bit_equal(lones[0], dict(step["renders"][0], grads=step["again"]), f"{tag} second backward of render 0")
    fl.expect_shared_sum(lones, shared, tag)
    if check_step is not None:
        check_step(step)


# ---- A ------------------------------------------------------------------------------------------------------------------------------
def test_a_stock_default_in_reference_order(fx):
    """Default options (streaming per-Gaussian kernel at this P, atomics): expectation 1 for all B renders and the targets between
    them; the composited masks of the B live renders differ pairwise, belong to their render, and cover every gradient."""
    from gaussian_transformer_amd.rasterizer import composited_mask
    masks = []

    def grab(live):
        masks.extend(composited_mask(r["color"]).cpu().numpy() for r in live)
    step = fl.run_step(fx, shared=False, before_backward=grab)
    assert _lib.get_option("pergauss_path") == 2                     # streaming kernel, LDS tile for the dL/dshs rows
    fl.expect_step_parity(fx, step, "A")
    for i in range(fl.B):
        for j in range(i + 1, fl.B):
            assert (masks[i] != masks[j]).sum() > 50, (i, j)
        g = step["renders"][i]["grads"]
        has = (step["renders"][i]["radii"] > 0) & np.any([np.abs(g[k]).reshape(len(masks[i]), -1).max(axis=1) > 0 for k in fl.GRADS], axis=0)
        assert has.sum() > 200 and not (has & ~masks[i].astype(bool)).any(), i
    shared = fl.run_step(fx, shared=True)
    for k, v in shared["shared"].items():
        assert np.isfinite(v).all() and np.abs(v).max() > 0, k


# ---- B ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at", [1, 2, 0])
def test_b_dense_stage_with_live_announcements(fx, at):
    """dense_pergauss = 1: every prediction forward announces its gradient tensors, the next forward call drops the announcement,
    only the step's last render can hand a prefilled set to its backward call (target first, so that the step ends with a
    prediction render) -- on an allocator whose free blocks hold NaN."""
    from gaussian_transformer_amd.rasterizer import get_backend
    be = get_backend()
    seen = []
    _det_case(fx, f"B prefill_at={at}", dict(dense_pergauss=1, prefill_at=at), path=3, poison=True, target_first=True,
              before_backward=lambda live: seen.append(0 in be._announced))
    assert seen == [True, True]                                        # an announcement was live when backward began
    # and in the reference's order (a target render last: no announcement survives)
    _det_case(fx, f"B prefill_at={at} target last", dict(dense_pergauss=1, prefill_at=at), path=3, poison=True)


# ---- C, D ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["one", "forward", "retain"])
def test_c_backward_orders(fx, order):
    _det_case(fx, f"C {order}", {}, path=2, order=order)


def test_d_no_grad_block_in_the_middle(fx):
    logged = []
    _det_case(fx, "D", {}, middle=lambda: logged.append(fl.forward_only(fx, "logged")))
    for run in logged:
        for i in range(fl.B):
            fl.expect_forward_only(fx, "logged", i, run[i], "D")


# ---- raw C ABI calls with the caller's own workspaces -------------------------------------------------------------------------------
def _p(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


class _Raw:
    """gsr_forward / gsr_backward through ctypes on workspaces the caller owns."""

    def __init__(self, sc, cam):
        from gaussian_transformer_amd.rasterizer import get_backend
        self.be = get_backend()
        t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)
        self.P, self.M, self.D = sc.P, int(sc.shs.shape[1]), sc.sh_degree
        self.W, self.H = cam.image_width, cam.image_height
        self.x = dict(means3D=t(sc.means3D), shs=t(sc.shs), opac=t(sc.opacities.reshape(-1)), scales=t(sc.scales), rots=t(sc.rotations), bg=t(sc.bg))
        self.sizes = self.be._sizes(self.P, self.W, self.H)
        self.set_camera(cam)

    def set_camera(self, cam):
        t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)
        self.cam = dict(vm=t(cam.world_view_transform), pm=t(cam.full_proj_transform), cp=t(cam.camera_center), tx=cam.tanfovx, ty=cam.tanfovy)

    def workspace(self, fill=0):
        return torch.full((self.sizes[0],), fill, dtype=torch.uint8, device=DEV)

    def forward(self, geom, alloc=None):
        x, c = self.x, self.cam
        color = torch.empty((3, self.H, self.W), device=DEV)
        radii = torch.empty((self.P,), dtype=torch.int32, device=DEV)
        img = torch.empty((self.sizes[1],), dtype=torch.uint8, device=DEV)
        held = []

        def torch_alloc(_user, nbytes):
            held.append(torch.empty((max(int(nbytes), 1),), dtype=torch.uint8, device=DEV))
            return held[-1].data_ptr()
        cb = _lib.ALLOC_FN(alloc if alloc is not None else torch_alloc)
        n = C.c_int64(0)
        rc = self.be.lib.gsr_forward(torch.cuda.current_stream().cuda_stream, self.P, self.D, self.M, self.W, self.H, _p(x["bg"]), _p(x["means3D"]),
                                     _p(x["shs"]), None, _p(x["opac"]), _p(x["scales"]), 1.0, _p(x["rots"]), None, _p(c["vm"]), _p(c["pm"]), _p(c["cp"]),
                                     c["tx"], c["ty"], 0, 0, color.data_ptr(), radii.data_ptr(), geom.data_ptr(), geom.numel(), cb, None,
                                     img.data_ptr(), img.numel(), C.byref(n), None, 0)
        return rc, dict(n=int(n.value), color=color, radii=radii, geom=geom, img=img, binning=held[0] if held else None)

    def backward(self, f, dL):
        x, c = self.x, self.cam
        bbs = C.c_size_t()
        _lib.check(self.be.lib.gsr_backward_workspace_bytes(self.P, f["n"], C.byref(bbs)), "gsr_backward_workspace_bytes")
        ws = torch.empty((bbs.value,), dtype=torch.uint8, device=DEV)
        g = self.be._gradient_outputs(torch.device(DEV, torch.cuda.current_device()), self.P, self.M, 0, True, False, False, None)
        g_means3D, g_means2D, g_sh, _, g_opacity, g_scales, g_rots, _, _ = g
        rc = self.be.lib.gsr_backward(torch.cuda.current_stream().cuda_stream, self.P, self.D, self.M, f["n"], self.W, self.H, _p(x["bg"]), _p(x["means3D"]),
                                      _p(f["radii"]), _p(x["shs"]), None, _p(x["scales"]), 1.0, _p(x["rots"]), None, _p(c["vm"]), _p(c["pm"]), _p(c["cp"]),
                                      c["tx"], c["ty"], _p(dL), _p(f["geom"]), f["geom"].numel(), _p(f["binning"]), 0 if f["binning"] is None else f["binning"].numel(),
                                      _p(f["img"]), f["img"].numel(), _p(ws), ws.numel(), _p(g_means2D), _p(g_opacity), None, _p(g_means3D), None,
                                      _p(g_sh), _p(g_scales), _p(g_rots), 0, None, 0, None)
        _lib.check(rc, "gsr_backward")
        return dict(means3D=g_means3D, means2D=g_means2D, shs=g_sh, opacities=g_opacity, scales=g_scales, rotations=g_rots)

    def mask(self, f):
        return self.be.composited_mask(f["geom"], self.P)


# ---- E ------------------------------------------------------------------------------------------------------------------------------
def test_e_rejected_calls_in_the_middle(fx):
    """Two calls the library refuses on the host, caught as the trainer catches RuntimeError, between the forwards of a step: an
    invalid argument (SH degree 4, through the backend) and an allocation failure (gsr_forward through ctypes with an allocator
    that returns NULL -- that one returns after kernels were queued).  The pending backward passes and the next whole step must
    still meet expectations 1 and 2, and gsr_last_error() carries the text."""
    from gaussian_transformer_amd import GaussianRasterizer
    raw = _Raw(fx.scenes["logged"], fx.cams[2])
    lib = raw.be.lib
    errors = []

    def reject(i):
        if i == 1:
            try:
                with torch.no_grad():
                    lv = fx.fixed_leaves("target")
                    GaussianRasterizer(raster_settings=fx.settings("target", i)._replace(sh_degree=4))(
                        means2D=torch.zeros_like(lv["means3D"]), **lv)
                errors.append(None)
            except RuntimeError as e:
                errors.append((str(e), lib.gsr_last_error().decode()))
        if i == 2:
            rc, f = raw.forward(raw.workspace(), alloc=lambda _u, _n: None)
            errors.append((rc, f["n"], lib.gsr_last_error().decode()))
    _det_case(fx, "E", {}, after_render=reject)
    assert len(errors) == 4                                            # two steps (per-render and shared leaves), two refusals each
    for inv, alc in (errors[:2], errors[2:]):
        assert inv is not None and "code 1" in inv[0] and "SH degree 4" in inv[0] and "SH degree 4" in inv[1], inv
        assert alc[0] == 2 and alc[1] > 0 and "binning allocator returned NULL" in alc[2], alc
    _det_case(fx, "E next step", {})                                  # the next whole step


# ---- F ------------------------------------------------------------------------------------------------------------------------------
def test_f_fused_path_mixed_in():
    """Renders 0 and 2 through render(), 1 and 3 through render_fused(), clamp(nan_to_num(image)) into a batch tensor, one
    backward (tests/inflight.MixedStep).  In training the two reach the raw leaves differently: render()'s gradient through
    torch's activation autograd, render_fused()'s written by the kernels.  Per-render GaussianParams copies: every render, of
    either kind, under assert_parity against the float64 chain of tests/fused_ref.py (expectation 1) and bit for bit against the
    same call done alone (2).  ONE GaussianParams for all four: .grad of every raw leaf against the float64 sum of the lone
    gradients within (B - 1) * 2^-24 * sum |g_i| (3)."""
    mx = fl.MixedStep(DEV, ("render", "fused", "render", "fused"))
    with options(deterministic_bwd=1):
        lones = [mx.lone(i) for i in range(fl.B)]
        step = mx.step(shared=False)
        torch.cuda.synchronize()
        assert _lib.get_option("pergauss_path") == 2                   # the last backward call is render 0's: unsplit rows, LDS tile
        shared = mx.step(shared=True)
    for i in range(fl.B):
        fl.expect_raw_parity(mx, i, step["renders"][i], "F")
        fl.expect_bit_equal(lones[i], step["renders"][i], f"F render {i}", keys=fl.RAW)
    fl.expect_shared_sum(lones, shared, "F", keys=fl.RAW, bounds=dict(rotation=mx.rotation_sum_bound(lones)))
    # the two kinds of call did differ (another rounding of the activations), and agree as two float32 evaluations do
    d = np.abs(lones[0]["grads"]["opacity"] - mx.orc[0].raw32["opacity"]).max()
    assert d > 0


# ---- G ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["whole_step", "forwards_only"])
def test_g_side_stream(fx, variant):
    """The whole step on a side stream; or the forwards there and the backward on the default stream after wait_stream."""
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    if variant == "whole_step":
        with torch.cuda.stream(side):
            _det_case(fx, "G whole step", dict(dense_pergauss=1), path=3)
        return
    ctx = contextlib.ExitStack()

    def enter():
        ctx.enter_context(torch.cuda.stream(side))

    def leave(_live):
        ctx.close()
        torch.cuda.current_stream().wait_stream(side)
    with options(deterministic_bwd=1, dense_pergauss=1):
        lones = [fx.lone("pred", i) for i in range(fl.B)]
        steps = []
        for shared in (False, True):
            enter()
            try:
                steps.append(fl.run_step(fx, shared=shared, before_backward=leave))
            finally:
                ctx.close()
            side.synchronize()
    assert _lib.get_option("pergauss_path") == 3
    fl.expect_step_parity(fx, steps[0], "G forwards on the side stream")
    for i in range(fl.B):
        fl.expect_bit_equal(lones[i], steps[0]["renders"][i], f"G render {i}")
    fl.expect_shared_sum(lones, steps[1], "G")


# ---- H ------------------------------------------------------------------------------------------------------------------------------
def test_h_segment_options(fx):
    """persistent_bwd = 1, segment_entries = 64 for the whole step: every render's checkpoints live in its own image workspace.
    With atomics (checkpoints are taken: expectation 1) and with the deterministic reverse pass (2 and 3)."""
    with options(persistent_bwd=1, segment_entries=64):
        step = fl.run_step(fx, shared=False)
    fl.expect_step_parity(fx, step, "H")
    _det_case(fx, "H deterministic", dict(persistent_bwd=1, segment_entries=64), path=2)


# ---- I ------------------------------------------------------------------------------------------------------------------------------
def test_i_gradient_arenas_with_renders_in_flight(fx):
    """Supported: an arena per render in flight (the second camera into a scratch arena, then add_).  Not supported: ONE arena
    around the forward calls of several renders that all wait for their backward -- their gradient views are the same memory
    (every .grad would show the render that ran backward last; shared leaves would add a tensor to itself): refused with a GsrError
    at the second forward call, through the fused entry point too, and the first render is unharmed.  The claim ends with the
    owner's backward call, or with its graph if that call never comes."""
    from gaussian_transformer_amd.rasterizer import arena_floats, gradient_arena, rasterize_gaussians_fused
    P = fx.scenes["pred"].P
    n = arena_floats(P, 16)
    order = ("means3D", "shs", "opacities", "scales", "rotations")
    flat = lambda g: np.concatenate([g[k].reshape(-1) for k in order])
    with options(deterministic_bwd=1, dense_pergauss=1):
        lones = [fx.lone("pred", i) for i in range(2)]
        # dL/dshs sits 3 P floats into an arena: the dense stage needs it 16-byte aligned, so the arena starts (-3 P) mod 4 floats in
        pad = (-3 * P) % 4
        stores = [torch.full((n + 8,), NAN, device=DEV) for _ in range(3)]
        arenas = [st[pad:pad + n] for st in stores[:2]]
        live = []
        for i in range(2):
            with gradient_arena(arenas[i]):
                lv = fx.leaves("pred", True)
                color, radii, m2 = fx.render("pred", i, lv)
            live.append((lv, color, m2))
        for i in (1, 0):
            lv, color, m2 = live[i]
            with gradient_arena(arenas[i]):
                g = torch.autograd.grad(torch.clamp(torch.nan_to_num(color), 0.0, 1.0), [lv[k] for k in order], grad_outputs=fx.t(fx.dL[i]))
            assert g[0].data_ptr() == arenas[i].data_ptr()
            assert _lib.get_option("pergauss_path") == 3
        each = [a.cpu().numpy() for a in arenas]
        arenas[0].add_(arenas[1])
        total = arenas[0].cpu().numpy()
        # ---- ONE arena around both forward calls
        one = stores[2][pad:pad + n]
        with gradient_arena(one):
            lv0 = fx.leaves("pred", True)
            c0, _, m20 = fx.render("pred", 0, lv0)
            with pytest.raises(_lib.GsrError, match="gradient arena is still owned by another render in flight"):
                fx.render("pred", 1, fx.leaves("pred", True))
            with pytest.raises(_lib.GsrError, match="gradient arena is still owned by another render in flight"):
                lvf = fx.leaves("pred", True)
                rasterize_gaussians_fused(lvf["means3D"], torch.zeros_like(lvf["means3D"]), lvf["shs"][:, :1], lvf["shs"][:, 1:], lvf["opacities"],
                                          lvf["scales"], lvf["rotations"], fx.settings("pred", 1))
            torch.clamp(torch.nan_to_num(c0), 0.0, 1.0).backward(fx.t(fx.dL[0]))
            first = one.cpu().numpy()
            # its backward call has run: the arena is free for the next render (whose forward call zero-fills it again)
            c1, _, _ = fx.render("pred", 1, fx.leaves("pred", True))
            torch.clamp(torch.nan_to_num(c1), 0.0, 1.0).backward(fx.t(fx.dL[1]))
            second = one.cpu().numpy()
            # a render with gradients that is dropped without a backward call: its claim goes with its graph
            c0, _, _ = fx.render("pred", 0, fx.leaves("pred", True))
            with pytest.raises(_lib.GsrError, match="gradient arena is still owned by another render in flight"):
                fx.render("pred", 1, fx.leaves("pred", True))
            del c0
            c1, _, _ = fx.render("pred", 1, fx.leaves("pred", True))
            torch.clamp(torch.nan_to_num(c1), 0.0, 1.0).backward(fx.t(fx.dL[1]))
            after_drop = one.cpu().numpy()
    for i in range(2):
        assert np.array_equal(each[i], flat(lones[i]["grads"])), i
    a, b = flat(lones[0]["grads"]).astype(np.float64), flat(lones[1]["grads"]).astype(np.float64)
    assert np.all(np.abs(total - (a + b)) <= 2.0 ** -24 * (np.abs(a) + np.abs(b)))         # one float32 addition
    assert np.array_equal(first, flat(lones[0]["grads"])) and np.array_equal(second, flat(lones[1]["grads"]))
    assert np.array_equal(after_drop, flat(lones[1]["grads"]))
    for st in stores:
        assert bool(torch.isnan(st[:pad]).all()) and bool(torch.isnan(st[pad + n:]).all()), "written outside an arena"


# ---- J ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stale", ["constant_byte", "previous_camera"])
def test_j_stale_composited_marks(stale):
    """The `touched` bytes of a geometry workspace are never cleared and the frame mark cycles through 1..255: a workspace that held
    the constant byte v everywhere, reused for 256 consecutive frames, meets a frame whose mark is v; a workspace that holds another
    camera's marks from exactly 255 frames earlier meets that mark again.  Every frame's gradients must equal the fresh-workspace
    gradients bit for bit (deterministic reverse pass: the extra marked Gaussians only get exact zeros), the composited mask must
    cover every Gaussian with a gradient, and at least one frame must have had extra marked Gaussians."""
    sc = synth.make_scene(P=500, width=64, height=64, sh_degree=3, s0=0.05, seed=391, bg=(0.1, 0.2, 0.3))
    sc.means3D[::3, 0] -= 5.0             # a third off camera a's screen to the left (camera b, turned that way, sees many of them) ...
    sc.means3D[1::6, 2] *= -1.0           # ... and a sixth behind both cameras: a real share is never composited
    cam_a = sc.camera
    cam_b = look_at_camera(np.array([1.5, 0.0, 0.0]), np.array([-3.0, 0.0, 6.0]), (0.0, -1.0, 0.0), cam_a.FoVx, 64, 64)
    raw = _Raw(sc, cam_a)
    dL = torch.tensor(np.random.default_rng(1391).normal(size=(3, 64, 64)).astype(np.float32), device=DEV)

    def frame(geom):
        rc, f = raw.forward(geom)
        _lib.check(rc, "gsr_forward")
        m = raw.mask(f)
        return f, m, raw.backward(f, dL)

    def check(f, m, g, ref_f, ref_m, ref_g, what):
        for k, v in ref_g.items():
            assert torch.equal(v, g[k]), (what, k)
        assert torch.equal(f["color"], ref_f["color"]) and torch.equal(f["radii"], ref_f["radii"]), what
        has = (f["radii"] > 0) & (torch.cat([v.reshape(raw.P, -1) for v in g.values()], dim=1) != 0).any(dim=1)
        assert not bool((has & ~m).any()), what
        assert not bool((ref_m & ~m).any()), what                     # a superset of the fresh workspace's mask
        return int((m & ~ref_m).sum())

    with options(deterministic_bwd=1):
        ref_f, ref_m, ref_g = frame(raw.workspace(0))                 # marks are 1..255: a zeroed workspace holds none
        assert int(ref_m.sum()) > 50 and int((~ref_m).sum()) > 50 and float(ref_g["means3D"].abs().max()) > 0
        if stale == "constant_byte":
            geom = raw.workspace(77)
            extra = [check(*frame(geom), ref_f, ref_m, ref_g, f"frame {k}") for k in range(256)]
            assert max(extra) == int((~ref_m).sum())                  # the frame whose mark is 77: every Gaussian reads as marked
            assert sum(e > 0 for e in extra) <= 2                     # ... and it is that frame (and its return after 255) only
        else:
            geom, other = raw.workspace(0), raw.workspace(0)
            raw.set_camera(cam_b)
            mb = frame(geom)[1].clone()                               # camera b leaves its marks, value m, in `geom`
            raw.set_camera(cam_a)
            for k in range(254):                                      # 254 frames elsewhere: the next one has mark m again
                check(*frame(other), ref_f, ref_m, ref_g, f"elsewhere {k}")
            extra = check(*frame(geom), ref_f, ref_m, ref_g, "camera a over camera b's marks")
            assert extra == int((mb & ~ref_m).sum()) and extra > 0   # exactly camera b's marks show through
