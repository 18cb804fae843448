"""-m gpu: the multi-view image loss (loss.multi_view_loss, csrc/ssim_loss.hip: views_loss_*) against the float64 torch formulation of
tests/views_loss_ref.py, with the float32 torch formulation as the yardstick:
    max|g_hip - g64| <= 2 max|g_torch32 - g64| + 1e-6 max|g64|      (all views together)
    |L_hip - L64|    <= 2 |L_torch32 - L64|    + 4 * 2^-24 |L64|

Every case prints its figures (VIEWS_LOSS lines under -s: err = max|g - g64| / max|g64|, dL = |L - L64| / |L64|) before it asserts.
No table from an MI355X is recorded yet; a float64 emulation of the kernels' window and formula on the CPU stands at
<= 0.15 of every bar of the noise cases below (with the exact products of the 1-D taps as the window, not the reference's float32
2-D window's sums, the per-view SSIM of 4x131x250-raw is at 3.0 of its bar, and so it came out on the card).
"""
import contextlib

import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib, loss
from tests import views_loss_ref as vr

pytestmark = pytest.mark.gpu

SHAPES = [(1, 16, 16), (3, 37, 29), (2, 7, 5), (4, 131, 250), (loss.MAX_VIEWS_PER_LAUNCH + 1, 10, 17)]
WEIGHTS = ["reference", (0.8, 0.2), (0.0, 1.0)]


def _weights(w, B):
    return vr.reference_weights(B) if w == "reference" else w


def _case(shape, sanitize):
    """Seeded noise: predictions U[-0.25, 1.25) under sanitising (a real share of the pixels is clamped), U[0, 1) without."""
    B, H, W = shape
    return (B, H, W, -0.25, 1.25, 100 + H) if sanitize else (B, H, W, 0.0, 1.0, 200 + H)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.mark.parametrize("w", WEIGHTS, ids=lambda w: w if isinstance(w, str) else f"{w[0]}-{w[1]}")
@pytest.mark.parametrize("sanitize", [True, False], ids=["sanitize", "raw"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_value_and_gradient_against_float64(shape, sanitize, w):
    key = _case(shape, sanitize)
    img, gt = vr.noise_views(*key)
    w_l1, w_ssim = _weights(w, shape[0])
    hip = vr.hip_loss(img, gt, w_l1, w_ssim, sanitize)
    t32 = vr.torch_loss(img, gt, w_l1, w_ssim, sanitize, torch.float32)
    r64 = vr.noise_reference64(*key, sanitize, w_l1, w_ssim)
    vr.judge(f"{shape} {'sanitize' if sanitize else 'raw'} w=({w_l1:.4g},{w_ssim:.4g})", hip, t32, r64)
    # per-view terms: same relative form as the loss
    for k, name in enumerate(("l1", "ssim", "sq")):
        dh, dt = np.abs(hip["terms"][:, k] - r64["terms"][:, k]), np.abs(t32["terms"][:, k] - r64["terms"][:, k])
        assert (dh <= 2 * dt + 4 * vr.U24 * np.abs(r64["terms"][:, k])).all(), (name, dh, dt)
    if sanitize:
        outside = ~((img >= 0) & (img <= 1))
        assert outside.any() and (hip["grad"][outside] == 0).all()


def test_sanitising():
    B, H, W = 3, 37, 29
    base_img, base_gt = vr.noise_views(B, H, W, -0.5, 1.5, 7)
    img, gt, masks = vr.plant(base_img, base_gt)
    for k, m in masks.items():
        assert all(m[b].any() for b in range(B)), k            # every kind in every view
    w_l1, w_ssim = vr.reference_weights(B)
    hip = vr.hip_loss(img, gt, w_l1, w_ssim, True)
    t32 = vr.torch_loss(img, gt, w_l1, w_ssim, True, torch.float32)
    r64 = vr.torch_loss(img, gt, w_l1, w_ssim, True, torch.float64)
    assert np.isfinite(hip["loss"]) and np.isfinite(hip["terms"]).all() and np.isfinite(hip["grad"]).all()
    dead = ~np.isfinite(img) | (img < 0) | (img > 1)
    assert (masks["nan"] | masks["pinf"] | masks["ninf"]).sum() > 0 and dead.sum() > (masks["nan"] | masks["pinf"] | masks["ninf"]).sum()
    g32 = np.stack([g.cpu().numpy() for g in hip["grads"]])
    assert (g32.view(np.uint32)[dead] == 0).all()              # +0.0, bit for bit
    assert (r64["grad"][dead] == 0).all()
    vr.judge("planted (3, 37, 29) all elements", hip, t32, r64)
    edge = masks["zero"] | masks["one"]
    assert (r64["grad"][edge] != 0).all()                      # the gradient passes at the bounds themselves
    vr.judge("planted (3, 37, 29) at exact 0.0 / 1.0", hip, t32, r64, where=edge)


def test_views_do_not_leak():
    B, H, W = 3, 37, 29
    img, gt = vr.noise_views(B, H, W, -0.25, 1.25, 11)
    other = img.copy()
    other[1] = vr.noise_views(B, H, W, -0.25, 1.25, 12)[0][1]
    a = vr.hip_loss(img, gt, 0.8, 0.2, True)
    b = vr.hip_loss(other, gt, 0.8, 0.2, True)
    assert torch.equal(_bits(a["grads"][0]), _bits(b["grads"][0])) and torch.equal(_bits(a["terms_t"][0]), _bits(b["terms_t"][0]))
    assert torch.equal(_bits(a["grads"][2]), _bits(b["grads"][2])) and torch.equal(_bits(a["terms_t"][2]), _bits(b["terms_t"][2]))
    assert not torch.equal(_bits(a["grads"][1]), _bits(b["grads"][1])) and not torch.equal(_bits(a["terms_t"][1]), _bits(b["terms_t"][1]))


@pytest.mark.parametrize("shape", [(3, 37, 29), (loss.MAX_VIEWS_PER_LAUNCH + 1, 10, 17)], ids=lambda s: "x".join(map(str, s)))
def test_determinism(shape):
    img, gt = vr.noise_views(*shape, -0.25, 1.25, 13)
    a = vr.hip_loss(img, gt, 0.8, 0.2, True)
    b = vr.hip_loss(img, gt, 0.8, 0.2, True)
    assert torch.equal(_bits(a["L"]), _bits(b["L"])) and torch.equal(_bits(a["terms_t"]), _bits(b["terms_t"]))
    for x, y in zip(a["grads"], b["grads"]):
        assert torch.equal(_bits(x), _bits(y))


# ---------------------------------------------------------------------------------------------
# interface
# ---------------------------------------------------------------------------------------------
def _dev(a, grad=False):
    return torch.tensor(np.ascontiguousarray(a), device="cuda", requires_grad=grad)


def test_list_and_batch_tensor_inputs_agree_bit_for_bit():
    img, gt = vr.noise_views(3, 37, 29, -0.25, 1.25, 14)
    a = vr.hip_loss(img, gt, 0.8, 0.2, True, as_list=True)
    x = _dev(img, True)
    L = loss.multi_view_loss(x, _dev(gt), 0.8, 0.2)
    (L * vr.UP).backward()
    assert torch.equal(_bits(L), _bits(a["L"])) and torch.equal(_bits(L.terms), _bits(a["terms_t"]))
    assert x.grad.shape == x.shape and torch.equal(_bits(x.grad), _bits(torch.stack(a["grads"])))
    assert L.terms.shape == (3, 3) and not L.terms.requires_grad
    # a list of images against one batch tensor of targets
    xs = [_dev(v, True) for v in img]
    L2 = loss.multi_view_loss(xs, _dev(gt), 0.8, 0.2)
    assert torch.equal(_bits(L2), _bits(L))


def test_a_view_that_does_not_require_grad_gets_none():
    img, gt = vr.noise_views(3, 37, 29, -0.25, 1.25, 14)
    full = vr.hip_loss(img, gt, 0.8, 0.2, True)
    xs = [_dev(img[0], True), _dev(img[1], False), _dev(img[2], True)]
    L = loss.multi_view_loss(xs, [_dev(v, True) for v in gt], 0.8, 0.2)         # targets that require grad get none either
    (L * vr.UP).backward()
    assert xs[1].grad is None
    assert torch.equal(_bits(xs[0].grad), _bits(full["grads"][0])) and torch.equal(_bits(xs[2].grad), _bits(full["grads"][2]))
    assert torch.equal(_bits(L), _bits(full["L"]))


def test_non_contiguous_image():
    img, gt = vr.noise_views(2, 37, 29, -0.25, 1.25, 15)
    full = vr.hip_loss(img, gt, 0.8, 0.2, True)
    base = torch.zeros((3, 37, 58), device="cuda"); base[:, :, ::2] = _dev(img[0])
    base.requires_grad_(True)
    hwc = _dev(img[1]).permute(1, 2, 0).contiguous().requires_grad_(True)
    views = [base[:, :, ::2], hwc.permute(2, 0, 1)]
    assert not views[0].is_contiguous() and not views[1].is_contiguous()
    L = loss.multi_view_loss(views, _dev(gt), 0.8, 0.2)
    (L * vr.UP).backward()
    assert torch.equal(_bits(L), _bits(full["L"]))
    assert torch.equal(_bits(base.grad[:, :, ::2]), _bits(full["grads"][0])) and (base.grad[:, :, 1::2] == 0).all()
    assert torch.equal(_bits(hwc.grad.permute(2, 0, 1)), _bits(full["grads"][1]))


def test_backward_twice_on_a_retained_graph():
    img, gt = vr.noise_views(2, 37, 29, -0.25, 1.25, 15)
    xs = [_dev(v, True) for v in img]
    L = loss.multi_view_loss(xs, _dev(gt), 0.8, 0.2)
    L.backward(retain_graph=True)
    first = [x.grad.clone() for x in xs]
    for x in xs:
        x.grad = None
    L.backward(retain_graph=True)
    assert all(torch.equal(_bits(x.grad), _bits(f)) for x, f in zip(xs, first))
    L.backward()
    assert all(torch.equal(_bits(x.grad), _bits(f * 2)) for x, f in zip(xs, first))


def test_two_graphs_interleaved():
    cases = [vr.noise_views(2, 37, 29, -0.25, 1.25, s) for s in (16, 17)]
    solo = [vr.hip_loss(i, g, 0.8, 0.2, True, up=1.0) for i, g in cases]
    xs = [[_dev(v, True) for v in i] for i, _ in cases]
    L1 = loss.multi_view_loss(xs[0], _dev(cases[0][1]), 0.8, 0.2)
    L2 = loss.multi_view_loss(xs[1], _dev(cases[1][1]), 0.8, 0.2)
    L1.backward(); L2.backward()
    for k in range(2):
        assert all(torch.equal(_bits(x.grad), _bits(g)) for x, g in zip(xs[k], solo[k]["grads"]))
    assert not torch.equal(_bits(solo[0]["grads"][0]), _bits(solo[1]["grads"][0]))


def test_on_a_second_stream():
    img, gt = vr.noise_views(2, 37, 29, -0.25, 1.25, 15)
    want = vr.hip_loss(img, gt, 0.8, 0.2, True, up=1.0)
    xs = [_dev(v, True) for v in img]; g = _dev(gt)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.default_stream().cuda_stream
    with torch.cuda.stream(s):
        L = loss.multi_view_loss(xs, g, 0.8, 0.2)
        L.backward()
    s.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(_bits(L), _bits(want["L"])) and all(torch.equal(_bits(x.grad), _bits(w)) for x, w in zip(xs, want["grads"]))


def test_terms_reproduce_psnr_and_view_metrics():
    B, H, W = 3, 37, 29
    img, gt, _ = vr.plant(*vr.noise_views(B, H, W, -0.5, 1.5, 7))
    t32 = vr.torch_loss(img, gt, 0.8, 0.2, True, torch.float32)
    r64 = vr.torch_loss(img, gt, 0.8, 0.2, True, torch.float64)
    L = loss.multi_view_loss(_dev(img), _dev(gt), 0.8, 0.2)
    psnr = (20 * torch.log10(1.0 / torch.sqrt(L.terms[:, 2]))).cpu().numpy().astype(np.float64)
    dh, dt = np.abs(psnr - r64["psnr"]), np.abs(t32["psnr"] - r64["psnr"])
    print(f"VIEWS_LOSS psnr: hip {psnr}, float64 {r64['psnr']}, err_hip {dh}, err_torch32 {dt}")
    assert (dh <= 2 * dt + 4 * vr.U24 * np.abs(r64["psnr"])).all()
    m = loss.view_metrics(_dev(img), _dev(gt), sanitize=True)
    assert torch.equal(_bits(m["l1"]), _bits(L.terms[:, 0])) and torch.equal(_bits(m["ssim"]), _bits(L.terms[:, 1]))
    assert np.array_equal(m["psnr"].cpu().numpy().astype(np.float64), psnr) and not m["psnr"].requires_grad
    # sanitize = False on in-range images: the metrics of train.py's report
    img2, gt2 = vr.noise_views(B, H, W, 0.0, 1.0, 8)
    m2 = loss.view_metrics([_dev(v) for v in img2], [_dev(v) for v in gt2])
    r = vr.torch_loss(img2, gt2, 0.8, 0.2, False, torch.float64)
    assert np.abs(m2["psnr"].cpu().numpy() - r["psnr"]).max() <= 1e-5 * np.abs(r["psnr"]).max()
    assert np.abs(m2["ssim"].cpu().numpy() - r["terms"][:, 1]).max() <= 1e-5


@pytest.mark.parametrize("lam", [0.2, 1.0])
def test_one_view_against_the_single_image_kernel(lam):
    """B = 1, in-range inputs, weights (1 - lambda, lambda): the loss of train.py.  The new call meets the float64 bar at both lambdas;
    the single-image kernel is held to it at train.py's lambda = 0.2 (bit equality is not asked: it rounds 1 - lambda itself).  At
    lambda = 1 its figures are printed only: it normalises its window by the taps added one by one in float32, one place below torch's
    sum (tests/test_aux_references.py), which alone puts 1 - SSIM of this noise 4.0e-7 from loss.ssim in float64 where the bar allows
    2 * 1.1e-8 + 2.4e-7 (float64 evaluation with that window; DESIGN.md section 7, "The window").  That kernel is not changed here."""
    img, gt = vr.noise_views(1, 37, 29, 0.0, 1.0, 18)
    w_l1, w_ssim = 1.0 - lam, lam
    t32 = vr.torch_loss(img, gt, w_l1, w_ssim, False, torch.float32)
    r64 = vr.torch_loss(img, gt, w_l1, w_ssim, False, torch.float64)
    a = _dev(img[0], True)
    Ls = loss.fused_l1_ssim_loss(a, _dev(gt[0]), lam)
    (Ls * vr.UP).backward()
    single = dict(loss=float(Ls.detach()), grad=a.grad.cpu().numpy().astype(np.float64)[None])
    if lam == 0.2:
        vr.judge(f"single-image kernel lam={lam}", single, t32, r64)
    else:
        L64 = r64["loss"]
        print(f"VIEWS_LOSS single-image kernel lam={lam} (not asserted): dL_hip={abs(single['loss'] - L64) / abs(L64):9.3e} "
              f"dL_torch32={abs(t32['loss'] - L64) / abs(L64):9.3e} err_hip={np.abs(single['grad'] - r64['grad']).max() / np.abs(r64['grad']).max():9.3e}")
    vr.judge(f"one view lam={lam}", vr.hip_loss(img, gt, w_l1, w_ssim, False), t32, r64)
    vr.judge(f"one view, sanitised, lam={lam}", vr.hip_loss(img, gt, w_l1, w_ssim, True), t32, r64)


# ---------------------------------------------------------------------------------------------
# with the rasterizer
# ---------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _options(**kw):
    saved = {k: _lib.get_option(k) for k in set(kw) | {"depth_log_map"}}
    try:
        for k, v in kw.items():
            _lib.set_option(k, v)
        yield
    finally:
        for k, v in saved.items():
            _lib.set_option(k, v)


def test_two_renders_in_flight_then_one_loss():
    """Two cameras on a tiny scene, each render on a gradient arena of its own and both waiting for their backward; stacked_image_loss;
    one backward().  The dL/dimage each render receives is judged against the float64 reference evaluated on the rendered images."""
    from gaussian_transformer_amd import GaussianRasterizationSettings, GaussianRasterizer, synth
    from gaussian_transformer_amd.camera import look_at_camera
    from gaussian_transformer_amd.rasterizer import arena_floats, gradient_arena
    P, W, H = 300, 64, 48
    sc = synth.make_scene(P=P, width=W, height=H, sh_degree=1, s0=0.08, seed=31, bg=(0.1, 0.2, 0.3))
    cams = [sc.camera, look_at_camera(np.array((1.0, 0.3, 0.0)), np.array((0.0, 0.0, 6.0)), (0.0, -1.0, 0.0), sc.camera.FoVx, W, H)]
    t = lambda a, grad=False: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda").requires_grad_(grad)

    def leaves(grad, opacities=None):
        op = sc.opacities if opacities is None else opacities
        return dict(means3D=t(sc.means3D, grad), opacities=t(np.asarray(op).reshape(P, 1), grad), shs=t(sc.shs, grad),
                    scales=t(sc.scales, grad), rotations=t(sc.rotations, grad))

    def render(c, lv):
        rs = GaussianRasterizationSettings(H, W, c.tanfovx, c.tanfovy, t(sc.bg), 1.0, t(c.world_view_transform), t(c.full_proj_transform),
                                           sc.sh_degree, t(c.camera_center), False, False)
        m2 = torch.zeros((P, 3), dtype=torch.float32, device="cuda", requires_grad=lv["means3D"].requires_grad)
        return GaussianRasterizer(raster_settings=rs)(means2D=m2, **lv)

    dimmed = np.clip(np.asarray(sc.opacities) * np.random.default_rng(3).uniform(0.6, 1.0, np.asarray(sc.opacities).shape), 0.0, 1.0).astype(np.float32)
    n = arena_floats(P, 4)
    pad = (-3 * P) % 4
    stores = [torch.zeros((n + 8,), device="cuda") for _ in cams]
    with _options(deterministic_bwd=1):
        with torch.no_grad():
            targets = [render(c, leaves(False, dimmed))[0] for c in cams]
        live, seen = [], {}
        for i, c in enumerate(cams):
            lv = leaves(True)
            with gradient_arena(stores[i][pad:pad + n]):
                color, radii = render(c, lv)
            color.register_hook(lambda g, i=i: seen.__setitem__(i, g.detach().clone()))
            live.append((lv, color, radii))
        L = loss.stacked_image_loss([color for _, color, _ in live], targets)
        L.backward()
    assert sorted(seen) == [0, 1]
    img = np.stack([color.detach().cpu().numpy() for _, color, _ in live]); gt = np.stack([x.cpu().numpy() for x in targets])
    assert not np.array_equal(img[0], img[1]) and not np.array_equal(img, gt)
    w_l1, w_ssim = vr.reference_weights(2)
    t32 = vr.torch_loss(img, gt, w_l1, w_ssim, True, torch.float32, up=1.0)
    r64 = vr.torch_loss(img, gt, w_l1, w_ssim, True, torch.float64, up=1.0)
    hip = dict(loss=float(L.detach()), grad=np.stack([seen[i].cpu().numpy() for i in range(2)]).astype(np.float64))
    vr.judge("two renders 64x48", hip, t32, r64)
    for i, (lv, _, radii) in enumerate(live):
        for k, p in lv.items():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), (i, k)
        visible = radii > 0
        assert int(visible.sum()) > 20 and bool((lv["means3D"].grad[visible] != 0).any()), i
