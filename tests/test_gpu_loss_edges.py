"""-m gpu: the fused L1 + SSIM kernel (include/gsr_loss.h, csrc/ssim_loss.hip) in the regimes training puts it in and uniform noise
never does -- smooth against smooth (variance small against the squared mean), flat regions, an image converged onto its target,
values outside [0, 1] -- at the shapes where a 16-pixel tile with a 5-pixel halo goes wrong, and through the wrapper's API edges.

Three evaluations of the same float32 arrays: the kernel, loss.training_loss in float32 on the GPU (torch's conv2d and autograd:
the yardstick), oracle/ssim_ref.py in float64 (the truth; pinned on these very inputs by tests/test_aux_references.py).  With g64 the
oracle's gradient,
    max|g_hip - g64| <= 2 max|g_torch - g64| + 1e-6 max|g64|         (every element; err_hip <= 2 err_torch + 1e-6, multiplied out so
    |L_hip - L64|    <= 2 |L_torch - L64|    + 4 * 2^-24 |L64|        that a true gradient of 0 needs no division)
The factor 2 is the margin tests/helpers.py::assert_parity gives one float32 evaluation over another.  Note that the oracle's and
the kernel's window are the same numbers, while torch's differs in the last place of its normaliser (test_aux_references.py:
test_window_normalisation_differs_from_torch_in_the_last_place), which alone moves SSIM of smooth images by ~1e-5: on the smooth
and flat families err_torch is that difference, not conv2d's rounding, and the yardstick is lenient there.  The table therefore
records err_hip absolutely as well, as the number a later regression of the kernel is to be held against.

Measured on the MI355X (err = max|g - g64| / max|g64| at lambda 0.2 unless marked, dL = |L - L64| / |L64|):
    case                             err_hip err_torch   abs_hip      dL_hip  dL_torch
    smooth                         1.587e-06 7.518e-05 2.818e-09   3.739e-07 8.599e-06
    flat_different                 2.030e-06 7.834e-05 8.485e-10   1.721e-07 2.013e-05
    flat_different lam 1           5.171e-06 1.912e-04 4.283e-09   1.003e-06 1.032e-04
    flat_vs_noise                  1.031e-07 9.611e-07 1.221e-10   3.808e-08 3.917e-08
    noise_vs_flat                  9.983e-08 1.711e-06 4.563e-11   4.334e-08 3.508e-08
    flat_black                     1.135e-07 9.229e-07 1.704e-10   1.666e-08 1.666e-08
    pixel_corner                   1.587e-06 2.337e-05 1.125e-09   1.631e-08 1.229e-04
    pixel_seam_x15                 4.198e-07 4.379e-05 1.125e-09   3.035e-08 1.069e-04
    pixel_seam_x16                 4.198e-07 4.518e-05 1.125e-09   3.035e-08 1.065e-04
    pixel_seam_y15                 4.198e-07 4.518e-05 1.125e-09   3.035e-08 1.063e-04
    pixel_seam_y16                 4.198e-07 4.562e-05 1.125e-09   3.035e-08 1.069e-04
    pixel_interior                 4.198e-07 4.562e-05 1.125e-09   3.035e-08 1.070e-04
    converged_1e-3                 1.366e-06 1.060e-04 4.048e-10   3.473e-06 2.659e-05
    converged_1e-6                 3.650e-07 5.972e-05 9.209e-11   1.613e-05 8.976e-02
    out_of_range                   6.781e-08 3.442e-07 2.360e-11   9.470e-09 9.470e-09
    pixels_at_50                   9.884e-07 4.574e-05 1.670e-09   7.083e-09 2.356e-06
    smooth (3, 10, 17)             4.213e-07 1.045e-05 3.012e-09   1.123e-07 1.783e-07
    one pixel@0 (3, 16, 32) lam 1  2.392e-06 2.838e-05 1.973e-08   5.722e-07 5.654e-04
    one pixel@0 (4, 11, 11) lam 1  7.346e-07 6.030e-06 1.923e-08   2.849e-07 7.529e-05
    smooth (3, 1080, 1920)         2.232e-06 1.497e-04 5.569e-12   5.633e-07 1.622e-05
    smooth (3, 1079, 1921)         2.391e-06 1.547e-04 6.110e-12   6.794e-07 1.689e-05
    render-like 3x131x250          2.289e-06 1.273e-04 2.758e-10   1.909e-07 4.151e-06

The kernels carry the blurred moments, the SSIM map and the blur of the derivative maps in float64 (csrc/ssim_loss.hip); with
float32 moments the flat cases stood at twice torch's error (flat_different at lambda 1: |L - L64| / |L64| = 2.1e-4 against torch's
1.0e-4; one bright pixel on 3x16x32: err_hip 6.0e-5 against 2.8e-5), the variance s11 - m1*m1 of a flat patch being rounded at
2^-24 c^2 against C2 = 9e-4.  Worst err_hip now: 5.2e-6, apart from
image == target (true gradient 0, the kernel returns 1e-16 where torch returns 1e-8) and converged_1e-6 at lambda 1 (true gradient
2e-7 of the usual size: err_hip 2.3e-3, err_torch 0.52).  The float64 blur costs 17 us of 183 us per forward + backward at 1080p.
"""
import numpy as np
import pytest
import torch

from gaussian_transformer_amd import loss
from oracle import ssim_ref
from tests import aux_inputs

pytestmark = pytest.mark.gpu

UP = -1.75                              # upstream factor of backward()
LAMBDAS = (0.0, 0.2, 1.0)


def _hip(img, gt, lam, up=UP):
    a = torch.tensor(img, device="cuda", requires_grad=True)
    L = loss.fused_l1_ssim_loss(a, torch.tensor(gt, device="cuda"), lam)
    (L * up).backward()
    return float(L.detach()), a.grad.cpu().numpy().astype(np.float64)


def _torch32(img, gt, lam, up=UP):
    a = torch.tensor(img, device="cuda", requires_grad=True)
    L = loss.training_loss(a, torch.tensor(gt, device="cuda"), lam)
    (L * up).backward()
    return float(L.detach()), a.grad.cpu().numpy().astype(np.float64)


def _judge(name, img, gt, lam, all_equal=False):
    Lh, gh = _hip(img, gt, lam)
    Lt, gt32 = _torch32(img, gt, lam)
    L64, _, _, g64 = ssim_ref.l1_ssim_loss(img, gt, lam)
    g64 = UP * g64
    assert np.isfinite(Lh) and np.isfinite(gh).all()
    scale = np.abs(g64).max()
    eh, et = np.abs(gh - g64).max(), np.abs(gt32 - g64).max()
    print(f"LOSS_EDGE {name:34s} lam={lam:3.1f} err_hip={eh / max(scale, 1e-300):9.3e} err_torch={et / max(scale, 1e-300):9.3e} max|g64|={scale:9.3e} "
          f"abs_hip={eh:9.3e} dL_hip={abs(Lh - L64) / max(abs(L64), 1e-300):9.3e} dL_torch={abs(Lt - L64) / max(abs(L64), 1e-300):9.3e} L64={L64:.6e}")
    assert abs(Lh - L64) <= 2 * abs(Lt - L64) + 4 * 2.0 ** -24 * abs(L64), (name, lam, Lh, Lt, L64)
    if all_equal and lam == 0.0:
        assert Lh == 0.0 and (gh == 0).all()           # L1 of equal images: exactly 0, and sign(0) = 0 everywhere
        return
    if not all_equal:
        assert scale > 0
    assert eh <= 2 * et + 1e-6 * scale, (name, lam, eh, et, scale, np.unravel_index(np.abs(gh - g64).argmax(), gh.shape))


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("name", list(aux_inputs.loss_families()))
def test_family(name, lam):
    img, gt = aux_inputs.loss_families()[name]
    _judge(name, img, gt, lam, all_equal=name in aux_inputs.ALL_EQUAL)


def test_equal_images_value():
    """image == target: the L1 term is exactly 0, and what is left is lambda (1 - SSIM) with SSIM = 1 up to the rounding of the
    per-pixel quotient: a1 a2 / (b1 b2) with a == b in exact arithmetic, ~6 float32 roundings per pixel, not accumulating in a mean."""
    for name in aux_inputs.ALL_EQUAL:
        img, gt = aux_inputs.loss_families()[name]
        L0, g0 = _hip(img, gt, 0.0)
        assert L0 == 0.0 and (g0 == 0).all()
        L1, _ = _hip(img, gt, 1.0)
        print(f"LOSS_EDGE equal images {name}: 1 - SSIM = {L1:.3e}")
        assert abs(L1) <= 8 * 2.0 ** -24


@pytest.mark.parametrize("shape", aux_inputs.EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edge_shapes(shape):
    i = aux_inputs.EDGE_SHAPES.index(shape)
    _judge(f"smooth {shape}", *aux_inputs.smooth_pair(shape, i), 0.2)
    _judge(f"one pixel {shape}", *aux_inputs.flat_one_pixel(shape, shape[1] - 1, shape[2] - 1), 0.2)
    _judge(f"one pixel@0 {shape}", *aux_inputs.flat_one_pixel(shape, 0, 0), 1.0)


@pytest.mark.parametrize("shape", [(3, 1080, 1920), (3, 1079, 1921)], ids=lambda s: "x".join(map(str, s)))
def test_smooth_at_full_size(shape):
    _judge(f"smooth {shape}", *aux_inputs.smooth_pair(shape, 11), 0.2)


def test_render_like_pair():
    """A rasterizer render at 250x131 against the same scene with perturbed opacities: what the loss sees in training."""
    from gaussian_transformer_amd import synth
    from tests.helpers import hip_forward_backward, oracle_scene
    sc = synth.make_scene(P=3000, width=250, height=131, sh_degree=1, s0=0.04, seed=5, bg=(0.1, 0.2, 0.3))
    img = hip_forward_backward(oracle_scene(sc))["color"]
    op = np.clip(np.asarray(sc.opacities) * np.random.default_rng(3).uniform(0.7, 1.0, np.asarray(sc.opacities).shape), 0.0, 1.0)
    gt = hip_forward_backward(oracle_scene(sc, opacities=op.astype(np.float32)))["color"]
    assert img.shape == (3, 131, 250) and not np.array_equal(img, gt)
    for lam in LAMBDAS:
        _judge("render-like 3x131x250", np.ascontiguousarray(img), np.ascontiguousarray(gt), lam)


# ---------------------------------------------------------------------------------------------
# API edges
# ---------------------------------------------------------------------------------------------
def _pair(shape=(3, 37, 50), seed=4):
    return aux_inputs.smooth_pair(shape, seed)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.mark.parametrize("layout", ["every_other_column", "permuted_hwc"])
def test_non_contiguous_image(layout):
    """The wrapper copies a strided image; value and gradient are those of the contiguous copy bit for bit, and the gradient reaches the
    caller's tensor in the caller's layout."""
    img, gt = _pair()
    if layout == "every_other_column":
        base = torch.zeros((3, 37, 100), device="cuda"); base[:, :, ::2] = torch.tensor(img, device="cuda")
        base.requires_grad_(True)
        view = base[:, :, ::2]
    else:
        base = torch.tensor(img, device="cuda").permute(1, 2, 0).contiguous().requires_grad_(True)     # [H, W, C] storage
        view = base.permute(2, 0, 1)
    assert not view.is_contiguous() and torch.equal(view.detach(), torch.tensor(img, device="cuda"))
    g = torch.tensor(gt, device="cuda")
    L = loss.fused_l1_ssim_loss(view, g, 0.2); (L * UP).backward()
    c = torch.tensor(img, device="cuda", requires_grad=True)
    Lc = loss.fused_l1_ssim_loss(c, g, 0.2); (Lc * UP).backward()
    assert torch.equal(_bits(L), _bits(Lc))
    assert base.grad.shape == base.shape
    if layout == "every_other_column":
        assert torch.equal(_bits(base.grad[:, :, ::2]), _bits(c.grad)) and (base.grad[:, :, 1::2] == 0).all()
    else:
        assert torch.equal(_bits(base.grad.permute(2, 0, 1)), _bits(c.grad))


def test_backward_twice_on_a_retained_graph():
    img, gt = _pair()
    a = torch.tensor(img, device="cuda", requires_grad=True)
    L = loss.fused_l1_ssim_loss(a, torch.tensor(gt, device="cuda"), 0.2)
    L.backward(retain_graph=True)
    first = a.grad.clone()
    a.grad = None
    L.backward(retain_graph=True)
    assert torch.equal(_bits(a.grad), _bits(first))            # the saved workspace is read, never consumed
    L.backward()
    assert torch.equal(_bits(a.grad), _bits(first * 2))        # accumulated: exactly doubled


def test_two_graphs_interleaved():
    """forward, forward, backward, backward: each graph owns its workspace."""
    (i1, g1), (i2, g2) = _pair(seed=4), _pair(seed=5)
    solo = []
    for i, g in ((i1, g1), (i2, g2)):
        a = torch.tensor(i, device="cuda", requires_grad=True)
        loss.fused_l1_ssim_loss(a, torch.tensor(g, device="cuda"), 0.2).backward()
        solo.append(a.grad.clone())
    a1 = torch.tensor(i1, device="cuda", requires_grad=True); a2 = torch.tensor(i2, device="cuda", requires_grad=True)
    L1 = loss.fused_l1_ssim_loss(a1, torch.tensor(g1, device="cuda"), 0.2)
    L2 = loss.fused_l1_ssim_loss(a2, torch.tensor(g2, device="cuda"), 0.2)
    L1.backward(); L2.backward()
    assert torch.equal(_bits(a1.grad), _bits(solo[0])) and torch.equal(_bits(a2.grad), _bits(solo[1]))
    assert not torch.equal(_bits(solo[0]), _bits(solo[1]))


def test_on_a_second_stream():
    img, gt = _pair()
    a = torch.tensor(img, device="cuda", requires_grad=True); b = torch.tensor(gt, device="cuda")
    L0 = loss.fused_l1_ssim_loss(a, b, 0.2); L0.backward()
    want_L, want_g = L0.detach().clone(), a.grad.clone()
    a.grad = None
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.default_stream().cuda_stream
    with torch.cuda.stream(s):
        L = loss.fused_l1_ssim_loss(a, b, 0.2)
        L.backward()
    s.synchronize()
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(_bits(L), _bits(want_L)) and torch.equal(_bits(a.grad), _bits(want_g))


def test_target_that_requires_grad_gets_none():
    img, gt = _pair()
    a = torch.tensor(img, device="cuda", requires_grad=True); b = torch.tensor(gt, device="cuda", requires_grad=True)
    loss.fused_l1_ssim_loss(a, b, 0.2).backward()
    assert b.grad is None and a.grad is not None and torch.isfinite(a.grad).all()
