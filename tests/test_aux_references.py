"""CPU only: the float64 references that judge the loss, Adam and kNN kernels (oracle/ssim_ref.py, oracle/aux_ref.py) agree with an
independent second route each, on the very inputs the GPU edge tests use -- before any kernel is judged by them."""
import numpy as np
import pytest
import torch

from gaussian_transformer_amd import loss
from oracle import aux_ref, ssim_ref
from tests import aux_inputs


def test_adam_reference_matches_torch_adam_in_float64():
    """20 steps of the edge tests' schedule (decade-scaled gradients, exact zeros, a learning-rate change), two groups with different
    betas / eps: equal to torch.optim.Adam on float64 CPU tensors to 1e-12 relative."""
    lengths = [1, 5, 4097, 300]
    lrs = [0.00016, 0.0025, 0.05, 0.01]
    hyper = [((0.9, 0.999), 1e-15)] * 3 + [((0.8, 0.99), 1e-8)]
    p0 = aux_inputs.adam_params(lengths)
    tp = [torch.tensor(p, dtype=torch.float64, requires_grad=True) for p in p0]
    opt = torch.optim.Adam([dict(params=[p], lr=lr, betas=b, eps=e) for p, lr, (b, e) in zip(tp, lrs, hyper)])
    ref = [aux_ref.Adam64(p) for p in p0]
    lrs = list(lrs)
    for step in range(20):
        for p, r, g, lr, (b, e) in zip(tp, ref, aux_inputs.adam_grads(lengths, step), lrs, hyper):
            p.grad = torch.tensor(g, dtype=torch.float64)
            r.update(g, lr, b, e)
        opt.step()
        if step == aux_inputs.ADAM_LR_CHANGE_AFTER:
            opt.param_groups[0]["lr"] = lrs[0] = aux_inputs.ADAM_LR_CHANGED
    for p, r in zip(tp, ref):
        st = opt.state[p]
        assert int(st["step"]) == r.step == 20
        for got, want in ((r.p, p.detach().numpy()), (r.m, st["exp_avg"].numpy()), (r.v, st["exp_avg_sq"].numpy())):
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_adam_reference_skips_a_tensor_without_gradient():
    r = aux_ref.Adam64(np.ones(3, np.float32))
    r.update(None, 0.1)
    assert r.step == 0 and (r.p == 1).all() and (r.m == 0).all() and (r.v == 0).all()


def _torch_f64(img, gt, lam):
    a = torch.tensor(img, dtype=torch.float64, requires_grad=True)
    L = loss.training_loss(a, torch.tensor(gt, dtype=torch.float64), lam)
    L.backward()
    return float(L), a.grad.numpy()


def _torch_window():
    """The 11x11 window as loss.training_loss (and the reference) builds it with torch ops, as float64."""
    return loss._window(11, 1, torch.zeros(1, dtype=torch.float64))[0, 0].numpy()


def _check_oracle(img, gt, lam):
    """Same window on both sides: what is pinned is the oracle's arithmetic (moments, SSIM map, hand-derived gradient) by torch's
    conv2d and autograd."""
    L, _, _, g = ssim_ref.l1_ssim_loss(img, gt, lam, w=_torch_window())
    Lt, gt_ = _torch_f64(img, gt, lam)
    # 1e-10 relative; the additive term is float64's own rounding of SSIM, a number next to 1, which 1 - SSIM inherits absolutely on
    # both routes (2^-53 each for the mean and the subtraction) -- it only shows where the loss itself is below 1e-6 (converged_*)
    assert abs(L - Lt) <= 1e-10 * abs(Lt) + 4 * 2.0 ** -53
    # relative to the largest gradient element, and where image == target everywhere (true gradient 0: both routes return rounding
    # noise) to 1/n, the size of the L1 term's gradient elements
    assert np.abs(g - gt_).max() <= 1e-10 * max(np.abs(gt_).max(), 1.0 / img.size)


def test_window_normalisation_differs_from_torch_in_the_last_place():
    """The 1-D window is 11 float32 numbers divided by their float32 sum, and that sum depends on the order of the additions:
    numpy's (oracle/ssim_ref.py) and a sequential loop (csrc/ssim_loss.hip: make_weights) give 3.7592325, torch's (loss._window,
    the reference's utils/loss_utils.py) the correctly rounded 3.7592328.  One unit in the last place of the normaliser moves
    SSIM of smooth images by ~1e-5 relative (the variance of a nearly flat patch is c^2 S (1 - S) with S the window's sum), which
    is why _check_oracle hands torch's window to the oracle, and why the GPU edge tests judge the kernel by the oracle's own."""
    import math
    e = np.array([math.exp(-(x - 5) ** 2 / 4.5) for x in range(11)], dtype=np.float32)
    seq = np.float32(0)
    for v in e:
        seq = np.float32(seq + v)
    g = e / seq
    assert np.array_equal((g[:, None] * g[None, :]).astype(np.float32).astype(np.float64), ssim_ref.window())   # the kernel's == the oracle's
    rel = np.abs(_torch_window() - ssim_ref.window()) / ssim_ref.window()
    assert rel.max() <= 4 * 2.0 ** -24                       # and torch's within rounding of it


@pytest.mark.parametrize("lam", [0.0, 0.2, 1.0])
def test_ssim_oracle_matches_torch_float64_on_every_family(lam):
    for name, (img, gt) in aux_inputs.loss_families().items():
        _check_oracle(img, gt, lam)


def test_ssim_oracle_matches_torch_float64_on_edge_shapes():
    for i, shape in enumerate(aux_inputs.EDGE_SHAPES):
        _check_oracle(*aux_inputs.smooth_pair(shape, i), 0.2)
        _check_oracle(*aux_inputs.flat_one_pixel(shape, shape[1] - 1, shape[2] - 1), 0.2)


def test_families_are_what_they_claim():
    fam = aux_inputs.loss_families()
    for name in aux_inputs.ALL_EQUAL:
        assert np.array_equal(*fam[name])
    x, y = fam["smooth"]
    assert 0.19 < x.min() and x.max() < 0.91 and np.corrcoef(x.ravel(), y.ravel())[0, 1] > 0.9
    assert fam["out_of_range"][0].min() < -0.4 and fam["out_of_range"][0].max() > 2.4 and (fam["pixels_at_50"][0] == 50).sum() == 5
    hs, ws = {s[1] for s in aux_inputs.EDGE_SHAPES}, {s[2] for s in aux_inputs.EDGE_SHAPES}
    assert hs == ws == {1, 2, 10, 11, 12, 15, 16, 17, 26, 27, 31, 32, 33} and {s[0] for s in aux_inputs.EDGE_SHAPES} == {1, 2, 3, 4}


def test_knn_brute_force_matches_kdtree_with_duplicates():
    p = aux_inputs.cloud("duplicates", 3000, seed=4)
    assert len(np.unique(p, axis=0)) < 2500
    a, b = aux_ref.knn_mean_dist2_brute(p, chunk=700), aux_ref.knn_mean_dist2_kdtree(p)
    assert (a == 0).any()                                     # points that occur four times
    assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max() and (np.abs(a - b) <= 1e-12 * b).all()


def test_knn_brute_force_below_four_points():
    """The rule of include/gsr_knn.h: mean over the neighbours that exist, 0 for a single point."""
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0]], np.float32)
    assert aux_ref.knn_mean_dist2_brute(p[:1]).tolist() == [0.0]
    assert aux_ref.knn_mean_dist2_brute(p[:2]).tolist() == [1.0, 1.0]
    assert aux_ref.knn_mean_dist2_brute(p).tolist() == [2.5, 3.0, 4.5]
    assert aux_ref.knn_mean_dist2_brute(np.zeros((0, 3), np.float32)).shape == (0,)
