"""tests/normals_ref.py against what can be known without it: a tilted plane's normal, the loss of a normal map that agrees with the
depth map, unit normals that face the camera, and -- for the seeds and sizes tests/test_gpu_gaussian_normals.py and
tests/test_gpu_normal_loss.py use -- no borderline row and no borderline pixel, so that the device's decisions can be held to the
reference's exactly."""
import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib
from tests import normals_ref as nr

GPU_P = (0, 1, 63, 64, 65, 255, 256, 257, 4001)
TX, TY = _lib.NORMAL_TILE_X, _lib.NORMAL_TILE_Y
NO_INTERIOR = ((1, 1), (2, 2), (1, 7), (7, 1))
GPU_SIZES = NO_INTERIOR + ((3, 3), (TY - 1, TX - 1), (TY, TX), (TY + 1, TX + 1), (2 * TY + 1, 2 * TX + 1), (96, 160))      # (H, W)


@pytest.mark.parametrize("normal", [(0.3, -0.2, -0.93), (0.0, 0.0, -1.0), (-0.5, 0.4, -0.6)])
def test_a_tilted_plane_gives_its_normal_at_every_interior_pixel(normal):
    H, W = 23, 37
    depth, alpha, N, n = nr.plane(H, W, normal)
    r = nr.loss(depth, alpha, N, *nr.TANFOV, grad=False)
    assert bool(r["valid"][1:-1, 1:-1].all()) and int(r["valid"].sum()) == (H - 2) * (W - 2)
    err = (r["surf"][:, 1:-1, 1:-1] - torch.tensor(n)[:, None, None]).abs().max()
    assert float(err) <= 1e-12, float(err)
    assert not r["surf"][:, 0].any() and not r["surf"][:, :, 0].any() and not r["surf"][:, -1].any() and not r["surf"][:, :, -1].any()
    # N = A n: the loss is mean (A - A^2) over the valid pixels
    A = torch.tensor(alpha)
    want = (A - A * A)[r["valid"]].mean()
    got = r["loss"] * (H * W) / r["valid"].sum()
    assert abs(float(got - want)) <= 1e-12 and r["fraction"] == (H - 2) * (W - 2) / (H * W)


def test_a_fronto_parallel_plane_faces_the_camera():
    depth, alpha, N, n = nr.plane(9, 11, (0.0, 0.0, -1.0))
    surf = nr.loss(depth, alpha, N, *nr.TANFOV, grad=False)["surf"]
    assert float((surf[:, 4, 5] - torch.tensor([0.0, 0.0, -1.0])).abs().max()) <= 1e-12


@pytest.mark.parametrize("P", [1, 257, 4001])
def test_normals_of_unit_quaternions_are_unit_and_face_the_camera(P):
    means, scales, q, V = nr.rows(P)
    g = nr.gaussian_normals(means, scales, q, V)
    n = g["normals"]
    assert float((n.norm(dim=1) - 1).abs().max()) <= 1e-6          # float32 quaternions are unit to a few 1e-8
    assert bool(((n * g["pv"]).sum(1) <= 0).all())
    assert set(np.unique(g["axis"] & 3)) <= {0, 1, 2}
    k = g["axis"] & 3
    assert np.array_equal(k, np.argmin(scales, axis=1))              # no ties in random scales: any argmin agrees
    if P > 100:
        assert (g["axis"] & 4).any() and not (g["axis"] & 4).all() and len(set(k)) == 3


def test_ties_go_to_the_lowest_index():
    s = np.array([[2, 1, 1], [1, 1, 1], [1, 2, 1], [3, 2, 1], [1, 1, 2]], np.float32)
    assert list(nr.axis_of(s)) == [1, 0, 0, 2, 0]


def test_the_gradient_reaches_the_rotations_only_and_matches_differences():
    means, scales, q, V = nr.rows(40, seed=3)
    G = np.random.default_rng(1).normal(size=(40, 3))
    g = nr.gaussian_normals_grad(means, scales, q, V, G)
    eps = 1e-6
    for col in range(4):
        qp, qm = q.astype(np.float64).copy(), q.astype(np.float64).copy()
        qp[:, col] += eps; qm[:, col] -= eps
        fp = (nr.gaussian_normals(means, scales, torch.tensor(qp), V)["normals"] * torch.tensor(G)).sum(1)
        fm = (nr.gaussian_normals(means, scales, torch.tensor(qm), V)["normals"] * torch.tensor(G)).sum(1)
        assert float(((fp - fm) / (2 * eps) - g[:, col]).abs().max()) <= 1e-7


def test_the_loss_gradients_match_differences():
    H, W = 6, 7
    depth, alpha, N = nr.maps(H, W, holes=False)
    r = nr.loss(depth, alpha, N, *nr.TANFOV)
    eps = 1e-6
    for name, idx in (("g_depth", 0), ("g_alpha", 1), ("g_normals", 2)):
        for pos in ((2, 3), (1, 1), (4, 5)):
            args = [np.asarray(depth, np.float64).copy(), np.asarray(alpha, np.float64).copy(), np.asarray(N, np.float64).copy()]
            lo = [a.copy() for a in args]
            at = pos if idx < 2 else (1,) + pos
            args[idx][at] += eps; lo[idx][at] -= eps
            # A is a constant of the loss: the alpha in front of the bracket must not move with the input
            fd = (float(nr.loss(*args, *nr.TANFOV, grad=False)["loss"]) - float(nr.loss(*lo, *nr.TANFOV, grad=False)["loss"])) / (2 * eps)
            if idx == 1:
                n = r["surf"][:, pos[0], pos[1]]
                fd -= float(1 - (torch.tensor(np.asarray(N, np.float64))[:, pos[0], pos[1]] * n).sum()) / (H * W)
            assert abs(fd - float(r[name][at])) <= 2e-8, (name, pos, fd, float(r[name][at]))


@pytest.mark.parametrize("P", GPU_P)
def test_the_gpu_tests_rows_are_not_borderline(P):
    assert nr.borderline_rows(*nr.rows(P)) == 0


@pytest.mark.parametrize("hw", GPU_SIZES, ids=[f"{h}x{w}" for h, w in GPU_SIZES])
def test_the_gpu_tests_pixels_are_not_borderline(hw):
    H, W = hw
    for holes in (False, True):
        depth, alpha, _N = nr.maps(H, W, holes=holes)
        assert nr.borderline_pixels(depth, alpha, *nr.TANFOV) == 0
        r = nr.loss(depth, alpha, _N, *nr.TANFOV, grad=False)
        if hw in NO_INTERIOR:
            assert r["fraction"] == 0 and float(r["loss"]) == 0
        elif holes and H * W > 200:
            assert 0 < r["fraction"] < (H - 2) * (W - 2) / (H * W)      # the holes do take stencils out
        elif not holes:
            assert r["fraction"] == (H - 2) * (W - 2) / (H * W)
    depth, alpha, _N, _n = nr.plane(H, W, dtype=np.float32)
    assert nr.borderline_pixels(depth, alpha, *nr.TANFOV) == 0
