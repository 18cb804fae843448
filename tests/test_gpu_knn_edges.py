"""-m gpu: distCUDA2 (include/gsr_knn.h, csrc/knn.hip) at its edges -- fewer than four points, coincident points, massive ties,
clouds far from the origin, a million points, a strided input -- each point against a float64 reference computed from the same
float32 coordinates (oracle/aux_ref.py: brute force up to 20 k points, scipy's k-d tree above).

Bound, per point (KNN_BOUND below): the kernel's arithmetic per candidate is "subtract, square, add" in float32.  With u = 2^-24:
  * dx = fl(xj - xi) = (xj - xi)(1 + d), |d| <= u, wherever the cloud lies (the inputs are exact float32 numbers)      1 rounding
  * dx * dx: the error of dx twice and one rounding of the product (none where the compiler contracts it into an fma)   3 roundings
  * the sum of the three squares, all non-negative: two additions, each (1 + d) on the running sum                      5 roundings
  * the three smallest of these, chosen among computed values: the k-th smallest of values that are each within a factor
    (1 +- u)^5 of the true ones lies within that factor of the true k-th smallest, whatever the ties
  * their mean: two additions and one division                                                                          8 roundings
so got = ref (1 + theta), |theta| <= (1 + u)^8 - 1 <= 8u / (1 - 8u) (gamma_8), and got == 0 exactly where ref == 0 (differences of
equal floats are exact zeros).  The float64 reference's own rounding, ~1e-16 relative, is eight orders below that.

Measured on the MI355X, worst |got - ref| / (u * ref) per cloud (the bound is 8):
    n=1                    N =        1   0.000
    n=2                    N =        2   0.000
    n=3                    N =        3   0.000
    n=4                    N =        4   0.571
    identical              N =     1000   0.000
    interleaved copies     N =     5000   2.318
    four copies            N =     2800   0.000
    collinear              N =     4001   2.593
    grid                   N =    10000   1.693
    sfm_like + 300         N =   300000   3.328
    sfm_like + 3000        N =   300000   2.246
    clustered + 300        N =    50000   2.586
    clustered + 3000       N =    50000   1.975
    uniform 1e6+3          N =  1000003   3.516
    strided view           N =     3001   2.665
"""
import numpy as np
import pytest
import torch

from oracle import aux_ref
from tests import aux_inputs

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GAMMA8 = 8 * U / (1 - 8 * U)
TINY = 2.0 ** -149                      # the smallest float32 above 0: only decides ref == 0, where got must be 0 as well


def knn_bound(ref):
    return GAMMA8 * ref + TINY


def _dist(p, **kw):
    from simple_knn._C import distCUDA2
    return distCUDA2(torch.tensor(p, device="cuda", **kw)).cpu().numpy().astype(np.float64)


def _check(name, p, got=None):
    ref = aux_ref.knn_mean_dist2_brute(p) if len(p) <= 20000 else aux_ref.knn_mean_dist2_kdtree(p)
    got = _dist(p) if got is None else got
    assert got.shape == ref.shape and np.isfinite(got).all()
    err = np.abs(got - ref)
    nz = ref > 0
    worst = float((err[nz] / (U * ref[nz])).max()) if nz.any() else 0.0
    print(f"KNN_EDGE {name:28s} N={len(p):8d} worst |got-ref|/(u*ref) = {worst:6.3f}   zeros: {int((~nz).sum())}")
    bad = np.nonzero(err > knn_bound(ref))[0]
    assert bad.size == 0, (name, bad[:10], got[bad[:10]], ref[bad[:10]])
    assert (got[~nz] == 0).all()
    return got, ref


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_fewer_than_four_points_give_finite_scales(n):
    """Mean over the neighbours that exist, 0 for one point (include/gsr_knn.h) -- and what create_from_pcd makes of it is finite."""
    p = np.array([[0.5, 1.0, -2.0], [1.5, 1.0, -2.0], [0.5, 3.0, -2.0], [0.5, 1.0, 1.0]], np.float32)[:n]
    got, ref = _check(f"n={n}", p)
    assert ref.tolist() == {1: [0.0], 2: [1.0, 1.0], 3: [2.5, 3.0, 4.5], 4: [14 / 3, 16 / 3, 22 / 3, 32 / 3]}[n]
    scales = torch.log(torch.sqrt(torch.clamp_min(torch.tensor(got, dtype=torch.float32), 0.0000001)))
    assert torch.isfinite(scales).all()


def test_empty_cloud():
    from simple_knn._C import distCUDA2
    assert distCUDA2(torch.zeros((0, 3), device="cuda")).shape == (0,)


def test_identical_points_are_exactly_zero():
    got, _ = _check("identical", aux_inputs.cloud("identical", 1000))
    assert (got == 0).all()


def test_two_interleaved_copies_of_a_cloud():
    """Every point has one twin at distance 0 and shares its other neighbours with it: never 0 (the twin counts once), and the
    two copies agree bit for bit."""
    half = aux_inputs.cloud("uniform", 2500, seed=5)
    p = np.repeat(half, 2, axis=0)
    got, ref = _check("interleaved copies", p)
    assert np.array_equal(got[0::2], got[1::2])
    four = np.repeat(half[:700], 4, axis=0)                   # four copies: the three nearest are the other three, exactly 0
    got4, _ = _check("four copies", four)
    assert (got4 == 0).all()


@pytest.mark.parametrize("kind,n", [("collinear", 4001), ("grid", 10000)])
def test_massive_ties(kind, n):
    _check(kind, aux_inputs.cloud(kind, n, seed=6))


@pytest.mark.parametrize("shift", [(300.0, -120.0, 40.0), (3000.0, 3000.0, 3000.0)])
@pytest.mark.parametrize("kind,n", [("sfm_like", 300000), ("clustered", 50000)])
def test_cloud_far_from_the_origin(kind, n, shift):
    """The reference sees the translated float32 coordinates: what is tested is the kernel's arithmetic, not the input's rounding."""
    p = (aux_inputs.cloud(kind, n, seed=7).astype(np.float64) + np.array(shift)).astype(np.float32)
    _check(f"{kind} + {shift[0]:g}", p)


def test_a_million_and_three_points():
    _check("uniform 1e6+3", aux_inputs.cloud("uniform", 1000003, seed=8))


def test_strided_input_is_accepted_and_correct():
    """big[:, :3] of an [N, 4] tensor: copied by the wrapper, never read with the wrong stride."""
    from simple_knn._C import distCUDA2
    p = aux_inputs.cloud("uniform", 3001, seed=9)
    big = torch.tensor(np.concatenate([p, np.full((len(p), 1), 1e6, np.float32)], 1), device="cuda")
    view = big[:, :3]
    assert not view.is_contiguous()
    got = distCUDA2(view).cpu().numpy().astype(np.float64)
    _check("strided view", p, got)
    assert np.array_equal(got, _dist(p))
