"""-m gpu: the HIP Chamfer distance (csrc/chamfer.hip through chamfer_distance.ChamferDistance) against the float64 reference of
tests/chamfer_ref.py.  Bounds: chamfer_ref.dist_bound / backward_bound (derived there from the float32 format, not measured)."""
import numpy as np
import pytest
import torch

from chamfer_distance import ChamferDistance, ChamferDistanceFunction
from gaussian_transformer_amd import _lib
from tests import chamfer_ref as cr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 8192, 8192, 26), (1, 16384, 5000, 26), (4, 1000, 777, 3), (1, 1, 1, 1), (2, 65, 4097, 26), (1, 5000, 3, 64), (3, 257, 129, 7)]
KINDS = ["normal", "dup", "wide"]


def _gpu(x, **kw):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV, **kw)


def _forward(x1, x2):
    with torch.no_grad():
        d1, d2, i1, i2 = ChamferDistance()(_gpu(x1), _gpu(x2))
    assert d1.dtype == torch.float32 and d2.dtype == torch.float32 and i1.dtype == torch.int32 and i2.dtype == torch.int32
    assert d1.shape == x1.shape[:2] and d2.shape == x2.shape[:2] and i1.shape == d1.shape and i2.shape == d2.shape
    return d1.cpu().numpy(), d2.cpu().numpy(), i1.cpu().numpy(), i2.cpu().numpy()


def _check_forward(x1, x2, got, tag):
    D = x1.shape[2]
    d1, d2, i1, i2 = got
    r1, _, r2, _ = cr.chamfer_ref(x1, x2)
    for side, (d, i, r, a, b) in enumerate(((d1, i1, r1, x1, x2), (d2, i2, r2, x2, x1))):
        assert (i >= 0).all() and (i < b.shape[1]).all()
        at = cr.dist_to(a, b, i)                         # float64 distance to the row the GPU chose
        e_min = np.abs(d - r) / cr.dist_bound(r, D)
        e_at = np.abs(d - at) / cr.dist_bound(at, D)
        slack = at / (r * (1 + 2 * (D + 3) * cr.U) + 2 * D * cr.TINY)
        print(f"{tag} side {side + 1}: |dist - ref| / bound max {e_min.max():.3f}; |dist - d(idx)| / bound max {e_at.max():.3f}; "
              f"d(idx) / allowed max {slack.max():.9f}")
        assert (np.abs(d - r) <= cr.dist_bound(r, D)).all()                                   # every element
        assert (at <= r * (1 + 2 * (D + 3) * cr.U) + 2 * D * cr.TINY).all()                    # (a) the chosen row is a nearest one up to rounding
        assert (np.abs(d - at) <= cr.dist_bound(at, D)).all()                                 # (b) and dist is the distance to it


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_against_float64(shape, kind):
    x1, x2 = cr.make_cloud(kind, *shape, seed=1000 + sum(shape))
    _check_forward(x1, x2, _forward(x1, x2), f"{shape} {kind}")


@pytest.mark.parametrize("D", [26, 3])
def test_exact_on_integers_ties_and_run_to_run_bits(D):
    x1, x2 = cr.make_integer_cloud(400, 400, D, seed=5 + D)
    r1, j1, r2, j2 = cr.chamfer_ref(x1, x2)
    full = cr.pair_dist(x1[0], x2[0])
    assert ((full == full.min(1, keepdims=True)).sum(1) > 1).sum() >= 50        # genuine ties
    runs = [_forward(x1, x2) for _ in range(5)]
    d1, d2, i1, i2 = runs[0]
    assert (d1.view(np.uint32) == r1.astype(np.float32).view(np.uint32)).all() and (d2.view(np.uint32) == r2.astype(np.float32).view(np.uint32)).all()
    assert (i1 == j1).all() and (i2 == j2).all()                                # first occurrence, exactly
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert a.tobytes() == b.tobytes()


def test_run_to_run_bits_at_the_reference_shape():
    x1, x2 = cr.make_cloud("dup", 1, 8192, 8192, 26, seed=77)
    runs = [_forward(x1, x2) for _ in range(5)]
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert a.tobytes() == b.tobytes()


def test_nan_and_inf_rows_then_a_normal_call():
    x1, x2 = cr.make_cloud("normal", 1, 300, 200, 26, seed=4)
    a, b = x1.copy(), x2.copy()
    a[0, 5, 11] = np.nan          # a query row with a NaN: every distance is NaN
    a[0, 7, 0] = np.inf           # inf against finite rows: +inf; against b's inf row: inf - inf = NaN
    b[0, 3, 0] = np.inf
    d1, d2, i1, i2 = _forward(a, b)
    assert np.isnan(d1[0, 5]) and i1[0, 5] == 0
    assert d1[0, 7] == np.inf and i1[0, 7] == 0                      # all candidates +inf but row 3 (NaN): the lowest index
    assert d2[0, 3] == np.inf and i2[0, 3] == 0                      # b's inf row: +inf to every finite row, NaN to rows 5 and 7
    # every other row: as if rows 5, 7 of a and row 3 of b were not there
    keep_a = np.array([i for i in range(300) if i not in (5, 7)]); keep_b = np.array([j for j in range(200) if j != 3])
    r1, j1, r2, j2 = cr.chamfer_ref(a[:, keep_a], b[:, keep_b])
    assert (np.abs(d1[0, keep_a] - r1[0]) <= cr.dist_bound(r1[0], 26)).all() and (i1[0, keep_a] == keep_b[j1[0]]).all()
    assert (np.abs(d2[0, keep_b] - r2[0]) <= cr.dist_bound(r2[0], 26)).all() and (i2[0, keep_b] == keep_a[j2[0]]).all()
    # every candidate NaN: (NaN, 0) on both sides, whichever workgroup arrives first
    c = x2.copy(); c[0, :, 2] = np.nan
    d1, d2, i1, i2 = _forward(x1, c)
    assert np.isnan(d1).all() and np.isnan(d2).all() and (i1 == 0).all() and (i2 == 0).all()
    # a backward through such values neither faults nor hangs
    t1 = _gpu(a).requires_grad_(True); t2 = _gpu(b).requires_grad_(True)
    o = ChamferDistance()(t1, t2)
    (o[0].sum() + o[1].sum()).backward()
    torch.cuda.synchronize()
    assert t1.grad.shape == t1.shape and t2.grad.shape == t2.shape
    # the device is left usable
    _check_forward(x1, x2, _forward(x1, x2), "after NaN / inf")


def test_empty_and_invalid_sizes():
    chd = ChamferDistance()
    z = lambda *s: torch.zeros(*s, device=DEV)
    d1, d2, i1, i2 = chd(z(0, 5, 26), z(0, 7, 26))
    assert d1.shape == (0, 5) and i2.shape == (0, 7)
    d1, d2, i1, i2 = chd(z(2, 0, 3), z(2, 0, 3))
    assert d1.shape == (2, 0) and d2.shape == (2, 0)
    with pytest.raises(_lib.GsrError, match="no nearest neighbour"):
        chd(z(2, 0, 3), z(2, 4, 3))
    with pytest.raises(_lib.GsrError, match="no nearest neighbour"):
        chd(z(1, 4, 3), z(1, 0, 3))
    x1, x2 = cr.make_cloud("normal", 1, 50, 40, 3, seed=2)
    _check_forward(x1, x2, _forward(x1, x2), "after invalid sizes")


def _backward_case(shape, kind, use_g2=True, x2_grad=True, seed=0):
    B, N, M, D = shape
    x1, x2 = cr.make_cloud(kind, *shape, seed=seed)
    rng = np.random.default_rng(seed + 1)
    g1 = rng.normal(size=(B, N)).astype(np.float32)
    g2 = rng.normal(size=(B, M)).astype(np.float32) if use_g2 else None
    t1 = _gpu(x1).requires_grad_(True); t2 = _gpu(x2).requires_grad_(x2_grad)
    d1, d2, i1, i2 = ChamferDistance()(t1, t2)
    assert not i1.requires_grad and not i2.requires_grad
    loss = (d1 * _gpu(g1)).sum()
    if use_g2:
        loss = loss + (d2 * _gpu(g2)).sum()
    loss.backward()
    rx1, rx2, a1, a2, k1, k2 = cr.backward_ref(x1, x2, i1.cpu().numpy(), i2.cpu().numpy(), g1, g2)    # with the GPU's own indices
    pairs = [("dx1", t1.grad.cpu().numpy(), rx1, a1, k1)]
    if x2_grad:
        pairs.append(("dx2", t2.grad.cpu().numpy(), rx2, a2, k2))
    else:
        assert t2.grad is None
    for name, got, ref, ab, k in pairs:
        bound = cr.backward_bound(ab, k)
        err = np.abs(got - ref)
        print(f"{shape} {kind} g2={use_g2} {name}: max |got - ref| / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}, most terms in a row {k.max()}")
        assert (err <= bound).all()
    return k1, k2


@pytest.mark.parametrize("shape,kind", [((1, 8192, 8192, 26), "normal"), ((2, 65, 4097, 26), "dup"), ((4, 1000, 777, 3), "wide"), ((3, 257, 129, 7), "normal")],
                         ids=["8192x8192x26", "2x65x4097x26", "4x1000x777x3", "3x257x129x7"])
def test_backward_random_g1_g2(shape, kind):
    _backward_case(shape, kind, seed=11)


def test_backward_only_dist1_in_the_loss():
    k1, k2 = _backward_case((2, 65, 4097, 26), "normal", use_g2=False, seed=12)
    assert (k2 == 0).any()            # targets nobody chose: their gradient rows are exact zeros (bound 0)


def test_backward_only_x1_requires_grad():
    _backward_case((3, 257, 129, 7), "normal", x2_grad=False, seed=13)


def test_backward_many_to_one():
    k1, k2 = _backward_case((1, 5000, 3, 64), "normal", seed=14)
    assert k2.max() > 1000            # thousands of atomics meet in one row


def test_function_rejects_other_dtypes_and_module_casts():
    x1, x2 = cr.make_cloud("normal", 1, 100, 90, 26, seed=3)
    with pytest.raises(_lib.GsrError, match="float32"):
        ChamferDistanceFunction.apply(_gpu(x1).double(), _gpu(x2).double())
    for dt in (torch.float64, torch.bfloat16):
        t1 = _gpu(x1).to(dt).requires_grad_(True)
        d1, d2, i1, i2 = ChamferDistance()(t1, _gpu(x2).to(dt))
        assert d1.dtype == torch.float32
        (d1.mean() + d2.mean()).backward()
        assert t1.grad.dtype == dt and torch.isfinite(t1.grad).all()


@pytest.mark.parametrize("variant", ["plain", "view", "float16", "stream"])
def test_drop_in_use_through_a_linear_layer(variant):
    """train_stacked_transformer.py:193-196,245: non-leaf [N,26] predictions, unsqueeze(0), dist1.mean() + dist2.mean(), backward;
    the Linear's weight gradient against the float64 chain.

    Propagated bound, u = 2^-24.  The chamfer op sees the float32 (or float16) predictions P the GPU produced, so the reference
    takes those values and the GPU's indices: dP_ref = backward_ref(P, T, idx, g = 1/N, 1/M), and the op's own error per element is
    e = backward_bound (chamfer_ref).  float16 variant: autograd rounds dP to float16 on the way back, one more relative 2^-11 and,
    for values below float16's normal range, an absolute 2^-25: e16 = e + 2^-11 (|dP_ref| + e) + 2^-25.  The weight gradient is
    the float32 matrix product W.grad[o,f] = sum_n dP[n,o] z[n,f] of N terms in unknown order:
        |W.grad - sum_n dP_ref z| <= sum_n e |z| + (N + 1) u sum_n (|dP_ref| + e) |z|."""
    torch.manual_seed(0)
    N, M, F = 2000, 1500, 16
    width = 52 if variant == "view" else 26
    lin = torch.nn.Linear(F, width).to(DEV)
    z = torch.randn(N, F, device=DEV)
    tgt = torch.randn(M, 26, device=DEV)
    side = torch.cuda.Stream(device=DEV) if variant == "stream" else None
    if side is not None:
        side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side) if side is not None else torch.cuda.stream(torch.cuda.current_stream(DEV)):
        pred = lin(z)
        if variant == "view":
            pred = pred[:, ::2]
            assert not pred.is_contiguous()
        if variant == "float16":
            pred = pred.half()
        assert not pred.is_leaf
        pred.retain_grad()
        dist1, dist2, idx1, idx2 = ChamferDistance()(pred.unsqueeze(0), tgt.unsqueeze(0))
        chamfer = dist1.mean() + dist2.mean()
        chamfer.backward()
    if side is not None:
        side.synchronize()
    torch.cuda.synchronize()
    P = pred.detach().double().cpu().numpy()[None]
    T = tgt.double().cpu().numpy()[None]
    g1 = np.full((1, N), 1.0 / N); g2 = np.full((1, M), 1.0 / M)
    dP, _, a1, _, k1, _ = cr.backward_ref(P, T, idx1.cpu().numpy(), idx2.cpu().numpy(), g1, g2)
    dP, e = dP[0], cr.backward_bound(a1, k1)[0]
    got_dP = pred.grad.double().cpu().numpy()
    if variant == "float16":
        e = e + 2.0 ** -11 * (np.abs(dP) + e) + 2.0 ** -25
    assert (np.abs(got_dP - dP) <= e).all()
    zz = np.abs(z.double().cpu().numpy())
    ref_w = dP.T @ z.double().cpu().numpy()                                  # [26, F]
    bound_w = e.T @ zz + (N + 1) * cr.U * ((np.abs(dP) + e).T @ zz)
    got_w = lin.weight.grad.double().cpu().numpy()
    if variant == "view":
        assert (got_w[1::2] == 0).all()
        got_w = got_w[::2]
    err = np.abs(got_w - ref_w)
    print(f"{variant}: max |W.grad - ref| / bound = {(err / bound_w).max():.4f}; chamfer = {float(chamfer):.6f}")
    assert (err <= bound_w).all()
    ref_loss = cr.dist_to(P, T, idx1.cpu().numpy()).mean() + cr.dist_to(T, P, idx2.cpu().numpy()).mean()
    # each dist within (26 + 3) u of its float64 value, a float32 mean of n <= N values within n u, one more for the final add
    assert abs(float(chamfer.detach()) - ref_loss) <= (N + 26 + 4) * cr.U * ref_loss


def test_second_device_or_current_device_guard():
    """The call runs on the tensors' device whatever torch's current device is."""
    if torch.cuda.device_count() < 2:
        dev = "cuda:0"
    else:
        dev = "cuda:1"
    x1, x2 = cr.make_cloud("normal", 1, 300, 200, 26, seed=8)
    with torch.cuda.device(0):
        d1, d2, i1, i2 = ChamferDistance()(torch.from_numpy(x1).to(dev), torch.from_numpy(x2).to(dev))
    assert str(d1.device) == dev
    _check_forward(x1, x2, (d1.cpu().numpy(), d2.cpu().numpy(), i1.cpu().numpy(), i2.cpu().numpy()), dev)
