"""-m gpu: the per-Gaussian normals (include/gsr_normals.h: gsr_gaussian_normals_*) against tests/normals_ref.py, and the normal map end
to end -- render(normals=True) -> gaussian_normals -> the feature route -- against the oracle's feature-map reference
(tests/features_ref.py) chained through the float64 normal reference.

P: 0, 1 and the wave and block edges (63, 64, 65, 255, 256, 257), and 4001.  The two decisions are held to the reference exactly: the
argmin of float32 scales is exact, and tests/test_normals_ref_host.py asserts that no row of these seeds has |n_v . p_v| below
1e-5 |p_v|.  Values and gradients: within twice the float32 reference's own maximum error against float64 on the same inputs, plus 1e-7.
"""
import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib, synth
from gaussian_transformer_amd.model import GaussianParams
from gaussian_transformer_amd.rasterizer import GaussianRasterizationSettings, gaussian_normals
from gaussian_transformer_amd.render import PipelineParams, TorchCamera, render
from tests import features_ref as fr
from tests import normals_ref as nr
from tests.helpers import F32_P99_MAX, GRAD_RTOL, grad_rows, oracle_scene
from tests.test_normals_ref_host import GPU_P

pytestmark = pytest.mark.gpu
DEV = "cuda"


def settings(V, H=4, W=4):
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=DEV)
    return GaussianRasterizationSettings(H, W, 0.5, 0.5, t(np.zeros(3)), 1.0, t(V), t(np.eye(4)), 0, t(np.zeros(3)), False, False)


def native(means, scales, q, V, G=None):
    """(normals, axis, dL/drotations or None) from the two C calls."""
    P = len(means)
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=DEV)
    m, s, r, v = t(means), t(scales), t(q), t(V)
    out = torch.full((P, 3), float("nan"), device=DEV)
    axis = torch.full((P,), -1, dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    _lib.call("gsr_gaussian_normals_forward", st, P, _lib.ptr(m), _lib.ptr(s), _lib.ptr(r), _lib.ptr(v), _lib.ptr(out), _lib.ptr(axis))
    g = None
    if G is not None:
        g = torch.full((P, 4), float("nan"), device=DEV)
        gn = t(G)
        _lib.call("gsr_gaussian_normals_backward", st, P, _lib.ptr(r), _lib.ptr(v), _lib.ptr(axis), _lib.ptr(gn), _lib.ptr(g))
        g = g.cpu().numpy()
    return out.cpu().numpy(), axis.cpu().numpy(), g


@pytest.mark.parametrize("P", GPU_P)
def test_against_float64_within_twice_the_float32_reference(P):
    means, scales, q, V = nr.rows(P)
    G = np.random.default_rng(9).normal(size=(P, 3)).astype(np.float32)
    got_n, got_axis, got_g = native(means, scales, q, V, G)
    r64 = nr.gaussian_normals(means, scales, q, V, torch.float64)
    r32 = nr.gaussian_normals(means, scales, q, V, torch.float32)
    assert np.array_equal(got_axis, r64["axis"])                          # the axis and the flip, every row
    if P == 0:
        assert got_n.shape == (0, 3) and got_g.shape == (0, 4)
        return
    assert np.isfinite(got_n).all() and np.isfinite(got_g).all()
    n64 = r64["normals"].numpy()
    e, e32 = np.abs(got_n - n64).max(), np.abs(r32["normals"].numpy().astype(np.float64) - n64).max()
    g64 = nr.gaussian_normals_grad(means, scales, q, V, G, torch.float64).numpy()
    g32 = nr.gaussian_normals_grad(means, scales, q, V, G, torch.float32).numpy().astype(np.float64)
    eg, eg32 = np.abs(got_g - g64).max(), np.abs(g32 - g64).max()
    print(f"P {P}: normals {e:.2e}/{e32:.2e}  dL_drots {eg:.2e}/{eg32:.2e}")
    assert e <= 2.0 * e32 + 1e-7 and eg <= 2.0 * eg32 + 1e-7, (e, e32, eg, eg32)


def test_hand_built_rows():
    V = nr.rows(1)[3]
    eye = np.eye(4, dtype=np.float32)
    ident = np.array([1, 0, 0, 0], np.float32)
    # ties of the scales: two equal smallest -> the lower index; three equal -> 0
    scales = np.array([[2, 1, 1], [1, 1, 1], [1, 2, 1], [3, 2, 1], [1, 1, 2], [0.5, 0.5, 0.25]], np.float32)
    P = len(scales)
    means = np.tile(np.array([[0.3, -0.2, 4.0]], np.float32), (P, 1))
    _n, axis, _ = native(means, scales, np.tile(ident, (P, 1)), eye)
    assert list(axis & 3) == [1, 0, 0, 2, 0, 2]
    # a dot product of exactly 0 does not flip: the normal (1, 0, 0) against a mean on the plane x = 0; one just either side does what it must
    m = np.array([[0.0, 1.5, 3.0], [1e-3, 1.5, 3.0], [-1e-3, 1.5, 3.0]], np.float32)
    n, axis, _ = native(m, np.tile(np.array([[0.1, 1, 1]], np.float32), (3, 1)), np.tile(ident, (3, 1)), eye)
    assert list(axis) == [0, 4, 0] and np.array_equal(n, np.array([[1, 0, 0], [-1, 0, 0], [1, 0, 0]], np.float32))
    # a non-unit quaternion gives the polynomial's value, not a normalised one
    q = np.array([[2.0, 0.5, -1.0, 0.25], [0.1, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]], np.float32)
    sc = np.array([[1, 0.1, 1], [1, 1, 0.1], [0.1, 1, 1]], np.float32)
    mm = np.tile(np.array([[0.2, 0.1, 2.0]], np.float32), (3, 1))
    n, axis, g = native(mm, sc, q, V, np.ones((3, 3), np.float32))
    want = nr.gaussian_normals(mm, sc, q, V, torch.float64)
    assert np.array_equal(axis, want["axis"]) and np.abs(n - want["normals"].numpy()).max() <= 1e-5
    norms = np.linalg.norm(n, axis=1)
    # column 1 of q = (2, .5, -1, .25) as given is (-2, 0.375, 1.5), of length 2.53; the other two rows have x = y = z = 0: the identity
    assert abs(norms[0] - np.sqrt(4 + 0.375 ** 2 + 2.25)) < 1e-5 and abs(norms[1] - 1.0) < 1e-6 and abs(norms[2] - 1.0) < 1e-6
    g64 = nr.gaussian_normals_grad(mm, sc, q, V, np.ones((3, 3)), torch.float64).numpy()
    assert np.abs(g - g64).max() <= 1e-5 * max(1.0, np.abs(g64).max())


def test_the_autograd_function_gives_rotations_their_gradient_and_nothing_else():
    means, scales, q, V = nr.rows(257)
    t = lambda a: torch.tensor(a, device=DEV).requires_grad_(True)
    m, s, r = t(means), t(scales), t(q)
    rs = settings(V)
    n = gaussian_normals(m, s, r, rs)
    got_n, _axis, got_g = native(means, scales, q, V, np.ones((257, 3), np.float32))
    assert np.array_equal(n.detach().cpu().numpy(), got_n)
    n.sum().backward()
    assert m.grad is None and s.grad is None and np.array_equal(r.grad.cpu().numpy(), got_g)
    with torch.no_grad():
        assert gaussian_normals(m, s, r, rs).grad_fn is None
    assert gaussian_normals(m[:0], s[:0], r[:0], rs).shape == (0, 3)


# ---- end to end: 160 x 96, about 2 000 Gaussians ----
@pytest.fixture(scope="module")
def scene():
    sc = synth.make_scene(P=2000, width=160, height=96, sh_degree=1, s0=0.05, seed=4)
    return sc, TorchCamera(sc.camera, DEV), torch.tensor(np.asarray(sc.bg, np.float32), device=DEV)


def test_the_normal_map_is_the_feature_map_of_the_normals(scene):
    sc, cam, bg = scene
    pc = GaussianParams.from_synthetic(sc, DEV)
    P = 2000
    with torch.no_grad():
        a = render(cam, pc, PipelineParams(), bg, normals=True)
        from gaussian_transformer_amd.rasterizer import camera_settings
        rs = camera_settings(cam, bg, 1.0, pc.active_sh_degree, False)
        n_g = gaussian_normals(pc.get_xyz, pc.get_scaling, pc.get_rotation, rs)
        b = render(cam, pc, PipelineParams(), bg, features=n_g)
        assert a["normals"].shape == (3, 96, 160) and "features" not in a
        assert torch.equal(a["normals"], b["features"]) and torch.equal(a["render"], b["render"])
        assert float(a["normals"].abs().max()) > 0.1
        for C in (1, 61):
            F = torch.rand((P, C), device=DEV)
            both = render(cam, pc, PipelineParams(), bg, features=F, normals=True)
            alone = render(cam, pc, PipelineParams(), bg, features=F)
            assert both["features"].shape == (C, 96, 160) and both["normals"].shape == (3, 96, 160)
            # the same channels in another chunk of the feature kernel: the same terms, possibly contracted differently
            assert float((both["features"] - alone["features"]).abs().max()) <= 1e-5
            assert float((both["normals"] - a["normals"]).abs().max()) <= 1e-5
        with pytest.raises(_lib.GsrError, match="features may have at most 61 columns beside it, got 62"):
            render(cam, pc, PipelineParams(), bg, features=torch.rand((P, 62), device=DEV), normals=True)


def test_rotation_gradients_against_the_oracle_chained_through_the_normal_reference(scene):
    sc, cam, bg = scene
    S = oracle_scene(sc)
    P = 2000
    V = np.asarray(S.viewmatrix, np.float32).reshape(4, 4)
    r64n = nr.gaussian_normals(S.means3D, S.scales, S.rotations, V, torch.float64)
    F = r64n["normals"].numpy().astype(np.float32)                       # what the map blends
    G = fr.map_grad(S, 3)
    want = {}
    for prec, dt in (("f32", torch.float32), ("f64", torch.float64)):
        t = fr.trick_forward(S, F, prec)
        g = fr.trick_backward(t, G, prec)
        chain = nr.gaussian_normals_grad(S.means3D, S.scales, S.rotations, V, g["dL_dfeatures"], dt).numpy().astype(np.float64)
        want[prec] = np.asarray(g["dL_drots"], np.float64).reshape(P, 4) + chain
    pc = GaussianParams.from_synthetic(sc, DEV)
    out = render(cam, pc, PipelineParams(), bg, normals=True)
    (out["normals"] * torch.tensor(G, device=DEV)).sum().backward()
    # GaussianParams normalises its quaternions, which are unit already: the gradient with respect to the activated rotations is wanted
    q = torch.tensor(np.asarray(sc.rotations, np.float32), device=DEV).requires_grad_(True)
    rs_out = render(cam, _Activated(pc, q), PipelineParams(), bg, normals=True)
    (rs_out["normals"] * torch.tensor(G, device=DEV)).sum().backward()
    got = q.grad.cpu().numpy().astype(np.float64)
    st, base, v32 = grad_rows(got, want["f64"]), grad_rows(want["f32"], want["f64"]), grad_rows(got, want["f32"])
    print("dL/drotations of <G, normals>:", st["p99"], base["p99"], v32["p99"], v32["fail_frac"])
    assert st["fail_frac"] <= 2.0 * base["fail_frac"] + 1e-3 and st["p99"] <= max(GRAD_RTOL, 2.0 * base["p99"]), (st, base)
    assert v32["fail_frac"] <= 2e-3 and v32["p99"] <= F32_P99_MAX, v32
    assert np.isfinite(pc._rotation.grad.cpu().numpy()).all()


class _Activated:
    """A model's activated tensors with the rotations replaced by a leaf, so that dL/drotations as the rasterizer sees it can be read."""

    def __init__(self, pc, q):
        self.get_xyz, self.get_opacity, self.get_scaling, self.get_features = (x.detach() for x in (pc.get_xyz, pc.get_opacity, pc.get_scaling, pc.get_features))
        self.get_rotation, self.active_sh_degree, self.max_sh_degree = q, pc.active_sh_degree, pc.max_sh_degree
