"""CPU tests of the Chamfer distance's host side: the drop-in module name, the header / ctypes contract, validation without a
GPU, and the float64 reference (tests/chamfer_ref.py) with the error bound the GPU tests assert."""
import os
import re

import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib
from tests import chamfer_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_drop_in_module_name():
    from chamfer_distance import ChamferDistance, ChamferDistanceFunction
    from gaussian_transformer_amd import chamfer
    assert ChamferDistance is chamfer.ChamferDistance and ChamferDistanceFunction is chamfer.ChamferDistanceFunction
    m = ChamferDistance()                                   # train_stacked_transformer.py:184
    assert isinstance(m, torch.nn.Module) and not list(m.parameters())
    assert issubclass(ChamferDistanceFunction, torch.autograd.Function)


def test_header_declares_exactly_what_the_ctypes_stub_binds():
    header = open(os.path.join(ROOT, "include", "gsr_chamfer.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)     # declarations only: the comment block speaks of gsr_chamfer_workspace too
    decls = dict(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", code, flags=re.S))
    assert set(decls) == {"gsr_chamfer_workspace", "gsr_chamfer_forward", "gsr_chamfer_backward"}
    assert set(_lib.CHAMFER_SIGNATURES) == set(decls)
    for name, args in decls.items():
        assert len(_lib.CHAMFER_SIGNATURES[name][1]) == len(args.split(",")), name
    assert not set(_lib.CHAMFER_SIGNATURES) & set(_lib.SIGNATURES)
    assert "#define GSR_ABI_VERSION 2" in open(os.path.join(ROOT, "include", "gsr.h")).read()   # purely additive
    assert "parity unpinned" in header.lower()
    from gaussian_transformer_amd import build
    assert "chamfer.hip" in build.SOURCES
    lib = _lib.load()                                       # built by build(): the three symbols resolve
    for name in decls:
        assert hasattr(lib, name)


def test_validation_names_the_argument_before_any_native_call(monkeypatch):
    from chamfer_distance import ChamferDistance
    def no_native():
        raise AssertionError("the native library was reached")
    monkeypatch.setattr(_lib, "load", no_native)
    chd = ChamferDistance()
    a, b = torch.zeros(1, 5, 26), torch.zeros(1, 7, 26)
    with pytest.raises(RuntimeError, match=r"xyz1 must be on a HIP device.*no CPU fallback"):
        chd(a, b)
    with pytest.raises(_lib.GsrError, match="xyz1"):
        chd(a.requires_grad_(True), b)
    meta = lambda *s: torch.empty(*s, device="meta")        # neither CPU nor HIP: still refused by name
    with pytest.raises(_lib.GsrError, match="xyz1 must be on a HIP device"):
        chd(meta(1, 5, 26), meta(1, 7, 26))
    with pytest.raises(_lib.GsrError, match="xyz1 must be a torch.Tensor"):
        chd(np.zeros((1, 5, 26), np.float32), b)
    if not torch.cuda.is_available():
        return
    dev = "cuda:0"
    g = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(_lib.GsrError, match="xyz2 must be on a HIP device"):
        chd(g(1, 5, 26), b)
    with pytest.raises(_lib.GsrError, match=r"xyz2 has batch size B=2 but xyz1 has B=1"):
        chd(g(1, 5, 26), g(2, 7, 26))
    with pytest.raises(_lib.GsrError, match=r"xyz2 has D=3 features per row but xyz1 has D=26"):
        chd(g(1, 5, 26), g(1, 7, 3))
    with pytest.raises(_lib.GsrError, match=r"xyz1 has D=65"):
        chd(g(1, 5, 65), g(1, 7, 65))
    with pytest.raises(_lib.GsrError, match=r"xyz2 must have shape \[B, N, D\]"):
        chd(g(1, 5, 26), g(7, 26))


def test_shape_validation_without_a_device():
    """B / D mismatches are found before any native call, by a function of the shapes alone."""
    from gaussian_transformer_amd import chamfer
    chamfer._validate_shapes((2, 5, 26), (2, 9, 26))
    with pytest.raises(_lib.GsrError, match="xyz2 has batch size B=3 but xyz1 has B=2"):
        chamfer._validate_shapes((2, 5, 26), (3, 5, 26))
    with pytest.raises(_lib.GsrError, match="xyz2 has D=3 features per row but xyz1 has D=26"):
        chamfer._validate_shapes((2, 5, 26), (2, 5, 3))
    with pytest.raises(_lib.GsrError, match="supported: 1..64"):
        chamfer._validate_shapes((2, 5, 0), (2, 5, 0))
    with pytest.raises(_lib.GsrError, match="supported: 1..64"):
        chamfer._validate_shapes((2, 5, 65), (2, 5, 65))


@pytest.mark.parametrize("D", [3, 26])
def test_reference_agrees_with_kdtree(D):
    from scipy.spatial import cKDTree
    x1, x2 = cr.make_cloud("normal", 2, 700, 450, D, seed=D)
    d1, i1, d2, i2 = cr.chamfer_ref(x1, x2)
    for b in range(2):
        a, c = x1[b].astype(np.float64), x2[b].astype(np.float64)
        for (q, t, d, i) in ((a, c, d1[b], i1[b]), (c, a, d2[b], i2[b])):
            kd, ki = cKDTree(t).query(q, k=1)
            assert (ki == i).all()
            np.testing.assert_allclose(kd ** 2, d, rtol=1e-12, atol=0)
    np.testing.assert_allclose(cr.dist_to(x1, x2, i1), d1, rtol=1e-14)


def test_reference_first_minimum_on_exact_ties():
    x1, x2 = cr.make_integer_cloud(400, 400, 26, seed=5)
    d1, i1, d2, i2 = cr.chamfer_ref(x1, x2)
    full = cr.pair_dist(x1[0], x2[0])
    assert (i1[0] == full.argmin(1)).all() and (i2[0] == full.argmin(0)).all()
    assert (cr.pair_dist(x1[0], x2[0], np.float32) == full).all()          # every float32 operation is exact on this cloud
    ties = ((full == full.min(1, keepdims=True)).sum(1) > 1).sum()
    assert ties >= 50, ties                                                 # the duplicated targets give genuine ties


@pytest.mark.parametrize("kind", ["normal", "dup", "wide"])
@pytest.mark.parametrize("D", [3, 7, 26, 64])
def test_float32_difference_form_stays_inside_dist_bound(kind, D):
    """Pins the bound the GPU tests use: a float32 evaluation (sequential sum, no FMA) against float64, every pair."""
    x1, x2 = cr.make_cloud(kind, 1, 512, 384, D, seed=100 + D)
    d64 = cr.pair_dist(x1[0], x2[0])
    d32 = cr.pair_dist(x1[0], x2[0], np.float32).astype(np.float64)
    err = np.abs(d32 - d64)
    print(kind, D, "worst error / (u * ref) =", float((err / (cr.U * d64 + 1e-300)).max()))
    assert (err <= cr.dist_bound(d64, D)).all()
    assert (err <= (D + 2) * cr.U * d64 + D * cr.TINY).all()               # the first-order bound already holds: (D + 3) has margin


def test_backward_formula_by_directional_finite_difference():
    """L = sum g1 dist1 + sum g2 dist2 in float64; its derivative along a random direction against the formula's."""
    rng = np.random.default_rng(3)
    x1, x2 = (a.astype(np.float64) for a in cr.make_cloud("normal", 2, 60, 45, 26, seed=9))
    g1, g2 = rng.normal(size=(2, 60)), rng.normal(size=(2, 45))
    v1, v2 = rng.normal(size=x1.shape), rng.normal(size=x2.shape)
    def loss(a, b):
        d1, _, d2, _ = cr.chamfer_ref(a, b)
        return (g1 * d1).sum() + (g2 * d2).sum()
    _, i1, _, i2 = cr.chamfer_ref(x1, x2)
    dx1, dx2, a1, a2, k1, k2 = cr.backward_ref(x1, x2, i1, i2, g1, g2)
    eps = 1e-6
    fd = (loss(x1 + eps * v1, x2 + eps * v2) - loss(x1 - eps * v1, x2 - eps * v2)) / (2 * eps)
    an = (dx1 * v1).sum() + (dx2 * v2).sum()
    assert abs(fd - an) <= 1e-7 * (np.abs(dx1 * v1).sum() + np.abs(dx2 * v2).sum()), (fd, an)
    assert (k1 >= 1).all() and k1.sum() == 2 * (60 + 45) and k2.sum() == 2 * (60 + 45)
    # one side only: the other side's direct term disappears, its rows keep what was scattered into them
    ex1, ex2, *_ = cr.backward_ref(x1, x2, i1, i2, g1, None)
    fd = ((g1 * cr.chamfer_ref(x1 + eps * v1, x2 + eps * v2)[0]).sum() - (g1 * cr.chamfer_ref(x1 - eps * v1, x2 - eps * v2)[0]).sum()) / (2 * eps)
    an = (ex1 * v1).sum() + (ex2 * v2).sum()
    assert abs(fd - an) <= 1e-7 * (np.abs(ex1 * v1).sum() + np.abs(ex2 * v2).sum())
