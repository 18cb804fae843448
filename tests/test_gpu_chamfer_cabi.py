"""-m gpu: a plain C program (tests/cabi/chamfer_client.c) drives the Chamfer entry points of libgsr_hip.so directly -- forward and
backward on a 100 x 80 x 26 problem against values computed here in float64 (tests/chamfer_ref.py), and the error paths."""
import numpy as np
import pytest

from tests import cabi_client as cc
from tests import chamfer_ref as cr

pytestmark = pytest.mark.gpu


def test_plain_c_client_chamfer(tmp_path):
    B, N, M, D = 1, 100, 80, 26
    x1, x2 = cr.make_cloud("normal", B, N, M, D, seed=21)
    rng = np.random.default_rng(22)
    g1 = rng.normal(size=(B, N)).astype(np.float32); g2 = rng.normal(size=(B, M)).astype(np.float32)
    d1, i1, d2, i2 = cr.chamfer_ref(x1, x2)
    dx1, dx2, a1, a2, k1, k2 = cr.backward_ref(x1, x2, i1, i2, g1, g2)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    # tolerances: the bounds of chamfer_ref plus half an ulp for rounding the expected value itself to float32
    tol = [cr.dist_bound(d1, D) + cr.U * d1, cr.dist_bound(d2, D) + cr.U * d2,
           cr.backward_bound(a1, k1) + cr.U * np.abs(dx1), cr.backward_bound(a2, k2) + cr.U * np.abs(dx2)]
    prob = tmp_path / "problem.bin"
    with open(prob, "wb") as f:
        f.write(np.array([B, N, M, D], dtype=np.int32).tobytes())
        for a in (x1, x2, g1, g2, f32(d1), f32(d2), i1.astype(np.int32), i2.astype(np.int32), f32(dx1), f32(dx2), *map(f32, tol)):
            f.write(np.ascontiguousarray(a).tobytes())
    cc.run(cc.build(tmp_path, "chamfer_client"), prob)
