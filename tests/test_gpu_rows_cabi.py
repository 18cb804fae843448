"""-m gpu: a plain C program (tests/cabi/rows_client.c) drives gsr_rows_unpack and gsr_rows_grad_pack of libgsr_hip.so directly
at P = 1501, D = 26, B = 3 -- both results bit for bit against tests/rows_ref.py -- and their error paths."""
import numpy as np
import pytest

from tests import cabi_client as cc
from tests import rows_ref as rr

pytestmark = pytest.mark.gpu


def test_plain_c_client_rows(tmp_path):
    P, D, B = 1501, 26, 3
    rows = rr.planted_rows(P, D, seed=21)
    want = rr.unpack_ref(rows)
    arenas = rr.planted_arenas(B, P, D, seed=22)
    want_grad = rr.pack_ref(arenas, P, D)
    prob = tmp_path / "problem.bin"
    with open(prob, "wb") as f:
        f.write(np.asarray([P, D, B], dtype=np.int32).tobytes())
        for t in [rows] + [want[k] for k in ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")] + arenas + [want_grad]:
            f.write(np.ascontiguousarray(t.numpy()).tobytes())
    cc.run(cc.build(tmp_path, "rows_client"), prob)
