"""-m gpu: a plain C program (tests/cabi/absgrad_client.c) drives gsr_forward and gsr_absgrad_backward of libgsr_hip.so directly on
depth_ref.SCENES[1] (P = 64, 40 x 24, partial tiles) under the background and the upstream gradient of tests/absgrad_ref.py: every
refusal with its code and its text, in the header's order, on outputs that hold a pattern and must keep it; P == 0; R == 0 with and
without accumulate; then the result with the signed sums and the same view accumulated onto it, which the Python side holds against
the reference walks by tests/test_gpu_absgrad.py's gates."""
import numpy as np
import pytest

from tests import absgrad_ref as ar
from tests import cabi_client as cc
from tests import depth_ref as dr
from tests.helpers import F32_FAIL_FRAC_MAX, F32_P99_MAX, grad_rows
from tests.test_gpu_absgrad import gate1

pytestmark = pytest.mark.gpu


def test_plain_c_client_absgrad(tmp_path):
    S, dL, w32, w64 = ar.walks(dr.SCENES[1])
    P = int(np.asarray(S.means3D).shape[0])
    assert S.scale_modifier == 1.0                                      # depth_ref's scenes are unscaled
    prob, res = tmp_path / "problem.bin", tmp_path / "result.bin"
    with open(prob, "wb") as f:
        cc.write_scene(f, S)
        f.write(cc.f32(dL))
    cc.run(cc.build(tmp_path, "absgrad_client"), prob, res)
    got = cc.read_result(res, [("R", np.int64, ())] + [(k, np.float32, (P, 2)) for k in ("absgrad", "signed", "twice", "zeros")])
    a, s, twice, zeros = (got[k].astype(np.float64) for k in ("absgrad", "signed", "twice", "zeros"))
    assert int(got["R"]) > 0

    gate1(a, w32, w64, "C client")
    st = grad_rows(s, w32["signed"])
    print("C client, signed sums against the float32 walk:", st)
    assert st["rows"] > 0 and st["fail_frac"] <= F32_FAIL_FRAC_MAX and st["p99"] <= F32_P99_MAX, st
    assert (a >= np.abs(s) * (1 - 1e-5)).all() and (a > 0).any()
    st = grad_rows(twice, 2.0 * a)
    assert st["fail_frac"] == 0.0 and st["max"] <= 1e-5, st              # the same view again, up to the order of the float atomics
    assert not zeros.any() and not np.signbit(zeros).any()
