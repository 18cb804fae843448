"""-m gpu: a plain C program (tests/cabi/absgrad_client.c) drives gsr_forward and gsr_absgrad_backward of libgsr_hip.so directly on
depth_ref.SCENES[1] (P = 64, 40 x 24, partial tiles) under the background and the upstream gradient of tests/absgrad_ref.py: every
refusal with its code and its text, in the header's order, on outputs that hold a pattern and must keep it; P == 0; R == 0 with and
without accumulate; then the result with the signed sums and the same view accumulated onto it, which the Python side holds against
the reference walks by tests/test_gpu_absgrad.py's gates."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import absgrad_ref as ar
from tests import depth_ref as dr
from tests.helpers import F32_FAIL_FRAC_MAX, F32_P99_MAX, grad_rows
from tests.test_gpu_absgrad import gate1

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_c_client_absgrad(tmp_path):
    S, dL, w32, w64 = ar.walks(dr.SCENES[1])
    P, M = int(np.asarray(S.means3D).shape[0]), int(np.asarray(S.shs).shape[1])
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, np.float32)).tobytes()
    prob, res = tmp_path / "problem.bin", tmp_path / "result.bin"
    with open(prob, "wb") as f:
        f.write(np.asarray([P, S.sh_degree, M, S.W, S.H], dtype=np.int32).tobytes())
        f.write(np.asarray([S.tanfovx, S.tanfovy], dtype=np.float32).tobytes())
        for a in (S.bg, S.means3D, S.shs, S.opacities, S.scales, S.rotations, S.viewmatrix, S.projmatrix, S.campos, dL):
            f.write(f32(a))
    pkg = os.path.join(ROOT, "gaussian_transformer_amd")
    exe = str(tmp_path / "absgrad_client")
    cc = shutil.which("gcc") or "gcc"
    cmd = [cc, "-std=c11", "-O1", os.path.join(ROOT, "tests", "cabi", "absgrad_client.c"), "-I", os.path.join(ROOT, "include"),
           "-I/opt/rocm/include", "-L", pkg, "-lgsr_hip", "-L/opt/rocm/lib", "-lamdhip64", "-lm",
           f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    r = subprocess.run([exe, str(prob), str(res)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "absgrad C client ok" in r.stdout
    raw = open(res, "rb").read()
    R = int(np.frombuffer(raw, dtype=np.int64, count=1)[0])
    rows = lambda k: np.frombuffer(raw, dtype=np.float32, count=2 * P, offset=8 + 8 * P * k).reshape(P, 2).astype(np.float64)
    a, s, twice, zeros = rows(0), rows(1), rows(2), rows(3)
    assert 8 + 32 * P == len(raw) and R > 0

    gate1(a, w32, w64, "C client")
    st = grad_rows(s, w32["signed"])
    print("C client, signed sums against the float32 walk:", st)
    assert st["rows"] > 0 and st["fail_frac"] <= F32_FAIL_FRAC_MAX and st["p99"] <= F32_P99_MAX, st
    assert (a >= np.abs(s) * (1 - 1e-5)).all() and (a > 0).any()
    st = grad_rows(twice, 2.0 * a)
    assert st["fail_frac"] == 0.0 and st["max"] <= 1e-5, st              # the same view again, up to the order of the float atomics
    assert not zeros.any() and not np.signbit(zeros).any()
