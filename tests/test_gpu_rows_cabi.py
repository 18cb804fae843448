"""-m gpu: a plain C program (tests/cabi/rows_client.c) drives gsr_rows_unpack and gsr_rows_grad_pack of libgsr_hip.so directly
at P = 1501, D = 26, B = 3 -- both results bit for bit against tests/rows_ref.py -- and their error paths."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import rows_ref as rr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    pkg = os.path.join(ROOT, "gaussian_transformer_amd")
    exe = str(tmp_path / "rows_client")
    cc = shutil.which("gcc") or "gcc"
    cmd = [cc, "-std=c11", "-O1", os.path.join(ROOT, "tests", "cabi", "rows_client.c"), "-I", os.path.join(ROOT, "include"),
           "-I/opt/rocm/include", "-L", pkg, "-lgsr_hip", "-L/opt/rocm/lib", "-lamdhip64", "-lm",
           f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    r = subprocess.run([exe, str(prob)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rows C client ok" in r.stdout
