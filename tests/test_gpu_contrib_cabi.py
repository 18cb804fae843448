"""-m gpu: a plain C program (tests/cabi/contrib_client.c) drives gsr_forward, gsr_contrib_accumulate and gsr_contrib_read of
libgsr_hip.so directly on depth_ref.SCENES[2] (P = 500, 64 x 48): every refusal of the two calls with its code and its text, in the
header's order, on rows that hold a pattern and must keep it; P == 0 and R == 0; the all-NULL read; then one view and the same view
again, whose rows the Python side compares byte for byte with the public collector's and with integer arithmetic."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from gaussian_transformer_amd.rasterizer import ContributionStats, GaussianRasterizer, collect_contribution
from tests import depth_ref as dr
from tests.test_gpu_depth import scene, tensors

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW = np.dtype([("sum_q32", "<u8"), ("max_bits", "<u4"), ("count", "<u4")])


def test_plain_c_client_contrib(tmp_path):
    S = scene(dr.SCENES[2])
    P, M = int(np.asarray(S.means3D).shape[0]), int(np.asarray(S.shs).shape[1])
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, np.float32)).tobytes()
    prob, res = tmp_path / "problem.bin", tmp_path / "result.bin"
    with open(prob, "wb") as f:
        f.write(np.asarray([P, S.sh_degree, M, S.W, S.H], dtype=np.int32).tobytes())
        f.write(np.asarray([S.tanfovx, S.tanfovy], dtype=np.float32).tobytes())
        for a in (S.bg, S.means3D, S.shs, S.opacities, S.scales, S.rotations, S.viewmatrix, S.projmatrix, S.campos):
            f.write(f32(a))
    pkg = os.path.join(ROOT, "gaussian_transformer_amd")
    exe = str(tmp_path / "contrib_client")
    cc = shutil.which("gcc") or "gcc"
    cmd = [cc, "-std=c11", "-O1", os.path.join(ROOT, "tests", "cabi", "contrib_client.c"), "-I", os.path.join(ROOT, "include"),
           "-I/opt/rocm/include", "-L", pkg, "-lgsr_hip", "-L/opt/rocm/lib", "-lamdhip64", "-lm",
           f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    r = subprocess.run([exe, str(prob), str(res)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "contrib C client ok" in r.stdout
    raw = open(res, "rb").read()
    R = int(np.frombuffer(raw, dtype=np.int64, count=1)[0])
    one = np.frombuffer(raw, dtype=ROW, count=P, offset=8)
    two = np.frombuffer(raw, dtype=ROW, count=P, offset=8 + 16 * P)
    off = 8 + 32 * P
    w_sum = np.frombuffer(raw, dtype=np.float32, count=P, offset=off)
    w_max = np.frombuffer(raw, dtype=np.float32, count=P, offset=off + 4 * P)
    n_pix = np.frombuffer(raw, dtype=np.int32, count=P, offset=off + 8 * P)
    assert off + 12 * P == len(raw) and R > 0

    # the public collector on the same scene: the same bytes
    rs, inp = tensors(S, grad=False)
    st = ContributionStats(P, "cuda")
    with collect_contribution(st), torch.no_grad():
        GaussianRasterizer(rs)(**inp)
    want = st.rows.cpu().numpy().view(ROW).reshape(P)
    assert want["count"].any()
    np.testing.assert_array_equal(one, want)
    # the same view again, in integers
    np.testing.assert_array_equal(two["sum_q32"], 2 * one["sum_q32"])
    np.testing.assert_array_equal(two["count"], 2 * one["count"])
    np.testing.assert_array_equal(two["max_bits"], one["max_bits"])
    # the three outputs, read by two calls with NULLs among them
    np.testing.assert_array_equal(w_sum, (two["sum_q32"].astype(np.float64) * 2.0 ** -32).astype(np.float32))
    np.testing.assert_array_equal(w_max.view(np.uint32), two["max_bits"])
    np.testing.assert_array_equal(n_pix, two["count"].astype(np.int32))
