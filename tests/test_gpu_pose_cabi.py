"""-m gpu: a plain C program (tests/cabi/pose_client.c) drives gsr_forward, gsr_backward and gsr_pose_backward of libgsr_hip.so through
include/gsr_pose.h at P = 1501 -- the camera gradients against tests/pose_ref.py in float64 at the gate of tests/test_gpu_pose.py
(twice the float32 reference's own error + 1e-6), the refusals, NULL outputs, P = 0 and R = 0."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from gaussian_transformer_amd import synth
from tests import pose_ref
from tests.helpers import oracle_scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_c_client_pose(tmp_path):
    P, W, H, D = 1501, 100, 52, 2
    sc = synth.make_scene(P=P, width=W, height=H, sh_degree=D, max_sh_degree=3, s0=0.05, seed=6)
    S = oracle_scene(sc, scale_modifier=0.9)
    dL = np.random.default_rng(5).normal(size=(3, H, W)).astype(np.float32)
    g64, g32 = pose_ref.colour_grads(S, dL, "f64"), pose_ref.colour_grads(S, dL, "f32")
    keys = ("viewmatrix", "projmatrix", "campos")
    bounds = [2 * pose_ref.rel_err(g32[k], g64[k]) + 1e-6 for k in keys]
    M = int(np.asarray(S.shs).shape[1])
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, np.float32)).tobytes()
    prob = tmp_path / "problem.bin"
    with open(prob, "wb") as f:
        f.write(np.asarray([P, D, M, W, H], dtype=np.int32).tobytes())
        f.write(np.asarray([S.tanfovx, S.tanfovy, S.scale_modifier], dtype=np.float32).tobytes())
        for a in (S.bg, S.means3D, S.shs, S.opacities, S.scales, S.rotations, S.viewmatrix, S.projmatrix, S.campos, dL):
            f.write(f32(a))
        f.write(np.concatenate([g64[k] for k in keys]).astype(np.float64).tobytes())
        f.write(np.asarray(bounds, np.float64).tobytes())
    pkg = os.path.join(ROOT, "gaussian_transformer_amd")
    exe = str(tmp_path / "pose_client")
    cc = shutil.which("gcc") or "gcc"
    cmd = [cc, "-std=c11", "-O1", os.path.join(ROOT, "tests", "cabi", "pose_client.c"), "-I", os.path.join(ROOT, "include"),
           "-I/opt/rocm/include", "-L", pkg, "-lgsr_hip", "-L/opt/rocm/lib", "-lamdhip64", "-lm",
           f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    r = subprocess.run([exe, str(prob)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pose C client ok" in r.stdout
