"""-m gpu: a plain C program (tests/cabi/pose_client.c) drives gsr_forward, gsr_backward and gsr_pose_backward of libgsr_hip.so through
include/gsr_pose.h at P = 1501 -- the camera gradients against tests/pose_ref.py in float64 at the gate of tests/test_gpu_pose.py
(twice the float32 reference's own error + 1e-6), the refusals, NULL outputs, P = 0 and R = 0."""
import numpy as np
import pytest

from gaussian_transformer_amd import synth
from tests import cabi_client as cc
from tests import pose_ref
from tests.helpers import oracle_scene

pytestmark = pytest.mark.gpu


def test_plain_c_client_pose(tmp_path):
    P, W, H, D = 1501, 100, 52, 2
    sc = synth.make_scene(P=P, width=W, height=H, sh_degree=D, max_sh_degree=3, s0=0.05, seed=6)
    S = oracle_scene(sc, scale_modifier=0.9)
    dL = np.random.default_rng(5).normal(size=(3, H, W)).astype(np.float32)
    g64, g32 = pose_ref.colour_grads(S, dL, "f64"), pose_ref.colour_grads(S, dL, "f32")
    keys = ("viewmatrix", "projmatrix", "campos")
    bounds = [2 * pose_ref.rel_err(g32[k], g64[k]) + 1e-6 for k in keys]
    M = int(np.asarray(S.shs).shape[1])
    prob = tmp_path / "problem.bin"
    with open(prob, "wb") as f:
        cc.write_scene(f, S, dims=[P, D, M, W, H])
        f.write(cc.f32(dL))
        f.write(np.concatenate([g64[k] for k in keys]).astype(np.float64).tobytes())
        f.write(np.asarray(bounds, np.float64).tobytes())
    print(cc.run(cc.build(tmp_path, "pose_client"), prob))
