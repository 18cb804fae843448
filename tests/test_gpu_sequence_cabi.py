"""-m gpu: a plain C program (tests/cabi/sequence_client.c) drives the sequence entry points of libgsr_hip.so directly -- a box
sort against the restatement of tests/sequence_ref.py, bit for bit, a two-camera visibility pass against the radii of the float32
CPU oracle, and the error paths."""
import numpy as np
import pytest

from gaussian_transformer_amd import synth
from oracle import ref
from tests import cabi_client as cc
from tests import sequence_ref as sr
from tests.helpers import oracle_scene

pytestmark = pytest.mark.gpu


def test_plain_c_client_sequence(tmp_path):
    P, D, col, n = 5000, 26, 17, 40
    rows = sr.planted_rows(P, D, col, n, seed=31)
    want_rows, want_perm, want_count = sr.box_sort_vec(rows, col, n)
    sc = synth.make_scene(2000, 256, 256, sh_degree=0, seed=12, zmin=-2.0)
    cams = [sc.camera, synth.identity_camera(120, 200, tanfovx=0.3)]
    r32 = ref.get("f32")
    radii = []
    for cam in cams:
        S = oracle_scene(sc, W=cam.image_width, H=cam.image_height, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
                         viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, campos=cam.camera_center)
        radii.append(np.asarray(r32.forward(S)["radii"], dtype=np.int32))
    assert 0 < (radii[0] > 0).sum() < sc.P
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    prob = tmp_path / "problem.bin"
    with open(prob, "wb") as f:
        f.write(i32([P, D, col, n, sc.P, len(cams)]).tobytes())
        for a in (rows, want_rows, want_perm, i32([want_count]), f32(sc.means3D), f32(sc.scales), f32(sc.rotations),
                  f32([c.world_view_transform for c in cams]), f32([c.full_proj_transform for c in cams]),
                  f32([c.tanfovx for c in cams]), f32([c.tanfovy for c in cams]), i32([c.image_width for c in cams]),
                  i32([c.image_height for c in cams]), i32(radii)):
            f.write(np.ascontiguousarray(a).tobytes())
    cc.run(cc.build(tmp_path, "sequence_client"), prob)
