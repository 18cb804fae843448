"""-m gpu: a plain C program (tests/cabi/normals_client.c) drives the five calls of include/gsr_normals.h directly: every refusal with its
code and its exact text, in the header's order, on outputs that hold a pattern and must keep it; the calls with nothing to do; then the
calls themselves on 257 Gaussians and a 17 x 65 image with alpha holes (tiles crossed in both axes), which the Python side holds
against tests/normals_ref.py under the tolerances of tests/test_gpu_gaussian_normals.py and tests/test_gpu_normal_loss.py."""
import numpy as np
import pytest
import torch

from tests import cabi_client as cc
from tests import normals_ref as nr

pytestmark = pytest.mark.gpu


def rel(x, x64):
    scale = np.abs(x64).max()
    return float(np.abs(np.asarray(x, np.float64) - x64).max() / scale)


def test_plain_c_client_normals(tmp_path):
    P, H, W = 257, 17, 65
    means, scales, q, V = nr.rows(P)
    G = np.random.default_rng(9).normal(size=(P, 3)).astype(np.float32)
    depth, alpha, N = nr.maps(H, W, holes=True)
    tx, ty = nr.TANFOV
    prob, res = tmp_path / "problem.bin", tmp_path / "result.bin"
    with open(prob, "wb") as f:
        f.write(np.asarray([P, H, W], dtype=np.int32).tobytes())
        f.write(np.asarray([tx, ty, nr.ALPHA_MIN], dtype=np.float32).tobytes())
        for a in (means, scales, q, V, G, depth, alpha, N):
            f.write(cc.f32(a))
    cc.run(cc.build(tmp_path, "normals_client"), prob, res)
    px = H * W
    got = cc.read_result(res, [("normals", np.float32, 3 * P), ("axis", np.int32, P), ("g_rots", np.float32, 4 * P), ("out2", np.float32, 2),
                               ("surf", np.float32, 3 * px), ("g_depth", np.float32, px), ("g_alpha", np.float32, px), ("g_normals", np.float32, 3 * px),
                               ("g_depth_quarter", np.float32, px)])

    r64, r32 = nr.gaussian_normals(means, scales, q, V, torch.float64), nr.gaussian_normals(means, scales, q, V, torch.float32)
    assert np.array_equal(got["axis"], r64["axis"])
    n64 = r64["normals"].numpy().reshape(-1)
    assert np.abs(got["normals"] - n64).max() <= 2.0 * np.abs(r32["normals"].numpy().reshape(-1).astype(np.float64) - n64).max() + 1e-7
    g64 = nr.gaussian_normals_grad(means, scales, q, V, G, torch.float64).numpy().reshape(-1)
    g32 = nr.gaussian_normals_grad(means, scales, q, V, G, torch.float32).numpy().reshape(-1).astype(np.float64)
    assert np.abs(got["g_rots"] - g64).max() <= 2.0 * np.abs(g32 - g64).max() + 1e-7

    l64, l32 = nr.loss(depth, alpha, N, tx, ty, dtype=torch.float64), nr.loss(depth, alpha, N, tx, ty, dtype=torch.float32)
    assert got["out2"][1] == np.float32(l64["fraction"]) and 0 < l64["fraction"] < 1
    assert not got["surf"].reshape(3, H, W)[:, ~l64["valid"].numpy()].any()
    for name, key in (("out2", "loss"), ("surf", "surf"), ("g_depth", "g_depth"), ("g_alpha", "g_alpha"), ("g_normals", "g_normals")):
        w64 = np.asarray(l64[key], np.float64).reshape(-1)
        v = got[name][:1] if name == "out2" else got[name]
        assert rel(v, w64) <= 2.0 * rel(np.asarray(l32[key], np.float64).reshape(-1), w64) + 1e-7, name
    assert np.array_equal(got["g_depth_quarter"], got["g_depth"] * np.float32(0.25)) and got["g_depth"].any()


def test_the_refusals_alone_need_no_device(tmp_path):
    """The same refusals on made-up addresses: the stand-alone form a host-side sanitizer build of the client runs."""
    cc.run(cc.build(tmp_path, "normals_client"), "--refusals", timeout=60, ok="normals C client: refusals ok")
