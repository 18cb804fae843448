"""-m gpu: a plain C program (tests/cabi/normals_client.c) drives the five calls of include/gsr_normals.h directly: every refusal with its
code and its exact text, in the header's order, on outputs that hold a pattern and must keep it; the calls with nothing to do; then the
calls themselves on 257 Gaussians and a 17 x 65 image with alpha holes (tiles crossed in both axes), which the Python side holds
against tests/normals_ref.py under the tolerances of tests/test_gpu_gaussian_normals.py and tests/test_gpu_normal_loss.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import normals_ref as nr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_client(tmp_path):
    pkg = os.path.join(ROOT, "gaussian_transformer_amd")
    exe = str(tmp_path / "normals_client")
    cc = shutil.which("gcc") or "gcc"
    subprocess.check_call([cc, "-std=c11", "-O1", os.path.join(ROOT, "tests", "cabi", "normals_client.c"), "-I", os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", "-L", pkg, "-lgsr_hip", "-L/opt/rocm/lib", "-lamdhip64", "-lm",
                           f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def rel(x, x64):
    scale = np.abs(x64).max()
    return float(np.abs(np.asarray(x, np.float64) - x64).max() / scale)


def test_plain_c_client_normals(tmp_path):
    P, H, W = 257, 17, 65
    means, scales, q, V = nr.rows(P)
    G = np.random.default_rng(9).normal(size=(P, 3)).astype(np.float32)
    depth, alpha, N = nr.maps(H, W, holes=True)
    tx, ty = nr.TANFOV
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, np.float32)).tobytes()
    prob, res = tmp_path / "problem.bin", tmp_path / "result.bin"
    with open(prob, "wb") as f:
        f.write(np.asarray([P, H, W], dtype=np.int32).tobytes())
        f.write(np.asarray([tx, ty, nr.ALPHA_MIN], dtype=np.float32).tobytes())
        for a in (means, scales, q, V, G, depth, alpha, N):
            f.write(f32(a))
    exe = build_client(tmp_path)
    r = subprocess.run([exe, str(prob), str(res)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "normals C client ok" in r.stdout
    raw = open(res, "rb").read()
    px = H * W
    sizes = [("normals", np.float32, 3 * P), ("axis", np.int32, P), ("g_rots", np.float32, 4 * P), ("out2", np.float32, 2), ("surf", np.float32, 3 * px),
             ("g_depth", np.float32, px), ("g_alpha", np.float32, px), ("g_normals", np.float32, 3 * px), ("g_depth_quarter", np.float32, px)]
    got, off = {}, 0
    for name, dt, cnt in sizes:
        got[name] = np.frombuffer(raw, dtype=dt, count=cnt, offset=off)
        off += 4 * cnt
    assert off == len(raw)

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
    r = subprocess.run([build_client(tmp_path), "--refusals"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "normals C client: refusals ok" in r.stdout, r.stdout + r.stderr
