"""scripts/benchkit.py, what the thirteen feature benchmarks share: the two summaries, the alternation, the writer and the scene helper
on literal inputs, and every script's command line as far as --help (no GPU, no native library; no benchmark is started)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gaussian_transformer_amd import synth
from scripts import benchkit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = ["absgrad_bench.py", "chamfer_bench.py", "contrib_bench.py", "density_bench.py", "depth_bench.py", "features_bench.py", "mcmc_bench.py",
           "normals_bench.py", "pose_bench.py", "rows_render_bench.py", "sequence_bench.py", "sparse_adam_bench.py", "views_loss_bench.py"]
XS = [3, 1, 2, 4, 10]


def test_stats_quantiles():
    """median 3, min 1, p10 1.4, p90 7.6, n 5.  All exact but p90: the form the scripts have always used (np.quantile, kept as it was so that
    no committed figure changes) interpolates at 0.9 * 4 - 3, which is not 0.6 in binary, and gives 7.6000000000000005, the float next to 7.6.
    One unit in the last place is what the test allows there, and nothing anywhere else."""
    s = benchkit.stats_quantiles(XS)
    assert list(s) == ["median_ms", "min_ms", "p10_ms", "p90_ms", "n"]
    assert (s["median_ms"], s["min_ms"], s["p10_ms"], s["n"]) == (3.0, 1.0, 1.4, 5) and type(s["n"]) is int
    assert abs(s["p90_ms"] - 7.6) <= math.ulp(7.6)


def test_stats_minmax():
    assert benchkit.stats_minmax(XS, count="reps") == {"min_ms": 1, "median_ms": 3, "max_ms": 10, "reps": 5}
    assert benchkit.stats_minmax(XS) == benchkit.stats_minmax(XS, count="reps")
    assert benchkit.stats_minmax(XS, count="steps") == {"min_ms": 1, "median_ms": 3, "max_ms": 10, "steps": 5}
    assert benchkit.stats_minmax(XS, count=None) == {"min_ms": 1, "median_ms": 3, "max_ms": 10}
    assert benchkit.stats_minmax([1.23456, 2.0], digits=4)["min_ms"] == 1.2346
    assert benchkit.stats_minmax([1.23456, 2.0])["min_ms"] == 1.23456


def run_alternate(names, **kw):
    """alternate() over functions that log their names, under a fake window that hands out 0, 1, 2, ... as the samples."""
    order, clock = [], iter(range(100))

    def fake_timed(fn):
        return next(clock), fn()
    ts = benchkit.alternate({k: (lambda k=k: order.append(k)) for k in names}, reps=2, warmup=1, timed=fake_timed, **kw)
    return "".join(order), ts


def test_alternate_rotates_and_drops_the_warmup():
    order, ts = run_alternate("abc")
    assert order == "abc" "bca" "cab"
    # samples 0 - 2 were the warm-up; b, c, a took 3, 4, 5 and c, a, b took 6, 7, 8
    assert ts == {"a": [5, 7], "b": [3, 8], "c": [4, 6]}
    assert list(ts) == ["a", "b", "c"]


def test_alternate_fixed_order():
    order, ts = run_alternate("abc", rotate=False)
    assert order == "abc" * 3
    assert ts == {"a": [3, 6], "b": [4, 7], "c": [5, 8]}


def test_alternate_of_two_is_the_flip():
    order, ts = run_alternate("ab")
    assert order == "ab" "ba" "ab"
    assert ts == {"a": [3, 4], "b": [2, 5]}


def test_write_json(tmp_path, capsys):
    obj = {"device": "x", "results": [{"P": 3, "step": {"median_ms": 0.25}}]}
    indented = tmp_path / "not" / "yet" / "there" / "bench.json"
    benchkit.write_json(obj, str(indented))
    with open(indented) as f:
        assert json.load(f) == obj
    assert indented.read_text().count("\n") > 1
    assert capsys.readouterr().out == f"wrote {indented}\n"
    line = tmp_path / "line.json"
    benchkit.write_json(obj, str(line), indent=None)
    assert line.read_text() == json.dumps(obj) + "\n"
    assert capsys.readouterr().out == json.dumps(obj) + "\n"


def test_scene_helpers_on_the_cpu():
    sc = synth.make_scene(P=8, width=32, height=16, sh_degree=1)
    x = benchkit.scene_tensors(sc, "cpu")
    assert {k: tuple(v.shape) for k, v in x.items()} == dict(means3D=(8, 3), shs=(8, 4, 3), opacities=(8, 1), scales=(8, 3), rotations=(8, 4))
    assert all(v.dtype == torch.float32 and v.is_contiguous() and not v.requires_grad for v in x.values())
    assert all(v.requires_grad for v in benchkit.scene_tensors(sc, "cpu", requires_grad=True).values())
    for k, v in x.items():
        assert np.array_equal(v.numpy(), np.asarray(getattr(sc, k), np.float32).reshape(v.shape))

    cam = sc.camera
    f32 = lambda a: np.asarray(a, np.float32)
    rs = benchkit.scene_settings(sc, "cpu")
    assert rs._fields == ("image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix", "sh_degree",
                          "campos", "prefiltered", "debug")
    assert (rs.image_height, rs.image_width, rs.tanfovx, rs.tanfovy) == (16, 32, cam.tanfovx, cam.tanfovy)
    assert type(rs.image_height) is int and type(rs.image_width) is int
    assert (rs.scale_modifier, rs.sh_degree, rs.prefiltered, rs.debug) == (1.0, 1, False, False)
    expected = dict(bg=f32(sc.bg), viewmatrix=f32(cam.world_view_transform).reshape(4, 4), projmatrix=f32(cam.full_proj_transform).reshape(4, 4),
                    campos=f32(cam.camera_center))
    for k, want in expected.items():
        got = getattr(rs, k)
        assert got.dtype == torch.float32 and not got.requires_grad and tuple(got.shape) == want.shape and np.array_equal(got.numpy(), want), k
    assert expected["bg"].shape == (3,) and expected["campos"].shape == (3,)

    # the three knobs: a background in place of the scene's, the SH degree, and camera tensors that take a gradient
    black = torch.zeros(3)
    rs0 = benchkit.scene_settings(sc, "cpu", bg=black, sh_degree=0)
    assert rs0.bg is black and rs0.sh_degree == 0 and torch.equal(rs0.viewmatrix, rs.viewmatrix)
    pose = benchkit.scene_settings(sc, "cpu", camera_grad=True)
    assert pose.viewmatrix.requires_grad and pose.projmatrix.requires_grad and pose.campos.requires_grad and not pose.bg.requires_grad
    assert torch.equal(pose.projmatrix.detach(), rs.projmatrix)


def test_importing_benchkit_loads_no_library():
    code = ("import sys, torch; from scripts import benchkit; from gaussian_transformer_amd import _lib; "
            "sys.exit(int(torch.cuda.is_initialized()) + 2 * int(_lib._lib is not None))")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0


@pytest.mark.parametrize("script", SCRIPTS)
def test_help(script):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--out" in r.stdout and ("--steps" if script == "rows_render_bench.py" else "--reps") in r.stdout and "--warmup" in r.stdout
