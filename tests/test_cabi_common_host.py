"""What the plain-C clients share, without a GPU: tests/cabi/common_selftest.c includes tests/cabi/client_common.h and stands in for
the few HIP calls it makes with malloc / memcpy / memset, so it links against neither the HIP runtime nor libgsr_hip.so.  Held here:
the three refusal macros pass on a call that matches and fail on a wrong code, a wrong text, a written output or a missing message;
and the scene block is one format on both sides -- what tests/cabi_client.py write_scene() writes, cabi_scene_read() reads back byte
for byte, and a file one byte short is refused."""
import os
import subprocess

import numpy as np
import pytest

from oracle import ref
from tests import cabi_client as cc


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cabi") / "common_selftest")
    subprocess.check_call([cc.CC, "-std=c11", "-O1", "-Wall", "-Werror", os.path.join(cc.CABI, "common_selftest.c"), *cc.INCLUDES, "-o", exe])
    return exe


def small_scene():
    P, M, W, H = 3, 4, 5, 3
    rng = np.random.default_rng(17)
    a = lambda *shape: rng.normal(size=shape).astype(np.float32)
    return ref.Scene(W=W, H=H, tanfovx=0.37, tanfovy=0.61, viewmatrix=a(4, 4), projmatrix=a(4, 4), campos=a(3), means3D=a(P, 3), opacities=a(P, 1),
                     bg=a(3), sh_degree=1, shs=a(P, M, 3), scales=a(P, 3), rotations=a(P, 4), scale_modifier=0.9)


def test_refusal_macros_catch_what_they_pin(selftest):
    cc.run(selftest, ok="common selftest ok", timeout=60)


def test_scene_block_is_one_format_on_both_sides(selftest, tmp_path):
    S = small_scene()
    prob, res = tmp_path / "problem.bin", tmp_path / "result.bin"
    with open(prob, "wb") as f:
        cc.write_scene(f, S)
    wrote = open(prob, "rb").read()
    assert len(wrote) == 5 * 4 + 3 * 4 + 4 * (3 + 3 * 3 + 3 * 4 * 3 + 3 + 3 * 3 + 3 * 4 + 16 + 16 + 3)
    cc.run(selftest, prob, res, ok="common selftest: scene ok", timeout=60)
    assert open(res, "rb").read() == wrote
    # the fields are where the format says: the header, and a value of every array
    got = cc.read_result(res, [("dims", np.int32, 5), ("par", np.float32, 3), ("bg", np.float32, 3), ("means3D", np.float32, (3, 3)),
                               ("shs", np.float32, (3, 4, 3)), ("opacities", np.float32, 3), ("scales", np.float32, (3, 3)),
                               ("rotations", np.float32, (3, 4)), ("viewmatrix", np.float32, 16), ("projmatrix", np.float32, 16), ("campos", np.float32, 3)])
    assert got["dims"].tolist() == [3, 1, 4, 5, 3] and got["par"].tolist() == [np.float32(0.37), np.float32(0.61), np.float32(0.9)]
    for k in ("bg", "means3D", "shs", "scales", "rotations", "campos"):
        assert np.array_equal(got[k], getattr(S, k)), k
    assert np.array_equal(got["opacities"], S.opacities[:, 0]) and np.array_equal(got["projmatrix"], S.projmatrix.reshape(16))

    # `dims` replaces the five integers and nothing else
    with open(prob, "wb") as f:
        cc.write_scene(f, S, dims=[3, 0, 4, 5, 3])
    assert open(prob, "rb").read() == np.asarray([3, 0, 4, 5, 3], np.int32).tobytes() + wrote[20:]


@pytest.mark.parametrize("cut, code, said", [(1, 3, "short problem file"), (-1, 3, "bytes after the scene block")])
def test_a_file_of_another_length_is_refused(selftest, tmp_path, cut, code, said):
    prob = tmp_path / "problem.bin"
    with open(prob, "wb") as f:
        cc.write_scene(f, small_scene())
    raw = open(prob, "rb").read()
    open(prob, "wb").write(raw[:-1] if cut > 0 else raw + b"\0")
    r = subprocess.run([selftest, str(prob), str(tmp_path / "result.bin")], capture_output=True, text=True, timeout=60)
    assert r.returncode == code and said in r.stdout, r.stdout + r.stderr


def test_result_reader_wants_the_whole_file_and_no_more(tmp_path):
    path = tmp_path / "result.bin"
    open(path, "wb").write(np.int64(7).tobytes() + np.arange(6, dtype=np.float32).tobytes())
    fields = [("R", np.int64, ()), ("rows", np.float32, (3, 2))]
    got = cc.read_result(path, fields)
    assert int(got["R"]) == 7 and got["rows"].tolist() == [[0, 1], [2, 3], [4, 5]]
    with pytest.raises(AssertionError):
        cc.read_result(path, fields[:1])                     # bytes left over
    with pytest.raises(AssertionError):
        cc.read_result(path, fields + [("more", np.float32, 1)])
