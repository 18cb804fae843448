"""The Python side of the plain-C clients under tests/cabi/: build one against libgsr_hip.so, run it, write the scene block of a problem
file (the block tests/cabi/client_common.h cabi_scene_read() reads) and read a result file back.  tests/test_cabi_common_host.py holds
the writer against the C reader without a GPU."""
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CABI = os.path.join(ROOT, "tests", "cabi")
CC = shutil.which("gcc") or "gcc"
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include"]


def build(tmp_path, name, extra_flags=()):
    """tests/cabi/<name>.c linked against the package's libgsr_hip.so, as tmp_path/<name>: the path of the program."""
    pkg = os.path.join(ROOT, "gaussian_transformer_amd")
    exe = str(tmp_path / name)
    subprocess.check_call([CC, "-std=c11", "-O1", *extra_flags, os.path.join(CABI, name + ".c"), *INCLUDES, "-L", pkg, "-lgsr_hip",
                           "-L/opt/rocm/lib", "-lamdhip64", "-lm", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def ok_line(exe):
    """"<name> C client ok" of tests/cabi/<name>_client.c ("views loss" for views_loss_client), "C client ok" of c_client.c."""
    label = os.path.basename(exe)[:-len("_client")].replace("_", " ")
    return "C client ok" if label == "c" else f"{label} C client ok"


def run(exe, *args, timeout=120, ok=None):
    """Runs a client to exit code 0 and its ok line (`ok`: another line to ask for); returns what it printed."""
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (ok or ok_line(exe)) in r.stdout, r.stdout + r.stderr
    return r.stdout


def f32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).tobytes()


def write_scene(f, S, dims=None):
    """The scene block from an oracle Scene: int32 P D M W H (`dims`: these five, instead of S's own), float32 tanfovx tanfovy
    scale_modifier, then float32 bg, means3D, shs, opacities, scales, rotations, viewmatrix, projmatrix, campos."""
    P, M = int(np.asarray(S.means3D).shape[0]), int(np.asarray(S.shs).shape[1])
    f.write(np.asarray(dims if dims is not None else [P, S.sh_degree, M, S.W, S.H], dtype=np.int32).tobytes())
    f.write(np.asarray([S.tanfovx, S.tanfovy, S.scale_modifier], dtype=np.float32).tobytes())
    for a in (S.bg, S.means3D, S.shs, S.opacities, S.scales, S.rotations, S.viewmatrix, S.projmatrix, S.campos):
        f.write(f32(a))


def read_result(path, fields):
    """A result file as {name: array} from (name, dtype, shape) triples in the file's order; the file holds these and nothing more."""
    raw = open(path, "rb").read()
    got, off = {}, 0
    for name, dtype, shape in fields:
        count = int(np.prod(shape, dtype=np.int64))
        assert off + count * np.dtype(dtype).itemsize <= len(raw), (name, off, len(raw))
        got[name] = np.frombuffer(raw, dtype=dtype, count=count, offset=off).reshape(shape)
        off += got[name].nbytes
    assert off == len(raw), (off, len(raw))
    return got
