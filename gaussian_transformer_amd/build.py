"""Builds libgsr_hip.so (the C-ABI HIP library, include/gsr.h) in-tree with hipcc for gfx950.

    python -m gaussian_transformer_amd.build [--force] [--verbose]

hipcc cross-compiles without a GPU.  The .so is git-ignored but travels to the GPU box with the
repo snapshot.  No torch headers are involved: the library links only against libamdhip64.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "_obj")
LIB = os.path.join(HERE, "libgsr_hip.so")
ARCH = "gfx950"

# translation unit -> extra flags
# -ffp-contract=off on the per-Gaussian stages: bit-parity of radii / tile rects / depth keys with
# the float32 CPU restatement (see csrc/gsr_device.h).  The compositing kernels keep FMA
# contraction and use native no-return float atomics.
SOURCES = {
    "gsr_api.hip": [],
    "preprocess.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],
    "pergauss_bwd.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],
    "binning.hip": ["-ffp-contract=off"],     # the tile-row span test must round exactly as in preprocess.hip
    "depth_order.hip": ["-ffp-contract=off"],
    "tile_lists.hip": ["-ffp-contract=off"],      # same tile-row spans as preprocess.hip, bit for bit
    "supertile_sort.hip": ["-ffp-contract=off"],  # likewise
    # -fno-slp-vectorize: the SLP pass packs pairs of scalar f32 ops into v_pk_* and pays for it in v_mov shuffles and
    # registers (bwd: 86 -> 71 VGPRs, 5 -> 7 waves/SIMD; fwd 178 -> 157 us, bwd 387 -> 352 us at config 3, measured)
    "composite_fwd.hip": ["-fno-slp-vectorize"],
    "composite_bwd.hip": ["-munsafe-fp-atomics", "-fno-slp-vectorize"],
    "ssim_loss.hip": [],
    "knn.hip": [],
    "adam.hip": [],
    # FMA contraction left ON: the (D + 3) ulp bound of a difference-form distance holds with or without it (tests/chamfer_ref.py) and
    # it halves the inner loop; -munsafe-fp-atomics: the scattered gradient term uses the native float atomic add, as composite_bwd.hip;
    # -fno-slp-vectorize: packed f32 ops have no higher rate here and cost v_movs (ISA of the D = 26 loop per 4 distances: 104 v_pk_* + 27 v_mov + 49 others
    # packed, 208 v_sub / v_fmac + 16 others scalar; read from the ISA, not timed)
    "chamfer.hip": ["-munsafe-fp-atomics", "-fno-slp-vectorize"],
    "sequence.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],   # as preprocess.hip: gsr_visible_union's radii must round as gsr_forward's
    "density.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],    # record's norm and the split children round as written (include/gsr_density.h)
    # as density.hip: a draw's t_j is one IEEE double multiply and the regularisers' gradients round as written (include/gsr_mcmc.h)
    "mcmc.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],
    "rows.hip": [],               # copies and float adds only (include/gsr_rows.h): nothing to contract
    # as composite_bwd.hip, whose staging, replica rows and LDS reduction it shares (csrc/composite_common.h) under recurrences of its own
    # for the depth and alpha maps (include/gsr_depth.h): native float atomic add, no packed f32 pairs
    "depth_maps.hip": ["-munsafe-fp-atomics", "-fno-slp-vectorize"],
    # as depth_maps.hip, whose walks it restates for C channels per Gaussian (include/gsr_features.h): the alpha decisions are the colour
    # pass's bit for bit under the same flags
    "feature_maps.hip": ["-munsafe-fp-atomics", "-fno-slp-vectorize"],
    # as pergauss_bwd.hip, whose chain (csrc/pergauss_chain.h) it calls up to the terms the camera gradient shares with dL/dmeans3D
    # (include/gsr_pose.h)
    "pose_grad.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],
    # as depth_maps.hip, whose forward walk it restates with an integer reduction per entry (include/gsr_contrib.h): FMA contraction as
    # there, so the weights are depth_fwd_kernel's bits; its atomics are integer ones, so no float-atomic flag
    "contrib_stats.hip": ["-fno-slp-vectorize"],
    # as depth_maps.hip, whose reverse walk it restates for the colour loss with |.| per (pixel, Gaussian) term (include/gsr_absgrad.h)
    "absgrad.hip": ["-munsafe-fp-atomics", "-fno-slp-vectorize"],
    # as pergauss_bwd.hip: the argmin of the scales and the sign of n_v . p_v round as written (include/gsr_normals.h)
    "normals.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],
}
COMMON = ["-O3", "-fPIC", "-std=c++17", f"--offload-arch={ARCH}", "-Wall", "-Wno-unused-result", "-fno-gpu-rdc"]


def hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: the HIP extension cannot be built on this machine")
    return exe


def _dep_headers():
    """What every object file depends on besides its own source: each header of csrc/ and include/, and this file (the flags)."""
    inc = os.path.join(HERE, "..", "include")
    return [os.path.join(d, h) for d in (CSRC, inc) for h in sorted(os.listdir(d)) if h.endswith(".h")] + [os.path.abspath(__file__)]


def _newer(src_list, target) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in src_list)


def build_variant(tag: str, defines, verbose: bool = False, force: bool = False) -> str:
    """Variant build: every TU recompiled with extra -D flags into libgsr_hip_<tag>.so (ablations; "dbg" = the capacity-assert build,
    -DGSR_DEBUG_BOUNDS, csrc/gsr_internal.h).  Loaded instead of the product library through GSR_LIB_PATH."""
    cc = hipcc()
    out = os.path.join(HERE, f"libgsr_hip_{tag}.so")
    odir = os.path.join(OBJ, tag)
    os.makedirs(odir, exist_ok=True)
    headers = _dep_headers()
    jobs, objs = [], []
    for src, extra in SOURCES.items():
        s, o = os.path.join(CSRC, src), os.path.join(odir, src.replace(".hip", ".o"))
        objs.append(o)
        if force or _newer([s] + headers, o):
            jobs.append([cc, "-c", s, "-o", o] + COMMON + extra + [f"-D{d}" for d in defines])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed:\n{r.stdout}\n{r.stderr}")
    with ThreadPoolExecutor(max_workers=min(4, max(1, len(jobs)))) as ex:
        list(ex.map(run, jobs))
    if force or jobs or _newer(objs, out):
        subprocess.check_call([cc, "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", out] + objs)
    return out


def build_debug_bounds(force: bool = False, verbose: bool = False) -> str:
    return build_variant("dbg", ["GSR_DEBUG_BOUNDS"], verbose=verbose, force=force)


def build_hip(force: bool = False, verbose: bool = False) -> str:
    os.makedirs(OBJ, exist_ok=True)
    headers = _dep_headers()
    cc = hipcc()
    jobs = []
    for src, extra in SOURCES.items():
        s = os.path.join(CSRC, src)
        o = os.path.join(OBJ, src.replace(".hip", ".o"))
        if force or _newer([s] + headers, o):
            jobs.append((src, [cc, "-c", s, "-o", o] + COMMON + extra))

    def run(job):
        name, cmd = job
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {name}:\n{r.stdout}\n{r.stderr}")
        if verbose and r.stderr.strip():
            print(r.stderr)
        return name

    with ThreadPoolExecutor(max_workers=min(4, max(1, len(jobs)))) as ex:
        list(ex.map(run, jobs))
    objs = [os.path.join(OBJ, s.replace(".hip", ".o")) for s in SOURCES]
    if force or jobs or _newer(objs, LIB):
        cmd = [cc, "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
    return LIB


if __name__ == "__main__":
    print(build_hip(force="--force" in sys.argv, verbose="--verbose" in sys.argv or "-v" in sys.argv))
    if "--debug-bounds" in sys.argv:
        print(build_debug_bounds(force="--force" in sys.argv, verbose="--verbose" in sys.argv or "-v" in sys.argv))
