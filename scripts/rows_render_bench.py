"""Times rendering B cameras from flat Gaussian rows, forward + backward, two ways in one process on one card.

    python scripts/rows_render_bench.py [--steps 50] [--warmup 10] [--out profiles/rows/bench.json]

The stacked trainer's shape: P = 65 536 rows of 26 columns, B = 4 cameras at 800 x 800.  Per step, with rows.requires_grad:
  views : B x render_fused(cam, unflatten_gaussians(rows)), the images' gradients fed to one torch.autograd.backward
  rows  : rows.render_rows(cameras, rows), the same
Both launch the same rasterizer kernels; `rows` replaces the per-camera contiguous() copies and the slice / reshape backward
nodes by one gsr_rows_unpack and one gsr_rows_grad_pack.  The two alternate inside every step; a step's time is the host clock
from before the forward calls to after a device synchronise behind the backward pass.  Reported: min / median / max wall
milliseconds per step for both, and the device time of the two new kernels alone (events around a run of launches, per launch).
The two must agree (images equal, gradients within 1e-4 of the largest entry: the reverse pass uses float atomics by default) or
the script fails.  One JSON line to --out.  Needs a HIP device."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

import benchkit
from gaussian_transformer_amd import _lib, synth
from gaussian_transformer_amd.model import GaussianParams
from gaussian_transformer_amd.rasterizer import arena_floats
from gaussian_transformer_amd.render import PipelineParams, TorchCamera, render_fused
from gaussian_transformer_amd.rows import render_rows
from gaussian_transformer_amd.sequence import flatten_gaussians, unflatten_gaussians

P, B, W, H = 65536, 4, 800, 800
TANFOVX = (0.5773502691896257, 0.5, 0.45, 0.65)


def views_step(cams, rows, pipe, bg, G):
    images = [render_fused(cam, unflatten_gaussians(rows), pipe, bg)["render"] for cam in cams]
    torch.autograd.backward(images, G)
    return images


def rows_step(cams, rows, pipe, bg, G):
    images = render_rows(cams, rows, pipe, bg)["renders"]
    torch.autograd.backward(images, G)
    return images


FORMS = (("views", views_step), ("rows", rows_step))


def kernel_times(rows, reps=200):
    """Device microseconds per launch of gsr_rows_unpack and gsr_rows_grad_pack (B arenas) at this shape."""
    lib = _lib.load()
    Pn, D = rows.shape
    K = (D - 14) // 3
    dev = rows.device
    stream = torch.cuda.current_stream(dev).cuda_stream
    outs = [torch.empty(Pn * w + 16, device=dev) for w in (3, 3, 3 * (K - 1), 1, 3, 4)]
    arenas = [torch.randn(arena_floats(Pn, K), device=dev) for _ in range(B)]
    grad = torch.empty((Pn, D), device=dev)
    ptrs = (C.c_void_p * B)(*[a.data_ptr() for a in arenas])
    unpack = lambda: _lib.check(lib.gsr_rows_unpack(stream, Pn, D, rows.data_ptr(), *[o.data_ptr() for o in outs]), "gsr_rows_unpack")
    pack = lambda: _lib.check(lib.gsr_rows_grad_pack(stream, Pn, D, B, ptrs, grad.data_ptr()), "gsr_rows_grad_pack")
    res = {}
    for name, fn in (("rows_unpack_us", unpack), ("rows_grad_pack_us", pack)):
        for _ in range(20):
            fn()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        res[name] = t0.elapsed_time(t1) * 1e3 / reps
    res["unpack_bytes_moved"] = Pn * (2 * D - 3) * 4                      # rows read, the six buffers written
    res["grad_pack_bytes_moved"] = Pn * (B * (D - 3) + D) * 4             # B arenas read, grad_rows written
    return res


def main():
    args = benchkit.parse(benchkit.parser(50, 10, "rows", reps_flag="--steps"))
    dev = "cuda:0"
    sc = synth.make_scene(P, W, H, sh_degree=1, s0=0.01, seed=7)
    rows = flatten_gaussians(GaussianParams.from_synthetic(sc, dev, requires_grad=False)).contiguous().requires_grad_()
    cams = [TorchCamera(synth.identity_camera(W, H, tanfovx=t), dev) for t in TANFOVX]
    pipe, bg = PipelineParams(), torch.zeros(3, device=dev)
    G = [torch.tensor(np.random.default_rng(70 + b).normal(size=(3, H, W)).astype(np.float32) / (3 * H * W), device=dev) for b in range(B)]
    ms = {n: [] for n, _ in FORMS}
    first = {}
    for step in range(args.warmup + args.steps):
        for name, fn in FORMS:                                            # alternating: both see the same box noise
            rows.grad = None
            _dev_ms, t, images = benchkit.timed_dev_wall(lambda: fn(cams, rows, pipe, bg, G))
            if step == 0:
                first[name] = ([im.detach().clone() for im in images], rows.grad.clone())
            if step >= args.warmup:
                ms[name].append(t)
    for a, b in zip(first["views"][0], first["rows"][0]):
        if not torch.equal(a, b):
            raise SystemExit("render_rows and render_fused disagree on an image")
    ga, gb = first["views"][1], first["rows"][1]
    dg = float((ga - gb).abs().max()) / float(ga.abs().max())
    if not dg <= 1e-4:
        raise SystemExit(f"render_rows and render_fused disagree on the row gradient: {dg:.3e} of the largest entry")
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "what": "forward + backward of B renders from rows, wall ms per step",
              "P": P, "D": int(rows.shape[1]), "B": B, "W": W, "H": H, "warmup": args.warmup,
              "views": benchkit.stats_minmax(ms["views"], count="steps"), "rows": benchkit.stats_minmax(ms["rows"], count="steps"), "grad_max_diff_over_max": dg}
    result["rows_median_over_views_median"] = result["rows"]["median_ms"] / result["views"]["median_ms"]
    result["kernels"] = kernel_times(rows.detach())
    benchkit.write_json(result, args.out, indent=None)


if __name__ == "__main__":
    main()
