#!/usr/bin/env python3
"""What the camera gradients cost (informational; bench.py is the headline metric): forward + L1 + backward of one camera

  (a) without camera gradients -- the settings' viewmatrix, projmatrix and campos are constants: _RasterizeGaussians, as before;
  (b) with them -- the three tensors require grad: _RasterizeGaussiansPose, i.e. the same forward and reverse pass, then
      gsr_pose_backward (include/gsr_pose.h: pose_terms_kernel + pose_sum_kernel) on the reverse pass's workspace.

One process; the two variants alternate inside every repetition on the same inputs and target, each timed with device events around
forward + loss + backward.  Also timed alone: gsr_pose_backward over back-to-back launches on one reverse pass's workspace (both
kernels; the split per kernel, next to pergauss_bwd_kernel of the same reverse pass, comes from running this script under a kernel
trace, in a run of its own: --trace-friendly keeps that run short).

    python scripts/pose_bench.py [--reps 30] [--warmup 5] [--configs cfg2_table_300k_800 cfg3_synth_1M_1080p] [--out profiles/pose/bench.json]
"""
import json
import numpy as np
import torch
import benchkit
from benchkit import alternate, stats_quantiles as stats
from gaussian_transformer_amd import synth
from gaussian_transformer_amd.rasterizer import GaussianRasterizer


def bench_config(name, reps, warmup, burst, dev):
    sc = synth.make_config(name)
    par = benchkit.scene_tensors(sc, dev, requires_grad=True)
    rs_plain, rs_pose = benchkit.scene_settings(sc, dev), benchkit.scene_settings(sc, dev, camera_grad=True)
    P, H, W = int(sc.means3D.shape[0]), rs_plain.image_height, rs_plain.image_width
    target = torch.rand((3, H, W), device=dev, generator=torch.Generator(device=dev).manual_seed(1))

    def step(rs):
        for p in par.values():
            p.grad = None
        for c in (rs.viewmatrix, rs.projmatrix, rs.campos):
            c.grad = None
        m2 = torch.zeros((P, 3), device=dev, requires_grad=True)
        color, _ = GaussianRasterizer(rs)(means2D=m2, **par)
        (color - target).abs().mean().backward()

    ts = alternate(dict(a=lambda: step(rs_plain), b=lambda: step(rs_pose)), reps, warmup)
    ta, tb = ts["a"], ts["b"]
    assert rs_plain.viewmatrix.grad is None and all(c.grad is not None for c in (rs_pose.viewmatrix, rs_pose.projmatrix, rs_pose.campos))

    # the new call alone, back to back on one reverse pass's workspace
    f = benchkit.Forward(rs_plain, {k: p.detach() for k, p in par.items()})
    ws = f.backward(torch.sign(f.color - target) / f.color.numel(), return_ws=True)[-1]
    x, e = f.x, f.empty
    call = lambda: f.be.pose_backward(rs_plain, 0, f.n, x["means3D"], f.radii, x["shs"], e, x["scales"], x["rotations"], e, f.geom, ws)

    def many():
        for _ in range(burst):
            call()
    alone = [ms / burst for ms in alternate(dict(many=many), reps, warmup)["many"]]
    mask = f.be.composited_mask(f.geom, P) & (f.radii > 0)
    return dict(config=name, P=P, W=W, H=H, num_rendered=int(f.n), gaussians_with_gradient=int(mask.sum()),
                without_camera_gradients=stats(ta), with_camera_gradients=stats(tb),
                extra_median_ms=float(np.median(tb) - np.median(ta)), ratio_median=float(np.median(tb) / np.median(ta)),
                gsr_pose_backward_alone=dict(stats(alone), launches_per_sample=burst))


def main():
    ap = benchkit.parser(30, 5, "pose", configs=True, trace_friendly=True)
    ap.add_argument("--burst", type=int, default=20, help="back-to-back gsr_pose_backward calls per timed sample (2 with --trace-friendly)")
    args = benchkit.parse(ap)
    if args.trace_friendly:
        args.burst = 2
    dev = torch.device("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, results=[])
    for name in args.configs:
        r = bench_config(name, args.reps, args.warmup, args.burst, dev)
        print(json.dumps(r), flush=True)
        out["results"].append(r)
    if not args.trace_friendly:
        benchkit.write_json(out, args.out)


if __name__ == "__main__":
    main()
