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
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from gaussian_transformer_amd import rasterizer, synth
from gaussian_transformer_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer


def stats(xs):
    a = np.sort(np.asarray(xs, np.float64))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), p10_ms=float(np.quantile(a, 0.1)), p90_ms=float(np.quantile(a, 0.9)), n=int(a.size))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); r = fn(); e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def bench_config(name, reps, warmup, burst, dev):
    sc = synth.make_config(name)
    cam = sc.camera
    t = lambda a, g=False: torch.tensor(np.asarray(a, np.float32), device=dev).requires_grad_(g)
    P, H, W = int(sc.means3D.shape[0]), int(cam.image_height), int(cam.image_width)
    par = dict(means3D=t(sc.means3D, True), opacities=t(np.asarray(sc.opacities).reshape(P, 1), True), shs=t(sc.shs, True),
               scales=t(sc.scales, True), rotations=t(sc.rotations, True))
    mk = lambda g: GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=t(sc.bg), scale_modifier=1.0,
        viewmatrix=t(np.asarray(cam.world_view_transform).reshape(4, 4), g), projmatrix=t(np.asarray(cam.full_proj_transform).reshape(4, 4), g),
        sh_degree=sc.sh_degree, campos=t(cam.camera_center, g), prefiltered=False, debug=False)
    rs_plain, rs_pose = mk(False), mk(True)
    target = torch.rand((3, H, W), device=dev, generator=torch.Generator(device=dev).manual_seed(1))

    def step(rs):
        for p in par.values():
            p.grad = None
        for c in (rs.viewmatrix, rs.projmatrix, rs.campos):
            c.grad = None
        m2 = torch.zeros((P, 3), device=dev, requires_grad=True)
        color, _ = GaussianRasterizer(rs)(means2D=m2, **par)
        (color - target).abs().mean().backward()

    ta, tb = [], []
    for i in range(warmup + reps):
        for rs, ts in ((rs_plain, ta), (rs_pose, tb)) if i % 2 == 0 else ((rs_pose, tb), (rs_plain, ta)):
            ms, _ = timed(lambda: step(rs))
            if i >= warmup:
                ts.append(ms)
    assert rs_plain.viewmatrix.grad is None and all(c.grad is not None for c in (rs_pose.viewmatrix, rs_pose.projmatrix, rs_pose.campos))

    # the new call alone, back to back on one reverse pass's workspace
    be = rasterizer.get_backend()
    empty = torch.empty(0, device=dev)
    det = {k: p.detach() for k, p in par.items()}
    n, color, radii, geom, binning, img = be.forward(rs_plain, det["means3D"], det["shs"], empty, det["opacities"], det["scales"], det["rotations"], empty)
    gC = torch.sign(color - target) / color.numel()
    ws = be.backward(rs_plain, n, gC, det["means3D"], radii, det["shs"], empty, det["scales"], det["rotations"], empty, geom, binning, img, return_ws=True)[-1]
    call = lambda: be.pose_backward(rs_plain, 0, n, det["means3D"], radii, det["shs"], empty, det["scales"], det["rotations"], empty, geom, ws)

    def many():
        for _ in range(burst):
            call()
    alone = []
    for i in range(warmup + reps):
        ms, _ = timed(many)
        if i >= warmup:
            alone.append(ms / burst)
    mask = be.composited_mask(geom, P) & (radii > 0)
    return dict(config=name, P=P, W=W, H=H, num_rendered=int(n), gaussians_with_gradient=int(mask.sum()),
                without_camera_gradients=stats(ta), with_camera_gradients=stats(tb),
                extra_median_ms=float(np.median(tb) - np.median(ta)), ratio_median=float(np.median(tb) / np.median(ta)),
                gsr_pose_backward_alone=dict(stats(alone), launches_per_sample=burst))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--burst", type=int, default=20, help="back-to-back gsr_pose_backward calls per timed sample")
    ap.add_argument("--trace-friendly", action="store_true", help="3 repetitions, 1 warm-up, bursts of 2, nothing written: for a run under a kernel trace")
    ap.add_argument("--configs", nargs="+", default=["cfg2_table_300k_800", "cfg3_synth_1M_1080p"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose", "bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pose_bench.py measures on a HIP device; none found (no CPU fallback, no number)")
    if args.trace_friendly:
        args.reps, args.warmup, args.burst = 3, 1, 2
    dev = torch.device("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, results=[])
    for name in args.configs:
        r = bench_config(name, args.reps, args.warmup, args.burst, dev)
        print(json.dumps(r), flush=True)
        out["results"].append(r)
    if args.trace_friendly:
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
