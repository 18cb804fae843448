#!/usr/bin/env python3
"""Colour + depth + alpha of one camera, forward and backward, two ways (informational; bench.py is the headline metric):

  (a) two renders -- what had to be done before include/gsr_depth.h existed: the scene as it is, then a second time with
      colors_precomp = (v, 1, 0), v = z or 1 / z formed in torch from means3D (so that dL/dv reaches the means), and a zero background:
      a second per-Gaussian stage, a second list build, a second reverse pass;
  (b) GaussianRasterizer.forward(depth=...): one render, then the depth walk over its lists; backward = the colour pass, then the map pass
      adding into its tensors.

One process; the two routes alternate inside every repetition on the same inputs and upstream gradients, each timed with device events
around forward + loss + backward.  Also timed alone: the calls gsr_depth_forward (one kernel: the forward walk) and gsr_depth_backward
(clear, reverse walk, per-Gaussian chain, finishing kernel), accumulate 0 and 1.  Per-kernel times of the two walks come from running this
script under a kernel trace (kernel names depth_fwd_kernel / depth_bwd_kernel), in a run of its own.

    python scripts/depth_bench.py [--reps 30] [--warmup 5] [--mode expected] [--configs cfg2_table_300k_800 cfg3_synth_1M_1080p]
                                  [--out profiles/depth/bench.json]
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


def bench_config(name, mode, reps, warmup, dev):
    sc = synth.make_config(name)
    cam = sc.camera
    t = lambda a, g=False: torch.tensor(np.asarray(a, np.float32), device=dev).requires_grad_(g)
    P, H, W = int(sc.means3D.shape[0]), int(cam.image_height), int(cam.image_width)
    par = dict(means3D=t(sc.means3D, True), opacities=t(np.asarray(sc.opacities).reshape(P, 1), True), shs=t(sc.shs, True),
               scales=t(sc.scales, True), rotations=t(sc.rotations, True))
    vm = t(np.asarray(cam.world_view_transform).reshape(4, 4))
    mk = lambda bg: GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=bg, scale_modifier=1.0, viewmatrix=vm,
        projmatrix=t(np.asarray(cam.full_proj_transform).reshape(4, 4)), sh_degree=sc.sh_degree, campos=t(cam.camera_center), prefiltered=False, debug=False)
    rs, rs0 = mk(t(sc.bg)), mk(torch.zeros(3, device=dev))
    gen = torch.Generator(device=dev).manual_seed(1)
    gC = torch.randn((3, H, W), device=dev, generator=gen) / (H * W)
    gD = torch.randn((H, W), device=dev, generator=gen) / (H * W)
    gA = torch.randn((H, W), device=dev, generator=gen) / (H * W)

    def zero():
        for p in par.values():
            p.grad = None

    def route_a():
        zero()
        m2 = torch.zeros((P, 3), device=dev, requires_grad=True)
        color, _ = GaussianRasterizer(rs)(means2D=m2, **par)
        z = par["means3D"] @ vm[:3, 2] + vm[3, 2]
        v = z if mode == "expected" else 1.0 / z
        col = torch.stack([v, torch.ones_like(v), torch.zeros_like(v)], 1)
        m2b = torch.zeros((P, 3), device=dev, requires_grad=True)
        maps, _ = GaussianRasterizer(rs0)(means3D=par["means3D"], means2D=m2b, opacities=par["opacities"], colors_precomp=col,
                                          scales=par["scales"], rotations=par["rotations"])
        ((color * gC).sum() + (maps[0] * gD).sum() + (maps[1] * gA).sum()).backward()
        return maps[0].detach(), maps[1].detach()

    def route_b():
        zero()
        m2 = torch.zeros((P, 3), device=dev, requires_grad=True)
        color, _, depth, alpha = GaussianRasterizer(rs)(means2D=m2, depth=mode, **par)
        ((color * gC).sum() + (depth[0] * gD).sum() + (alpha[0] * gA).sum()).backward()
        return depth[0].detach(), alpha[0].detach()

    ta, tb = [], []
    for i in range(warmup + reps):
        for which in ((route_a, ta), (route_b, tb)) if i % 2 == 0 else ((route_b, tb), (route_a, ta)):
            ms, _ = timed(which[0])
            if i >= warmup:
                which[1].append(ms)
    # same results: the two routes agree on the maps and on the gradients (atomics reorder; the second render rounds v on its own)
    da, aa = route_a(); ga = {k: p.grad.clone() for k, p in par.items()}
    db, ab = route_b(); gb = {k: p.grad.clone() for k, p in par.items()}
    agree = dict(depth_max_abs=float((da - db).abs().max()), alpha_max_abs=float((aa - ab).abs().max()),
                 grads_rel_max={k: float((ga[k] - gb[k]).abs().max() / ga[k].abs().max().clamp_min(1e-30)) for k in par})

    # the new calls alone, on one forward pass's workspaces
    be = rasterizer.get_backend()
    empty = torch.empty(0, device=dev)
    det = {k: p.detach() for k, p in par.items()}
    mode_i = rasterizer.DEPTH_MODES[mode]
    n, _color, radii, geom, binning, img = be.forward(rs, det["means3D"], det["shs"], empty, det["opacities"], det["scales"], det["rotations"], empty)
    g = be.backward(rs, n, gC, det["means3D"], radii, det["shs"], empty, det["scales"], det["rotations"], empty, geom, binning, img)
    into = (g[0], g[1], g[4], g[5], g[6], g[7])
    calls = {"gsr_depth_forward": lambda: be.depth_forward(rs, P, n, mode_i, geom, binning, img),
             "gsr_depth_backward(accumulate=0)": lambda: be.depth_backward(rs, n, mode_i, gD, gA, det["means3D"], radii, det["scales"], det["rotations"], empty, geom, binning, img),
             "gsr_depth_backward(accumulate=1)": lambda: be.depth_backward(rs, n, mode_i, gD, gA, det["means3D"], radii, det["scales"], det["rotations"], empty, geom, binning, img, into=into)}
    alone = {k: [] for k in calls}
    for i in range(warmup + reps):
        for k, fn in calls.items():
            ms, _ = timed(fn)
            if i >= warmup:
                alone[k].append(ms)
    return dict(config=name, P=P, W=W, H=H, mode=mode, num_rendered=int(n), two_renders=stats(ta), one_render_with_maps=stats(tb),
                speedup_median=float(np.median(ta) / np.median(tb)), routes_agree=agree, calls_alone={k: stats(v) for k, v in alone.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mode", default="expected", choices=sorted(rasterizer.DEPTH_MODES))
    ap.add_argument("--configs", nargs="+", default=["cfg2_table_300k_800", "cfg3_synth_1M_1080p"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth", "bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("depth_bench.py measures on a HIP device; none found (no CPU fallback, no number)")
    dev = torch.device("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, results=[])
    for name in args.configs:
        r = bench_config(name, args.mode, args.reps, args.warmup, dev)
        print(json.dumps(r), flush=True)
        out["results"].append(r)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
