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
import json
import numpy as np
import torch
import benchkit
from benchkit import alternate, stats_quantiles as stats
from gaussian_transformer_amd import rasterizer, synth
from gaussian_transformer_amd.rasterizer import GaussianRasterizer


def bench_config(name, mode, reps, warmup, dev):
    sc = synth.make_config(name)
    par = benchkit.scene_tensors(sc, dev, requires_grad=True)
    rs, rs0 = benchkit.scene_settings(sc, dev), benchkit.scene_settings(sc, dev, bg=torch.zeros(3, device=dev))
    P, H, W, vm = int(sc.means3D.shape[0]), rs.image_height, rs.image_width, rs.viewmatrix
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

    ts = alternate(dict(a=route_a, b=route_b), reps, warmup)
    ta, tb = ts["a"], ts["b"]
    # same results: the two routes agree on the maps and on the gradients (atomics reorder; the second render rounds v on its own)
    da, aa = route_a(); ga = {k: p.grad.clone() for k, p in par.items()}
    db, ab = route_b(); gb = {k: p.grad.clone() for k, p in par.items()}
    agree = dict(depth_max_abs=float((da - db).abs().max()), alpha_max_abs=float((aa - ab).abs().max()),
                 grads_rel_max={k: float((ga[k] - gb[k]).abs().max() / ga[k].abs().max().clamp_min(1e-30)) for k in par})

    # the new calls alone, on one forward pass's workspaces
    mode_i = rasterizer.DEPTH_MODES[mode]
    f = benchkit.Forward(rs, {k: p.detach() for k, p in par.items()})
    g = f.backward(gC)
    into = (g[0], g[1], g[4], g[5], g[6], g[7])
    calls = {"gsr_depth_forward": lambda: f.be.depth_forward(rs, P, f.n, mode_i, f.geom, f.binning, f.img),
             "gsr_depth_backward(accumulate=0)": lambda: f.be.depth_backward(rs, f.n, mode_i, gD, gA, *f.geo),
             "gsr_depth_backward(accumulate=1)": lambda: f.be.depth_backward(rs, f.n, mode_i, gD, gA, *f.geo, into=into)}
    alone = alternate(calls, reps, warmup, rotate=False)
    return dict(config=name, P=P, W=W, H=H, mode=mode, num_rendered=int(f.n), two_renders=stats(ta), one_render_with_maps=stats(tb),
                speedup_median=float(np.median(ta) / np.median(tb)), routes_agree=agree, calls_alone={k: stats(v) for k, v in alone.items()})


def main():
    ap = benchkit.parser(30, 5, "depth", configs=True)
    ap.add_argument("--mode", default="expected", choices=sorted(rasterizer.DEPTH_MODES))
    args = benchkit.parse(ap)
    dev = torch.device("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, results=[])
    for name in args.configs:
        r = bench_config(name, args.mode, args.reps, args.warmup, dev)
        print(json.dumps(r), flush=True)
        out["results"].append(r)
    benchkit.write_json(out, args.out)


if __name__ == "__main__":
    main()
