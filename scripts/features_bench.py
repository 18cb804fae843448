#!/usr/bin/env python3
"""Colour plus a C-channel feature map of one camera, forward and backward, two ways (informational; bench.py is the headline metric):

  (a) the colour trick -- the only route before include/gsr_features.h existed: 1 + ceil(C / 3) renders, the scene as it is and then once
      per triple of channels with colors_precomp = F[:, 3k:3k+3] (the last triple zero-padded) and a zero background: a per-Gaussian
      stage, a list build, a compositing pass and a reverse pass per triple, the gradients added by autograd.  Uses nothing of the
      feature maps, so this route runs unchanged on a checkout without them (only it is then measured);
  (b) GaussianRasterizer.forward(features=F): one render, then the feature walk over its lists; backward = the colour pass, then the
      feature pass adding into its tensors.

One process; the two routes alternate inside every repetition on the same inputs and upstream gradients, each timed with device events
around forward + loss + backward; medians over --reps repetitions.  Also timed alone, by device events, on one forward pass's workspaces:
gsr_features_forward (one kernel: the forward walk), gsr_features_backward with and without dL/dF (clear, reverse walk, per-Gaussian
chain, finishing kernels), beside gsr_depth_forward and gsr_depth_backward of the same render.

    python scripts/features_bench.py [--reps 50] [--warmup 5] [--channels 3 16 32] [--configs cfg2_table_300k_800 cfg3_synth_1M_1080p]
                                     [--out profiles/features/bench.json]
"""
import json
import numpy as np
import torch
import benchkit
from benchkit import alternate, stats_quantiles as stats
from gaussian_transformer_amd import rasterizer, synth
from gaussian_transformer_amd.rasterizer import GaussianRasterizer

HAS_FEATURES = hasattr(rasterizer, "_RasterizeGaussiansFeatures")


def bench_config(name, C, reps, warmup, dev):
    sc = synth.make_config(name)
    par = benchkit.scene_tensors(sc, dev, requires_grad=True)
    rs, rs0 = benchkit.scene_settings(sc, dev), benchkit.scene_settings(sc, dev, bg=torch.zeros(3, device=dev))
    P, H, W = int(sc.means3D.shape[0]), rs.image_height, rs.image_width
    gen = torch.Generator(device=dev).manual_seed(1)
    F = (torch.rand((P, C), device=dev, generator=gen) * 4 - 2).requires_grad_(True)
    gC = torch.randn((3, H, W), device=dev, generator=gen) / (H * W)
    gF = torch.randn((C, H, W), device=dev, generator=gen) / (H * W)
    triples = [(lo, min(lo + 3, C)) for lo in range(0, C, 3)]

    def zero():
        for p in list(par.values()) + [F]:
            p.grad = None

    def route_a():
        zero()
        color, _ = GaussianRasterizer(rs)(means2D=torch.zeros((P, 3), device=dev, requires_grad=True), **par)
        loss = (color * gC).sum()
        maps = []
        for lo, hi in triples:
            col = F[:, lo:hi] if hi - lo == 3 else torch.cat([F[:, lo:hi], F.new_zeros((P, 3 - (hi - lo)))], 1)
            m, _ = GaussianRasterizer(rs0)(means3D=par["means3D"], means2D=torch.zeros((P, 3), device=dev, requires_grad=True),
                                           opacities=par["opacities"], colors_precomp=col, scales=par["scales"], rotations=par["rotations"])
            maps.append(m[:hi - lo])
            loss = loss + (m[:hi - lo] * gF[lo:hi]).sum()
        loss.backward()
        return torch.cat([m.detach() for m in maps])

    def route_b():
        zero()
        color, _, feat = GaussianRasterizer(rs)(means2D=torch.zeros((P, 3), device=dev, requires_grad=True), features=F, **par)
        ((color * gC).sum() + (feat * gF).sum()).backward()
        return feat.detach()

    ts = alternate(dict(a=route_a, b=route_b) if HAS_FEATURES else dict(a=route_a), reps, warmup)
    res = dict(config=name, P=P, W=W, H=H, C=C, renders_of_the_trick=1 + len(triples), trick_renders=stats(ts["a"]))
    if not HAS_FEATURES:
        return res
    # same results: the two routes agree on the map and on the gradients (atomics reorder)
    ma = route_a(); ga = {k: p.grad.clone() for k, p in list(par.items()) + [("features", F)]}
    mb = route_b(); gb = {k: p.grad.clone() for k, p in list(par.items()) + [("features", F)]}
    res.update(one_render_with_features=stats(ts["b"]), speedup_median=float(np.median(ts["a"]) / np.median(ts["b"])),
               routes_agree=dict(map_max_abs=float((ma - mb).abs().max()),
                                 grads_rel_max={k: float((ga[k] - gb[k]).abs().max() / ga[k].abs().max().clamp_min(1e-30)) for k in ga}))

    # the new calls alone, beside the depth pass's, on one forward pass's workspaces
    Fd = F.detach()
    gD = torch.randn((H, W), device=dev, generator=gen) / (H * W)
    f = benchkit.Forward(rs, {k: p.detach() for k, p in par.items()})
    g = f.backward(gC)
    into = (g[0], g[1], g[4], g[5], g[6], g[7])
    be, n, ws, geo = f.be, f.n, (f.geom, f.binning, f.img), f.geo
    calls = {"gsr_features_forward": lambda: be.features_forward(rs, P, n, Fd, *ws),
             "gsr_features_backward(accumulate=0)": lambda: be.features_backward(rs, n, Fd, gF, *geo),
             "gsr_features_backward(accumulate=1)": lambda: be.features_backward(rs, n, Fd, gF, *geo, into=into),
             "gsr_features_backward(accumulate=1, dL_dfeatures=NULL)": lambda: be.features_backward(rs, n, Fd, gF, *geo, into=into, want_features_grad=False),
             "gsr_depth_forward": lambda: be.depth_forward(rs, P, n, 0, *ws),
             "gsr_depth_backward(accumulate=1)": lambda: be.depth_backward(rs, n, 0, gD, None, *geo, into=into)}
    alone = alternate(calls, reps, warmup, rotate=False)
    res.update(num_rendered=int(n), calls_alone={k: stats(v) for k, v in alone.items()})
    return res


def main():
    ap = benchkit.parser(50, 5, "features", configs=True)
    ap.add_argument("--channels", type=int, nargs="+", default=[3, 16, 32])
    args = benchkit.parse(ap)
    dev = torch.device("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, has_feature_maps=HAS_FEATURES, results=[])
    for name in args.configs:
        for C in args.channels:
            r = bench_config(name, C, args.reps, args.warmup, dev)
            print(json.dumps(r), flush=True)
            out["results"].append(r)
    benchkit.write_json(out, args.out)


if __name__ == "__main__":
    main()
