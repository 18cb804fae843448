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
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from gaussian_transformer_amd import rasterizer, synth
from gaussian_transformer_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer

HAS_FEATURES = hasattr(rasterizer, "_RasterizeGaussiansFeatures")


def stats(xs):
    a = np.sort(np.asarray(xs, np.float64))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), p10_ms=float(np.quantile(a, 0.1)), p90_ms=float(np.quantile(a, 0.9)), n=int(a.size))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); r = fn(); e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def bench_config(name, C, reps, warmup, dev):
    sc = synth.make_config(name)
    cam = sc.camera
    t = lambda a, g=False: torch.tensor(np.asarray(a, np.float32), device=dev).requires_grad_(g)
    P, H, W = int(sc.means3D.shape[0]), int(cam.image_height), int(cam.image_width)
    par = dict(means3D=t(sc.means3D, True), opacities=t(np.asarray(sc.opacities).reshape(P, 1), True), shs=t(sc.shs, True),
               scales=t(sc.scales, True), rotations=t(sc.rotations, True))
    mk = lambda bg: GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=bg, scale_modifier=1.0,
        viewmatrix=t(np.asarray(cam.world_view_transform).reshape(4, 4)), projmatrix=t(np.asarray(cam.full_proj_transform).reshape(4, 4)),
        sh_degree=sc.sh_degree, campos=t(cam.camera_center), prefiltered=False, debug=False)
    rs, rs0 = mk(t(sc.bg)), mk(torch.zeros(3, device=dev))
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

    routes = [(route_a, [])] + ([(route_b, [])] if HAS_FEATURES else [])
    for i in range(warmup + reps):
        for fn, ts in routes if i % 2 == 0 else routes[::-1]:
            ms, _ = timed(fn)
            if i >= warmup:
                ts.append(ms)
    res = dict(config=name, P=P, W=W, H=H, C=C, renders_of_the_trick=1 + len(triples), trick_renders=stats(routes[0][1]))
    if not HAS_FEATURES:
        return res
    # same results: the two routes agree on the map and on the gradients (atomics reorder)
    ma = route_a(); ga = {k: p.grad.clone() for k, p in list(par.items()) + [("features", F)]}
    mb = route_b(); gb = {k: p.grad.clone() for k, p in list(par.items()) + [("features", F)]}
    res.update(one_render_with_features=stats(routes[1][1]), speedup_median=float(np.median(routes[0][1]) / np.median(routes[1][1])),
               routes_agree=dict(map_max_abs=float((ma - mb).abs().max()),
                                 grads_rel_max={k: float((ga[k] - gb[k]).abs().max() / ga[k].abs().max().clamp_min(1e-30)) for k in ga}))

    # the new calls alone, beside the depth pass's, on one forward pass's workspaces
    be = rasterizer.get_backend()
    empty = torch.empty(0, device=dev)
    det = {k: p.detach() for k, p in par.items()}
    Fd = F.detach()
    gD = torch.randn((H, W), device=dev, generator=gen) / (H * W)
    n, _color, radii, geom, binning, img = be.forward(rs, det["means3D"], det["shs"], empty, det["opacities"], det["scales"], det["rotations"], empty)
    g = be.backward(rs, n, gC, det["means3D"], radii, det["shs"], empty, det["scales"], det["rotations"], empty, geom, binning, img)
    into = (g[0], g[1], g[4], g[5], g[6], g[7])
    geo = (det["means3D"], radii, det["scales"], det["rotations"], empty, geom, binning, img)
    calls = {"gsr_features_forward": lambda: be.features_forward(rs, P, n, Fd, geom, binning, img),
             "gsr_features_backward(accumulate=0)": lambda: be.features_backward(rs, n, Fd, gF, *geo),
             "gsr_features_backward(accumulate=1)": lambda: be.features_backward(rs, n, Fd, gF, *geo, into=into),
             "gsr_features_backward(accumulate=1, dL_dfeatures=NULL)": lambda: be.features_backward(rs, n, Fd, gF, *geo, into=into, want_features_grad=False),
             "gsr_depth_forward": lambda: be.depth_forward(rs, P, n, 0, geom, binning, img),
             "gsr_depth_backward(accumulate=1)": lambda: be.depth_backward(rs, n, 0, gD, None, *geo, into=into)}
    alone = {k: [] for k in calls}
    for i in range(warmup + reps):
        for k, fn in calls.items():
            ms, _ = timed(fn)
            if i >= warmup:
                alone[k].append(ms)
    res.update(num_rendered=int(n), calls_alone={k: stats(v) for k, v in alone.items()})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--channels", type=int, nargs="+", default=[3, 16, 32])
    ap.add_argument("--configs", nargs="+", default=["cfg2_table_300k_800", "cfg3_synth_1M_1080p"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "features", "bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("features_bench.py measures on a HIP device; none found (no CPU fallback, no number)")
    dev = torch.device("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, has_feature_maps=HAS_FEATURES, results=[])
    for name in args.configs:
        for C in args.channels:
            r = bench_config(name, C, args.reps, args.warmup, dev)
            print(json.dumps(r), flush=True)
            out["results"].append(r)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
