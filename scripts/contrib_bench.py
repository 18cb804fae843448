#!/usr/bin/env python3
"""What the blend-weight statistics cost (informational; bench.py is the headline metric).  On one colors_precomp = (1, 0, 0) render
per configuration, alternating inside every repetition, each timed with device events:

  (a) gsr_contrib_accumulate alone (include/gsr_contrib.h: contrib_walk_kernel);
  (b) gsr_depth_forward, depth only, on the same render: the same walk without the reduction and the atomics -- the floor for a
      kernel of this shape; (a) - (b) is the price of the reduction;
  (c) the only other route to the sum: gsr_backward with a gradient of ones in channel 0 (dL_dcolors[:, 0] is the sum);
  (d) gsr_contrib_read, in microseconds and GB/s (16 bytes read and 12 written per Gaussian).

Also (a) on the scene of tests/test_gpu_depth.py with one Gaussian over all 272 tiles (69 632 pixels into one 16-byte row), with and
without that Gaussian: what one hot row costs the direct form.

    python scripts/contrib_bench.py [--reps 50] [--warmup 5] [--configs cfg2_table_300k_800 cfg3_synth_1M_1080p] [--out profiles/contrib/bench.json]
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from gaussian_transformer_amd import _lib, rasterizer, synth
from gaussian_transformer_amd.rasterizer import ContributionStats, GaussianRasterizationSettings


def stats(xs):
    a = np.sort(np.asarray(xs, np.float64))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), p10_ms=float(np.quantile(a, 0.1)), p90_ms=float(np.quantile(a, 0.9)), n=int(a.size))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); r = fn(); e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


class Render:
    """One forward pass of `sc` with the colour (1, 0, 0), and the calls that re-read its workspaces."""

    def __init__(self, sc, dev):
        cam = sc.camera
        t = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
        self.P, self.H, self.W = int(sc.means3D.shape[0]), int(cam.image_height), int(cam.image_width)
        P = self.P
        self.x = dict(means3D=t(sc.means3D), opacities=t(np.asarray(sc.opacities).reshape(P, 1)), scales=t(sc.scales), rotations=t(sc.rotations))
        self.colors = torch.zeros((P, 3), device=dev); self.colors[:, 0] = 1.0
        self.rs = GaussianRasterizationSettings(
            image_height=self.H, image_width=self.W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=torch.zeros(3, device=dev), scale_modifier=1.0,
            viewmatrix=t(np.asarray(cam.world_view_transform).reshape(4, 4)), projmatrix=t(np.asarray(cam.full_proj_transform).reshape(4, 4)),
            sh_degree=0, campos=t(cam.camera_center), prefiltered=False, debug=False)
        self.dev, self.be, self.empty = dev, rasterizer.get_backend(), torch.empty(0, device=dev)
        x, e = self.x, self.empty
        self.n, self.color, self.radii, self.geom, self.binning, self.img = self.be.forward(
            self.rs, x["means3D"], e, self.colors, x["opacities"], x["scales"], x["rotations"], e)
        self.stats = ContributionStats(P, dev)
        self.depth = torch.empty((self.H, self.W), device=dev)
        self.ones = torch.zeros((3, self.H, self.W), device=dev); self.ones[0] = 1.0
        self.ws3 = (_lib.ptr(self.geom), self.geom.numel(), _lib.ptr(self.binning), self.binning.numel(), _lib.ptr(self.img), self.img.numel())

    def accumulate(self):
        _lib.call("gsr_contrib_accumulate", _lib.stream(self.dev), self.P, self.W, self.H, self.n, *self.ws3, _lib.ptr(self.stats.rows))

    def depth_only(self):
        _lib.call("gsr_depth_forward", _lib.stream(self.dev), self.P, self.W, self.H, self.n, _lib.DEPTH_EXPECTED, *self.ws3, _lib.ptr(self.depth), None)

    def backward(self):
        x, e = self.x, self.empty
        return self.be.backward(self.rs, self.n, self.ones, x["means3D"], self.radii, e, self.colors, x["scales"], x["rotations"], e,
                                self.geom, self.binning, self.img)

    def read(self):
        return self.stats.read()


def alternate(fns, reps, warmup):
    """Every function once per repetition, the order rotated from one repetition to the next."""
    names = list(fns)
    ts = {k: [] for k in names}
    for i in range(warmup + reps):
        for k in names[i % len(names):] + names[:i % len(names)]:
            ms, _ = timed(fns[k])
            if i >= warmup:
                ts[k].append(ms)
    return ts


def bench_config(name, reps, warmup, dev):
    r = Render(synth.make_config(name), dev)
    ts = alternate(dict(a=r.accumulate, b=r.depth_only, c=r.backward, d=r.read), reps, warmup)
    # what was measured is what the tests check: one view's sum against the backward pass's
    r.stats.reset(); r.accumulate()
    w_sum, _, n_pix = r.read()
    g = r.backward()[3][:, 0]
    err = float((w_sum - g).abs().max() / g.abs().max())
    a, b, c, d = (float(np.median(ts[k])) for k in "abcd")
    return dict(config=name, P=r.P, W=r.W, H=r.H, num_rendered=int(r.n), blended_pairs=int(n_pix.to(torch.int64).sum()),
                accumulate=stats(ts["a"]), depth_forward_depth_only=stats(ts["b"]), backward_ones=stats(ts["c"]), read=stats(ts["d"]),
                reduction_price_ms=a - b, accumulate_over_backward=a / c, read_us=1e3 * d, read_GBps=28.0 * r.P / (d * 1e-3) / 1e9,
                sum_against_backward_max_rel=err)


def bench_replica(reps, warmup, dev):
    out = {}
    scenes = {}
    for hot in (True, False):
        sc = synth.make_scene(P=201, width=272, height=256, sh_degree=1, s0=0.05, seed=0)
        if hot:
            sc.scales[0] = np.array([8.0, 8.0, 8.0], np.float32)
            sc.opacities[0] = 0.6
        scenes["with_hot" if hot else "without_hot"] = Render(sc, dev)
    ts = alternate({k: r.accumulate for k, r in scenes.items()}, reps, warmup)
    for k, r in scenes.items():
        r.stats.reset(); r.accumulate()
        n_pix = r.read()[2]
        out[k] = dict(stats(ts[k]), num_rendered=int(r.n), blended_pairs=int(n_pix.to(torch.int64).sum()), largest_count=int(n_pix.max()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace-friendly", action="store_true", help="3 repetitions, 1 warm-up, nothing written: for a run under a profiler")
    ap.add_argument("--configs", nargs="+", default=["cfg2_table_300k_800", "cfg3_synth_1M_1080p"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contrib", "bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("contrib_bench.py measures on a HIP device; none found (no CPU fallback, no number)")
    if args.trace_friendly:
        args.reps, args.warmup = 3, 1
    dev = torch.device("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, results=[])
    for name in args.configs:
        r = bench_config(name, args.reps, args.warmup, dev)
        print(json.dumps(r), flush=True)
        out["results"].append(r)
    out["replica"] = bench_replica(args.reps, args.warmup, dev)
    print(json.dumps(out["replica"]), flush=True)
    if args.trace_friendly:
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
