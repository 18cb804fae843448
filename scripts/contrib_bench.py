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
import json
import numpy as np
import torch
import benchkit
from benchkit import alternate, stats_quantiles as stats
from gaussian_transformer_amd import _lib, synth
from gaussian_transformer_amd.rasterizer import ContributionStats


class Render(benchkit.Forward):
    """One forward pass of `sc` with the colour (1, 0, 0), and the calls that re-read its workspaces."""

    def __init__(self, sc, dev):
        self.P, self.dev = int(sc.means3D.shape[0]), dev
        colors = torch.zeros((self.P, 3), device=dev); colors[:, 0] = 1.0
        super().__init__(benchkit.scene_settings(sc, dev, bg=torch.zeros(3, device=dev), sh_degree=0), benchkit.scene_tensors(sc, dev, shs=False), colors)
        self.H, self.W = self.rs.image_height, self.rs.image_width
        self.stats = ContributionStats(self.P, dev)
        self.depth = torch.empty((self.H, self.W), device=dev)
        self.ones = torch.zeros((3, self.H, self.W), device=dev); self.ones[0] = 1.0
        self.ws3 = self.workspace_args()

    def accumulate(self):
        _lib.call("gsr_contrib_accumulate", _lib.stream(self.dev), self.P, self.W, self.H, self.n, *self.ws3, _lib.ptr(self.stats.rows))

    def depth_only(self):
        _lib.call("gsr_depth_forward", _lib.stream(self.dev), self.P, self.W, self.H, self.n, _lib.DEPTH_EXPECTED, *self.ws3, _lib.ptr(self.depth), None)

    def backward_ones(self):
        return self.backward(self.ones)

    def read(self):
        return self.stats.read()


def bench_config(name, reps, warmup, dev):
    r = Render(synth.make_config(name), dev)
    ts = alternate(dict(a=r.accumulate, b=r.depth_only, c=r.backward_ones, d=r.read), reps, warmup)
    # what was measured is what the tests check: one view's sum against the backward pass's
    r.stats.reset(); r.accumulate()
    w_sum, _, n_pix = r.read()
    g = r.backward_ones()[3][:, 0]
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
    args = benchkit.parse(benchkit.parser(50, 5, "contrib", configs=True, trace_friendly=True))
    dev = torch.device("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, results=[])
    for name in args.configs:
        r = bench_config(name, args.reps, args.warmup, dev)
        print(json.dumps(r), flush=True)
        out["results"].append(r)
    out["replica"] = bench_replica(args.reps, args.warmup, dev)
    print(json.dumps(out["replica"]), flush=True)
    if not args.trace_friendly:
        benchkit.write_json(out, args.out)


if __name__ == "__main__":
    main()
