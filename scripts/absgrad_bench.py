#!/usr/bin/env python3
"""What absgrad costs (informational; bench.py is the headline metric).  On one render per configuration, with SH colours and a random
upstream gradient, alternating inside every repetition, each timed with device events:

  (a) forward + backward through the backend without a collector: the step as it is without this feature;
  (b) the same step inside rasterizer.collect_absgrad: (b) - (a) is what the collector adds to a training step, workspace included;
  (c) gsr_absgrad_backward alone, accumulate = 1, no signed sums (include/gsr_absgrad.h: zeroing, walk, finish -- what the collector calls);
  (d) the same with the signed sums (the instantiation the tests hold against gsr_backward);
  (e) gsr_depth_backward on the same render, both map gradients: the reverse map walk absgrad rides beside, with its per-Gaussian chain.

    python scripts/absgrad_bench.py [--reps 50] [--warmup 5] [--configs cfg2_table_300k_800 cfg3_synth_1M_1080p] [--out profiles/absgrad/bench.json]
"""
import json
import numpy as np
import torch
import benchkit
from benchkit import alternate, stats_quantiles as stats
from gaussian_transformer_amd import _lib, synth
from gaussian_transformer_amd.rasterizer import AbsGrad, collect_absgrad


class Step:
    """The inputs of one configuration, a render of them whose workspaces the stand-alone calls re-read, and the step itself."""

    def __init__(self, sc, dev):
        self.x, self.rs = benchkit.scene_tensors(sc, dev), benchkit.scene_settings(sc, dev)
        self.P, self.H, self.W = int(sc.means3D.shape[0]), self.rs.image_height, self.rs.image_width
        self.dev = dev
        gen = torch.Generator().manual_seed(0)
        self.dL = (torch.randn((3, self.H, self.W), generator=gen) / (3 * self.H * self.W)).to(dev)
        self.gD = (torch.randn((self.H, self.W), generator=gen) / (self.H * self.W)).to(dev)
        self.gA = (torch.randn((self.H, self.W), generator=gen) / (self.H * self.W)).to(dev)
        self.buf = AbsGrad(self.P, dev)
        self.signed = torch.zeros((self.P, 2), device=dev)
        self.fwd = benchkit.Forward(self.rs, self.x)
        self.ws3 = self.fwd.workspace_args()
        self.ws = _lib.workspace("gsr_absgrad_workspace_bytes", dev, self.P)

    def step(self):
        return benchkit.Forward(self.rs, self.x, empty=self.fwd.empty).backward(self.dL)

    def step_collecting(self):
        with collect_absgrad(self.buf):
            return self.step()

    def absgrad(self, signed=False):
        p = _lib.ptr
        _lib.call("gsr_absgrad_backward", _lib.stream(self.dev), self.P, self.W, self.H, self.fwd.n, p(self.rs.bg), p(self.dL), *self.ws3,
                  p(self.ws), self.ws.numel(), 1, p(self.buf.grad), p(self.signed) if signed else None)

    def depth_backward(self):
        return self.fwd.be.depth_backward(self.rs, self.fwd.n, _lib.DEPTH_EXPECTED, self.gD, self.gA, *self.fwd.geo)


def bench_config(name, reps, warmup, dev):
    r = Step(synth.make_config(name), dev)
    ts = alternate(dict(a=r.step, b=r.step_collecting, c=r.absgrad, d=lambda: r.absgrad(True), e=r.depth_backward), reps, warmup)
    # what was measured is what the tests check: the signed sums against the same render's gsr_backward
    r.buf.zero_(); r.signed.zero_(); r.absgrad(True)
    m2d = r.fwd.backward(r.dL)[1][:, :2]
    err = float((r.signed - m2d).abs().max() / m2d.abs().max())
    na, ns = r.buf.grad.norm(dim=1), m2d.norm(dim=1)
    ok = ns > 0
    a, b, c, d, e = (float(np.median(ts[k])) for k in "abcde")
    return dict(config=name, P=r.P, W=r.W, H=r.H, num_rendered=int(r.fwd.n), step=stats(ts["a"]), step_collecting=stats(ts["b"]),
                absgrad_call=stats(ts["c"]), absgrad_call_signed=stats(ts["d"]), depth_backward_call=stats(ts["e"]),
                collector_price_ms=b - a, collector_price_frac=(b - a) / a, absgrad_over_depth_backward=c / e,
                signed_against_backward_max_rel=err, ratio_median=float((na[ok] / ns[ok]).median()))


def main():
    args = benchkit.parse(benchkit.parser(50, 5, "absgrad", configs=True, trace_friendly=True))
    dev = torch.device("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, results=[])
    for name in args.configs:
        r = bench_config(name, args.reps, args.warmup, dev)
        print(json.dumps(r), flush=True)
        out["results"].append(r)
    if not args.trace_friendly:
        benchkit.write_json(out, args.out)


if __name__ == "__main__":
    main()
