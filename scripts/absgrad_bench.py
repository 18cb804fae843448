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
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from gaussian_transformer_amd import _lib, rasterizer, synth
from gaussian_transformer_amd.rasterizer import AbsGrad, GaussianRasterizationSettings, collect_absgrad


def stats(xs):
    a = np.sort(np.asarray(xs, np.float64))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), p10_ms=float(np.quantile(a, 0.1)), p90_ms=float(np.quantile(a, 0.9)), n=int(a.size))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); r = fn(); e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


class Step:
    """The inputs of one configuration, a render of them whose workspaces the stand-alone calls re-read, and the step itself."""

    def __init__(self, sc, dev):
        cam = sc.camera
        t = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
        self.P, self.H, self.W = int(sc.means3D.shape[0]), int(cam.image_height), int(cam.image_width)
        P = self.P
        self.x = dict(means3D=t(sc.means3D), shs=t(sc.shs), opacities=t(np.asarray(sc.opacities).reshape(P, 1)), scales=t(sc.scales), rotations=t(sc.rotations))
        self.rs = GaussianRasterizationSettings(
            image_height=self.H, image_width=self.W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=t(sc.bg), scale_modifier=1.0,
            viewmatrix=t(np.asarray(cam.world_view_transform).reshape(4, 4)), projmatrix=t(np.asarray(cam.full_proj_transform).reshape(4, 4)),
            sh_degree=sc.sh_degree, campos=t(cam.camera_center), prefiltered=False, debug=False)
        self.dev, self.be, self.empty = dev, rasterizer.get_backend(), torch.empty(0, device=dev)
        gen = torch.Generator().manual_seed(0)
        self.dL = (torch.randn((3, self.H, self.W), generator=gen) / (3 * self.H * self.W)).to(dev)
        self.gD = (torch.randn((self.H, self.W), generator=gen) / (self.H * self.W)).to(dev)
        self.gA = (torch.randn((self.H, self.W), generator=gen) / (self.H * self.W)).to(dev)
        self.buf = AbsGrad(P, dev)
        self.signed = torch.zeros((P, 2), device=dev)
        self.fwd = self.forward()
        self.ws = _lib.workspace("gsr_absgrad_workspace_bytes", dev, P)

    def forward(self):
        x, e = self.x, self.empty
        return self.be.forward(self.rs, x["means3D"], x["shs"], e, x["opacities"], x["scales"], x["rotations"], e)

    def backward(self, fwd):
        x, e = self.x, self.empty
        n, _color, radii, geom, binning, img = fwd
        return self.be.backward(self.rs, n, self.dL, x["means3D"], radii, x["shs"], e, x["scales"], x["rotations"], e, geom, binning, img)

    def step(self):
        return self.backward(self.forward())

    def step_collecting(self):
        with collect_absgrad(self.buf):
            return self.step()

    def absgrad(self, signed=False):
        n, _color, _radii, geom, binning, img = self.fwd
        p = _lib.ptr
        _lib.call("gsr_absgrad_backward", _lib.stream(self.dev), self.P, self.W, self.H, n, p(self.rs.bg), p(self.dL), p(geom), geom.numel(),
                  p(binning), binning.numel(), p(img), img.numel(), p(self.ws), self.ws.numel(), 1, p(self.buf.grad), p(self.signed) if signed else None)

    def depth_backward(self):
        x, e = self.x, self.empty
        n, _color, radii, geom, binning, img = self.fwd
        return self.be.depth_backward(self.rs, n, _lib.DEPTH_EXPECTED, self.gD, self.gA, x["means3D"], radii, x["scales"], x["rotations"], e, geom, binning, img)


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
    r = Step(synth.make_config(name), dev)
    ts = alternate(dict(a=r.step, b=r.step_collecting, c=r.absgrad, d=lambda: r.absgrad(True), e=r.depth_backward), reps, warmup)
    # what was measured is what the tests check: the signed sums against the same render's gsr_backward
    r.buf.zero_(); r.signed.zero_(); r.absgrad(True)
    m2d = r.backward(r.fwd)[1][:, :2]
    err = float((r.signed - m2d).abs().max() / m2d.abs().max())
    na, ns = r.buf.grad.norm(dim=1), m2d.norm(dim=1)
    ok = ns > 0
    a, b, c, d, e = (float(np.median(ts[k])) for k in "abcde")
    return dict(config=name, P=r.P, W=r.W, H=r.H, num_rendered=int(r.fwd[0]), step=stats(ts["a"]), step_collecting=stats(ts["b"]),
                absgrad_call=stats(ts["c"]), absgrad_call_signed=stats(ts["d"]), depth_backward_call=stats(ts["e"]),
                collector_price_ms=b - a, collector_price_frac=(b - a) / a, absgrad_over_depth_backward=c / e,
                signed_against_backward_max_rel=err, ratio_median=float((na[ok] / ns[ok]).median()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace-friendly", action="store_true", help="3 repetitions, 1 warm-up, nothing written: for a run under a profiler")
    ap.add_argument("--configs", nargs="+", default=["cfg2_table_300k_800", "cfg3_synth_1M_1080p"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "absgrad", "bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("absgrad_bench.py measures on a HIP device; none found (no CPU fallback, no number)")
    if args.trace_friendly:
        args.reps, args.warmup = 3, 1
    dev = torch.device("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, results=[])
    for name in args.configs:
        r = bench_config(name, args.reps, args.warmup, dev)
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
