"""Times the HIP Chamfer distance against the formulation a user has without it, in one process on one card.

    python scripts/chamfer_bench.py [--reps 30] [--warmup 5] [--out profiles/chamfer/bench.json]

Shapes: the reference's (B 1, N = M = 8192 and 16384, D = 26) and the classic (B 4, N = M = 4096, D = 3).  For each, forward and
forward+backward (loss = dist1.mean() + dist2.mean()) of
  hip   : chamfer_distance.ChamferDistance (csrc/chamfer.hip)
  torch : torch.cdist(x1, x2).square(), .min(2) and .min(1), autograd
timed with device events after a warm-up, the two alternating inside every repetition; min / median / max in milliseconds and
torch's peak allocated memory above what was allocated before the call.  One JSON line to --out.  Needs a HIP device: no fallback."""
from __future__ import annotations

import torch

import benchkit
from chamfer_distance import ChamferDistance

SHAPES = [(1, 8192, 8192, 26), (1, 16384, 16384, 26), (4, 4096, 4096, 3)]


def hip_chamfer(chd, x1, x2):
    d1, d2, _, _ = chd(x1, x2)
    return d1, d2


def torch_chamfer(_chd, x1, x2):
    d = torch.cdist(x1, x2).square()
    return d.min(2).values, d.min(1).values


def main():
    args = benchkit.parse(benchkit.parser(30, 5, "chamfer"))
    if args.reps < 20:
        raise SystemExit("--reps must be at least 20")
    dev = "cuda:0"
    chd = ChamferDistance()
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "loss": "dist1.mean() + dist2.mean()", "shapes": []}
    for (B, N, M, D) in SHAPES:
        g = torch.Generator(device=dev).manual_seed(N + D)
        x1 = torch.randn(B, N, D, device=dev, generator=g).requires_grad_(True)
        x2 = torch.randn(B, M, D, device=dev, generator=g).requires_grad_(True)

        def clear():
            x1.grad = x2.grad = None

        def call(fn, backward):
            d1, d2 = fn(chd, x1, x2)
            if backward:
                (d1.mean() + d2.mean()).backward()
            return d1, d2                                                    # alive until the window has closed and the peak is read
        entry = {"B": B, "N": N, "M": M, "D": D, "inputs_bytes": 4 * B * (N + M) * D}
        for backward in (False, True):
            ms = {"hip": [], "torch": []}
            peak = {"hip": 0, "torch": 0}
            for rep in range(args.warmup + args.reps):
                for name, fn in (("hip", hip_chamfer), ("torch", torch_chamfer)):      # alternating: both see the same box noise
                    t, p, _ = benchkit.timed_peak(lambda: call(fn, backward), clear)
                    if rep >= args.warmup:
                        ms[name].append(t)
                        peak[name] = max(peak[name], p)
            key = "fwd_bwd" if backward else "fwd"
            entry[key] = {n: dict(benchkit.stats_minmax(ms[n]), peak_extra_bytes=peak[n]) for n in ms}
            h, t = entry[key]["hip"], entry[key]["torch"]
            spread = (h["max_ms"] - h["min_ms"]) + (t["max_ms"] - t["min_ms"])
            entry[key]["torch_median_minus_hip_median_ms"] = t["median_ms"] - h["median_ms"]
            entry[key]["sum_of_min_max_spreads_ms"] = spread
            entry[key]["hip_faster_beyond_spread"] = bool(t["median_ms"] - h["median_ms"] > spread)
        result["shapes"].append(entry)
    benchkit.write_json(result, args.out, indent=None)


if __name__ == "__main__":
    main()
