"""Times the native sequence preparation against what a user has without it, in one process on one card.

    python scripts/sequence_bench.py [--reps 20] [--warmup 3] [--out profiles/sequence/bench.json]

Box sort (D = 26, xyz_col = 17, uniform coordinates with 1 % of the rows out of range):
  hip   : sequence.box_sort_rows (csrc/sequence.hip), n = 40, P = 300 000 and 1 000 000
  torch : the same result on the same device: torch.bucketize on the boundary table, a stable argsort of the box, a gather
  loop  : the reference's Python loop over the n^3 boxes (model/box_sort.py:55-66), only at n = 10 and P = 300 000, once
Visibility (B = 4 and 8 ring cameras):
  hip    : sequence.visible_union
  render : B no_grad render() calls, `radii > 0` OR-ed (train_stacked_transformer.py:93-96)
  at 300 000 Gaussians / 800 x 800 and 1 000 000 / 1920 x 1080.
Each pair alternates inside every repetition and is timed with device events after a warm-up, with a host synchronisation
around every timed call; min / median / max in milliseconds.  One JSON line to --out.  Needs a HIP device: no fallback."""
from __future__ import annotations

import time

import numpy as np
import torch

import benchkit
from benchkit import timed_drained as timed
from gaussian_transformer_amd import sequence as seq, synth
from gaussian_transformer_amd.model import GaussianParams
from gaussian_transformer_amd.render import PipelineParams, TorchCamera, render

DEV = "cuda:0"


def boundaries(n):
    return torch.tensor([(1.0 / n) * k for k in range(n + 1)], dtype=torch.float32, device=DEV)


def torch_box_sort(rows, xyz_col, n, b):
    xyz = rows[:, xyz_col:xyz_col + 3]
    valid = ((xyz >= b[0]) & (xyz < b[n])).all(1)
    cell = torch.bucketize(xyz.contiguous(), b, right=True) - 1
    key = torch.where(valid, cell[:, 0] + n * cell[:, 1] + n * n * cell[:, 2], n ** 3)
    skey, order = torch.sort(key, stable=True)
    count = valid.sum()
    out = rows[order] * (skey < n ** 3)[:, None]
    return out, order, count


def loop_box_sort(rows, xyz_col, n):
    """What the reference's loop costs (model/box_sort.py:55-66), not its text: per box, the two corners go up as fresh float32
    host tensors, six comparisons run over all rows, and a boolean gather synchronises the host."""
    out = torch.empty_like(rows)
    xyz = rows[:, xyz_col:xyz_col + 3]
    step = 1.0 / n
    filled = 0
    for box in range(n ** 3):
        cell = (box % n, (box // n) % n, box // (n * n))
        lo = torch.tensor([step * c for c in cell], dtype=torch.float32).to(DEV)
        hi = torch.tensor([step * (c + 1) for c in cell], dtype=torch.float32).to(DEV)
        inside = rows[((xyz >= lo) & (xyz < hi)).all(1)]
        out[filled:filled + len(inside)] = inside
        filled += len(inside)
    return out, filled


def compare(fns, reps, warmup):
    """alternating, in a fixed order: both see the same box noise"""
    return {k: benchkit.stats_minmax(v) for k, v in benchkit.alternate(fns, reps, warmup, timed=timed, rotate=False).items()}


def main():
    ap = benchkit.parser(20, 3, "sequence")
    ap.add_argument("--no-loop", action="store_true", help="skip the reference's Python loop (about a second at n = 10)")
    args = benchkit.parse(ap)
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "box_sort": [], "visible_union": []}
    g = torch.Generator(device=DEV).manual_seed(1)
    for P in (300_000, 1_000_000):
        rows = torch.rand(P, 26, device=DEV, generator=g)
        rows[::100, 18] = 1.0                                         # dropped rows, as after min-max normalisation
        n = 40
        b = boundaries(n)
        a, t = seq.box_sort_rows(rows, 17, n), torch_box_sort(rows, 17, n, b)
        c = int(a[2].item())
        same = bool(c == int(t[2]) and torch.equal(a[0], t[0]) and torch.equal(a[1][:c].long(), t[1][:c]))
        entry = {"P": P, "D": 26, "n": n, "count": c, "torch_formulation_equal": same}
        entry.update(compare({"hip": lambda: seq.box_sort_rows(rows, 17, n), "torch": lambda: torch_box_sort(rows, 17, n, b)}, args.reps, args.warmup))
        if P == 300_000 and not args.no_loop:
            w0 = time.perf_counter()
            ms, (ref_rows, last) = timed(lambda: loop_box_sort(rows, 17, 10))
            hip10 = seq.box_sort_rows(rows, 17, 10)
            entry["reference_loop_n10"] = {"ms": ms, "wall_s": time.perf_counter() - w0, "launch_bound_extrapolation_to_n40_ms": ms * 64.0,
                                           "equal_to_hip": bool(last == int(hip10[2].item()) and torch.equal(ref_rows[:last], hip10[0][:last]))}
            entry["hip_n10"] = compare({"hip": lambda: seq.box_sort_rows(rows, 17, 10)}, args.reps, args.warmup)["hip"]
        result["box_sort"].append(entry)
    bg = torch.zeros(3, device=DEV)
    for name, cfg, W, H in (("300k_800", "generic_300k_800", 800, 800), ("1M_1080p", "cfg3_synth_1M_1080p", 1920, 1080)):
        sc = synth.make_config(cfg)
        pc = GaussianParams.from_synthetic(sc, DEV, requires_grad=False)
        centre = sc.means3D.mean(0)
        for B in (4, 8):
            cams = [TorchCamera(sc.camera, DEV)] + [TorchCamera(c, DEV) for c in synth.tiramisu_ring_cameras(B - 1, W, H, centre=centre, radius=float(np.linalg.norm(centre)))]

            def by_render():
                vis = torch.zeros(sc.P, dtype=torch.bool, device=DEV)
                with torch.no_grad():
                    for cam in cams:
                        vis |= render(cam, pc, PipelineParams(), bg)["visibility_filter"]
                return vis
            same = bool(torch.equal(seq.visible_union(cams, pc), by_render()))
            entry = {"config": name, "P": sc.P, "W": W, "H": H, "B": B, "equal_to_render": same}
            entry.update(compare({"hip": lambda: seq.visible_union(cams, pc), "render": by_render}, args.reps, args.warmup))
            result["visible_union"].append(entry)
    benchkit.write_json(result, args.out, indent=None)


if __name__ == "__main__":
    main()
