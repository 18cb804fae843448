"""Times the multi-view image loss against the two formulations a user has without it, in one process on one card.

    python scripts/views_loss_bench.py [--reps 30] [--warmup 5] [--out profiles/views_loss/bench.json]

The image loss of the stacked trainer's step (train_stacked_transformer.py:203-222) for B = 4 and 8 views at 800x800 and 1600x900,
forward + backward down to the B prediction images (separate tensors, as B renders are), of
  torch : clamp(nan_to_num(.)) of every view written into [B,3,H,W] buffers, loss.l1_loss and loss.ssim on the batch, autograd
  fused : the same sanitising and torch.stack, then loss.fused_l1_ssim_loss on the batch seen as [3B,H,W]
  views : loss.stacked_image_loss on the B tensors (csrc/ssim_loss.hip: views_loss_*)
timed with device events after a warm-up, the three alternating inside every repetition; min / median / max in milliseconds and
torch's peak allocated memory above what was allocated before the call.  The three must agree on loss and gradients (float32
formulations of one formula: 1e-4 of the largest gradient) or the script fails.  One JSON line to --out.  Needs a HIP device."""
from __future__ import annotations

import torch

import benchkit
from gaussian_transformer_amd import loss

SHAPES = [(4, 800, 800), (8, 800, 800), (4, 900, 1600), (8, 900, 1600)]      # B, H, W


def _sanitise(x):
    return torch.clamp(torch.nan_to_num(x), 0.0, 1.0)


def torch_form(xs, gts):
    B = len(xs)
    images = torch.zeros((B,) + tuple(xs[0].shape), dtype=torch.float32, device=xs[0].device)
    targets = torch.zeros_like(images)
    for i in range(B):
        images[i] = _sanitise(xs[i])
        targets[i] = _sanitise(gts[i])
    return loss.STACKED_W_L1 / B * loss.l1_loss(images, targets) + loss.STACKED_W_SSIM / B * (1.0 - loss.ssim(images, targets))


def fused_form(xs, gts):
    B, (_, H, W) = len(xs), xs[0].shape
    images = torch.stack([_sanitise(x) for x in xs]).reshape(3 * B, H, W)
    targets = torch.stack([_sanitise(g) for g in gts]).reshape(3 * B, H, W)
    total = (loss.STACKED_W_L1 + loss.STACKED_W_SSIM) / B
    return total * loss.fused_l1_ssim_loss(images, targets, loss.STACKED_W_SSIM / (loss.STACKED_W_L1 + loss.STACKED_W_SSIM))


def views_form(xs, gts):
    return loss.stacked_image_loss(xs, gts)


FORMS = (("torch", torch_form), ("fused", fused_form), ("views", views_form))


def main():
    args = benchkit.parse(benchkit.parser(30, 5, "views_loss"))
    if args.reps < 20:
        raise SystemExit("--reps must be at least 20")
    dev = "cuda:0"
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "what": "forward + backward, ms", "shapes": []}
    for (B, H, W) in SHAPES:
        g = torch.Generator(device=dev).manual_seed(B * H + W)
        xs = [(torch.rand(3, H, W, device=dev, generator=g) * 1.5 - 0.25).requires_grad_(True) for _ in range(B)]
        gts = [torch.rand(3, H, W, device=dev, generator=g) for _ in range(B)]

        def clear():
            for x in xs:
                x.grad = None

        def call(fn):
            L = fn(xs, gts)
            L.backward()
            return L
        ms = {n: [] for n, _ in FORMS}
        peak = {n: 0 for n, _ in FORMS}
        first = {}
        for rep in range(args.warmup + args.reps):
            for name, fn in FORMS:                                   # alternating: all three see the same box noise
                t, p, L = benchkit.timed_peak(lambda: call(fn), clear)
                L = L.detach()                                       # the graph goes now, not under the next call's starting allocation
                if rep == 0:
                    first[name] = (float(L), [x.grad.clone() for x in xs])
                if rep >= args.warmup:
                    ms[name].append(t)
                    peak[name] = max(peak[name], p)
        entry = {"B": B, "H": H, "W": W, "map_entries": 3 * B * H * W}
        scale = max(float(gr.abs().max()) for gr in first["torch"][1])
        for name in ("fused", "views"):
            dl = abs(first[name][0] - first["torch"][0]) / abs(first["torch"][0])
            dg = max(float((a - b).abs().max()) for a, b in zip(first[name][1], first["torch"][1])) / scale
            entry[f"{name}_vs_torch"] = {"loss_rel": dl, "grad_max_over_max": dg}
            if not (dl <= 1e-4 and dg <= 1e-4):
                raise SystemExit(f"{name} disagrees with torch at B={B} {H}x{W}: loss {dl:.3e}, gradient {dg:.3e}")
        for name in ms:
            entry[name] = dict(benchkit.stats_minmax(ms[name]), peak_extra_bytes=peak[name])
        v, f = entry["views"], entry["fused"]
        spread = (v["max_ms"] - v["min_ms"]) + (f["max_ms"] - f["min_ms"])
        entry["fused_median_minus_views_median_ms"] = f["median_ms"] - v["median_ms"]
        entry["sum_of_min_max_spreads_ms"] = spread
        entry["views_faster_than_fused_beyond_spread"] = bool(f["median_ms"] - v["median_ms"] > spread)
        result["shapes"].append(entry)
        del xs, gts, first
        torch.cuda.empty_cache()
    benchkit.write_json(result, args.out, indent=None)


if __name__ == "__main__":
    main()
