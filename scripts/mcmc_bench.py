"""Times MCMC density control on the device (densify.FusedMCMCController, csrc/mcmc.hip) against the torch index arithmetic it
sits beside (densify.MCMCController on the same card: the yardstick), in one process.

    python scripts/mcmc_bench.py [--reps 50] [--warmup 5] [--train-runs 2] [--out profiles/mcmc/bench.json]

relocate   : 5 % of the rows dead, every parameter and both Adam moments present
grow       : 5 % more rows (cap far away)
add_noise  : the position noise of every iteration (the fused launch moves 68 B per Gaussian: its share of the card's HBM bandwidth,
             --hbm-gbs, is reported)
regularize : the two regularisers' gradients and means
at P = 1 000 000 with 16 SH coefficients and P = 300 000 with 4.  The two paths alternate inside every repetition.  Every call is
timed twice over: device time between two events on the stream, and wall time on the host from the call to the end of a device
synchronise (the torch path's cost is partly host waits, which device events do not see).  relocate and grow change the model, so
every timed call gets a fresh copy of the same state, made outside the timed window.  min / median / max in milliseconds.
train : scripts/train_synthetic.py at its defaults, --density hip, mcmc and mcmc_hip at the same final count: it/s of whole runs,
alternating, after one run each, and the final PSNR.  One JSON line to --out.  Needs a HIP device: no fallback."""
from __future__ import annotations

import torch

import benchkit
from benchkit import timed_dev_wall as timed
from density_bench import bench_train, controller_on, stats
from gaussian_transformer_amd.densify import FusedMCMCController, MCMCController, MCMCParams, OptimizationParams

DEV = "cuda:0"
CLASSES = {"hip": FusedMCMCController, "torch": MCMCController}


def make_state(P, M, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s: torch.rand(*s, device=DEV, generator=g)
    n = lambda *s: torch.randn(*s, device=DEV, generator=g)
    opacity = 1.5 * n(P, 1) - 1.0
    opacity = torch.where(r(P, 1) < 0.05, -7.0 - r(P, 1), opacity.clamp_min(-5.0))           # 5 % of the rows dead (logit <= -5.29)
    par = {"xyz": n(P, 3), "f_dc": n(P, 1, 3), "f_rest": n(P, M - 1, 3), "opacity": opacity,
           "scaling": torch.log(0.004 + 0.1 * r(P, 3) ** 3), "rotation": n(P, 4)}
    mom = {k: (0.01 * n(*v.shape), 1e-4 * r(*v.shape)) for k, v in par.items()}
    return {"par": par, "mom": mom}


def make_controller(cls, st):
    ctl = controller_on(lambda m: cls(m, MCMCParams(cap_max=10 ** 9), OptimizationParams(), adam="hip"), st)
    ctl.update_learning_rate(1000)
    return ctl


def bench_shape(P, M, reps, warmup, hbm_gbs):
    st = make_state(P, M, seed=P + M)
    out = {"P": P, "M": M, "state_bytes": 3 * 4 * (14 + 3 * (M - 1)) * P}
    g = torch.Generator(device=DEV).manual_seed(7)
    u, noise = torch.rand(P, device=DEV, generator=g), torch.randn(P, 3, device=DEV, generator=g)
    # ---- relocate, grow: a fresh copy of the state for every timed call ----
    for what in ("relocate", "grow"):
        dev_ms, wall_ms, counts = {k: [] for k in CLASSES}, {k: [] for k in CLASSES}, {}
        with torch.no_grad():
            for rep in range(warmup + reps):
                for name, cls in CLASSES.items():
                    ctl = make_controller(cls, st)
                    d, w, _ = timed((lambda: ctl.relocate(u=u)) if what == "relocate" else (lambda: ctl.grow(u=u)))
                    counts[name] = ctl.counts(what)
                    if rep >= warmup:
                        dev_ms[name].append(d); wall_ms[name].append(w)
                    del ctl
        out[what] = {"counts": counts, "same_counts": counts["hip"] == counts["torch"],
                     **{k: {"device": stats(dev_ms[k]), "wall": stats(wall_ms[k])} for k in CLASSES}}
    # ---- add_noise, regularize: the same controllers over and over ----
    ctls = {k: make_controller(cls, st) for k, cls in CLASSES.items()}
    for ctl in ctls.values():
        ctl.model._opacity.grad, ctl.model._scaling.grad = torch.zeros_like(ctl.model._opacity), torch.zeros_like(ctl.model._scaling)
    for what in ("add_noise", "regularize"):
        dev_ms, wall_ms = {k: [] for k in ctls}, {k: [] for k in ctls}
        with torch.no_grad():
            for rep in range(warmup + reps):
                for name, ctl in ctls.items():
                    d, w, _ = timed((lambda: ctl.add_noise(noise=noise)) if what == "add_noise" else ctl.regularize)
                    if rep >= warmup:
                        dev_ms[name].append(d); wall_ms[name].append(w)
        out[what] = {k: {"device": stats(dev_ms[k]), "wall": stats(wall_ms[k])} for k in ctls}
    gbs = 68 * P / (out["add_noise"]["hip"]["device"]["median_ms"] * 1e-3) / 1e9
    out["add_noise"]["hip"]["bytes_per_gaussian"] = 68
    out["add_noise"]["hip"]["achieved_gbs"] = round(gbs, 1)
    out["add_noise"]["hip"]["share_of_hbm"] = round(gbs / hbm_gbs, 3)
    return out


def main():
    ap = benchkit.parser(50, 5, "mcmc")
    ap.add_argument("--train-runs", type=int, default=2, help="0: skip the training loop")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the card's peak HBM bandwidth in GB/s (MI355X: 8 TB/s)")
    args = benchkit.parse(ap)
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hbm_gbs": args.hbm_gbs, "shapes": []}
    for P, M in ((1_000_000, 16), (300_000, 4)):
        result["shapes"].append(bench_shape(P, M, args.reps, args.warmup, args.hbm_gbs))
        torch.cuda.empty_cache()
    if args.train_runs > 0:
        result["train_synthetic"] = bench_train(args.train_runs, ("hip", "mcmc", "mcmc_hip"))
    benchkit.write_json(result, args.out, indent=None)


if __name__ == "__main__":
    main()
