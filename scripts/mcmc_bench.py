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

import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gaussian_transformer_amd.densify import GROUPS, FusedMCMCController, MCMCController, MCMCParams, OptimizationParams  # noqa: E402
from gaussian_transformer_amd.model import GaussianParams  # noqa: E402

DEV = "cuda:0"
ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling", "rotation": "_rotation"}
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
    m = GaussianParams(3)
    for k in GROUPS:
        setattr(m, ATTR[k], st["par"][k].clone().requires_grad_(True))
    ctl = cls(m, MCMCParams(cap_max=10 ** 9), OptimizationParams(), adam="hip")
    for grp in ctl.optimizer.param_groups:
        a, b = st["mom"][grp["name"]]
        ctl.optimizer.state[grp["params"][0]] = {"step": 3, "exp_avg": a.clone(), "exp_avg_sq": b.clone()}
    ctl.update_learning_rate(1000)
    return ctl


def timed(fn):
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    w0 = time.perf_counter()
    t0.record()
    out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), (time.perf_counter() - w0) * 1e3, out


def stats(ms):
    return {"min_ms": round(min(ms), 4), "median_ms": round(statistics.median(ms), 4), "max_ms": round(max(ms), 4), "reps": len(ms)}


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


def bench_train(runs):
    spec = importlib.util.spec_from_file_location("train_synthetic", os.path.join(ROOT, "scripts", "train_synthetic.py"))
    ts = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ts)
    rates = {"hip": [], "mcmc": [], "mcmc_hip": []}
    last = {}
    for rep in range(runs + 1):                                       # the first run of each is the warm-up
        for density in rates:
            r = ts.run(density=density)
            last[density] = {k: r[k] for k in ("P_end", "psnr", "loss_last")}
            if rep:
                rates[density].append(r["it_per_s"])
    return {k: {"it_per_s_min": min(v), "it_per_s_median": statistics.median(v), "it_per_s_max": max(v), "runs": len(v), **last[k]} for k, v in rates.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--train-runs", type=int, default=2, help="0: skip the training loop")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the card's peak HBM bandwidth in GB/s (MI355X: 8 TB/s)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcmc", "bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mcmc_bench.py needs a HIP device (nothing is timed on a CPU)")
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hbm_gbs": args.hbm_gbs, "shapes": []}
    for P, M in ((1_000_000, 16), (300_000, 4)):
        result["shapes"].append(bench_shape(P, M, args.reps, args.warmup, args.hbm_gbs))
        torch.cuda.empty_cache()
    if args.train_runs > 0:
        result["train_synthetic"] = bench_train(args.train_runs)
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
