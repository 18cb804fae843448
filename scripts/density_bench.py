"""Times density control on the device (densify.FusedDensityController, csrc/density.hip) against the torch index arithmetic it
sits beside (densify.DensityController), in one process on one card.

    python scripts/density_bench.py [--reps 10] [--warmup 3] [--train-runs 3] [--out profiles/density/bench.json]

record            : one view's statistics (train.py:113-116), `visibility = radii > 0` over 60 % of the rows
densify_and_prune : clone / split / prune of all parameters and both Adam moments (about 5 % of the rows cloned, 10 % split, 4 % pruned)
at P = 1 000 000 with 16 SH coefficients (config 3's cloud) and P = 300 000 with 4.  The two paths alternate inside every
repetition.  Every call is timed twice over: device time between two events on the stream, and wall time on the host from the
call to the end of a device synchronise (the torch path's cost is partly host waits, which device events do not see when the
device idles meanwhile).  densify_and_prune changes the model, so every timed call gets a fresh copy of the same state, made
outside the timed window.  min / median / max in milliseconds.
train : scripts/train_synthetic.py at its defaults, --density torch against hip, it/s of whole runs, alternating, after one run each.
One JSON line to --out.  Needs a HIP device: no fallback."""
from __future__ import annotations

import functools
import importlib.util
import os
import statistics

import torch

import benchkit
from benchkit import ROOT, timed_dev_wall as timed
from gaussian_transformer_amd.densify import GROUPS, DensityController, FusedDensityController, OptimizationParams
from gaussian_transformer_amd.model import GaussianParams

DEV = "cuda:0"
ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling", "rotation": "_rotation"}
EXTENT = 4.0


def make_state(P, M, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s: torch.rand(*s, device=DEV, generator=g)
    n = lambda *s: torch.randn(*s, device=DEV, generator=g)
    par = {"xyz": n(P, 3), "f_dc": n(P, 1, 3), "f_rest": n(P, M - 1, 3), "opacity": 1.5 * n(P, 1) - 2.6,
           "scaling": torch.log(0.004 + 0.1 * r(P, 3) ** 3), "rotation": n(P, 4)}
    mom = {k: (0.01 * n(*v.shape), 1e-4 * r(*v.shape)) for k, v in par.items()}
    denom = torch.randint(1, 6, (P, 1), device=DEV, generator=g).float()
    accum = denom * 2e-4 * torch.exp(1.2 * n(P, 1) - 1.25)                      # about 15 % of the rows over 0.0002
    return {"par": par, "mom": mom, "accum": accum, "denom": denom}


def controller_on(build, st):
    """build(model) -> a controller on a fresh copy of the state's parameters, its optimizer given copies of the state's Adam moments."""
    m = GaussianParams(3)
    for k in GROUPS:
        setattr(m, ATTR[k], st["par"][k].clone().requires_grad_(True))
    ctl = build(m)
    for grp in ctl.optimizer.param_groups:
        a, b = st["mom"][grp["name"]]
        ctl.optimizer.state[grp["params"][0]] = {"step": 3, "exp_avg": a.clone(), "exp_avg_sq": b.clone()}
    return ctl


def make_controller(cls, st):
    ctl = controller_on(lambda m: cls(m, OptimizationParams(), adam="hip"), st)
    ctl.model.xyz_gradient_accum, ctl.model.denom = st["accum"].clone(), st["denom"].clone()
    return ctl


stats = functools.partial(benchkit.stats_minmax, digits=4)


def bench_shape(P, M, reps, warmup):
    st = make_state(P, M, seed=P + M)
    out = {"P": P, "M": M}
    # ---- record: the same controller over and over (the statistics just grow) ----
    g = torch.Generator(device=DEV).manual_seed(7)
    vs = torch.zeros(P, 3, device=DEV)
    vs.grad = 1e-3 * torch.randn(P, 3, device=DEV, generator=g)
    radii = (torch.rand(P, device=DEV, generator=g) < 0.6).int() * torch.randint(1, 40, (P,), device=DEV, generator=g, dtype=torch.int32)
    vis = radii > 0
    ctls = {"hip": make_controller(FusedDensityController, st), "torch": make_controller(DensityController, st)}
    dev_ms, wall_ms = {k: [] for k in ctls}, {k: [] for k in ctls}
    with torch.no_grad():
        for rep in range(warmup + 3 * reps):
            for name, ctl in ctls.items():
                d, w, _ = timed(lambda: ctl.record(vs, vis, radii))
                if rep >= warmup:
                    dev_ms[name].append(d); wall_ms[name].append(w)
    same = all(torch.allclose(getattr(ctls["hip"].model, a), getattr(ctls["torch"].model, a), rtol=1e-5, atol=0) for a in ("xyz_gradient_accum", "denom", "max_radii2D"))
    out["record"] = {"visible": int(vis.sum()), "same_statistics": bool(same),
                     **{k: {"device": stats(dev_ms[k]), "wall": stats(wall_ms[k])} for k in ctls}}
    del ctls
    # ---- densify_and_prune: a fresh copy of the state for every timed call ----
    classes = {"hip": FusedDensityController, "torch": DensityController}
    dev_ms, wall_ms, events = {k: [] for k in classes}, {k: [] for k in classes}, {}
    with torch.no_grad():
        for rep in range(warmup + reps):
            for name, cls in classes.items():
                ctl = make_controller(cls, st)
                gen = torch.Generator(device=DEV).manual_seed(11)
                d, w, ev = timed(lambda: ctl.densify_and_prune(0.0002, 0.005, EXTENT, 20, generator=gen))
                events[name] = dict(ev, P_new=int(ctl.model._xyz.shape[0]))
                if rep >= warmup:
                    dev_ms[name].append(d); wall_ms[name].append(w)
                del ctl
    out["densify_and_prune"] = {"events": events, "same_counts": events["hip"] == events["torch"],
                                "state_bytes": 3 * 4 * (14 + 3 * (M - 1)) * P,
                                **{k: {"device": stats(dev_ms[k]), "wall": stats(wall_ms[k])} for k in classes}}
    return out


def bench_train(runs, densities=("torch", "hip")):
    spec = importlib.util.spec_from_file_location("train_synthetic", os.path.join(ROOT, "scripts", "train_synthetic.py"))
    ts = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ts)
    rates = {k: [] for k in densities}
    last = {}
    for rep in range(runs + 1):                                       # the first run of each is the warm-up
        for density in rates:
            r = ts.run(density=density)
            last[density] = {k: r[k] for k in ("P_end", "psnr", "loss_last")}
            if rep:
                rates[density].append(r["it_per_s"])
    return {k: {"it_per_s_min": min(v), "it_per_s_median": statistics.median(v), "it_per_s_max": max(v), "runs": len(v), **last[k]} for k, v in rates.items()}


def main():
    ap = benchkit.parser(10, 3, "density")
    ap.add_argument("--train-runs", type=int, default=3, help="0: skip the training loop")
    args = benchkit.parse(ap)
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "shapes": []}
    for P, M in ((1_000_000, 16), (300_000, 4)):
        result["shapes"].append(bench_shape(P, M, args.reps, args.warmup))
        torch.cuda.empty_cache()
    if args.train_runs > 0:
        result["train_synthetic"] = bench_train(args.train_runs)
    benchkit.write_json(result, args.out, indent=None)


if __name__ == "__main__":
    main()
