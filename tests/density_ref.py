"""The one-pass density-control rule of include/gsr_density.h in torch, in any dtype, and the inputs the density tests share.

`one_pass` decides every Gaussian once and writes the new state in the reference's row order (surviving non-split originals,
surviving clones, surviving children with child j of the k-th split row at j * n_split + k before the prune).  On the CPU in
float32 it equals DensityController.densify_and_prune -- the restatement of the reference's GaussianModel -- bit for bit
(tests/test_density_host.py); in float64 it is what the HIP path's split children are held to (tests/test_gpu_density.py).

`build_inputs` draws a cloud and then moves every row whose float64 quantity lies within a relative MARGIN of a threshold it
is compared with outside that margin: torch's exp and the kernel's expf may legitimately decide such a row differently.
After that it plants the rows whose decision is exact by construction.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from gaussian_transformer_amd.densify import GROUPS, quaternion_to_rotation

MARGIN = 1e-5
EXTENT, THRESHOLD, MIN_OPACITY, PERCENT_DENSE = 4.0, 0.0002, 0.005, 0.01
FAULTS = ("child_order", "screen_size", "strict_gradient")


def f32(v) -> float:
    """What torch compares a float32 tensor with when handed the Python number v."""
    return float(np.float32(v))


def one_pass(par, mom, accum, denom, noise_fn, max_screen_size, max_radii=None, extent=EXTENT, threshold=THRESHOLD,
             min_opacity=MIN_OPACITY, percent_dense=PERCENT_DENSE, N=2, fault=None):
    """par: {group: [P, ...]}, mom: {group: (exp_avg, exp_avg_sq)} or None, accum / denom [P, 1]; noise_fn(rows) -> [rows, 3]
    standard normal samples.  Returns (new par, new mom or None, {"cloned", "split", "pruned"}, P_new, {"xyz", "scaling"} of the
    surviving children).  `fault` plants one of FAULTS (the mutants the host test must tell from the rule)."""
    assert fault is None or fault in FAULTS
    dt = par["xyz"].dtype
    c = lambda v: torch.tensor(f32(v), dtype=dt)
    g = (accum / denom).reshape(-1)
    g[g.isnan()] = 0.0
    e = torch.exp(par["scaling"])
    size = e.max(dim=1).values
    hot = (g > c(threshold)) if fault == "strict_gradient" else (g >= c(threshold))
    cut = c(percent_dense * extent)
    clone, split = hot & (size <= cut), hot & (size > cut)
    low = torch.sigmoid(par["opacity"]).reshape(-1) < c(min_opacity)
    child_scaling = torch.log(e / (0.8 * N))
    if max_screen_size:
        world = c(0.1 * extent)
        big, childbig = size > world, torch.exp(child_scaling).max(dim=1).values > world
        if fault == "screen_size":
            big = big | (max_radii > max_screen_size)
    else:
        big = childbig = torch.zeros_like(low)
    keep_self, keep_clone, keep_child = ~split & ~(low | big), clone & ~(low | big), split & ~(low | childbig)
    n_split = int(split.sum())
    noise = noise_fn(N * n_split).to(dt)
    tile = (lambda t: t[split].repeat_interleave(N, dim=0)) if fault == "child_order" else \
        (lambda t: t[split].repeat(N, *([1] * (t.dim() - 1))))
    samples = noise * tile(e)
    R = quaternion_to_rotation(tile(par["rotation"]))
    child = {n: tile(par[n]) for n in GROUPS}
    child["xyz"] = torch.bmm(R, samples.unsqueeze(-1)).squeeze(-1) + tile(par["xyz"])
    child["scaling"] = tile(child_scaling)
    kc = tile(keep_child)
    new = {n: torch.cat((par[n][keep_self], par[n][keep_clone], child[n][kc]), dim=0) for n in GROUPS}
    new_mom = None
    if mom is not None:
        fresh = int(keep_clone.sum()) + int(kc.sum())
        new_mom = {n: tuple(torch.cat((t[keep_self], torch.zeros((fresh,) + tuple(t.shape[1:]), dtype=t.dtype)), dim=0) for t in mom[n])
                   for n in GROUPS}
    counts = {"cloned": int(clone.sum()), "split": n_split,
              "pruned": int((~split & ~keep_self).sum()) + int((clone & ~keep_clone).sum()) + N * int((split & ~keep_child).sum())}
    return new, new_mom, counts, new["xyz"].shape[0], {"xyz": child["xyz"][kc], "scaling": child["scaling"][kc]}


def _near(x64, t):
    return (x64 - t).abs() <= MARGIN * abs(t)


def _margins(d, max_screen_size_used=True):
    """Rows of the float32 inputs whose float64 quantities lie within MARGIN of a threshold, per quantity."""
    size = torch.exp(d["par"]["scaling"].double()).max(dim=1).values
    cut, world = f32(PERCENT_DENSE * EXTENT), f32(0.1 * EXTENT)
    near_size = _near(size, cut) | _near(size, world) | _near(size / (0.8 * 2), world)
    near_op = _near(torch.sigmoid(d["par"]["opacity"].double()).reshape(-1), f32(MIN_OPACITY))
    g = (d["accum"].double() / d["denom"].double()).reshape(-1)
    near_g = _near(torch.nan_to_num(g, nan=0.0, posinf=1e30), f32(THRESHOLD))
    return near_size, near_op, near_g


@functools.lru_cache(maxsize=None)
def build_inputs(P: int, rest_width: int, seed: int = 0, mode: str = "mixed"):
    """Float32 CPU inputs, shared and never modified by the tests (they clone).  mode: "mixed", or one of "none" (no row over the
    gradient threshold), "split", "clone" (every row, kept), "pruned" (every opacity under the threshold, nothing selected)."""
    gen = torch.Generator().manual_seed(1000 * P + 10 * rest_width + seed)
    r = lambda *s: torch.rand(*s, generator=gen)
    n = lambda *s: torch.randn(*s, generator=gen)
    lo, hi = np.log(0.004), np.log(1.2)                     # sizes across cut = 0.04, 0.1 extent = 0.4 and 1.6 x 0.4
    par = {"xyz": n(P, 3), "f_dc": n(P, 1, 3), "f_rest": n(P, rest_width, 3), "opacity": -2.0 + 3.0 * n(P, 1),
           "scaling": lo + (hi - lo) * r(P, 3), "rotation": n(P, 4) + 0.1}
    denom = torch.randint(0, 6, (P, 1), generator=gen).float()
    accum = denom * torch.exp(np.log(2e-5) + (np.log(2e-3) - np.log(2e-5)) * r(P, 1))
    if mode == "none":
        accum = accum * 0.0
    elif mode in ("split", "clone"):
        denom, accum = torch.ones(P, 1), torch.full((P, 1), 0.01)
        par["scaling"] = (np.log(0.1) if mode == "split" else np.log(0.01)) + 0.3 * r(P, 3)
        par["opacity"] = 1.0 + r(P, 1)
    elif mode == "pruned":
        accum, par["opacity"] = accum * 0.0, -8.0 - r(P, 1)
    d = {"par": par, "accum": accum, "denom": denom, "max_radii": 60.0 * r(P)}
    for _ in range(4):                                       # move borderline rows out of the margin
        near_size, near_op, near_g = _margins(d)
        par["scaling"][near_size] += 1e-3
        par["opacity"][near_op] += 1e-3
        d["accum"][near_g] *= 1.001
    assert not any(bool(m.any()) for m in _margins(d)), "a row is still within the margin of a threshold"
    planted = {}
    if mode == "mixed":                                      # decisions that are exact by construction
        thr = torch.tensor(f32(THRESHOLD))
        rows = {"exact": 0} if P < 4 else {"exact": P // 2, "nan": 1, "inf": P - 1}
        for what, i in rows.items():
            d["accum"][i] = {"exact": 2 * thr, "nan": 0.0, "inf": 0.001}[what]
            d["denom"][i] = 2.0 if what == "exact" else 0.0
        planted = rows
    d["planted"] = planted
    d["mom"] = {k: (0.01 * n(*v.shape), 1e-4 * r(*v.shape)) for k, v in par.items()}
    return d


def clone_inputs(d, device="cpu", dtype=None):
    t = lambda x: x.detach().clone().to(device=device, dtype=dtype or x.dtype)
    return {"par": {k: t(v) for k, v in d["par"].items()}, "mom": {k: (t(a), t(b)) for k, (a, b) in d["mom"].items()},
            "accum": t(d["accum"]), "denom": t(d["denom"]), "max_radii": t(d["max_radii"]), "planted": dict(d["planted"])}
