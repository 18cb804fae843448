#!/usr/bin/env python3
"""gsr_adam_step against gsr_adam_step_masked (include/gsr_optim.h) on the reference's six parameter groups, P Gaussians, SH degree 3
(row widths 3, 3, 45, 1, 3, 4: 59 floats per Gaussian, 944 MB of state and gradients at P = 1 M -- beyond the Infinity Cache, so
back-to-back launches measure HBM).  One process; the dense and the masked call alternate inside every repetition, on the same
buffers, timed with device events.  Informational (bench.py is the headline metric).

Masks: all rows, none, random 50 / 20 / 9 %, 9 % as runs of 1024 rows, and the radii > 0 and composited_mask() of one render of
BASELINE config 3 and of config 2 (the latter two at that scene's own P).  Gradients once as ordinary aligned tensors, once as
consecutive slices of one flat arena, and once as slices of an arena for P + 1 Gaussians (odd: every slice after the first starts
on a 4-byte boundary only, which is the kernels' scalar body).

Per case: the bytes the algorithm needs (28 w per visible row plus the mask's bytes) and the rate they were moved at.

    python scripts/sparse_adam_bench.py [--P 1000000] [--reps 50] [--out profiles/sparse_adam/bench.json]
"""
import json
import numpy as np
import torch
import benchkit
from gaussian_transformer_amd import _lib, rasterizer, synth
from gaussian_transformer_amd.model import GaussianParams
from gaussian_transformer_amd.render import PipelineParams, TorchCamera, render_fused

WIDTHS = [3, 3, 45, 1, 3, 4]
LRS = [0.00016, 0.0025, 0.0025 / 20.0, 0.05, 0.005, 0.001]
BETAS, EPS, STEP = (0.9, 0.999), 1e-15, 100


class State:
    def __init__(self, P, layout, dev):
        gen = torch.Generator(device=dev).manual_seed(P)
        r = lambda n: torch.randn(n, device=dev, generator=gen)
        self.P = P
        self.p = [r(P * w) for w in WIDTHS]
        self.m = [1e-2 * r(P * w) for w in WIDTHS]
        self.v = [1e-4 * torch.rand(P * w, device=dev, generator=gen) + 1e-8 for w in WIDTHS]
        if layout == "tensors":
            self.g = [r(P * w) for w in WIDTHS]
        else:
            self.arena = r(P * sum(WIDTHS))
            offs = np.concatenate(([0], np.cumsum([P * w for w in WIDTHS])))
            self.g = [self.arena[int(a):int(b)] for a, b in zip(offs[:-1], offs[1:])]
        self.misaligned = sum(t.data_ptr() % 16 != 0 for t in self.g)
        groups = [_lib.AdamGroup(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, STEP)
                  for p, g, m, v, lr in zip(self.p, self.g, self.m, self.v, LRS)]
        self.arr = (_lib.AdamGroup * len(groups))(*groups)
        self.lib = _lib.load()
        self.stream = torch.cuda.current_stream(dev).cuda_stream

    def dense(self):
        _lib.check(self.lib.gsr_adam_step(self.stream, len(WIDTHS), self.arr, BETAS[0], BETAS[1], EPS), "gsr_adam_step")

    def masked(self, mask):
        kind = _lib.ADAM_MASK_RADII if mask.dtype == torch.int32 else _lib.ADAM_MASK_BYTES
        _lib.check(self.lib.gsr_adam_step_masked(self.stream, len(WIDTHS), self.arr, BETAS[0], BETAS[1], EPS, self.P, mask.data_ptr(), kind),
                   "gsr_adam_step_masked")


def summary(xs):
    """benchkit's min / median / max, the median first: the key order these records have had from the first profile on."""
    s = benchkit.stats_minmax(xs, count=None, digits=4)
    return {k: s[k] for k in ("median_ms", "min_ms", "max_ms")}


def measure(state, mask, reps, warmup):
    dense, masked = [], []
    for it in range(warmup + reps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record(); state.dense(); e[1].record(); state.masked(mask); e[2].record()
        torch.cuda.synchronize()
        if it >= warmup:
            dense.append(e[0].elapsed_time(e[1])); masked.append(e[1].elapsed_time(e[2]))
    return dense, masked


def case(name, state, layout, mask, reps, warmup):
    n_vis = int((mask > 0).sum()) if mask.dtype == torch.int32 else int((mask != 0).sum())
    P = state.P
    need = 28 * sum(WIDTHS) * n_vis + mask.numel() * mask.element_size()
    dense_bytes = 28 * sum(WIDTHS) * P
    d, m = measure(state, mask, reps, warmup)
    md, mm = float(np.median(d)), float(np.median(m))
    rec = {"case": name, "layout": layout, "P": P, "misaligned_gradient_slices": int(state.misaligned), "mask_dtype": str(mask.dtype).replace("torch.", ""),
           "visible": n_vis, "visible_fraction": round(n_vis / max(P, 1), 4), "dense": summary(d), "masked": summary(m),
           "masked_over_dense": round(mm / md, 4), "dense_bytes": dense_bytes, "dense_GBps": round(dense_bytes / md / 1e6, 1),
           "needed_bytes": need, "needed_over_dense_bytes": round(need / dense_bytes, 4), "masked_needed_GBps": round(need / mm / 1e6, 1)}
    print(json.dumps(rec), flush=True)
    return rec


def synthetic_masks(P, dev):
    gen = torch.Generator(device=dev).manual_seed(7)
    u = torch.rand(P, device=dev, generator=gen)
    runs = torch.rand((P + 1023) // 1024, device=dev, generator=gen) < 0.09
    out = {"all rows (bytes)": torch.ones(P, dtype=torch.uint8, device=dev), "all rows (radii)": torch.full((P,), 5, dtype=torch.int32, device=dev),
           "none": torch.zeros(P, dtype=torch.uint8, device=dev)}
    for f in (0.5, 0.2, 0.09):
        out[f"random {f:g}"] = (u < f).to(torch.uint8)
    out["runs of 1024 rows, 9 %"] = runs.repeat_interleave(1024)[:P].to(torch.uint8)
    return out


def render_masks(config, dev):
    """radii (int32, as the render returns them) and composited_mask() of one render of a BASELINE config."""
    sc = synth.make_config(config)
    pc = GaussianParams.from_synthetic(sc, dev)
    pkg = render_fused(TorchCamera(sc.camera, dev), pc, PipelineParams(), torch.tensor(sc.bg, device=dev))
    comp = rasterizer.composited_mask()
    assert comp is not None, "the backend does not know the last forward pass"
    radii = pkg["radii"].to(torch.int32).contiguous().clone()
    comp = comp.to(torch.uint8).contiguous().clone()
    del pkg, pc
    return int(radii.numel()), {f"{config} radii > 0": radii, f"{config} composited": comp}


if __name__ == "__main__":
    ap = benchkit.parser(50, 5, "sparse_adam")
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--configs", default="cfg3_synth_1M_1080p,cfg2_table_300k_800")
    a = benchkit.parse(ap)
    dev = torch.device("cuda", 0)
    scene_masks = {}
    for cfg in [c for c in a.configs.split(",") if c]:
        P_cfg, masks = render_masks(cfg, dev)
        scene_masks.setdefault(P_cfg, {}).update(masks)
    torch.cuda.empty_cache()
    records = []
    for layout, P in (("tensors", a.P), ("arena", a.P), ("arena, odd P", a.P + 1)):
        st = State(P, "tensors" if layout == "tensors" else "arena", dev)
        masks = synthetic_masks(P, dev)
        if layout == "arena, odd P":
            masks = {k: masks[k] for k in ("all rows (bytes)", "random 0.09", "runs of 1024 rows, 9 %")}
        masks.update(scene_masks.get(P, {}))
        for name, mask in masks.items():
            records.append(case(name, st, layout, mask, a.reps, a.warmup))
        del st
        torch.cuda.empty_cache()
    for P, masks in scene_masks.items():
        if P in (a.P, a.P + 1):
            continue
        st = State(P, "tensors", dev)
        records.append(case("all rows (bytes)", st, "tensors", torch.ones(P, dtype=torch.uint8, device=dev), a.reps, a.warmup))
        for name, mask in masks.items():
            records.append(case(name, st, "tensors", mask, a.reps, a.warmup))
        del st
    benchkit.write_json({"what": "gsr_adam_step vs gsr_adam_step_masked, device events, alternating in one process", "widths": WIDTHS, "reps": a.reps,
                         "device": torch.cuda.get_device_name(0), "records": records}, a.out)
