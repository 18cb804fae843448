"""Writes tests/golden/box_sort.npz by running the REFERENCE's own model/box_sort.py on the CPU.

    python scripts/make_box_sort_golden.py --ref <reference checkout> [--out tests/golden]

Runs only where a checkout of the reference is present; the fixture it writes is data (inputs and recorded outputs) and is
committed, the reference never is.  As oracle/make_golden.py does for GaussianModel: `plyfile` gets an empty stand-in module,
`simple_knn._C` resolves to this repository's, device="cuda" literals and .cuda() calls are shimmed to stay on the CPU.
torch.empty_like is made to return NaN so that `last`, which box_sort does not return, can be read off its result: the
rows it never wrote.

The cloud is built so that normalisation is exact (every axis spans exactly [0, 1], so (x - 0) / (1 - 0) = x) and carries the
boundaries of n = 10 and n = 40, their one-ulp neighbours and the corners, besides random points.
"""
from __future__ import annotations

import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def make_inputs(P: int, seed: int):
    rng = np.random.default_rng(seed)
    q = lambda a: (np.round(a * 64) / 64).astype(np.float32)          # coarse values: the fixture compresses, the sort does not care
    xyz = rng.random((P, 3), dtype=np.float32)
    edges = []
    for n in (10, 40):
        b = np.array([(1.0 / n) * k for k in range(n + 1)], dtype=np.float32)
        edges += [b, np.nextafter(b, np.float32(-1)), np.nextafter(b, np.float32(2))]
    edges = np.clip(np.concatenate(edges), 0, 1).astype(np.float32)
    k = P // 4
    where = rng.choice(P, size=k, replace=False)
    xyz[where, rng.integers(0, 3, size=k)] = edges[rng.integers(0, len(edges), size=k)]
    xyz[0] = 0.0                                                     # the extrema: min 0 and max 1 on every axis
    xyz[1] = 1.0
    xyz[2] = (1.0, 0.5, 0.25)
    xyz[P // 2:P // 2 + 100] = xyz[100:200]                           # duplicates
    return {"xyz": xyz, "scaling": q(rng.normal(size=(P, 3)) - 4), "features_dc": q(rng.normal(size=(P, 1, 3))),
            "features_rest": q(rng.normal(size=(P, 3, 3)) * 0.1), "rotation": q(rng.normal(size=(P, 4))),
            "opacity": q(rng.normal(size=(P, 1)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("-P", type=int, default=2000)
    a = ap.parse_args()
    if not os.path.isdir(os.path.join(a.ref, "model")):
        sys.exit(f"{a.ref} is not a checkout of the reference")
    sys.modules.setdefault("plyfile", types.SimpleNamespace(PlyData=None, PlyElement=None))
    sys.path.insert(0, a.ref)
    sys.path.insert(1, ROOT)                                          # simple_knn._C of this repository (import only)
    _zeros, _cuda, _empty_like = torch.zeros, torch.Tensor.cuda, torch.empty_like

    def zeros_cpu(*args, **kw):
        kw.pop("device", None)
        return _zeros(*args, **kw)
    torch.zeros = zeros_cpu
    torch.Tensor.cuda = lambda self, *a_, **k_: self
    torch.empty_like = lambda t, *a_, **k_: torch.full_like(t, float("nan"))
    try:
        from model.box_sort import GaussianHandler, flattenGaussians
        from scene.gaussian_model import GaussianModel
        inp = make_inputs(a.P, 20261017)

        def model():
            g = GaussianModel(1)
            g.active_sh_degree = 1
            for name, arr in inp.items():
                setattr(g, "_" + name, torch.tensor(arr))
            return g
        out = {k: v for k, v in inp.items()}
        g = model()
        h = GaussianHandler(g, 10)
        out["world_min"], out["world_max"] = h.worldMin.numpy(), h.worldMax.numpy()
        out["scaling_min"], out["scaling_max"] = np.float32(h.scalingMin.item()), np.float32(h.scalingMax.item())
        out["rows"] = flattenGaussians(h.normalize(model())).numpy()          # the normalised rows the sort sees
        for n in (10, 40):
            res = GaussianHandler(model(), n).box_sort(model()).numpy()
            written = ~np.isnan(res).any(axis=1)
            last = int(written.sum())
            assert written[:last].all(), "the rows box_sort wrote are not a prefix"
            out[f"sorted_{n}"], out[f"last_{n}"] = res[:last], np.int32(last)
            print(f"n={n}: last={last} of P={a.P}")
    finally:
        torch.zeros, torch.Tensor.cuda, torch.empty_like = _zeros, _cuda, _empty_like
    path = os.path.join(a.out, "box_sort.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
