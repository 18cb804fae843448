"""-m gpu: the optimisation loop of tests/test_gpu_training.py (scripts/train_synthetic.py, same sizes, same four assertions) with
adam="hip_sparse": every step takes the view's radii as visibility, so the Gaussians outside the view stand still instead of coasting on
their momentum.  The dense run's figures are printed beside the sparse run's (-s)."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu


def test_training_loop_with_density_control_and_the_sparse_optimiser():
    path = os.path.join(os.path.dirname(__file__), "..", "scripts", "train_synthetic.py")
    spec = importlib.util.spec_from_file_location("train_synthetic", path)
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    sizes = dict(iters=240, P=6000, size=160, ncam=4, densify_from=60, densify_every=60)
    dense = mod.run(**sizes)
    out = mod.run(**sizes, adam="hip_sparse")
    for o in (dense, out):
        print("SPARSE_TRAINING", o["adam"], {k: o[k] for k in ("psnr_first", "psnr", "loss_first", "loss_last", "P_start", "P_end", "it_per_s")})
    assert out["adam"] == "hip_sparse" and dense["adam"] == "hip"
    assert out["loss_last"] < 0.75 * out["loss_first"], (out, dense["loss_last"])        # mean loss over all cameras, before / after
    assert out["psnr"] > out["psnr_first"] + 2.0, (out, dense["psnr"])
    assert out["P_end"] != out["P_start"], out
    assert any(h["event"] and (h["event"]["cloned"] + h["event"]["split"] + h["event"]["pruned"]) > 0 for h in out["history"]), out
