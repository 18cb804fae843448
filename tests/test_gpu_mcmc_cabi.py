"""-m gpu: a plain C program (tests/cabi/mcmc_client.c) drives gsr_mcmc_plan, gsr_mcmc_apply and gsr_mcmc_noise of libgsr_hip.so
directly at P = 65: the relocation against tests/mcmc_ref.py (counts and copies bit for bit, the corrected values within one float32
ulp), the noise against the float64 evaluation of the header's formula, and a few refusals."""
import numpy as np
import pytest
import torch

from gaussian_transformer_amd.densify import GROUPS, MCMCController
from tests import cabi_client as cc
from tests import mcmc_ref as mr
from tests.test_mcmc_host import mr_noise64

pytestmark = pytest.mark.gpu


def test_plain_c_client_mcmc(tmp_path):
    P, rest = 65, 3
    d = mr.build_inputs(P, rest, mode="mixed")
    u = mr.uniforms(P)
    noise = torch.randn(P, 3, generator=torch.Generator().manual_seed(8))
    gate_k, gate_t, scale = np.float32(100.0), np.float32(0.005), np.float32(5e5 * 0.00016)
    prob, res = tmp_path / "problem.bin", tmp_path / "result.bin"
    widths = [d["par"][n][0].numel() for n in GROUPS]
    with open(prob, "wb") as f:
        f.write(np.asarray([P] + widths, dtype=np.int32).tobytes())
        f.write(np.float32(mr.L).tobytes() + np.float64(mr.MIN_OPACITY).tobytes() + np.asarray([gate_k, gate_t, scale], dtype=np.float32).tobytes())
        f.write(u.numpy().tobytes() + noise.numpy().tobytes())
        for n in GROUPS:
            for t in (d["par"][n], d["mom"][n][0], d["mom"][n][1]):
                f.write(np.ascontiguousarray(t.numpy()).tobytes())
    cc.run(cc.build(tmp_path, "mcmc_client"), prob, res)
    got = cc.read_result(res, [("counts", np.uint32, 4)] + [((n, k), np.float32, tuple(d["par"][n].shape)) for n in GROUPS for k in range(3)] +
                         [("xyz_after", np.float32, (P, 3))])
    counts = got["counts"]
    t = lambda key: torch.from_numpy(got[key].copy())
    par, mom = {n: t((n, 0)) for n in GROUPS}, {n: (t((n, 1)), t((n, 2))) for n in GROUPS}
    xyz_after = t("xyz_after")
    ref = mr.cached_reference(P, rest, "mixed")
    assert dict(zip(("n_dead", "n_draws", "n_sources", "P_new"), (int(v) for v in counts))) == ref["counts"] and ref["counts"]["n_sources"] > 1
    worst = mr.assert_state(par, mom, d, ref, "C client")
    print(f"C client relocation: largest error {worst:.3f} float32 ulp")
    # the noise, on the relocated parameters
    ctl = mr.make_controller({"par": {k: v.clone() for k, v in par.items()}, "mom": mom}, MCMCController, moments=False)
    want = mr_noise64(par, noise, ctl.mcmc, scale)
    for g in ctl.optimizer.param_groups:
        if g["name"] == "xyz":
            g["lr"] = 0.00016
    ctl.add_noise(noise=noise)
    torch_err = float((ctl.model._xyz.detach().double() - want).abs().max())
    err = float((xyz_after.double() - want).abs().max())
    print(f"C client noise: torch f32 err {torch_err:.3e} hip err {err:.3e}")
    assert err <= 2 * torch_err + 1e-7
