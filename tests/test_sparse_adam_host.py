"""CPU tests of the visibility-masked Adam step (include/gsr_optim.h: gsr_adam_step_masked; optim.HipSparseAdam): the two restatements of
tests/sparse_adam_ref.py pinned against each other and against the dense float64 oracle, the semantics in the small (a row that is
never visible, a row first seen late), the binding, and everything the entry point refuses on the host before it enqueues anything."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib
from oracle import aux_ref
from tests import aux_inputs
from tests.sparse_adam_ref import SparseAdam64, TorchMaskedAdam, fresh_masks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = [3, 3, 45, 1, 3, 4]                      # the reference's six groups at M = 16
LRS = [0.00016, 0.0025, 0.000125, 0.05, 0.005, 0.001]
HYPER = dict(betas=(0.9, 0.999), eps=1e-15)


def inputs(P, seed=0):
    lens = [P * w for w in WIDTHS]
    return lens, [p.reshape(P, w) for p, w in zip(aux_inputs.adam_params(lens, seed=seed), WIDTHS)]


@pytest.mark.parametrize("P", [1, 37, 200])
def test_the_two_restatements_agree_in_float64(P):
    steps = 6
    lens, p0 = inputs(P)
    masks = fresh_masks(P, steps, seed=3, late=(1, 4))
    ref = [SparseAdam64(p) for p in p0]
    tor = TorchMaskedAdam(p0, [dict(lr=lr, **HYPER) for lr in LRS], dtype=torch.float64)
    for t in range(steps):
        gs = [g.reshape(P, w) for g, w in zip(aux_inputs.adam_grads(lens, t, seed=2), WIDTHS)]
        for r, g, lr in zip(ref, gs, LRS):
            r.update(g, masks[t], lr, **HYPER)
        tor.step(gs, masks[t])
    for i, r in enumerate(ref):
        st = tor.state(i)
        assert int(st["step"]) == r.step == steps
        for name, a, b in (("param", tor.params[i].detach(), r.p), ("exp_avg", st["exp_avg"], r.m), ("exp_avg_sq", st["exp_avg_sq"], r.v)):
            scale = max(np.abs(b).max(), 1e-300)
            assert np.abs(a.numpy() - b).max() <= 1e-12 * scale, (i, name)


def test_all_ones_mask_is_dense_adam():
    P, steps = 53, 5
    lens, p0 = inputs(P, seed=4)
    sparse = [SparseAdam64(p) for p in p0]
    dense = [aux_ref.Adam64(p) for p in p0]
    ones = np.ones(P, dtype=bool)
    for t in range(steps):
        gs = [g.reshape(P, w) for g, w in zip(aux_inputs.adam_grads(lens, t, seed=6), WIDTHS)]
        for s, d, g, lr in zip(sparse, dense, gs, LRS):
            s.update(g, ones, lr, **HYPER)
            d.update(g, lr, **HYPER)
    for s, d in zip(sparse, dense):
        assert s.step == d.step == steps
        assert np.array_equal(s.p, d.p) and np.array_equal(s.m, d.m) and np.array_equal(s.v, d.v)


def test_rows_never_visible_stay_initial_and_a_late_row_gets_that_steps_bias_correction():
    P, w, steps, late = 10, 3, 6, 3                                    # 0-based step 3 = step count 4
    rng = np.random.default_rng(0)
    p0 = rng.standard_normal((P, w))
    masks = fresh_masks(P, steps, seed=1, late=(1, late))
    never, first_late = np.arange(P) % 5 == 0, np.arange(P) % 5 == 1
    assert not any(m[never].any() for m in masks) and not any(m[first_late].any() for m in masks[:late]) and masks[late][first_late].all()
    s = SparseAdam64(p0)
    t32 = TorchMaskedAdam([p0], [dict(lr=0.01, **HYPER)], dtype=torch.float32)
    gs = [rng.standard_normal((P, w)) for _ in range(steps)]
    for t in range(late + 1):
        s.update(gs[t], masks[t], 0.01, **HYPER)
        t32.step([gs[t]], masks[t])
    # seen for the first time at step count 4: m = (1 - b1) g, v = (1 - b2) g^2, corrected with 1 - b^4 -- not with 1 - b^1
    g = gs[late][first_late]
    b1, b2, eps = 0.9, 0.999, 1e-15
    m, v = (1 - b1) * g, (1 - b2) * g * g
    want = p0[first_late] - (0.01 / (1 - b1 ** 4)) * (m / (np.sqrt(v) / np.sqrt(1 - b2 ** 4) + eps))
    assert np.allclose(s.p[first_late], want, rtol=1e-13, atol=0)
    first_step = p0[first_late] - 0.01 * np.sign(g)                    # what a per-row counter would have given
    assert np.abs(s.p[first_late] - first_step).min() > 1e-3
    for t in range(late + 1, steps):
        s.update(gs[t], masks[t], 0.01, **HYPER)
        t32.step([gs[t]], masks[t])
    assert s.step == steps
    assert np.array_equal(s.p[never], p0[never]) and not s.m[never].any() and not s.v[never].any()
    st = t32.state(0)
    assert torch.equal(t32.params[0].detach()[torch.tensor(never)], torch.tensor(p0, dtype=torch.float32)[torch.tensor(never)])
    assert not st["exp_avg"][torch.tensor(never)].any() and not st["exp_avg_sq"][torch.tensor(never)].any()


def test_binding_and_header_name_the_entry_point():
    header = open(os.path.join(ROOT, "include", "gsr_optim.h")).read()
    m = re.search(r"int32_t\s+gsr_adam_step_masked\s*\(([^;]*)\)\s*;", header)
    assert m, "include/gsr_optim.h does not declare gsr_adam_step_masked"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    res, argtypes = _lib.SIGNATURES["gsr_adam_step_masked"]
    assert res is C.c_int32 and len(argtypes) == len(args.split(",")) == 9
    assert re.search(r"#define\s+GSR_ADAM_MASK_BYTES\s+0\b", header) and re.search(r"#define\s+GSR_ADAM_MASK_RADII\s+1\b", header)
    assert (_lib.ADAM_MASK_BYTES, _lib.ADAM_MASK_RADII) == (0, 1)
    assert hasattr(_lib.load(), "gsr_adam_step_masked")


def test_hip_sparse_adam_on_cpu_parameters_raises():
    from gaussian_transformer_amd.optim import HipAdam, HipSparseAdam
    assert issubclass(HipSparseAdam, HipAdam)
    p = torch.zeros(5, 3, requires_grad=True)
    p.grad = torch.ones(5, 3)
    opt = HipSparseAdam([p], lr=0.1)
    with pytest.raises(_lib.GsrError, match="HIP device"):
        opt.step()
    with pytest.raises(_lib.GsrError, match="HIP device"):
        opt.step(visibility=torch.ones(5, dtype=torch.bool))
    for bad in (torch.ones(5), torch.ones(5, dtype=torch.int64), torch.ones(5, 1, dtype=torch.bool), [True] * 5):
        with pytest.raises(_lib.GsrError, match="visibility"):
            opt.step(visibility=bad)
    assert torch.equal(p.detach(), torch.zeros(5, 3)) and len(opt.state[p]) == 0


def test_density_controller_takes_the_name_and_refuses_others():
    from gaussian_transformer_amd.densify import DensityController
    from gaussian_transformer_amd.optim import HipSparseAdam
    from tests import density_ref as dr
    from tests.test_density_host import make_controller
    ctl = make_controller(dr.clone_inputs(dr.build_inputs(5, 3)), cls=DensityController, adam="hip_sparse")
    assert type(ctl.optimizer) is HipSparseAdam and [g["name"] for g in ctl.optimizer.param_groups] == ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"]
    with pytest.raises(ValueError, match="hip_sparse"):
        make_controller(dr.clone_inputs(dr.build_inputs(5, 3)), cls=DensityController, adam="sparse")


# ---- what the entry point refuses: all of it is decided on the host, before anything is enqueued, so no device is needed ----
def _call(n_groups, groups, P, mask, kind, betas=(0.9, 0.999)):
    lib = _lib.load()
    arr = (_lib.AdamGroup * max(1, len(groups)))(*groups)
    rc = lib.gsr_adam_step_masked(None, n_groups, arr if groups else None, betas[0], betas[1], 1e-8, P, mask, kind)
    return rc, ((lib.gsr_last_error() or b"").decode() if rc else "")


def test_refusals_of_the_c_entry_point():
    G = _lib.AdamGroup
    ok = G(64, 64, 64, 64, 12, 0.1, 1)                                 # never dereferenced: every call below is refused
    cases = {
        "0 groups": (0, [ok], 4, 64, 0), "17 groups": (_lib.ADAM_MAX_GROUPS + 1, [ok] * (_lib.ADAM_MAX_GROUPS + 1), 4, 64, 0),
        "no group array": (1, [], 4, 64, 0), "P < 0": (1, [ok], -1, 64, 0), "NULL mask": (1, [ok], 4, None, 0),
        "kind 2": (1, [ok], 4, 64, 2), "kind -1": (1, [ok], 4, 64, -1), "int32 mask off 4 bytes": (1, [ok], 4, 66, 1),
        "n no multiple of P": (1, [ok], 5, 64, 0), "n > 0 with P = 0": (1, [ok], 0, None, 0),
        "n = 2^31": (1, [G(64, 64, 64, 64, 2 ** 31, 0.1, 1)], 1, 64, 0), "n < 0": (1, [G(64, 64, 64, 64, -4, 0.1, 1)], 4, 64, 0),
        "second group bad": (2, [ok, G(64, 64, 64, 64, 13, 0.1, 1)], 4, 64, 0), "step 0": (1, [G(64, 64, 64, 64, 12, 0.1, 0)], 4, 64, 0),
    }
    for which in range(4):
        ptrs = [64, 64, 64, 64]
        ptrs[which] = None
        cases[f"NULL pointer {which}"] = (1, [G(*ptrs, 12, 0.1, 1)], 4, 64, 0)
    for name, args in cases.items():
        rc, text = _call(*args)
        assert rc == 1 and text.startswith("gsr_adam_step_masked"), (name, rc, text)      # GSR_ERR_INVALID_ARGUMENT
    assert _call(1, [ok], 4, 64, 0, betas=(1.0, 0.999))[0] == 1
    # legal and empty: P = 0, groups with n = 0 (their pointers may be NULL), a byte mask at an odd address with nothing to do
    assert _call(1, [G(None, None, None, None, 0, 0.1, 1)], 0, None, 0) == (0, "")
    assert _call(2, [G(None, None, None, None, 0, 0.1, 1), G(64, 64, 64, 64, 0, 0.1, 3)], 7, 65, 0) == (0, "")
    assert _call(1, [G(None, None, None, None, 0, 0.1, 1)], 7, 64, 1) == (0, "")
