"""CPU tests of the device density control's contract (include/gsr_density.h): the one-pass rule the kernels implement
(tests/density_ref.py) equals DensityController -- the restatement of the reference's GaussianModel -- bit for bit, three
planted faults are told from it, the header and the ctypes table agree, and there is no CPU fallback."""
import os
import re

import pytest
import torch

from gaussian_transformer_amd import _lib
from gaussian_transformer_amd.densify import GROUPS, DensityController, OptimizationParams
from gaussian_transformer_amd.model import GaussianParams
from tests import density_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
        "rotation": "_rotation"}
STEP = 3.0


def make_controller(d, cls=DensityController, moments=True, **kw):
    """A controller over the (cloned) inputs d, its optimiser state and statistics set from them."""
    m = GaussianParams(3)
    for k in GROUPS:
        setattr(m, ATTR[k], d["par"][k].requires_grad_(True))
    ctl = cls(m, OptimizationParams(), **kw)
    if moments:
        for g in ctl.optimizer.param_groups:
            a, b = d["mom"][g["name"]]
            ctl.optimizer.state[g["params"][0]] = {"step": torch.tensor(STEP), "exp_avg": a, "exp_avg_sq": b}
    m.xyz_gradient_accum, m.denom, m.max_radii2D = d["accum"], d["denom"], d["max_radii"]
    return ctl


def torch_path(d, mss, seed=5):
    ctl = make_controller(dr.clone_inputs(d))
    with torch.no_grad():
        counts = ctl.densify_and_prune(dr.THRESHOLD, dr.MIN_OPACITY, dr.EXTENT, mss, generator=torch.Generator().manual_seed(seed))
    return ctl, counts


def rule(d, mss, seed=5, fault=None):
    c = dr.clone_inputs(d)
    gen = torch.Generator().manual_seed(seed)
    noise_fn = lambda rows: torch.normal(mean=torch.zeros(rows, 3), std=torch.ones(rows, 3), generator=gen)
    return dr.one_pass(c["par"], c["mom"], c["accum"], c["denom"], noise_fn, mss, max_radii=c["max_radii"], fault=fault)


def same_state(ctl, counts, new, mom, want_counts):
    if counts != want_counts:
        return False
    for g in ctl.optimizer.param_groups:
        n, p = g["name"], g["params"][0]
        st = ctl.optimizer.state[p]
        if p.shape != new[n].shape or not (torch.equal(p.detach(), new[n]) and torch.equal(st["exp_avg"], mom[n][0]) and
                                           torch.equal(st["exp_avg_sq"], mom[n][1])):
            return False
    return True


@pytest.mark.parametrize("mss", [None, 20])
@pytest.mark.parametrize("rest", [0, 3, 15])
@pytest.mark.parametrize("P", [1, 65, 257, 5000])
def test_one_pass_rule_equals_the_density_controller(P, rest, mss):
    d = dr.build_inputs(P, rest)
    ctl, counts = torch_path(d, mss)
    new, mom, want, P_new, _ = rule(d, mss)
    assert counts == want
    if P >= 257:
        assert counts["cloned"] > 0 and counts["split"] > 1 and counts["pruned"] > 0
    for g in ctl.optimizer.param_groups:
        n, p = g["name"], g["params"][0]
        st = ctl.optimizer.state[p]
        assert p.shape == new[n].shape and p.shape[0] == P_new, n
        assert torch.equal(p.detach(), new[n]), n
        assert torch.equal(st["exp_avg"], mom[n][0]) and torch.equal(st["exp_avg_sq"], mom[n][1]), n
        assert float(st["step"]) == STEP
    m = ctl.model
    for t, shape in ((m.xyz_gradient_accum, (P_new, 1)), (m.denom, (P_new, 1)), (m.max_radii2D, (P_new,))):
        assert tuple(t.shape) == shape and not t.any()


def test_planted_rows_decide_as_torch_does():
    d = dr.build_inputs(257, 3)
    c = dr.clone_inputs(d)
    g = (c["accum"] / c["denom"]).reshape(-1)
    assert g[d["planted"]["exact"]] == dr.f32(dr.THRESHOLD) and g[d["planted"]["nan"]].isnan() and g[d["planted"]["inf"]].isinf()
    g[g.isnan()] = 0.0
    hot = g >= dr.THRESHOLD
    assert hot[d["planted"]["exact"]] and hot[d["planted"]["inf"]] and not hot[d["planted"]["nan"]]


@pytest.mark.parametrize("fault", dr.FAULTS)
def test_planted_faults_are_rejected(fault):
    d = dr.build_inputs(257, 3)
    ctl, counts = torch_path(d, 20)
    new, mom, want, _, _ = rule(d, 20)
    assert same_state(ctl, counts, new, mom, want)
    new, mom, want, _, _ = rule(d, 20, fault=fault)
    assert not same_state(ctl, counts, new, mom, want)


def test_header_declares_exactly_what_the_ctypes_stub_binds():
    header = open(os.path.join(ROOT, "include", "gsr_density.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decls = dict(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", code, flags=re.S))
    assert set(decls) == {"gsr_density_record", "gsr_densify_plan_workspace", "gsr_densify_plan", "gsr_densify_apply"}
    assert set(_lib.DENSITY_SIGNATURES) == set(decls)
    for name, args in decls.items():
        assert len(_lib.DENSITY_SIGNATURES[name][1]) == len(args.split(",")), name
    assert not set(_lib.DENSITY_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.CHAMFER_SIGNATURES) | set(_lib.SEQUENCE_SIGNATURES))
    fields = re.search(r"typedef struct \{(.*?)\} gsr_density_group_t;", code, flags=re.S).group(1)
    assert [f.split()[-1].lstrip("*") for f in fields.split(";") if f.strip()] == [n for n, _ in _lib.DensityGroup._fields_]
    assert f"#define GSR_DENSITY_MAX_GROUPS {_lib.DENSITY_MAX_GROUPS}" in header
    assert "#define GSR_ABI_VERSION 2" in open(os.path.join(ROOT, "include", "gsr.h")).read()   # purely additive
    assert "screen-size test is not part of the plan" in header.lower()                         # the quirk is documented
    from gaussian_transformer_amd import build
    assert build.SOURCES["density.hip"] == build.SOURCES["preprocess.hip"]                       # no contraction, as the other per-Gaussian units
    lib = _lib.load()
    for name in decls:
        assert hasattr(lib, name)


@pytest.mark.parametrize("change", ["prune_points", "append_points", "replace_tensor", "relocate", "grow"])
def test_every_change_of_the_set_leaves_optimiser_model_and_statistics_consistent(change):
    """After one torch.optim.Adam step on P = 65, whichever method changes the set: optimizer.state holds exactly the six installed
    parameters, each the very object in its group and on the model, with moments of its shape; the statistics have P rows."""
    from gaussian_transformer_amd.densify import MCMCController
    from tests import mcmc_ref as mr
    mcmc = change in ("relocate", "grow")
    d = mr.clone_inputs(mr.build_inputs(65, 3)) if mcmc else dr.clone_inputs(dr.build_inputs(65, 3))
    ctl = mr.make_controller(d, MCMCController, moments=False) if mcmc else make_controller(d, moments=False)
    for g in ctl.optimizer.param_groups:
        g["params"][0].grad = torch.ones_like(g["params"][0])
    ctl.optimizer.step()
    assert len(ctl.optimizer.state) == 6
    with torch.no_grad():
        if change == "prune_points":
            ctl.prune_points(torch.arange(65) % 3 == 0)
        elif change == "append_points":
            ctl.append_points({n: getattr(ctl.model, ATTR[n]).detach()[:7] for n in GROUPS})
        elif change == "replace_tensor":
            ctl.replace_tensor("opacity", torch.zeros(65, 1))
        elif change == "relocate":
            ctl.relocate(u=mr.uniforms(65))
            assert ctl.counts("relocate")["n_sources"] > 0
        else:
            assert ctl.grow(u=mr.uniforms(3)) == 68
    P = {"prune_points": 43, "append_points": 72, "replace_tensor": 65, "relocate": 65, "grow": 68}[change]
    state = ctl.optimizer.state
    assert len(state) == 6
    for g in ctl.optimizer.param_groups:
        p = g["params"][0]
        assert len(g["params"]) == 1 and p is getattr(ctl.model, ATTR[g["name"]]) and any(k is p for k in state), g["name"]
        assert isinstance(p, torch.nn.Parameter) and p.shape[0] == P
        assert state[p]["exp_avg"].shape == p.shape and state[p]["exp_avg_sq"].shape == p.shape, g["name"]
    m = ctl.model
    assert tuple(m.xyz_gradient_accum.shape) == (P, 1) and tuple(m.denom.shape) == (P, 1) and tuple(m.max_radii2D.shape) == (P,)


def test_fused_controller_has_no_cpu_fallback():
    from gaussian_transformer_amd.densify import FusedDensityController
    ctl = make_controller(dr.clone_inputs(dr.build_inputs(65, 3)), cls=FusedDensityController)
    assert isinstance(ctl, DensityController)
    with torch.no_grad():
        with pytest.raises(_lib.GsrError, match="no CPU fallback"):
            ctl.densify_and_prune(dr.THRESHOLD, dr.MIN_OPACITY, dr.EXTENT, 20)
        vs = torch.zeros(65, 3)
        vs.grad = torch.ones(65, 3)
        with pytest.raises(_lib.GsrError, match="no CPU fallback"):
            ctl.record(vs, torch.ones(65, dtype=torch.bool), torch.ones(65, dtype=torch.int32))
    assert ctl.model._xyz.shape[0] == 65                                                        # nothing was changed
