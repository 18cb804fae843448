"""CPU tests of MCMC density control's contract (include/gsr_mcmc.h): densify.MCMCController -- the torch restatement, the oracle
of the HIP path -- against tests/mcmc_ref.py (Python integers and 50-digit decimals): indices, counts and every copied row bit for
bit, the corrected opacity and scaling within one float32 ulp of the exact value, moments; the properties of the correction; the
generator's consumption; the header against the ctypes table; and the refusals of the C entry points that need no device
(in the manner of tests/test_cabi_refusals_host.py: every pointer is a made-up address that is only compared)."""
import ctypes as C
import os
import re
from decimal import Decimal

import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib
from gaussian_transformer_amd.densify import GROUPS, DensityController, FusedMCMCController, MCMCController, MCMCParams
from tests import mcmc_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def relocated(P, rest, mode, moments=True, **kw):
    d = mr.build_inputs(P, rest, mode=mode)
    ctl = mr.make_controller(mr.clone_inputs(d), MCMCController, moments=moments, **kw)
    with torch.no_grad():
        ctl.relocate(u=mr.uniforms(P))
    return d, ctl


@pytest.mark.parametrize("rest", [0, 3, 15])
@pytest.mark.parametrize("P", [1, 65, 257, 5000])
def test_relocation_equals_the_reference(P, rest):
    d, ctl = relocated(P, rest, "mixed")
    ref = mr.cached_reference(P, rest, "mixed")
    assert ctl.counts("relocate") == ref["counts"]
    dead, src, c, total = mr.make_controller(mr.clone_inputs(d), MCMCController)._draws(mr.uniforms(P), None)
    assert np.array_equal(dead.numpy(), ref["dead"]) and total == ref["total"]
    if total:
        assert src.tolist() == ref["src"] and np.array_equal(c.numpy(), ref["hist"])
    if P >= 257:
        assert ref["counts"]["n_dead"] > 1 and ref["counts"]["n_sources"] > 1 and (ref["hist"] > 1).any()
    par, mom, step = mr.state_of(ctl)
    worst = mr.assert_state(par, mom, d, ref, "relocate")
    print(f"relocate P={P} rest={rest}: largest error of MCMCController on the CPU {worst:.3f} float32 ulp")
    assert all(s == mr.STEP for s in step.values())


@pytest.mark.parametrize("mode", ["none", "all"])
def test_nothing_to_relocate_changes_nothing(mode):
    d, ctl = relocated(257, 3, mode)
    ref = mr.cached_reference(257, 3, mode)
    assert ctl.counts("relocate") == ref["counts"] and ref["counts"]["n_draws"] == 0
    par, mom, _ = mr.state_of(ctl)
    for n in GROUPS:
        assert torch.equal(par[n].detach(), d["par"][n]) and torch.equal(mom[n][0], d["mom"][n][0]) and torch.equal(mom[n][1], d["mom"][n][1])


def test_one_alive_row_reaches_the_clamp_of_51():
    d, ctl = relocated(257, 3, "one_alive")
    ref = mr.cached_reference(257, 3, "one_alive")
    assert ref["counts"] == {"n_dead": 256, "n_draws": 256, "n_sources": 1, "P_new": 257} and ref["N"].tolist() == [51]
    assert ctl.counts("relocate") == ref["counts"]
    par, mom, _ = mr.state_of(ctl)
    mr.assert_state(par, mom, d, ref, "one_alive")
    assert torch.equal(par["xyz"].detach(), d["par"]["xyz"][128].expand(257, 3))


def test_sources_with_N_1_are_unchanged():
    d, ctl = relocated(257, 3, "mixed", n_max=1)
    ref = mr.reference(d, mr.uniforms(257), n_max=1)
    assert (ref["N"] == 1).all() and len(ref["sources"]) > 1
    par, mom, _ = mr.state_of(ctl)
    mr.assert_state(par, mom, d, ref, "n_max=1")
    for n in ("opacity", "scaling"):
        assert torch.equal(par[n].detach()[ref["sources"]], d["par"][n][ref["sources"]]), n


def test_corrected_opacity_composites_back_to_the_original():
    """1 - (1 - sigmoid(opacity_new))^N = o wherever the clamp did not act: N copies at the new opacity cover what one did."""
    d, ctl = relocated(5000, 0, "mixed")
    ref = mr.cached_reference(5000, 0, "mixed")
    par, _, _ = mr.state_of(ctl)
    new = torch.sigmoid(par["opacity"].detach().double().reshape(-1)[ref["sources"]]).numpy()
    back = 1.0 - (1.0 - new) ** ref["N"]
    free = ~ref["clamped"]
    assert free.sum() > 100 and ref["clamped"].any()
    assert np.abs(back - ref["o"])[free].max() <= 1e-6


def test_D_is_positive_on_a_grid():
    for N in (1, 2, 3, 7, 20, 50, 51):
        for x in ("1e-9", "1e-4", "0.01", "0.1", "0.25", "0.5", "0.75", "0.9", "0.999", "1"):
            assert mr.D_exact(Decimal(x), N) > 0, (N, x)
    assert mr.D_exact(Decimal("0.3"), 1) == Decimal("0.3")
    # the header's single sum is the same number
    N, x = 9, Decimal("0.37")
    single = sum(mr.math.comb(N, k + 1) * (-1) ** k * x ** (k + 1) / Decimal(k + 1).sqrt() for k in range(N))
    assert abs(single - mr.D_exact(x, N)) < Decimal("1e-40")


@pytest.mark.parametrize("moments", [True, False])
@pytest.mark.parametrize("P,rest", [(1, 3), (65, 0), (257, 15), (5000, 3)])
def test_growth_equals_the_reference(P, rest, moments):
    d = mr.build_inputs(P, rest, mode="mixed")
    ctl = mr.make_controller(mr.clone_inputs(d), MCMCController, cap_max=10 ** 9, moments=moments)
    n = (P * 105) // 100 - P
    with torch.no_grad():
        P_new = ctl.grow(u=mr.uniforms(n) if n else None)
    assert P_new == P + n == ctl.model._xyz.shape[0]
    if n == 0:
        assert ctl.counts("grow")["P_new"] == P
        return
    ref = mr.cached_reference(P, rest, "mixed", grow_n=n)
    assert ctl.counts("grow") == ref["counts"]
    par, mom, _ = mr.state_of(ctl)
    assert (mom is None) == (not moments)
    mr.assert_state(par, mom, d, ref, "grow")
    for name in GROUPS:
        p = par[name]
        assert isinstance(p, torch.nn.Parameter) and p.is_leaf and p.requires_grad and p is getattr(ctl.model, mr.ATTR[name])


def test_growth_stops_at_the_cap_and_all_dead_growth_appends_plain_copies():
    d = mr.build_inputs(257, 3, mode="mixed")
    ctl = mr.make_controller(mr.clone_inputs(d), MCMCController, cap_max=260)
    with torch.no_grad():
        assert ctl.grow(u=mr.uniforms(3)) == 260 and ctl.grow() == 260      # (257 * 105) / 100 = 269 > cap; then at the cap: a no-op
    before = {n: p.detach().clone() for n, p in mr.state_of(ctl)[0].items()}
    gen = torch.Generator().manual_seed(1)
    state = gen.get_state()
    with torch.no_grad():
        ctl.grow(generator=gen)
    assert torch.equal(gen.get_state(), state)                              # a no-op draws nothing
    assert all(torch.equal(before[n], p.detach()) for n, p in mr.state_of(ctl)[0].items())
    capped = mr.make_controller(mr.clone_inputs(d), MCMCController, cap_max=100)         # a cap below P never shrinks the set
    with torch.no_grad():
        assert capped.grow() == 257
    d0 = mr.build_inputs(65, 3, mode="all")
    dead = mr.make_controller(mr.clone_inputs(d0), MCMCController)
    with torch.no_grad():
        assert dead.grow(u=mr.uniforms(3)) == 68
    ref = mr.cached_reference(65, 3, "all", grow_n=3)
    assert ref["counts"] == {"n_dead": 65, "n_draws": 0, "n_sources": 0, "P_new": 68} == dead.counts("grow")
    par, mom, _ = mr.state_of(dead)
    mr.assert_state(par, mom, d0, ref, "all dead")


def test_generator_consumption_does_not_depend_on_the_number_of_dead_rows():
    nexts = []
    for mode in ("none", "mixed", "all"):
        ctl = mr.make_controller(mr.clone_inputs(mr.build_inputs(257, 3, mode=mode)), MCMCController)
        gen = torch.Generator().manual_seed(77)
        with torch.no_grad():
            ctl.relocate(generator=gen)
        nexts.append(torch.rand(4, generator=gen))
    assert torch.equal(nexts[0], nexts[1]) and torch.equal(nexts[0], nexts[2])
    want = torch.Generator().manual_seed(77)
    torch.rand(257, generator=want)
    assert torch.equal(torch.rand(4, generator=want), nexts[0])


def test_noise_and_regularisers_on_the_cpu_against_float64():
    P = 257
    d = mr.build_inputs(P, 0, mode="mixed")
    ctl = mr.make_controller(mr.clone_inputs(d), MCMCController, moments=False)
    ctl.update_learning_rate(0)
    noise = torch.randn(P, 3, generator=torch.Generator().manual_seed(4))
    want = mr_noise64(d["par"], noise, ctl.mcmc, np.float32(ctl.mcmc.noise_lr * ctl._xyz_lr_now()))
    ctl.add_noise(noise=noise)
    got = ctl.model._xyz.detach().double()
    assert (got - want).abs().max() <= 1e-4 * max(1.0, float((want - d["par"]["xyz"].double()).abs().max()))
    terms = ctl.regularize()
    op, sc = d["par"]["opacity"].double(), d["par"]["scaling"].double()
    assert abs(float(terms[0]) - 0.01 * float(torch.sigmoid(op).mean())) < 1e-8 and abs(float(terms[1]) - 0.01 * float(torch.exp(sc).mean())) < 1e-8
    s = torch.sigmoid(op)
    assert (ctl.model._opacity.grad.double() - 0.01 / P * s * (1 - s)).abs().max() < 1e-9
    assert (ctl.model._scaling.grad.double() - 0.01 / (3 * P) * torch.exp(sc)).abs().max() < 1e-9


def mr_noise64(par, noise, mc, scale):
    """xyz after the noise step, the header's formula in float64."""
    from gaussian_transformer_amd.densify import quaternion_to_rotation
    o = torch.sigmoid(par["opacity"].double())
    f = 1.0 / (1.0 + torch.exp(float(np.float32(mc.gate_k)) * (o - float(np.float32(mc.gate_t)))))
    R = quaternion_to_rotation(par["rotation"].double())
    S2 = torch.diag_embed(torch.exp(par["scaling"].double()) ** 2)
    cov = R @ S2 @ R.transpose(1, 2)
    return par["xyz"].double() + (cov @ noise.double()[:, :, None]).squeeze(-1) * f * float(scale)


def test_schedule_on_the_cpu():
    P = 257
    ctl = mr.make_controller(mr.clone_inputs(mr.build_inputs(P, 3, mode="mixed")), MCMCController, cap_max=300, moments=False,
                             refine_start=0, refine_every=5, refine_stop=12)
    assert isinstance(ctl, DensityController)
    gen = torch.Generator().manual_seed(3)
    sizes = []
    for it in range(1, 16):
        ctl.update_learning_rate(it)
        for g in ctl.optimizer.param_groups:
            g["params"][0].grad = torch.full_like(g["params"][0], 1e-3)
        with torch.no_grad():
            ctl.after_backward(it)
        ctl.optimizer.step()
        with torch.no_grad():
            ctl.after_step(it, generator=gen)
        sizes.append(ctl.model._xyz.shape[0])
    assert sizes[3] == 257 and sizes[4] == 269 and sizes[9] == 282 and sizes[-1] == 282      # grown at 5 and 10; 15 is past refine_stop
    assert max(sizes) <= 300 and ctl.model.denom.shape == (282, 1)


def test_header_declares_exactly_what_the_ctypes_stub_binds():
    header = open(os.path.join(ROOT, "include", "gsr_mcmc.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decls = dict(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", code, flags=re.S))
    assert set(decls) == {"gsr_mcmc_plan_workspace", "gsr_mcmc_plan", "gsr_mcmc_apply", "gsr_mcmc_noise", "gsr_mcmc_regularize_workspace",
                          "gsr_mcmc_regularize"}
    assert set(_lib.MCMC_SIGNATURES) == set(decls)
    for name, args in decls.items():
        assert len(_lib.MCMC_SIGNATURES[name][1]) == len(args.split(",")), name
    assert not set(_lib.MCMC_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.DENSITY_SIGNATURES))
    fields = re.search(r"typedef struct \{(.*?)\} gsr_mcmc_group_t;", code, flags=re.S).group(1)
    assert [f.split()[-1].lstrip("*") for f in fields.split(";") if f.strip()] == [n for n, _ in _lib.McmcGroup._fields_]
    assert f"#define GSR_MCMC_MAX_GROUPS {_lib.MCMC_MAX_GROUPS}" in header and f"#define GSR_MCMC_N_MAX {_lib.MCMC_N_MAX}" in header
    assert "deviation from the published code" in header.lower()
    from gaussian_transformer_amd import build
    assert build.SOURCES["mcmc.hip"] == build.SOURCES["density.hip"]
    lib = _lib.load()
    for name in decls:
        assert hasattr(lib, name)
    assert MCMCParams(cap_max=5) == MCMCParams(5, 0.005, 5e5, 500, 25_000, 100, 105, 0.01, 0.01, 51, 100.0, 0.005)


def test_fused_controller_has_no_cpu_fallback():
    ctl = mr.make_controller(mr.clone_inputs(mr.build_inputs(65, 3)), FusedMCMCController)
    assert isinstance(ctl, MCMCController)
    with torch.no_grad():
        for call in (ctl.relocate, ctl.grow, ctl.add_noise, ctl.regularize):
            with pytest.raises(_lib.GsrError, match="no CPU fallback"):
                call()
    assert ctl.model._xyz.shape[0] == 65


# ---- what the entry points refuse, and what they accept without launching ----
OK, INVALID = 0, 1
SENTINEL = "gsr_set_option: unknown option 'sentinel'"
BIG, A = 1 << 40, 1 << 20


def groups(n, **kw):
    g = dict(src=A, sm=None, sv=None, dst=A, dm=None, dv=None, width=3, role=_lib.MCMC_COPY)
    g.update(kw)
    one = _lib.McmcGroup(g["src"], g["sm"], g["sv"], g["dst"], g["dm"], g["dv"], g["width"], g["role"])
    return (_lib.McmcGroup * n)(*([one] * n))


def plan(mode=0, P=10, n=0, m=0.005, n_max=51, opacity=A, u=3 * A, counts=4 * A, ws=5 * A):
    return lambda Lb: Lb.gsr_mcmc_plan(None, mode, P, opacity, 2 * A, mr.L, m, n_max, n, u, counts, ws, BIG)


def apply_(mode=0, P=10, n=0, k=1, g=None, ws=5 * A):
    return lambda Lb: Lb.gsr_mcmc_apply(None, mode, P, n, k, g, ws, BIG)


def noise(P=10, rot=3 * A, xyz=5 * A):
    return lambda Lb: Lb.gsr_mcmc_noise(None, P, A, 2 * A, rot, 4 * A, xyz, 100.0, 0.005, 80.0)


def reg(P=10, so=1, ss=3, means=5 * A, ws=6 * A, nbytes=BIG):
    return lambda Lb: Lb.gsr_mcmc_regularize(None, P, A, 2 * A, 3 * A, so, 4 * A, ss, 0.01, 0.01, means, ws, nbytes)


def size():
    return C.byref(C.c_size_t())


AP = "gsr_mcmc_apply: "
CASES = [
    (lambda Lb: Lb.gsr_mcmc_plan_workspace(10, 0, None), INVALID, "gsr_mcmc_plan_workspace: bytes is NULL"),
    (lambda Lb: Lb.gsr_mcmc_plan_workspace(-1, 0, size()), INVALID, "gsr_mcmc_plan_workspace: P=-1 is negative"),
    (lambda Lb: Lb.gsr_mcmc_plan_workspace(10, -2, size()), INVALID, "gsr_mcmc_plan_workspace: n_draws=-2 is negative"),
    (lambda Lb: Lb.gsr_mcmc_plan_workspace(1 << 30, 1 << 30, size()), INVALID, "gsr_mcmc_plan_workspace: P + n_draws = 2147483648, must stay below 2^31"),
    (plan(P=-3), INVALID, "gsr_mcmc_plan: P=-3 is negative"),
    (plan(mode=1, P=2 ** 31 - 1, n=1), INVALID, "gsr_mcmc_plan: P + n_draws = 2147483648, must stay below 2^31"),
    (plan(mode=2), INVALID, "gsr_mcmc_plan: unknown mode 2"),
    (plan(mode=0, n=4), INVALID, "gsr_mcmc_plan: n_draws=4 with relocation (it draws n_dead times; pass 0)"),
    (plan(counts=None), INVALID, "gsr_mcmc_plan: counts_host is NULL"),
    (plan(n_max=0), INVALID, "gsr_mcmc_plan: n_max=0 not in 1..51"),
    (plan(n_max=52), INVALID, "gsr_mcmc_plan: n_max=52 not in 1..51"),
    (plan(m=0.0), INVALID, "gsr_mcmc_plan: min_opacity=0, must lie in (0, 1)"),
    (plan(m=float("nan")), INVALID, "gsr_mcmc_plan: min_opacity=nan, must lie in (0, 1)"),
    (plan(opacity=None), INVALID, "gsr_mcmc_plan: null pointer"),
    (plan(u=None), INVALID, "gsr_mcmc_plan: null pointer"),
    (plan(ws=None), INVALID, "gsr_mcmc_plan: null pointer"),
    (apply_(P=-1), INVALID, AP + "P=-1 is negative"),
    (apply_(mode=7), INVALID, AP + "unknown mode 7"),
    (apply_(k=-1), INVALID, AP + "-1 groups (at most 16)"),
    (apply_(k=17, g=groups(17)), INVALID, AP + "17 groups (at most 16)"),
    (apply_(k=2, g=None), INVALID, AP + "2 groups (at most 16)"),
    (apply_(P=0, g=groups(1), ws=None), OK, SENTINEL),
    (apply_(g=groups(1), ws=None), INVALID, AP + "null pointer (ws)"),
    (apply_(g=groups(1, width=-1)), INVALID, AP + "group 0: width -1"),
    (apply_(mode=1, P=2 ** 30, n=2 ** 29, g=groups(1, dst=2 * A)), INVALID, AP + "group 0: (P + n_draws) * width must stay below 2^32"),
    (apply_(g=groups(1, src=None)), INVALID, AP + "group 0: src / dst NULL"),
    (apply_(g=groups(1, sm=2 * A)), INVALID, AP + "group 0: the four moment pointers must all be given or all be NULL"),
    (apply_(g=groups(1, dst=2 * A)), INVALID, AP + "group 0: relocation works in place (dst == src), growth into other buffers"),
    (apply_(mode=1, n=2, g=groups(1)), INVALID, AP + "group 0: relocation works in place (dst == src), growth into other buffers"),
    (apply_(g=groups(1, role=3)), INVALID, AP + "group 0: role 3"),
    (apply_(g=groups(1, role=_lib.MCMC_OPACITY)), INVALID, AP + "group 0: role 1 needs width 1, got 3"),
    (apply_(g=groups(1, role=_lib.MCMC_SCALING, width=1)), INVALID, AP + "group 0: role 2 needs width 3, got 1"),
    (noise(P=-1), INVALID, "gsr_mcmc_noise: P=-1 is negative"),
    (noise(P=0, rot=None, xyz=None), OK, SENTINEL),
    (noise(xyz=None), INVALID, "gsr_mcmc_noise: null pointer"),
    (noise(rot=3 * A + 4), INVALID, "gsr_mcmc_noise: rotation must be 16-byte aligned (a quaternion is one 16-byte load)"),
    (lambda Lb: Lb.gsr_mcmc_regularize_workspace(10, None), INVALID, "gsr_mcmc_regularize_workspace: bytes is NULL"),
    (lambda Lb: Lb.gsr_mcmc_regularize_workspace(-1, size()), INVALID, "gsr_mcmc_regularize_workspace: P=-1 is negative"),
    (reg(P=-1), INVALID, "gsr_mcmc_regularize: P=-1 is negative"),
    (reg(P=0, means=None, ws=None), OK, SENTINEL),
    (reg(so=0), INVALID, "gsr_mcmc_regularize: stride_o=0 stride_s=3, at least 1 and 3"),
    (reg(ss=2), INVALID, "gsr_mcmc_regularize: stride_o=1 stride_s=2, at least 1 and 3"),
    (reg(means=None), INVALID, "gsr_mcmc_regularize: null pointer"),
    (reg(means=5 * A + 4), INVALID, "gsr_mcmc_regularize: means_out must be 8-byte aligned"),
    (reg(P=257, nbytes=255), 4, "mcmc regularize workspace 255 < 256"),
]


@pytest.mark.parametrize("k", range(len(CASES)), ids=[f"{k:02d}-{'ok' if c[1] == OK else c[2][:44]}" for k, c in enumerate(CASES)])
def test_return_code_and_message(k):
    call, rc, text = CASES[k]
    lib = _lib.load()
    assert lib.gsr_set_option(b"sentinel", 0) == INVALID and lib.gsr_last_error().decode() == SENTINEL
    got = call(lib)
    assert (got, lib.gsr_last_error().decode()) == (rc, text)


def test_plan_of_nothing_writes_four_zeros_and_launches_nothing():
    lib = _lib.load()
    for mode in (_lib.MCMC_RELOCATE, _lib.MCMC_GROW):
        counts = (C.c_uint32 * 4)(7, 7, 7, 7)
        assert lib.gsr_set_option(b"sentinel", 0) == INVALID
        assert lib.gsr_mcmc_plan(None, mode, 0, None, None, mr.L, 0.005, 51, 0, None, counts, None, 0) == OK
        assert list(counts) == [0, 0, 0, 0] and lib.gsr_last_error().decode() == SENTINEL
    counts = (C.c_uint32 * 4)(7, 7, 7, 7)
    assert lib.gsr_mcmc_plan(None, _lib.MCMC_GROW, 0, None, None, mr.L, 0.005, 51, 3, None, counts, None, 0) == INVALID
    assert list(counts) == [7, 7, 7, 7] and lib.gsr_last_error().decode() == "gsr_mcmc_plan: n_draws=3 from an empty set"
    n = C.c_size_t(0)
    assert lib.gsr_mcmc_regularize_workspace(257, C.byref(n)) == OK and n.value == 256
    assert lib.gsr_mcmc_regularize_workspace(0, C.byref(n)) == OK and n.value == 256
