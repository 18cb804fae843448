"""-m gpu: MCMC density control on the device (include/gsr_mcmc.h, densify.FusedMCMCController) against MCMCController on the same
device, the same inputs and the same uniforms / normals, and both against tests/mcmc_ref.py (integers and 50-digit decimals).

Shapes: P = 1 (one lane), 63 / 64 / 65 (the wave edge), 257 (the group edge, odd, so no group's rows stay 16-byte aligned),
5000 (several scan blocks); f_rest widths 0, 3, 15 (rows of 0, 9 and 45 floats beside widths 1, 3 and 4).

Bars.  Corrected opacity / scaling: |value - exact| <= 1 float32 ulp of |exact| for both controllers (correct rounding gives 0.5, the
float64 evaluation adds about 5e-13 relative); the largest error of both is printed.  Noise and regulariser gradients (per tensor):
twice the largest error the torch float32 evaluation of the same formula shows against float64 on the same inputs, plus 1e-7; both
figures are printed.  Everything else is equality.  Measured on an MI355X: corrected values at most 0.500 ulp
for both controllers; noise 3e-6 - 6.6e-6 against torch's 1.1e-5 - 8.3e-5 (the kernel evaluates it in float64 and rounds once; a
plain float32 kernel was off by 6.5e-5 at P = 64 where torch's CPU evaluation happened to be off by 1.1e-5, and missed the bar).
"""
import functools

import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib
from gaussian_transformer_amd.densify import GROUPS, FusedMCMCController, MCMCController
from tests import mcmc_ref as mr
from tests.test_mcmc_host import mr_noise64

pytestmark = pytest.mark.gpu
DEV = "cuda"
PS = [1, 63, 64, 65, 257, 5000]
RESTS = [0, 3, 15]


def controllers(d, **kw):
    return [mr.make_controller(mr.clone_inputs(d, DEV), cls, **kw) for cls in (MCMCController, FusedMCMCController)]


def dev_u(n):
    return mr.uniforms(n).to(DEV)


def assert_pair_equal(a, b, skip=("opacity", "scaling")):
    """The two controllers' states: plain-copy groups and every moment bit-equal; opacity and scaling where they are not corrected."""
    (pa, ma, sa), (pb, mb, sb) = mr.state_of(a), mr.state_of(b)
    assert sa == sb and (ma is None) == (mb is None)
    for n in GROUPS:
        assert pa[n].shape == pb[n].shape, n
        if n not in skip:
            assert torch.equal(pa[n].detach(), pb[n].detach()), n
        if ma is not None:
            assert torch.equal(ma[n][0], mb[n][0]) and torch.equal(ma[n][1], mb[n][1]), n


def check_both(a, b, d, ref, label):
    worst = []
    for ctl in (a, b):
        par, mom, _ = mr.state_of(ctl)
        worst.append(mr.assert_state(par, mom, d, ref, label))
    print(f"{label}: largest error of a corrected value, MCMCController {worst[0]:.3f} ulp, FusedMCMCController {worst[1]:.3f} ulp")
    assert_pair_equal(a, b)


def step_once(ctl):
    for g in ctl.optimizer.param_groups:
        g["params"][0].grad = torch.full_like(g["params"][0], 0.5)
        g["lr"] = 1e-3
    ctl.optimizer.step()


@pytest.mark.parametrize("rest", RESTS)
@pytest.mark.parametrize("P", PS)
def test_relocation(P, rest):
    d = mr.build_inputs(P, rest, mode="mixed")
    ref = mr.cached_reference(P, rest, "mixed")
    a, b = controllers(d)
    with torch.no_grad():
        a.relocate(u=dev_u(P)); b.relocate(u=dev_u(P))
    assert a.counts("relocate") == b.counts("relocate") == ref["counts"]
    if P >= 257:
        assert ref["counts"]["n_dead"] > 1 and ref["counts"]["n_sources"] > 1 and (ref["hist"] > 1).any()
    check_both(a, b, d, ref, f"relocate P={P} rest={rest}")
    for n in GROUPS:                                        # in place: the installed parameters are the ones the model had
        assert mr.state_of(b)[0][n] is getattr(b.model, mr.ATTR[n])
    before = b.model._xyz.detach().clone()
    step_once(b)
    assert not torch.equal(before, b.model._xyz.detach()) and all(s == mr.STEP + 1 for s in mr.state_of(b)[2].values())


@pytest.mark.parametrize("mode", ["none", "all"])
@pytest.mark.parametrize("P", [1, 257])
def test_nothing_to_relocate_changes_nothing(mode, P):
    d = mr.build_inputs(P, 3, mode=mode)
    _, b = controllers(d)
    with torch.no_grad():
        b.relocate(u=dev_u(P))
    assert b.counts("relocate") == mr.cached_reference(P, 3, mode)["counts"]
    par, mom, _ = mr.state_of(b)
    for n in GROUPS:
        assert torch.equal(par[n].detach().cpu(), d["par"][n]) and torch.equal(mom[n][0].cpu(), d["mom"][n][0]) and torch.equal(mom[n][1].cpu(), d["mom"][n][1])


def test_one_alive_row_reaches_the_clamp_of_51():
    d = mr.build_inputs(257, 3, mode="one_alive")
    ref = mr.cached_reference(257, 3, "one_alive")
    assert ref["N"].tolist() == [51]
    a, b = controllers(d)
    with torch.no_grad():
        a.relocate(u=dev_u(257)); b.relocate(u=dev_u(257))
    assert b.counts("relocate") == ref["counts"] == {"n_dead": 256, "n_draws": 256, "n_sources": 1, "P_new": 257}
    check_both(a, b, d, ref, "one_alive")


def test_two_runs_are_bit_identical_and_n_max_1_changes_no_source():
    d = mr.build_inputs(5000, 15, mode="mixed")
    runs = []
    for _ in range(2):
        _, b = controllers(d)
        with torch.no_grad():
            b.relocate(u=dev_u(5000))
            b.grow(u=dev_u(250))
        runs.append(mr.state_of(b))
    for n in GROUPS:
        assert torch.equal(runs[0][0][n].detach(), runs[1][0][n].detach())
        assert torch.equal(runs[0][1][n][0], runs[1][1][n][0]) and torch.equal(runs[0][1][n][1], runs[1][1][n][1])
    d = mr.build_inputs(257, 3, mode="mixed")
    ref = mr.reference(d, mr.uniforms(257), n_max=1)
    _, b = controllers(d, n_max=1)
    with torch.no_grad():
        b.relocate(u=dev_u(257))
    par, mom, _ = mr.state_of(b)
    mr.assert_state(par, mom, d, ref, "n_max=1")
    for n in ("opacity", "scaling"):
        assert torch.equal(par[n].detach().cpu()[ref["sources"]], d["par"][n][ref["sources"]]), n


@pytest.mark.parametrize("adam", ["torch", "hip"])
@pytest.mark.parametrize("P", [65, 257])
def test_no_optimiser_state_yet_then_both_optimisers_step(P, adam):
    d = mr.build_inputs(P, 3, mode="mixed")
    ref = mr.cached_reference(P, 3, "mixed")
    a, b = controllers(d, moments=False, adam=adam)
    with torch.no_grad():
        a.relocate(u=dev_u(P)); b.relocate(u=dev_u(P))
    assert mr.state_of(b)[1] is None
    check_both(a, b, d, ref, f"no state P={P} {adam}")
    for ctl in (a, b):
        step_once(ctl)
    assert all(s == 1 for s in mr.state_of(b)[2].values())
    plain = np.nonzero(ref["hist"][ref["source_of"]] == 0)[0]
    for n in GROUPS:                                        # the first step after the surgery: identical on identical rows
        (pa, ma, _), (pb, mb, _) = mr.state_of(a), mr.state_of(b)
        assert torch.equal(pa[n].detach()[plain], pb[n].detach()[plain]) and torch.equal(ma[n][0], mb[n][0]), n
    u2 = torch.rand(P, generator=torch.Generator().manual_seed(9)).to(DEV)
    with torch.no_grad():                                   # and a second relocation with state present
        a.relocate(u=u2); b.relocate(u=u2)
    assert a.counts("relocate") == b.counts("relocate")
    assert_pair_equal(a, b)
    step_once(b)
    assert all(s == 2 for s in mr.state_of(b)[2].values())


@pytest.mark.parametrize("moments", [True, False])
@pytest.mark.parametrize("rest", RESTS)
@pytest.mark.parametrize("P", PS)
def test_growth(P, rest, moments):
    d = mr.build_inputs(P, rest, mode="mixed")
    n = (P * 105) // 100 - P
    a, b = controllers(d, moments=moments)
    with torch.no_grad():
        Pa, Pb = a.grow(u=dev_u(n) if n else None), b.grow(u=dev_u(n) if n else None)
    assert Pa == Pb == P + n == b.model._xyz.shape[0]
    assert b.model.denom.shape == (P + n, 1)
    if n == 0:
        assert b.counts("grow")["P_new"] == P
        return
    ref = mr.cached_reference(P, rest, "mixed", grow_n=n)
    assert a.counts("grow") == b.counts("grow") == ref["counts"]
    check_both(a, b, d, ref, f"grow P={P} rest={rest}")
    par, _, _ = mr.state_of(b)
    for name in GROUPS:
        p = par[name]
        assert isinstance(p, torch.nn.Parameter) and p.is_leaf and p.requires_grad and p is getattr(b.model, mr.ATTR[name])
    step_once(b)
    assert all(s == (mr.STEP + 1 if moments else 1) for s in mr.state_of(b)[2].values())


def test_growth_at_the_cap_and_from_nothing_alive():
    d = mr.build_inputs(257, 3, mode="mixed")
    a, b = controllers(d, cap_max=260)
    with torch.no_grad():
        assert a.grow(u=dev_u(3)) == b.grow(u=dev_u(3)) == 260
    ref = mr.cached_reference(257, 3, "mixed", grow_n=3)
    check_both(a, b, d, ref, "grow to the cap")
    before = {n: p for n, p in mr.state_of(b)[0].items()}
    with torch.no_grad():
        assert b.grow() == 260                              # at the cap: nothing happens, not even a new tensor
    assert all(p is before[n] for n, p in mr.state_of(b)[0].items())
    d0 = mr.build_inputs(65, 3, mode="all")
    a, b = controllers(d0)
    with torch.no_grad():
        assert a.grow(u=dev_u(3)) == b.grow(u=dev_u(3)) == 68
    ref = mr.cached_reference(65, 3, "all", grow_n=3)
    assert b.counts("grow") == ref["counts"] == a.counts("grow")
    check_both(a, b, d0, ref, "grow, all dead")


@functools.lru_cache(maxsize=None)
def noise_inputs(P):
    d = mr.clone_inputs(mr.build_inputs(P, 0, mode="mixed"))
    if P >= 63:
        d["par"]["opacity"][::7] = 0.0                      # sigmoid = 0.5: the gate leaves nothing of the noise
    return d, torch.randn(P, 3, generator=torch.Generator().manual_seed(40 + P))


@pytest.mark.parametrize("P", PS)
def test_noise(P):
    d, noise = noise_inputs(P)
    a = mr.make_controller(mr.clone_inputs(d), MCMCController, moments=False)              # the torch float32 evaluation, on the CPU
    b = mr.make_controller(mr.clone_inputs(d, DEV), FusedMCMCController, moments=False)
    for ctl in (a, b):
        ctl.update_learning_rate(0)
    scale = np.float32(a.mcmc.noise_lr * a._xyz_lr_now())
    want = mr_noise64(d["par"], noise, a.mcmc, scale)
    a.add_noise(noise=noise)
    b.add_noise(noise=noise.to(DEV))
    got = b.model._xyz.detach().cpu()
    torch_err = float((a.model._xyz.detach().double() - want).abs().max())
    err = float((got.double() - want).abs().max())
    moved = float((want - d["par"]["xyz"].double()).abs().max())
    print(f"noise P={P}: largest move {moved:.3e} torch f32 err {torch_err:.3e} hip err {err:.3e}")
    assert err <= 2 * torch_err + 1e-7
    if P >= 63:
        assert moved > 1e-3
        assert torch.equal(got[::7], d["par"]["xyz"][::7])                                  # bit for bit where the gate is shut
        q = d["par"]["rotation"].norm(dim=1)
        assert int(((q - 1.0).abs() > 0.05).sum()) > P // 2                                 # un-normalised quaternions


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("P", PS)
def test_regularize(P, strided):
    d = mr.build_inputs(P, 0, mode="mixed")
    gen = torch.Generator().manual_seed(P)
    g_op, g_sc = 1e-4 * torch.randn(P, 1, generator=gen), 1e-4 * torch.randn(P, 3, generator=gen)
    a = mr.make_controller(mr.clone_inputs(d), MCMCController, moments=False)
    a.model._opacity.grad, a.model._scaling.grad = g_op.clone(), g_sc.clone()
    ta = a.regularize()
    op, sc = d["par"]["opacity"].double(), d["par"]["scaling"].double()
    s = torch.sigmoid(op)
    want = {"opacity": g_op.double() + float(np.float32(0.01 / P)) * s * (1 - s), "scaling": g_sc.double() + float(np.float32(0.01 / (3 * P))) * torch.exp(sc)}
    want_terms = (0.01 * float(s.mean()), 0.01 * float(torch.exp(sc).mean()))
    outs = []
    for _ in range(2):
        b = mr.make_controller(mr.clone_inputs(d, DEV), FusedMCMCController, moments=False)
        if strided:                                          # views into a gradient arena: rows 11 floats apart
            arena = torch.full((P, 11), 7.0, device=DEV)
            arena[:, 2:3], arena[:, 5:8] = g_op.to(DEV), g_sc.to(DEV)
            b.model._opacity.grad, b.model._scaling.grad = arena[:, 2:3], arena[:, 5:8]
            assert P == 1 or not b.model._scaling.grad.is_contiguous()
        else:
            b.model._opacity.grad, b.model._scaling.grad = g_op.to(DEV), g_sc.to(DEV)
        tb = b.regularize()
        if strided:
            rest = torch.ones(11, dtype=torch.bool)
            rest[2], rest[5:8] = False, False
            assert bool((arena[:, rest.to(DEV)] == 7.0).all())
        outs.append((b.model._opacity.grad.cpu().clone(), b.model._scaling.grad.cpu().clone(), tb[0].cpu(), tb[1].cpu()))
    for x, y in zip(outs[0], outs[1]):
        assert torch.equal(x, y)                             # no atomics: bit-identical from run to run
    for n, got, ref32 in (("opacity", outs[0][0], a.model._opacity.grad), ("scaling", outs[0][1], a.model._scaling.grad)):
        torch_err = float((ref32.double() - want[n]).abs().max())
        err = float((got.double() - want[n]).abs().max())
        print(f"regularize P={P} {n}: torch f32 err {torch_err:.3e} hip err {err:.3e}")
        assert err <= 2 * torch_err + 1e-7
    s32 = 0.01 * torch.sigmoid(d["par"]["opacity"]).mean(), 0.01 * torch.exp(d["par"]["scaling"]).mean()      # the means in float32
    for k in (0, 1):
        torch_err = abs(float(s32[k]) - want_terms[k])
        err = abs(float(outs[0][2 + k]) - want_terms[k])
        print(f"regularize P={P} term {k}: torch f32 err {torch_err:.3e} hip err {err:.3e} (MCMCController {abs(float(ta[k]) - want_terms[k]):.3e})")
        assert err <= 2 * torch_err + 1e-7


def test_schedule_keeps_the_two_controllers_in_step():
    P = 257
    d = mr.build_inputs(P, 3, mode="mixed")
    a, b = controllers(d, cap_max=(P * 12) // 10, moments=False, refine_start=0, refine_every=10, adam="hip")
    gens = [torch.Generator(device=DEV).manual_seed(21) for _ in range(2)]
    grads = {n: 1e-3 * torch.randn(d["par"][n].shape, generator=torch.Generator().manual_seed(5)).to(DEV) for n in GROUPS}
    sizes = []
    for it in range(1, 31):
        for ctl, gen in zip((a, b), gens):
            ctl.update_learning_rate(it)
            for g in ctl.optimizer.param_groups:
                p = g["params"][0]
                base = grads[g["name"]]
                p.grad = base[torch.arange(p.shape[0], device=DEV) % P].clone() + (0.02 if g["name"] == "opacity" else 0.0)
            with torch.no_grad():
                ctl.after_backward(it)
            ctl.optimizer.step()
            with torch.no_grad():
                ctl.after_step(it, generator=gen)
        assert a.model._xyz.shape[0] == b.model._xyz.shape[0] <= (P * 12) // 10
        sizes.append(b.model._xyz.shape[0])
        if it % 10 == 0:
            for which in ("relocate", "grow"):
                assert a.counts(which) == b.counts(which), (it, which)
    assert sizes[8] == 257 and sizes[9] == 269 and sizes[19] == 282 and sizes[29] == 296
    assert a.counts("relocate")["n_dead"] > 0
    assert torch.equal(a.model._features_dc.detach(), b.model._features_dc.detach())        # untouched by noise and regularisers: same rows


def test_c_abi_edges():
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    import ctypes as C
    need = C.c_size_t(0)
    assert lib.gsr_mcmc_plan_workspace(0, 0, C.byref(need)) == 0 and need.value > 0
    assert lib.gsr_mcmc_plan_workspace(257, 12, C.byref(need)) == 0
    d = mr.clone_inputs(mr.build_inputs(257, 3, mode="mixed"), DEV)
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    counts = torch.full((4,), 7, dtype=torch.int32).pin_memory()
    u = dev_u(12)
    plan = lambda nbytes: lib.gsr_mcmc_plan(stream, _lib.MCMC_GROW, 257, d["par"]["opacity"].data_ptr(), d["par"]["scaling"].data_ptr(), mr.L, mr.MIN_OPACITY,
                                            51, 12, u.data_ptr(), counts.data_ptr(), ws.data_ptr(), nbytes)
    assert plan(need.value - 1) == 4 and b"mcmc workspace" in lib.gsr_last_error()
    assert plan(need.value) == 0
    torch.cuda.synchronize()
    assert dict(zip(("n_dead", "n_draws", "n_sources", "P_new"), counts.tolist())) == mr.cached_reference(257, 3, "mixed", grow_n=12)["counts"]
    # an apply that does not belong to the plan in the workspace (another n_draws) writes nothing
    dst = torch.full((257, 1), 5.0, device=DEV)
    grp = (_lib.McmcGroup * 1)(_lib.McmcGroup(d["par"]["opacity"].data_ptr(), None, None, dst.data_ptr(), None, None, 1, _lib.MCMC_OPACITY))
    need0 = C.c_size_t(0)
    assert lib.gsr_mcmc_plan_workspace(257, 0, C.byref(need0)) == 0 and need0.value <= need.value
    assert lib.gsr_mcmc_apply(stream, _lib.MCMC_GROW, 257, 0, 1, grp, ws.data_ptr(), need.value) == 0
    torch.cuda.synchronize()
    assert bool((dst == 5.0).all())
