"""-m gpu: density control on the device (include/gsr_density.h, densify.FusedDensityController) against DensityController on
the same device, the same inputs and the same generator seed: counts equal, every copied quantity bit for bit, the split
children against the float64 evaluation of the same formula on the same samples; the statistics of record against a float64
accumulation; the edge cases and the C ABI's error paths.

Shapes: P = 1 (one lane), 63 / 64 / 65 (the wave edge), 257 (the group edge, odd), 5000 (several scan blocks); f_rest widths 0, 3, 15
(rows of 0, 9 and 45 floats beside widths 1, 3 and 4; odd P so that no group's rows stay 16-byte aligned).

Bar of the children (per tensor): twice the largest error the torch float32 evaluation of the rule shows against float64 on the
same inputs, measured here on the CPU, plus 1e-7.  Measured on an MI355X at P = 5000: see DESIGN.md section 7, 8f-4.
"""
import ctypes as C
import functools

import pytest
import torch

from gaussian_transformer_amd import _lib
from gaussian_transformer_amd.densify import GROUPS, DensityController, FusedDensityController
from tests import density_ref as dr
from tests.test_density_host import STEP, make_controller

pytestmark = pytest.mark.gpu
DEV = "cuda"
PS = [1, 63, 64, 65, 257, 5000]
RESTS = [0, 3, 15]


def controllers(d, moments=True, **kw):
    return (make_controller(dr.clone_inputs(d, DEV), cls=cls, moments=moments, **kw) for cls in (DensityController, FusedDensityController))


def run(ctl, mss, seed=5, **kw):
    with torch.no_grad():
        return ctl.densify_and_prune(dr.THRESHOLD, dr.MIN_OPACITY, dr.EXTENT, mss, generator=torch.Generator(device=DEV).manual_seed(seed), **kw)


def state_of(ctl, name):
    p = next(g["params"][0] for g in ctl.optimizer.param_groups if g["name"] == name)
    return p, ctl.optimizer.state.get(p)


def assert_copied_equal(a, b, n_children, moments=True):
    """Everything that is a copy is bit-equal; of xyz and scaling, every row but the children at the end."""
    for n in GROUPS:
        (pa, sa), (pb, sb) = state_of(a, n), state_of(b, n)
        assert pa.shape == pb.shape, n
        rows = pa.shape[0] - (n_children if n in ("xyz", "scaling") else 0)
        assert torch.equal(pa.detach()[:rows], pb.detach()[:rows]), n
        assert pb.is_leaf and pb.requires_grad and isinstance(pb, torch.nn.Parameter) and pb is getattr(b.model, "_" + {"f_dc": "features_dc", "f_rest": "features_rest"}.get(n, n))
        if moments:
            assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), n
            assert float(sb["step"]) == STEP
        else:
            assert not sa and not sb


@functools.lru_cache(maxsize=None)
def cpu_rule(P, rest, mss, dtype, seed=5, mode="mixed"):
    """The rule on the CPU in `dtype` with the samples the device generator draws for this seed (fetched once)."""
    d = dr.clone_inputs(dr.build_inputs(P, rest, mode=mode), dtype=dtype)

    def noise_fn(rows):
        ones = torch.ones(rows, 3, device=DEV)
        return torch.normal(mean=torch.zeros_like(ones), std=ones, generator=torch.Generator(device=DEV).manual_seed(seed)).cpu()
    return dr.one_pass(d["par"], d["mom"], d["accum"], d["denom"], noise_fn, mss)


def assert_children(ctl, P, rest, mss, mode="mixed"):
    _, _, counts, P_new, c64 = cpu_rule(P, rest, mss, torch.float64, mode=mode)
    _, _, counts32, _, c32 = cpu_rule(P, rest, mss, torch.float32, mode=mode)
    assert counts == counts32
    n_children = c64["xyz"].shape[0]
    for n in ("xyz", "scaling"):
        got = state_of(ctl, n)[0].detach().cpu().double()
        assert got.shape[0] == P_new
        if n_children == 0:
            continue
        torch_err = float((c32[n].double() - c64[n]).abs().max())
        err = float((got[P_new - n_children:] - c64[n]).abs().max())
        print(f"children {n}: P={P} rest={rest} mss={mss} n={n_children} torch f32 err {torch_err:.3e} hip err {err:.3e}")
        assert err <= 2 * torch_err + 1e-7, (n, err, torch_err)
    return counts, P_new, n_children


@pytest.mark.parametrize("mss", [None, 20])
@pytest.mark.parametrize("rest", RESTS)
@pytest.mark.parametrize("P", PS)
def test_densify_and_prune_equals_the_torch_controller(P, rest, mss):
    d = dr.build_inputs(P, rest)
    a, b = controllers(d)
    ca, cb = run(a, mss), run(b, mss)
    assert ca == cb
    counts, P_new, n_children = assert_children(b, P, rest, mss)
    assert cb == counts and b.model._xyz.shape[0] == P_new == a.model._xyz.shape[0]
    if P >= 257:
        assert cb["cloned"] > 0 and cb["split"] > 1 and cb["pruned"] > 0 and n_children > 0
    assert_copied_equal(a, b, n_children)
    m = b.model
    for t, shape in ((m.xyz_gradient_accum, (P_new, 1)), (m.denom, (P_new, 1)), (m.max_radii2D, (P_new,))):
        assert tuple(t.shape) == shape and t.dtype == torch.float32 and not t.any()
    if P_new:                                               # a further optimiser step works on the installed tensors
        for g in b.optimizer.param_groups:
            g["params"][0].grad = torch.ones_like(g["params"][0])
            g["lr"] = 1e-3
        before = m._xyz.detach().clone()
        b.optimizer.step()
        assert not torch.equal(before, m._xyz.detach()) and float(state_of(b, "xyz")[1]["step"]) == STEP + 1


@pytest.mark.parametrize("adam", ["torch", "hip"])
@pytest.mark.parametrize("P", [65, 257])
def test_no_optimiser_state_yet_then_both_optimisers_step(P, adam):
    d = dr.build_inputs(P, 3)
    a, b = controllers(d, moments=False, adam=adam)
    assert run(a, 20) == run(b, 20)
    _, _, n_children = assert_children(b, P, 3, 20)
    assert_copied_equal(a, b, n_children, moments=False)
    for ctl in (a, b):
        for g in ctl.optimizer.param_groups:
            g["params"][0].grad = torch.full_like(g["params"][0], 0.5)
            g["lr"] = 1e-3
        ctl.optimizer.step()
    for n in GROUPS:                                        # the first step after the surgery: identical on identical rows
        (pa, sa), (pb, sb) = state_of(a, n), state_of(b, n)
        rows = pa.shape[0] - (n_children if n in ("xyz", "scaling") else 0)
        assert torch.equal(pa.detach()[:rows], pb.detach()[:rows]) and torch.equal(sa["exp_avg"], sb["exp_avg"]), n
    assert run(a, None, seed=9) == run(b, None, seed=9)     # and a second densification with state present
    assert a.model._xyz.shape == b.model._xyz.shape
    assert torch.equal(state_of(a, "f_rest")[0].detach(), state_of(b, "f_rest")[0].detach())
    assert torch.equal(state_of(a, "rotation")[1]["exp_avg_sq"], state_of(b, "rotation")[1]["exp_avg_sq"])


@pytest.mark.parametrize("mode,P", [("none", 257), ("split", 257), ("clone", 257), ("pruned", 257), ("split", 1), ("pruned", 1)])
def test_edge_selections(mode, P):
    d = dr.build_inputs(P, 3, mode=mode)
    a, b = controllers(d)
    ca, cb = run(a, 20), run(b, 20)
    assert ca == cb
    want = {"none": (0, 0), "split": (0, P), "clone": (P, 0), "pruned": (0, 0)}[mode]
    assert (cb["cloned"], cb["split"]) == want
    counts, P_new, n_children = assert_children(b, P, 3, 20, mode=mode)
    assert counts == cb and P_new == {"split": 2 * P, "clone": 2 * P, "pruned": 0}.get(mode, P_new) == b.model._xyz.shape[0]
    if mode == "pruned":
        assert cb["pruned"] == P and b.model.denom.shape == (0, 1)
    assert_copied_equal(a, b, n_children)


def test_normal_fn_and_run_to_run_identity():
    d = dr.build_inputs(5000, 15)
    fixed = torch.randn(20000, 3, generator=torch.Generator().manual_seed(3)).to(DEV)
    normal_fn = lambda stds: fixed[:stds.shape[0]] * stds
    outs = []
    for cls_i in (0, 1, 1):
        ctl = list(controllers(d))[cls_i]
        outs.append((ctl, run(ctl, 20, normal_fn=normal_fn)))
    (a, ca), (b, cb), (b2, cb2) = outs
    assert ca == cb == cb2 and cb["split"] > 1
    for n in GROUPS:                                        # two runs of the fused path: bit-identical, children included
        (p1, s1), (p2, s2) = state_of(b, n), state_of(b2, n)
        assert torch.equal(p1.detach(), p2.detach()) and torch.equal(s1["exp_avg"], s2["exp_avg"]) and torch.equal(s1["exp_avg_sq"], s2["exp_avg_sq"])
    # against the torch path on the same samples: children within the float32 rounding of the formula (values of size <= 10)
    n_children = cpu_rule(5000, 15, 20, torch.float32)[4]["xyz"].shape[0]       # the decisions do not depend on the samples
    assert 0 < n_children < 2 * cb["split"]                                      # some children are pruned
    assert_copied_equal(a, b, n_children)
    for n in ("xyz", "scaling"):
        pa, pb = state_of(a, n)[0].detach(), state_of(b, n)[0].detach()
        assert (pa - pb).abs().max() <= 16 * 2.0 ** -24 * max(1.0, float(pa.abs().max()))


@functools.lru_cache(maxsize=None)
def record_views(P):
    gen = torch.Generator().manual_seed(P)
    never = torch.arange(P) % 5 == 3                         # rows no view sees: they must stay as they were
    views = []
    for k in range(3):
        mag = torch.exp(torch.log(torch.tensor(1e-6)) + (torch.log(torch.tensor(1e-2)) - torch.log(torch.tensor(1e-6))) * torch.rand(P, 1, generator=gen))
        ang = 6.2831853 * torch.rand(P, 1, generator=gen)
        grad = torch.cat((mag * torch.cos(ang), mag * torch.sin(ang), torch.randn(P, 1, generator=gen)), dim=1)
        radii = torch.randint(-1, 40, (P,), generator=gen, dtype=torch.int32).clamp_min(0) * ~never
        vis = (radii > 0) if k != 1 else ((torch.rand(P, generator=gen) < 0.5) & ~never)      # view 1: an explicit mask that differs from radii > 0
        views.append((grad, radii, vis))
    return views


@pytest.mark.parametrize("P", PS)
def test_record(P):
    d = dr.build_inputs(P, 0)
    _, b = controllers(d)
    m = b.model
    start = [t.clone() for t in (m.xyz_gradient_accum, m.denom, m.max_radii2D)]
    acc64, den, mx = start[0].cpu().double(), start[1].cpu().clone(), start[2].cpu().clone()
    seen = torch.zeros(P, dtype=torch.bool)
    for k, (grad, radii, vis) in enumerate(record_views(P)):
        vs = torch.zeros(P, 3, device=DEV)
        if k == 2:                                           # a strided view into a gradient arena: rows 7 floats apart, offset 2
            arena = torch.full((P, 7), float("nan"), device=DEV)
            arena[:, 2:5] = grad.to(DEV)
            vs.grad = arena[:, 2:5]
            assert P == 1 or not vs.grad.is_contiguous()
        else:
            vs.grad = grad.to(DEV)
        with torch.no_grad():
            b.record(vs, None if k == 0 else vis.to(DEV), radii.to(DEV))
        acc64[vis] += torch.sqrt(grad[vis, 0:1].double() ** 2 + grad[vis, 1:2].double() ** 2)
        den[vis] += 1
        mx[vis] = torch.maximum(mx[vis], radii[vis].float())
        seen |= vis
    if P >= 63:
        assert seen.any() and not seen.all() and (record_views(P)[1][2] != (record_views(P)[1][1] > 0)).any()
    assert torch.equal(m.denom.cpu(), den) and torch.equal(m.max_radii2D.cpu(), mx)
    err = (m.xyz_gradient_accum.cpu().double() - acc64).abs()
    assert (err <= 3 * 3 * 2.0 ** -24 * acc64 + 1e-30).all(), float((err / acc64.clamp_min(1e-30)).max())
    for now, was in zip((m.xyz_gradient_accum, m.denom, m.max_radii2D), start):      # invisible rows: untouched, bit for bit
        assert torch.equal(now.cpu()[~seen], was.cpu()[~seen])


def test_c_abi_edges_and_errors():
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    need = C.c_size_t(0)
    assert lib.gsr_densify_plan_workspace(0, 2, C.byref(need)) == 0
    assert lib.gsr_density_record(stream, 0, None, 3, None, None, None, None, None) == 0
    counts = torch.full((4,), 7, dtype=torch.int32).pin_memory()
    assert lib.gsr_densify_plan(stream, 0, None, None, None, None, 2e-4, 0.005, 0.04, 0.4, 2, counts.data_ptr(), None, 0) == 0
    assert counts.tolist() == [0, 0, 0, 0]
    assert lib.gsr_densify_apply(stream, 0, 2, 0, 0, 0, None, None, None, None, None, 0) == 0
    # errors: each leaves a message, and the next call works
    P = 257
    d = dr.clone_inputs(dr.build_inputs(P, 3), DEV)
    assert lib.gsr_densify_plan_workspace(P, 2, C.byref(need)) == 0 and need.value > 0
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    plan = lambda N, nbytes: lib.gsr_densify_plan(stream, P, d["par"]["opacity"].data_ptr(), d["par"]["scaling"].data_ptr(), d["accum"].data_ptr(),
                                                  d["denom"].data_ptr(), dr.f32(dr.THRESHOLD), dr.f32(dr.MIN_OPACITY), dr.f32(0.04), dr.f32(0.4), N,
                                                  counts.data_ptr(), ws.data_ptr(), nbytes)
    assert plan(2, need.value - 1) == 4 and b"workspace" in lib.gsr_last_error()
    assert plan(0, need.value) == 1 and b"N=0" in lib.gsr_last_error()
    assert lib.gsr_densify_plan_workspace(P, 0, C.byref(need)) == 1
    assert lib.gsr_densify_plan_workspace(2 ** 30, 2, C.byref(need)) == 1 and b"2^31" in lib.gsr_last_error()
    assert lib.gsr_densify_plan_workspace(P, 2, C.byref(need)) == 0
    assert plan(2, need.value) == 0
    torch.cuda.synchronize()
    n_clone, n_split, n_pruned, P_new = counts.tolist()
    _, _, want, want_new, _ = cpu_rule(P, 3, 20, torch.float32)
    assert {"cloned": n_clone, "split": n_split, "pruned": n_pruned} == want and P_new == want_new
    dst = torch.empty(P_new, 1, device=DEV)
    grp = _lib.DensityGroup(d["par"]["opacity"].data_ptr(), None, None, dst.data_ptr(), None, None, 1, _lib.DENSITY_COPY)
    many = (_lib.DensityGroup * 17)(*([grp] * 17))
    apply = lambda n, arr: lib.gsr_densify_apply(stream, P, 2, n_split, P_new, n, arr, d["par"]["scaling"].data_ptr(),
                                                 d["par"]["rotation"].data_ptr(), None, ws.data_ptr(), need.value)
    assert apply(17, many) == 1 and b"17 groups" in lib.gsr_last_error()
    assert apply(1, many) == 0
    torch.cuda.synchronize()
    new, _, _, _, _ = cpu_rule(P, 3, 20, torch.float32)
    assert torch.equal(dst.cpu(), new["opacity"])
