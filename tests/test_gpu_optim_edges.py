"""-m gpu: HipAdam (include/gsr_optim.h, csrc/adam.hip, optim.py) on the branches no fresh, aligned, one-tensor-per-group test enters:
the scalar body (any of param / grad / exp_avg / exp_avg_sq off a 16-byte boundary, as the gradient arena's slices are for an odd
number of Gaussians), the float4 body's tail, more groups than one launch takes, several tensors / a missing gradient / an empty
tensor in a group, groups with different betas and eps, a strided gradient, the bias corrections at step 30 000, 0 / (0 + eps), a
second stream.

Every case runs three optimisers on the same float32 inputs: HipAdam, torch.optim.Adam in float32 on the GPU (the yardstick) and
oracle/aux_ref.py in float64 (the truth; pinned against torch.optim.Adam in float64 by tests/test_aux_references.py).  Per tensor and for
each of param, exp_avg, exp_avg_sq, with err_x = max|x - f64| / max|f64|:
    err_hip <= 2 err_torch + 4 * 2^-24
2: the margin tests/helpers.py::assert_parity gives one float32 evaluation over another; 4 * 2^-24: two units in the last place of
the tensor's scale, for the tensors (of one element, say) on which torch happens to be exact.  Besides: every tensor lives inside
a buffer of sentinels that must come back bit-identical, and nothing may be NaN or Inf.

Measured on the MI355X, worst tensor of each case (err_hip / err_torch, in units of 2^-24):
    misaligned param k=1,2,3             param 1.94/1.21  exp_avg 0.23/0.23  exp_avg_sq 1.69/1.69
    misaligned grad k=1,2,3              param 1.05/1.05  exp_avg 0.22/0.22  exp_avg_sq 4.28/2.98
    misaligned exp_avg k=1,2,3           param 1.82/1.82  exp_avg 0.83/0.83  exp_avg_sq 2.31/2.31
    misaligned exp_avg_sq k=1,2,3        param 0.56/0.56  exp_avg 0.84/0.84  exp_avg_sq 2.28/2.28
    misaligned all k=1,2,3               param 0.78/0.78  exp_avg 0.81/0.81  exp_avg_sq 1.71/1.71
    aligned                          param 2.60/0.69  exp_avg 0.08/0.08  exp_avg_sq 5.57/3.06
    arena P=1001 M=4                 param 2.55/2.55  exp_avg 1.57/1.57  exp_avg_sq 3.15/3.34
    arena P=333 M=16                 param 2.28/2.28  exp_avg 1.83/1.83  exp_avg_sq 3.82/3.82
    17 groups                        param 0.39/0.39  exp_avg 0.18/0.18  exp_avg_sq 0.34/0.34
    35 groups                        param 0.24/0.24  exp_avg 0.18/0.18  exp_avg_sq 1.49/0.68
    several tensors, None, empty     param 2.37/2.37  exp_avg 0.46/0.46  exp_avg_sq 3.37/2.28
    different betas / eps            param 1.33/1.33  exp_avg 0.47/0.47  exp_avg_sq 0.82/0.82
    transposed grad                  param 2.23/2.23  exp_avg 1.07/1.07  exp_avg_sq 3.65/3.31
    step 29 999 + 3                  param 0.33/0.33  exp_avg 0.86/0.86  exp_avg_sq 0.71/0.71
    zero gradient, eps 1e-15         param 0.00/0.00  exp_avg 0.00/0.00  exp_avg_sq 0.00/0.00
    second stream                    param 0.03/0.03  exp_avg 0.32/0.32  exp_avg_sq 3.76/3.76
"""
import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib
from oracle import aux_ref
from tests import aux_inputs

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENTINEL = 725000.5
GUARD = 32                              # floats on either side (128 bytes: the view's alignment is that of its offset k)
LENGTHS = [1, 3, 4, 5, 4095, 4096, 4097, 3 * 4096 + 1]       # one block is 4096 elements
LRS = [0.00016, 0.0025, 0.000125, 0.05, 0.005, 0.001, 0.01]
DEFAULT = dict(betas=(0.9, 0.999), eps=1e-15)


class Guarded:
    """`n` floats at offset `k` (in floats) from a 16-byte boundary, inside a buffer of sentinels."""

    def __init__(self, n, k=0, values=None):
        self.buf = torch.full((GUARD + n + GUARD + 4,), SENTINEL, dtype=torch.float32, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.lo, self.hi = GUARD + k, GUARD + k + n
        self.view = self.buf[self.lo:self.hi]
        self.view.copy_(torch.zeros(n) if values is None else torch.tensor(np.asarray(values, dtype=np.float32).reshape(-1)))
        assert self.view.data_ptr() % 16 == 4 * (k % 4)

    def intact(self):
        s = torch.tensor([SENTINEL], dtype=torch.float32, device="cuda").view(torch.int32)
        b = self.buf.view(torch.int32)
        return bool((b[:self.lo] == s).all()) and bool((b[self.hi:] == s).all())


def T(n, k=(0, 0, 0, 0), group=None, shape=None, grad=True, transposed_grad=False):
    """One parameter tensor of a case: k = float offsets of (param, grad, exp_avg, exp_avg_sq) from a 16-byte boundary."""
    return dict(n=n, k=k, group=group, shape=shape or (n,), grad=grad, transposed_grad=transposed_grad)


def run_case(name, tensors, groups=None, steps=aux_inputs.ADAM_STEPS, preset=None, lazy_state=False, zero_grads=False, grad_scale=1.0,
             grad_views=None, extra_guards=(), stream=None):
    """tensors: list of T(...), each in its own group unless T.group names one of `groups` (list of dicts lr / betas / eps).
    preset: (step, exp_avg list, exp_avg_sq list) to start from.  grad_views: ready-made gradient tensors (arena slices)."""
    from gaussian_transformer_amd.optim import HipAdam
    if groups is None:
        groups = [dict(lr=LRS[i % len(LRS)], **DEFAULT) for i in range(len(tensors))]
        for i, t in enumerate(tensors):
            t["group"] = i
    lengths = [t["n"] for t in tensors]
    p0 = aux_inputs.adam_params(lengths, seed=len(name))
    step0, m0, v0 = preset if preset is not None else (0, [None] * len(tensors), [None] * len(tensors))
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream())
    with ctx:
        # --- HipAdam on guarded, possibly misaligned storage
        hp, hg, hm, hv, hparams = [], [], [], [], []
        for i, t in enumerate(tensors):
            kp, kg, km, kv = t["k"]
            P = Guarded(t["n"], kp, p0[i]); hp.append(P)
            hparams.append(P.view.view(t["shape"]).detach().requires_grad_(True))
            assert hparams[-1].data_ptr() == P.view.data_ptr() and hparams[-1].is_contiguous()
            hm.append(Guarded(t["n"], km, m0[i])); hv.append(Guarded(t["n"], kv, v0[i]))
            hg.append(Guarded(t["n"], kg) if (t["grad"] and grad_views is None) else None)
        hopt = HipAdam([dict(params=[p for p, t in zip(hparams, tensors) if t["group"] == gi], **g) for gi, g in enumerate(groups)])
        if not lazy_state:
            for p, t, M, V in zip(hparams, tensors, hm, hv):
                if t["grad"]:
                    hopt.state[p] = dict(step=step0, exp_avg=M.view.view(t["shape"]), exp_avg_sq=V.view.view(t["shape"]))
        # --- torch.optim.Adam in float32 on the same device, ordinary tensors
        tparams = [torch.tensor(p0[i], device="cuda").view(t["shape"]).requires_grad_(True) for i, t in enumerate(tensors)]
        topt = torch.optim.Adam([dict(params=[p for p, t in zip(tparams, tensors) if t["group"] == gi], **g) for gi, g in enumerate(groups)])
        if preset is not None:
            for i, (p, t) in enumerate(zip(tparams, tensors)):
                topt.state[p] = dict(step=torch.tensor(float(step0)), exp_avg=torch.tensor(m0[i], device="cuda").view(t["shape"]),
                                     exp_avg_sq=torch.tensor(v0[i], device="cuda").view(t["shape"]))
        # --- float64
        ref = [aux_ref.Adam64(p0[i], m0[i], v0[i], step0) for i in range(len(tensors))]
        lrs = [g["lr"] for g in groups]
        for step in range(steps):
            gs = aux_inputs.adam_grads(lengths, step, seed=len(name) + 1)
            for i, t in enumerate(tensors):
                if not t["grad"]:
                    ref[i].update(None, 0.0)
                    continue
                g = gs[i] * np.float32(0.0 if zero_grads else grad_scale)
                gd = torch.tensor(g, device="cuda")
                if grad_views is not None:
                    grad_views[i].copy_(gd.view(grad_views[i].shape)); hparams[i].grad = grad_views[i]
                elif t["transposed_grad"]:
                    a, b = t["shape"]
                    view = hg[i].view.view(b, a).t()                       # [a, b] with strides (1, a)
                    view.copy_(gd.view(a, b)); hparams[i].grad = view
                    assert not hparams[i].grad.is_contiguous()
                else:
                    hg[i].view.copy_(gd); hparams[i].grad = hg[i].view.view(t["shape"])
                tparams[i].grad = gd.view(t["shape"]).clone()
                G = groups[t["group"]]
                ref[i].update(g, lrs[t["group"]], G["betas"], G["eps"])
            hopt.step(); topt.step()
            if step == aux_inputs.ADAM_LR_CHANGE_AFTER:
                hopt.param_groups[0]["lr"] = topt.param_groups[0]["lr"] = lrs[0] = aux_inputs.ADAM_LR_CHANGED
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    # --- verdict
    worst = dict(param=(0.0, 0.0), exp_avg=(0.0, 0.0), exp_avg_sq=(0.0, 0.0))
    for i, t in enumerate(tensors):
        for G in (hp[i], hm[i], hv[i], hg[i]) + tuple(extra_guards):
            assert G is None or G.intact(), (name, i, "an element outside the tensor was written")
        hst, tst = hopt.state.get(hparams[i], {}), topt.state.get(tparams[i], {})
        if not t["grad"]:                                                   # as torch: state untouched, step not advanced
            assert len(hst) == 0 and len(tst) == 0 and ref[i].step == step0
            assert np.array_equal(hparams[i].detach().cpu().numpy().reshape(-1), p0[i])
            continue
        assert int(hst["step"]) == int(tst["step"]) == ref[i].step == step0 + steps
        if not lazy_state:
            assert hst["exp_avg"].data_ptr() == hm[i].view.data_ptr() and hst["exp_avg_sq"].data_ptr() == hv[i].view.data_ptr()
        for key, h, tt, r in (("param", hparams[i], tparams[i], ref[i].p), ("exp_avg", hst["exp_avg"], tst["exp_avg"], ref[i].m),
                              ("exp_avg_sq", hst["exp_avg_sq"], tst["exp_avg_sq"], ref[i].v)):
            h = h.detach().cpu().numpy().reshape(-1).astype(np.float64); tt = tt.detach().cpu().numpy().reshape(-1).astype(np.float64)
            assert np.isfinite(h).all(), (name, i, key)
            if t["n"] == 0:
                continue
            scale = np.abs(r).max()
            if scale == 0:                                                  # all gradients 0: the moments stay exactly 0
                assert (h == 0).all(), (name, i, key)
                continue
            eh, et = np.abs(h - r).max() / scale, np.abs(tt - r).max() / scale
            if eh - 2 * et > worst[key][0] - 2 * worst[key][1] or worst[key] == (0.0, 0.0):
                worst[key] = (eh, et)
            assert eh <= 2 * et + 4 * U, (name, i, t["n"], key, eh / U, et / U)
    print(f"ADAM_EDGE {name:34s} " + "  ".join(f"{k} {a / U:6.2f}/{b / U:6.2f}" for k, (a, b) in worst.items()))
    return hparams, hopt, p0


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("which", ["param", "grad", "exp_avg", "exp_avg_sq", "all"])
def test_scalar_body_on_misaligned_tensors(which, k):
    """Views flat[k : k + n]: one pointer of the four off the 16-byte boundary is enough to leave the float4 body."""
    ks = tuple(k if which in (name, "all") else 0 for name in ("param", "grad", "exp_avg", "exp_avg_sq"))
    assert any(x % 4 for x in ks)                                           # Guarded asserts data_ptr() % 16 == 4 k
    run_case(f"misaligned {which} k={k}", [T(n, ks) for n in LENGTHS])


def test_float4_body_and_its_tail_on_aligned_tensors():
    run_case("aligned", [T(n) for n in LENGTHS])


@pytest.mark.parametrize("P,M", [(1001, 4), (333, 16)])
def test_gradients_that_are_slices_of_the_gradient_arena(P, M):
    """rasterizer.gradient_arena with an odd P: the backward pass hands out consecutive slices of one flat tensor, and every slice after
    the first starts on a 4-byte boundary only."""
    from gaussian_transformer_amd import rasterizer
    n = rasterizer.arena_floats(P, M)
    arena = Guarded(n, 0)
    g = rasterizer.get_backend()._gradient_outputs(torch.device("cuda", 0), P, M, 0, True, False, False, arena.view)
    views = [g[0], g[2], g[4], g[5], g[6]]                                  # means3D, shs, opacities, scales, rotations: the arena's order
    assert sum(v.numel() for v in views) == n and all(v.data_ptr() >= arena.view.data_ptr() for v in views)
    assert views[0].data_ptr() % 16 == 0 and sum(v.data_ptr() % 16 != 0 for v in views) >= 3
    run_case(f"arena P={P} M={M}", [T(v.numel(), shape=tuple(v.shape)) for v in views], grad_views=views, extra_guards=(arena,))


@pytest.mark.parametrize("n_groups", [_lib.ADAM_MAX_GROUPS + 1, 2 * _lib.ADAM_MAX_GROUPS + 3])
def test_more_groups_than_one_launch_takes(n_groups):
    assert n_groups > _lib.ADAM_MAX_GROUPS
    lens = LENGTHS + [7, 100, 8192]
    ts = [T(lens[(3 * i) % len(lens)], ((i % 4), (i // 2) % 4, 0, (i % 3))) if i % 3 else T(lens[(3 * i) % len(lens)]) for i in range(n_groups)]
    assert any(any(t["k"]) for t in ts) and any(not any(t["k"]) for t in ts)
    run_case(f"{n_groups} groups", ts)


def test_group_of_several_tensors_one_without_gradient_one_empty():
    groups = [dict(lr=0.0025, **DEFAULT), dict(lr=0.01, **DEFAULT)]
    ts = [T(900, group=0, shape=(300, 3)), T(12, group=0, grad=False), T(4097, (1, 0, 0, 0), group=0), T(0, group=0, shape=(0, 3)),
          T(5000, group=0, shape=(1250, 4)), T(17, group=1)]
    run_case("several tensors, None, empty", ts, groups)


def test_groups_with_different_betas_and_eps_in_one_step():
    groups = [dict(lr=0.0025, betas=(0.9, 0.999), eps=1e-15), dict(lr=0.01, betas=(0.8, 0.99), eps=1e-8),
              dict(lr=0.001, betas=(0.9, 0.999), eps=1e-8), dict(lr=0.02, betas=(0.5, 0.9), eps=1e-15)]
    ts = [T(4097, group=0), T(300, (0, 1, 0, 0), group=1), T(5, group=1), T(4096, group=2), T(12289, group=3), T(3, group=0)]
    _, hopt, _ = run_case("different betas / eps", ts, groups)
    assert len({(tuple(g["betas"]), g["eps"]) for g in hopt.param_groups}) == 4


def test_strided_gradient():
    run_case("transposed grad", [T(300 * 15, shape=(300, 15), transposed_grad=True), T(7 * 3, (0, 1, 0, 0), shape=(7, 3), transposed_grad=True)])


def test_bias_corrections_at_the_end_of_a_30k_run():
    lens = [4097, 5, 12289]
    rng = np.random.default_rng(3)
    m0 = [(1e-3 * rng.standard_normal(n)).astype(np.float32) for n in lens]
    v0 = [(1e-6 * rng.uniform(0.01, 1, n)).astype(np.float32) for n in lens]
    _, hopt, _ = run_case("step 29 999 + 3", [T(lens[0]), T(lens[1], (1, 1, 1, 1)), T(lens[2], (0, 2, 0, 0))], steps=3, preset=(29999, m0, v0),
                          grad_scale=1e-3)
    assert all(int(s["step"]) == 30002 for s in hopt.state.values())


def test_zero_gradient_from_empty_state_with_tiny_eps():
    """0 / (0 + 1e-15) at step 1: parameters do not move, the moments stay 0, nothing becomes NaN."""
    hparams, hopt, p0 = run_case("zero gradient, eps 1e-15", [T(4097), T(5, (1, 0, 0, 0)), T(4096, (0, 3, 0, 0))], steps=2, lazy_state=True,
                                 zero_grads=True)
    for p, q in zip(hparams, p0):
        assert np.array_equal(p.detach().cpu().numpy().view(np.int32), q.view(np.int32))
        st = hopt.state[p]
        assert int(st["step"]) == 2 and (st["exp_avg"] == 0).all() and (st["exp_avg_sq"] == 0).all()


def test_whole_run_on_a_second_stream():
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.default_stream().cuda_stream
    torch.cuda.synchronize()
    run_case("second stream", [T(n, (i % 4, 0, 0, 0)) for i, n in enumerate(LENGTHS)], stream=s)
