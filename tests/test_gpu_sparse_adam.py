"""-m gpu: the visibility-masked Adam step (include/gsr_optim.h: gsr_adam_step_masked, csrc/adam.hip: adam_masked_kernel; optim.HipSparseAdam).

What is asked of it, in the order of the tests:
  1. every row visible: param / exp_avg / exp_avg_sq equal gsr_adam_step's as int32, for row widths 1, 3, 4, 9, 45 and row counts around
     the wave and the 4096-element block (45 * 91 = 4095, 45 * 92 = 4140: a row straddles the block edge), both mask kinds, each of
     the four pointers 1, 2, 3 floats off a 16-byte boundary (the scalar body);
  2. partial masks: visible rows int32-equal to the dense result, invisible rows int32-equal to the inputs -- also when every element of
     every invisible row, in all four arrays, is a NaN with a payload, +-Inf, -0.0 or a denormal -- and the visible rows equal to the
     run without those; sentinels around every buffer intact, nothing visible NaN or Inf;
  3. the mask encodings: bytes 0 / 1 / 2 / 255, torch.bool, int32 -3 / 0 / 1 / 2^31 - 1, a byte mask at an odd address;
  4. several steps with a fresh mask each against float64 (tests/sparse_adam_ref.py), at the project's bar for one float32 evaluation
     against another:  err_hip <= 2 err_torch + 4 * 2^-24  per tensor, err = max|x - f64| / max|f64|, the yardstick being one dense
     torch.optim.Adam step in float32 followed by the restoration of the invisible rows;
  5. HipSparseAdam: visibility=None is HipAdam, the state layout, the step count under an empty mask, more groups than a launch takes,
     different betas / eps, a tensor without gradient, P = 0, a second stream;
  6. refusals from Python and through ctypes, each with a text, each leaving every buffer as it was;
  7. density control with adam="hip_sparse" on both controllers.

Measured on the MI355X (item 4, worst tensor of each case, err_hip / err_torch in units of 2^-24):
    P=333 ks=(0, 0, 0, 0)            param 1.42/1.42  exp_avg 1.24/1.24  exp_avg_sq 1.97/1.41
    P=333 ks=(0, 1, 0, 0)            param 1.42/1.42  exp_avg 1.24/1.24  exp_avg_sq 2.99/2.15
    P=1501 ks=(0, 0, 0, 0)           param 1.75/1.52  exp_avg 0.96/0.96  exp_avg_sq 1.90/1.20
    P=92 ks=(1, 2, 3, 0)             param 1.12/1.12  exp_avg 0.83/0.83  exp_avg_sq 1.14/1.02
    step 29 999 + 3                  param 0.57/0.57  exp_avg 0.44/0.44  exp_avg_sq 1.57/1.57
    all clear                        param 0.00/0.00  exp_avg 0.00/0.00  exp_avg_sq 0.00/0.00
    a second stream                  param 0.73/0.75  exp_avg 0.72/0.72  exp_avg_sq 1.18/1.18
"""
import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib
from tests import aux_inputs
from tests.sparse_adam_ref import SparseAdam64, TorchMaskedAdam, fresh_masks

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENTINEL = 725000.5
GUARD = 32                              # floats on either side (128 bytes: the view's alignment is that of its offset k)
WIDTHS = [1, 3, 4, 9, 45]
ROWS = [1, 63, 64, 65, 91, 92, 1501]    # 45 * 91 = 4095, 45 * 92 = 4140; 1501 rows: 2 to 17 blocks per group
LRS = [0.05, 0.00016, 0.001, 0.0025, 0.000125]
BETAS, EPS = (0.9, 0.999), 1e-15
STEP = 7
KINDS = {"bytes": _lib.ADAM_MASK_BYTES, "radii": _lib.ADAM_MASK_RADII}
SPECIALS = np.array([0x7fc12345, 0x7f800000, 0xff800000, 0x80000000, 0x00000001], dtype=np.uint32).view(np.int32)   # NaN+payload +Inf -Inf -0.0 denormal


class Guarded:
    """`n` floats at offset `k` (in floats) from a 16-byte boundary, inside a buffer of sentinels."""

    def __init__(self, n, k=0, values=None):
        self.buf = torch.full((GUARD + n + GUARD + 4,), SENTINEL, dtype=torch.float32, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.lo, self.hi = GUARD + k, GUARD + k + n
        self.view = self.buf[self.lo:self.hi]
        if values is None:
            self.view.zero_()
        else:                                                                # bit copy: NaN payloads and denormals as they are
            self.view.view(torch.int32).copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32).reshape(-1).view(np.int32)))
        assert n == 0 or self.view.data_ptr() % 16 == 4 * (k % 4)

    def intact(self):
        s = torch.tensor([SENTINEL], dtype=torch.float32, device="cuda").view(torch.int32)
        b = self.buf.view(torch.int32)
        return bool((b[:self.lo] == s).all()) and bool((b[self.hi:] == s).all())

    def bits(self):
        return self.view.view(torch.int32).cpu().numpy().copy()


def host_inputs(P, widths=WIDTHS, seed=0):
    """Per group (p, g, m, v) float32 arrays of P * w elements; the moments are those of a run in progress (non-zero)."""
    rng = np.random.default_rng([seed, P])
    out = []
    for w in widths:
        n = P * w
        out.append((rng.standard_normal(n).astype(np.float32), (rng.standard_normal(n) * 10.0 ** -rng.integers(0, 4, n)).astype(np.float32),
                    (1e-2 * rng.standard_normal(n)).astype(np.float32), (1e-4 * rng.uniform(0.01, 1.0, n)).astype(np.float32)))
    return out


class Device:
    """The groups of one call on the device, each array guarded; ks = float offsets of (param, grad, exp_avg, exp_avg_sq)."""

    def __init__(self, host, ks=(0, 0, 0, 0), lrs=LRS, step=STEP):
        self.arrays = [[Guarded(len(a), k, a) for a, k in zip(grp, ks)] for grp in host]
        self.lrs, self.step = lrs, step

    def groups(self):
        return [_lib.AdamGroup(*(a.view.data_ptr() if a.view.numel() else None for a in grp), grp[0].view.numel(), self.lrs[i % len(self.lrs)], self.step)
                for i, grp in enumerate(self.arrays)]

    def dense(self):
        g = self.groups()
        _lib.check(_lib.load().gsr_adam_step(torch.cuda.current_stream().cuda_stream, len(g), (_lib.AdamGroup * len(g))(*g), BETAS[0], BETAS[1], EPS),
                   "gsr_adam_step")
        return self

    def masked_rc(self, P, mask_ptr, kind, groups=None, n_groups=None):
        g = self.groups() if groups is None else groups
        return _lib.load().gsr_adam_step_masked(torch.cuda.current_stream().cuda_stream, len(g) if n_groups is None else n_groups,
                                                (_lib.AdamGroup * max(1, len(g)))(*g), BETAS[0], BETAS[1], EPS, P, mask_ptr, kind)

    def masked(self, P, mask, kind):
        _lib.check(self.masked_rc(P, mask.data_ptr() or None, kind), "gsr_adam_step_masked")
        return self

    def out(self):
        """int32 views of (param, exp_avg, exp_avg_sq) per group, after a synchronise."""
        torch.cuda.synchronize()
        return [(grp[0].bits(), grp[2].bits(), grp[3].bits()) for grp in self.arrays]

    def all_bits(self):
        torch.cuda.synchronize()
        return [tuple(a.bits() for a in grp) for grp in self.arrays]

    def intact(self):
        return all(a.intact() for grp in self.arrays for a in grp)


def encode(mask, kind):
    """A boolean numpy mask as a device tensor of the kind's dtype; visible rows carry varied legal values, not only 1."""
    mask = np.asarray(mask, dtype=bool)
    r = np.arange(mask.size)
    if kind == "radii":
        return torch.from_numpy(np.where(mask, 1 + (r * 37) % 900, -(r % 2)).astype(np.int32)).cuda()
    return torch.from_numpy(np.where(mask, 1 + (r * 37) % 255, 0).astype(np.uint8)).cuda()


def partial_masks(P):
    rng = np.random.default_rng(P)
    r = np.arange(P)
    first = np.zeros(P, bool); first[0] = True
    last = np.zeros(P, bool); last[-1] = True
    but_one = np.ones(P, bool); but_one[P // 2] = False
    return {"none": np.zeros(P, bool), "first row": first, "last row": last, "all but one": but_one, "alternating": r % 2 == 0,
            "runs of 64 from row 0": (r // 64) % 2 == 0, "runs of 64 from row 1": (r >= 1) & (((r - 1) // 64) % 2 == 0),
            "random 10 %": rng.random(P) < 0.1, "random 50 %": rng.random(P) < 0.5}


def elements(mask, w):
    return np.repeat(np.asarray(mask, dtype=bool), w)


def assert_finite_bits(a, where, what):
    f = a.view(np.float32)[where]
    assert np.isfinite(f).all(), what


# --------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("P", ROWS)
def test_all_rows_visible_equals_the_dense_step_bitwise(P, kind):
    host = host_inputs(P)
    want = Device(host).dense()
    got = Device(host).masked(P, encode(np.ones(P, bool), kind), KINDS[kind])
    for w, a, b in zip(WIDTHS, want.out(), got.out()):
        for name, x, y in zip(("param", "exp_avg", "exp_avg_sq"), a, b):
            assert np.array_equal(x, y), (P, w, name, int((x != y).sum()))
    assert want.intact() and got.intact()
    assert any(not np.array_equal(h[0].view(np.int32), o[0]) for h, o in zip(host, got.out()))       # it did step


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_all_rows_visible_with_one_pointer_off_the_16_byte_boundary(which, k):
    ks = tuple(k if i == which else 0 for i in range(4))
    for P, kind in ((65, "bytes"), (92, "radii"), (1501, "bytes")):
        host = host_inputs(P, seed=1)
        want = Device(host, ks).dense()
        got = Device(host, ks).masked(P, encode(np.ones(P, bool), kind), KINDS[kind])
        for w, a, b in zip(WIDTHS, want.out(), got.out()):
            for name, x, y in zip(("param", "exp_avg", "exp_avg_sq"), a, b):
                assert np.array_equal(x, y), (P, w, name, ks)
        assert want.intact() and got.intact()


# --------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("ks", [(0, 0, 0, 0), (0, 1, 0, 0), (3, 2, 1, 0)], ids=["aligned", "grad off by 1", "all off"])
@pytest.mark.parametrize("P", ROWS)
def test_partial_masks(P, ks):
    """(0, 1, 0, 0) is what the gradient arena's slices look like for an odd number of Gaussians: the scalar body."""
    host = host_inputs(P, seed=2)
    dense = Device(host, ks).dense().out()                                   # computed once, shared by every mask
    inputs = [(h[0].view(np.int32), h[2].view(np.int32), h[3].view(np.int32)) for h in host]
    for mi, (mname, mask) in enumerate(partial_masks(P).items()):
        kind = ("bytes", "radii")[mi % 2] if P != 1501 else ("radii", "bytes")[mi % 2]
        dmask = encode(mask, kind)
        plain = Device(host, ks).masked(P, dmask, KINDS[kind])
        # the same with every element of every invisible row, in all four arrays, a NaN with a payload, +-Inf, -0.0 or a denormal
        planted = []
        for w, grp in zip(WIDTHS, host):
            inv = ~elements(mask, w)
            fill = SPECIALS[np.arange(inv.sum()) % len(SPECIALS)]
            new = []
            for ai, a in enumerate(grp):
                b = a.view(np.int32).copy()
                b[inv] = np.roll(fill, ai)
                new.append(b.view(np.float32))
            planted.append(tuple(new))
        special = Device(planted, ks).masked(P, dmask, KINDS[kind])
        out_plain, out_special, all_special = plain.out(), special.out(), special.all_bits()
        for gi, w in enumerate(WIDTHS):
            vis = elements(mask, w)
            for ai, name in enumerate(("param", "exp_avg", "exp_avg_sq")):
                got, spc = out_plain[gi][ai], out_special[gi][ai]
                assert np.array_equal(got[vis], dense[gi][ai][vis]), (P, w, mname, kind, name, "a visible row differs from the dense step")
                assert np.array_equal(got[~vis], inputs[gi][ai][~vis]), (P, w, mname, kind, name, "an invisible row changed")
                assert np.array_equal(spc[vis], got[vis]), (P, w, mname, kind, name, "a special value of an invisible row reached a visible one")
                assert_finite_bits(spc, vis, (P, w, mname, name))
            for ai in range(4):                                              # all four arrays of the planted run: invisible rows bit for bit
                assert np.array_equal(all_special[gi][ai][~vis], planted[gi][ai].view(np.int32)[~vis]), (P, w, mname, kind, ai)
        assert plain.intact() and special.intact(), (P, mname, "an element outside the tensor was written")


# --------------------------------------------------------------------------------------------- 3
def check_against(host, dense, got, visible):
    for (w, h), d, o in zip(zip([3, 4, 45], host), dense, got):
        vis = elements(visible, w)
        for ai, hi in ((0, 0), (1, 2), (2, 3)):
            assert np.array_equal(o[ai][vis], d[ai][vis]) and np.array_equal(o[ai][~vis], h[hi].view(np.int32)[~vis]), (w, ai)


def test_mask_encodings():
    P, widths = 131, [3, 4, 45]
    host = host_inputs(P, widths, seed=3)
    dense = Device(host).dense().out()
    r = np.arange(P)
    # bytes 0 / 1 / 2 / 255
    vals = np.array([0, 1, 2, 255], dtype=np.uint8)[(r * 7 + r // 4) % 4]
    assert set(vals.tolist()) == {0, 1, 2, 255}
    d = Device(host).masked(P, torch.from_numpy(vals).cuda(), _lib.ADAM_MASK_BYTES)
    check_against(host, dense, d.out(), vals != 0)
    # torch.bool
    b = torch.from_numpy(r % 3 == 1).cuda()
    assert b.dtype == torch.bool
    d = Device(host).masked(P, b, _lib.ADAM_MASK_BYTES)
    check_against(host, dense, d.out(), r % 3 == 1)
    # int32 -3 / 0 / 1 / 2^31 - 1
    iv = np.array([-3, 0, 1, 2 ** 31 - 1], dtype=np.int32)[(r * 5 + r // 4) % 4]
    assert set(iv.tolist()) == {-3, 0, 1, 2 ** 31 - 1}
    d = Device(host).masked(P, torch.from_numpy(iv).cuda(), _lib.ADAM_MASK_RADII)
    check_against(host, dense, d.out(), iv > 0)
    # a byte mask at an odd address, between bytes that would make every row visible
    buf = torch.full((P + 8,), 255, dtype=torch.uint8, device="cuda")
    odd = buf[1:1 + P] if buf.data_ptr() % 2 == 0 else buf[2:2 + P]
    odd.copy_(torch.from_numpy(vals).cuda())
    assert odd.data_ptr() % 2 == 1
    d = Device(host).masked(P, odd, _lib.ADAM_MASK_BYTES)
    check_against(host, dense, d.out(), vals != 0)
    assert d.intact()


# --------------------------------------------------------------------------------------------- 4
REF_WIDTHS = [3, 3, 45, 1, 3, 4]                  # the reference's six groups at M = 16
REF_LRS = [0.00016, 0.0025, 0.000125, 0.05, 0.005, 0.001]


def run_steps(name, P, ks, steps, preset=None, grad_scale=1.0, all_clear=False, stream=None):
    """HipSparseAdam on guarded storage, the float32 torch yardstick and float64, `steps` steps with a fresh mask each."""
    from gaussian_transformer_amd.optim import HipSparseAdam
    lens = [P * w for w in REF_WIDTHS]
    p0 = aux_inputs.adam_params(lens, seed=len(name))
    step0, m0, v0 = preset if preset is not None else (0, [None] * len(lens), [None] * len(lens))
    hyper = dict(betas=BETAS, eps=EPS)
    masks = [np.zeros(P, bool)] * steps if all_clear else fresh_masks(P, steps, seed=len(name))
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        hp = [Guarded(n, ks[0], p) for n, p in zip(lens, p0)]
        hg = [Guarded(n, ks[1]) for n in lens]
        hm = [Guarded(n, ks[2], m) for n, m in zip(lens, m0)]
        hv = [Guarded(n, ks[3], v) for n, v in zip(lens, v0)]
        params = [g.view.view(P, w).detach().requires_grad_(True) for g, w in zip(hp, REF_WIDTHS)]
        opt = HipSparseAdam([dict(params=[p], lr=lr, **hyper) for p, lr in zip(params, REF_LRS)])
        if preset is not None:
            for p, M, V, w in zip(params, hm, hv, REF_WIDTHS):
                opt.state[p] = dict(step=step0, exp_avg=M.view.view(P, w), exp_avg_sq=V.view.view(P, w))
        tor = TorchMaskedAdam([p.reshape(P, w) for p, w in zip(p0, REF_WIDTHS)], [dict(lr=lr, **hyper) for lr in REF_LRS], device="cuda",
                              preset=preset)
        ref = [SparseAdam64(p.reshape(P, w), m, v, step0) for p, w, m, v in zip(p0, REF_WIDTHS, m0, v0)]
        for t in range(steps):
            gs = [g * np.float32(grad_scale) for g in aux_inputs.adam_grads(lens, t, seed=len(name) + 1)]
            kind = ("bytes", "radii")[t % 2]
            for p, G, g, w in zip(params, hg, gs, REF_WIDTHS):
                G.view.copy_(torch.from_numpy(g))
                p.grad = G.view.view(P, w)
            opt.step(visibility=encode(masks[t], kind))
            tor.step([g.reshape(P, w) for g, w in zip(gs, REF_WIDTHS)], masks[t])
            for r, g, lr in zip(ref, gs, REF_LRS):
                r.update(g, masks[t], lr, **hyper)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    worst = dict(param=(0.0, 0.0), exp_avg=(0.0, 0.0), exp_avg_sq=(0.0, 0.0))
    for i, w in enumerate(REF_WIDTHS):
        assert all(G.intact() for G in (hp[i], hg[i], hm[i], hv[i])), (name, i, "an element outside the tensor was written")
        hst, tst = opt.state[params[i]], tor.state(i)
        assert sorted(hst) == ["exp_avg", "exp_avg_sq", "step"]
        assert int(hst["step"]) == int(tst["step"]) == ref[i].step == step0 + steps
        for key, h, tt, r in (("param", params[i], tor.params[i], ref[i].p), ("exp_avg", hst["exp_avg"], tst["exp_avg"], ref[i].m),
                              ("exp_avg_sq", hst["exp_avg_sq"], tst["exp_avg_sq"], ref[i].v)):
            h = h.detach().cpu().numpy().reshape(-1).astype(np.float64); tt = tt.detach().cpu().numpy().reshape(-1).astype(np.float64)
            r = r.reshape(-1)
            assert np.isfinite(h).all(), (name, i, key)
            scale = np.abs(r).max()
            if scale == 0:                                                  # nothing was ever visible: the moments stay exactly 0
                assert (h == 0).all(), (name, i, key)
                continue
            eh, et = np.abs(h - r).max() / scale, np.abs(tt - r).max() / scale
            if eh - 2 * et > worst[key][0] - 2 * worst[key][1] or worst[key] == (0.0, 0.0):
                worst[key] = (eh, et)
            assert eh <= 2 * et + 4 * U, (name, i, w, key, eh / U, et / U)
    print(f"ADAM_SPARSE {name:34s} " + "  ".join(f"{k} {a / U:6.2f}/{b / U:6.2f}" for k, (a, b) in worst.items()))
    return params, opt, p0, masks


@pytest.mark.parametrize("P,ks", [(333, (0, 0, 0, 0)), (333, (0, 1, 0, 0)), (1501, (0, 0, 0, 0)), (92, (1, 2, 3, 0))])
def test_several_steps_with_a_fresh_mask_each_against_float64(P, ks):
    params, opt, p0, masks = run_steps(f"P={P} ks={ks}", P, ks, aux_inputs.ADAM_STEPS)
    seen = np.logical_or.reduce(masks)
    assert (~seen).any() and seen.any() and (seen & ~np.logical_or.reduce(masks[:8])).any()          # never visible; first seen late
    for p, q, w in zip(params, p0, REF_WIDTHS):                             # rows never visible: parameter and moments exactly initial
        never = elements(~seen, w)
        st = opt.state[p]
        assert np.array_equal(p.detach().cpu().numpy().reshape(-1).view(np.int32)[never], q.view(np.int32)[never])
        assert not st["exp_avg"].reshape(-1)[torch.from_numpy(never).cuda()].any() and not st["exp_avg_sq"].reshape(-1)[torch.from_numpy(never).cuda()].any()


def test_bias_corrections_at_the_end_of_a_30k_run():
    P = 333
    rng = np.random.default_rng(3)
    lens = [P * w for w in REF_WIDTHS]
    m0 = [(1e-3 * rng.standard_normal(n)).astype(np.float32) for n in lens]
    v0 = [(1e-6 * rng.uniform(0.01, 1, n)).astype(np.float32) for n in lens]
    _, opt, _, _ = run_steps("step 29 999 + 3", P, (0, 1, 0, 0), 3, preset=(29999, m0, v0), grad_scale=1e-3)
    assert all(int(s["step"]) == 30002 for s in opt.state.values())


def test_all_clear_masks_leave_the_moments_exactly_zero():
    params, opt, p0, _ = run_steps("all clear", 333, (0, 0, 0, 0), 3, all_clear=True)
    for p, q in zip(params, p0):
        st = opt.state[p]
        assert np.array_equal(p.detach().cpu().numpy().reshape(-1).view(np.int32), q.view(np.int32))
        assert int(st["step"]) == 3 and not st["exp_avg"].any() and not st["exp_avg_sq"].any()


# --------------------------------------------------------------------------------------------- 5
def optimisers(P, widths, ks_of, groups_of, with_grad=lambda i: True, seed=5, step0=6):
    """HipAdam and HipSparseAdam over identical guarded copies of the same tensors, state preset at step0."""
    from gaussian_transformer_amd.optim import HipAdam, HipSparseAdam
    host = host_inputs(P, widths, seed=seed)
    out = []
    for cls in (HipAdam, HipSparseAdam):
        dev = [[Guarded(len(a), k, a) for a, k in zip(grp, ks_of(i))] for i, grp in enumerate(host)]
        params = [grp[0].view.view(P, w).detach().requires_grad_(True) for grp, w in zip(dev, widths)]
        opt = cls([dict(params=[p], **groups_of(i)) for i, p in enumerate(params)])
        for i, (p, grp, w) in enumerate(zip(params, dev, widths)):
            if with_grad(i):
                p.grad = grp[1].view.view(P, w)
                opt.state[p] = dict(step=step0, exp_avg=grp[2].view.view(P, w), exp_avg_sq=grp[3].view.view(P, w))
        out.append((opt, params, dev))
    return host, out


def assert_one_step_matches(host, dense, sparse, widths, mask, with_grad=lambda i: True, step0=6):
    (dopt, dparams, ddev), (sopt, sparams, sdev) = dense, sparse
    torch.cuda.synchronize()
    for i, w in enumerate(widths):
        assert all(a.intact() for a in ddev[i] + sdev[i])
        if not with_grad(i):
            assert len(sopt.state.get(sparams[i], {})) == 0
            assert all(np.array_equal(a.bits(), h.view(np.int32)) for a, h in zip(sdev[i], host[i]))
            continue
        assert sorted(sopt.state[sparams[i]]) == ["exp_avg", "exp_avg_sq", "step"] and int(sopt.state[sparams[i]]["step"]) == step0 + 1
        vis = elements(mask, w)
        for ai in (0, 2, 3):
            got, want, before = sdev[i][ai].bits(), ddev[i][ai].bits(), host[i][ai].view(np.int32)
            assert np.array_equal(got[vis], want[vis]) and np.array_equal(got[~vis], before[~vis]), (i, w, ai)


def test_visibility_none_is_hip_adam_and_an_empty_mask_still_counts_the_step():
    P, widths = 257, [3, 45, 1, 4]
    host, (dense, sparse) = optimisers(P, widths, lambda i: (0, i % 2, 0, 0), lambda i: dict(lr=LRS[i], betas=BETAS, eps=EPS))
    dense[0].step(); sparse[0].step()
    assert_one_step_matches(host, dense, sparse, widths, np.ones(P, bool))
    before = [[a.bits() for a in grp] for grp in sparse[2]]
    torch.cuda.synchronize()
    sparse[0].step(visibility=torch.zeros(P, dtype=torch.bool, device="cuda"))
    sparse[0].step(visibility=torch.zeros(P, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    for p, grp, b in zip(sparse[1], sparse[2], before):
        assert int(sparse[0].state[p]["step"]) == 6 + 3
        assert all(np.array_equal(a.bits(), x) for a, x in zip(grp, b))


@pytest.mark.parametrize("n_groups", [_lib.ADAM_MAX_GROUPS + 1, 2 * _lib.ADAM_MAX_GROUPS + 3])
def test_more_groups_than_one_launch_takes(n_groups):
    P = 91
    widths = [WIDTHS[(3 * i) % len(WIDTHS)] for i in range(n_groups)]
    ks_of = lambda i: ((i % 4), (i // 2) % 4, 0, (i % 3)) if i % 3 else (0, 0, 0, 0)
    host, (dense, sparse) = optimisers(P, widths, ks_of, lambda i: dict(lr=LRS[i % len(LRS)], betas=BETAS, eps=EPS))
    mask = np.random.default_rng(n_groups).random(P) < 0.4
    dense[0].step(); sparse[0].step(visibility=encode(mask, "radii"))
    assert_one_step_matches(host, dense, sparse, widths, mask)


def test_groups_with_different_betas_and_eps_and_a_tensor_without_gradient():
    P, widths = 65, [3, 45, 9, 4, 1, 3]
    hyper = [dict(lr=0.0025, betas=(0.9, 0.999), eps=1e-15), dict(lr=0.01, betas=(0.8, 0.99), eps=1e-8), dict(lr=0.001, betas=(0.9, 0.999), eps=1e-8),
             dict(lr=0.02, betas=(0.5, 0.9), eps=1e-15), dict(lr=0.01, betas=(0.8, 0.99), eps=1e-8), dict(lr=0.0025, betas=(0.9, 0.999), eps=1e-15)]
    with_grad = lambda i: i != 2
    host, (dense, sparse) = optimisers(P, widths, lambda i: (0, 0, 0, 0), lambda i: hyper[i], with_grad=with_grad)
    mask = np.arange(P) % 3 != 0
    dense[0].step(); sparse[0].step(visibility=encode(mask, "bytes").bool())
    assert_one_step_matches(host, dense, sparse, widths, mask, with_grad=with_grad)
    assert len({(tuple(g["betas"]), g["eps"]) for g in sparse[0].param_groups}) == 4


def test_no_gaussians_at_all():
    from gaussian_transformer_amd.optim import HipSparseAdam
    ps = [torch.zeros((0, w), device="cuda", requires_grad=True) for w in (3, 45, 1)]
    opt = HipSparseAdam([dict(params=[p], lr=0.01) for p in ps], betas=BETAS, eps=EPS)
    for kind in (torch.bool, torch.int32, torch.uint8):
        for p in ps:
            p.grad = torch.zeros_like(p)
        opt.step(visibility=torch.zeros(0, dtype=kind, device="cuda"))
    torch.cuda.synchronize()
    assert all(int(opt.state[p]["step"]) == 3 and opt.state[p]["exp_avg"].shape == p.shape for p in ps)


def test_whole_run_on_a_second_stream_repeats_the_first_bit_for_bit():
    s = torch.cuda.Stream()
    assert s.cuda_stream != torch.cuda.default_stream().cuda_stream
    torch.cuda.synchronize()
    a, aopt, _, _ = run_steps("a second stream", 333, (0, 1, 0, 0), 6)
    b, bopt, _, _ = run_steps("a second stream", 333, (0, 1, 0, 0), 6, stream=s)
    for p, q in zip(a, b):                                                  # no atomics: a given mask gives the same bits on every run
        assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32))
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(aopt.state[p][key].view(torch.int32), bopt.state[q][key].view(torch.int32))


# --------------------------------------------------------------------------------------------- 6
def test_refusals_from_python_leave_everything_as_it_was():
    P, widths = 65, [3, 4]
    host, (_, sparse) = optimisers(P, widths, lambda i: (0, 0, 0, 0), lambda i: dict(lr=0.01, betas=BETAS, eps=EPS))
    opt, params, dev = sparse
    other = Guarded(66 * 3, 0, np.ones(66 * 3, np.float32))
    ok = torch.ones(P, dtype=torch.bool, device="cuda")
    bad = {"float mask": torch.ones(P, device="cuda"), "int64 mask": torch.ones(P, dtype=torch.int64, device="cuda"),
           "2-D mask": torch.ones((P, 1), dtype=torch.bool, device="cuda"), "CPU mask": torch.ones(P, dtype=torch.bool),
           "strided mask": torch.ones(2 * P, dtype=torch.bool, device="cuda")[::2],
           "wrong length": torch.ones(P + 1, dtype=torch.bool, device="cuda"), "empty": torch.ones(0, dtype=torch.int32, device="cuda")}
    for name, vis in bad.items():
        with pytest.raises(_lib.GsrError, match="visibility") as e:
            opt.step(visibility=vis)
        assert str(e.value), name
    # one parameter among several with another number of rows: named, and refused before the others are stepped
    q = other.view.view(66, 3).detach().requires_grad_(True)
    q.grad = torch.ones_like(q)
    opt.add_param_group(dict(params=[q], lr=0.01, name="odd one out"))
    with pytest.raises(_lib.GsrError, match=r"odd one out.*\(66, 3\).*65 rows"):
        opt.step(visibility=ok)
    torch.cuda.synchronize()
    for grp, h in zip(dev, host):
        assert all(np.array_equal(a.bits(), x.view(np.int32)) and a.intact() for a, x in zip(grp, h))
    assert all(int(opt.state[p]["step"]) == 6 for p in params) and len(opt.state.get(q, {})) == 0 and other.intact()
    assert (other.view == 1).all()


def test_refusals_through_ctypes_leave_everything_as_it_was():
    P = 65
    host = host_inputs(P, [3, 4], seed=6)
    d = Device(host)
    lib = _lib.load()
    mask8, mask32 = encode(np.ones(P, bool), "bytes"), torch.ones(P + 1, dtype=torch.int32, device="cuda")
    g = d.groups()
    G = _lib.AdamGroup

    def with_(k, **kw):
        f = {n: getattr(g[k], n) for n, _ in G._fields_}
        f.update(kw)
        out = list(g)
        out[k] = G(*(f[n] for n, _ in G._fields_))
        return out
    cases = {
        "0 groups": dict(P=P, mask_ptr=mask8.data_ptr(), kind=0, n_groups=0),
        "17 groups": dict(P=P, mask_ptr=mask8.data_ptr(), kind=0, groups=[g[0]] * 17),
        "P < 0": dict(P=-P, mask_ptr=mask8.data_ptr(), kind=0),
        "NULL mask": dict(P=P, mask_ptr=None, kind=0),
        "unknown kind": dict(P=P, mask_ptr=mask8.data_ptr(), kind=2),
        "int32 mask off a 4-byte boundary": dict(P=P, mask_ptr=mask32.data_ptr() + 2, kind=1),
        "n no multiple of P": dict(P=P - 1, mask_ptr=mask8.data_ptr(), kind=0),
        "n beyond 2^31 - 1": dict(P=1, mask_ptr=mask8.data_ptr(), kind=0, groups=with_(1, n=2 ** 31)),
        "NULL param": dict(P=P, mask_ptr=mask8.data_ptr(), kind=0, groups=with_(1, param=None)),
        "NULL grad": dict(P=P, mask_ptr=mask8.data_ptr(), kind=0, groups=with_(0, grad=None)),
        "NULL exp_avg": dict(P=P, mask_ptr=mask8.data_ptr(), kind=0, groups=with_(1, exp_avg=None)),
        "NULL exp_avg_sq": dict(P=P, mask_ptr=mask8.data_ptr(), kind=0, groups=with_(1, exp_avg_sq=None)),
    }
    for name, kw in cases.items():
        rc = d.masked_rc(**kw)
        text = lib.gsr_last_error().decode()
        assert rc == 1 and text.startswith("gsr_adam_step_masked:") and len(text) > 25, (name, rc, text)
        with pytest.raises(_lib.GsrError, match="gsr_adam_step_masked"):
            _lib.check(rc, "gsr_adam_step_masked")
    for grp, h in zip(d.all_bits(), host):
        assert all(np.array_equal(a, x.view(np.int32)) for a, x in zip(grp, h))
    assert d.intact()
    # and the legal edges: P = 0 with empty groups, n = 0 beside a real group
    assert d.masked_rc(P=0, mask_ptr=None, kind=1, groups=[G(None, None, None, None, 0, 0.1, 1)]) == 0
    assert d.masked_rc(P=P, mask_ptr=mask8.data_ptr(), kind=0, groups=[G(None, None, None, None, 0, 0.1, 1)] + g) == 0
    want = Device(host).dense().out()
    assert all(np.array_equal(x, y) for a, b in zip(want, d.out()) for x, y in zip(a, b))


# --------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("fused", [False, True], ids=["DensityController", "FusedDensityController"])
def test_density_control_with_the_sparse_optimiser(fused):
    from gaussian_transformer_amd.densify import GROUPS, DensityController, FusedDensityController
    from gaussian_transformer_amd.optim import HipSparseAdam
    from tests import density_ref as dr
    from tests.test_density_host import STEP as STEP0, make_controller
    P = 257
    ctl = make_controller(dr.clone_inputs(dr.build_inputs(P, 3), "cuda"), cls=FusedDensityController if fused else DensityController, adam="hip_sparse")
    assert type(ctl.optimizer) is HipSparseAdam
    par = lambda: {g["name"]: g["params"][0] for g in ctl.optimizer.param_groups}

    def give_gradients():
        for g in ctl.optimizer.param_groups:
            g["params"][0].grad = torch.full_like(g["params"][0], 0.5)
            g["lr"] = 1e-3
    # an iteration with a densification: backward, then densify_and_prune, then the step with the mask of the render before it
    give_gradients()
    radii = torch.from_numpy(((np.arange(P) % 3 == 0) * 7).astype(np.int32)).cuda()
    with torch.no_grad():
        counts = ctl.densify_and_prune(dr.THRESHOLD, dr.MIN_OPACITY, dr.EXTENT, 20, generator=torch.Generator(device="cuda").manual_seed(5))
    P_new = ctl.model._xyz.shape[0]
    assert P_new != P and counts["cloned"] > 0 and counts["split"] > 0 and all(p.shape[0] == P_new and p.grad is None for p in par().values())
    snap = {n: (p.detach().clone(), ctl.optimizer.state[p]["exp_avg"].clone(), ctl.optimizer.state[p]["exp_avg_sq"].clone()) for n, p in par().items()}
    # the appended rows (clones and split children that survived the pruning) are the tail, and the only rows whose moments are 0
    zero = ~snap["xyz"][2].reshape(P_new, -1).any(dim=1)
    appended = int(zero.sum())
    assert 0 < appended <= counts["cloned"] + 2 * counts["split"] and bool(zero[P_new - appended:].all())
    ctl.optimizer.step(visibility=radii)                                     # stale mask of the old P: nothing has a gradient, nothing happens
    torch.cuda.synchronize()
    for n, p in par().items():
        st = ctl.optimizer.state[p]
        assert float(st["step"]) == STEP0 and torch.equal(p.detach(), snap[n][0]) and torch.equal(st["exp_avg"], snap[n][1]) and torch.equal(st["exp_avg_sq"], snap[n][2])
        assert st["exp_avg"].shape == p.shape == st["exp_avg_sq"].shape
        assert not st["exp_avg"][P_new - appended:].any() and not st["exp_avg_sq"][P_new - appended:].any(), n
        assert bool(st["exp_avg_sq"][:P_new - appended].reshape(P_new - appended, -1).any(dim=1).all()), n
    # the next iteration: gradients and a mask of the new length
    give_gradients()
    with pytest.raises(_lib.GsrError, match="rows of visibility"):
        ctl.optimizer.step(visibility=radii)                                 # the old mask is now refused, before anything moves
    vis = np.arange(P_new) % 2 == 1
    vis[P_new - appended:] = np.arange(appended) % 2 == 0
    ctl.optimizer.step(visibility=torch.from_numpy(vis).cuda())
    torch.cuda.synchronize()
    tv = torch.from_numpy(vis).cuda()
    for n, p in par().items():
        st = ctl.optimizer.state[p]
        assert float(st["step"]) == STEP0 + 1, n
        assert torch.equal(p.detach()[~tv], snap[n][0][~tv]) and torch.equal(st["exp_avg"][~tv], snap[n][1][~tv]), n
        assert (p.detach()[tv] != snap[n][0][tv]).any() and (st["exp_avg_sq"][tv] > 0).all(), n
        assert not st["exp_avg"][P_new - appended:][~tv[P_new - appended:]].any(), n
        assert bool(torch.isfinite(p.detach()).all())
    assert set(par()) == set(GROUPS)
