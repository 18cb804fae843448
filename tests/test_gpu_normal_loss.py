"""-m gpu: the fused depth-normal consistency loss (include/gsr_normals.h: gsr_normal_loss_*) against tests/normals_ref.py.

Sizes: four without an interior; one stencil; T - 1, T, T + 1 and 2 T + 1 of the kernels' 32 x 8 tile in both axes, where the halo and the
gather cross tile borders; 160 x 96.  Inputs per size: a smooth noisy depth field without and with alpha holes, and the tilted plane.
tests/test_normals_ref_host.py asserts that none of them holds a pixel whose validity could round either way, so the valid fraction and
the zeros of out_surf are held to the float64 reference exactly.

Tolerance of every value compared: max |x - x64| / max |x64| <= 2 e32 + 1e-7, with e32 the same measure of the float32 torch formulation
on the same inputs, computed here.  The kernels do their per-pixel arithmetic in float64 and round once, so the measured ratios
(printed) lie far below 1.
"""
import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib, loss
from gaussian_transformer_amd.model import GaussianParams
from gaussian_transformer_amd.render import PipelineParams, TorchCamera, render
from gaussian_transformer_amd import synth
from tests import normals_ref as nr
from tests.helpers import F32_P99_MAX, GRAD_RTOL, grad_rows
from tests.test_normals_ref_host import GPU_SIZES, NO_INTERIOR

pytestmark = pytest.mark.gpu
DEV = "cuda"
TX, TY = nr.TANFOV
KINDS = ("smooth", "holes", "plane")


def inputs(H, W, kind):
    if kind == "plane":
        return nr.plane(H, W, dtype=np.float32)[:3]
    return nr.maps(H, W, holes=kind == "holes")


_refs = {}


def reference(H, W, kind):
    """(inputs, float64 result, float32 result) of one case: computed once, shared, never changed."""
    key = (H, W, kind)
    if key not in _refs:
        x = inputs(H, W, kind)
        _refs[key] = (x, nr.loss(*x, TX, TY, dtype=torch.float64), nr.loss(*x, TX, TY, dtype=torch.float32))
    return _refs[key]


def dev(a):
    return torch.tensor(np.asarray(a, np.float32), device=DEV)


def forward(d, a, n, surf=True, alpha_min=nr.ALPHA_MIN, fill=float("nan")):
    H, W = d.shape
    ws = _lib.workspace("gsr_normal_loss_workspace", d.device, H, W)
    out2 = torch.full((2,), fill, device=DEV)
    s = torch.full((3, H, W), fill, device=DEV) if surf else None
    _lib.call("gsr_normal_loss_forward", _lib.stream(d.device), H, W, TX, TY, alpha_min, _lib.ptr(d), _lib.ptr(a), _lib.ptr(n),
              _lib.ptr(out2), None if s is None else s.data_ptr(), _lib.ptr(ws), ws.numel())
    return out2, s


def backward(d, a, n, want=(True, True, True), grad_loss=None, fill=float("nan"), tan=(TX, TY)):
    H, W = d.shape
    outs = [torch.full(shape, fill, device=DEV) if w else None for w, shape in zip(want, ((H, W), (H, W), (3, H, W)))]
    g = None if grad_loss is None else torch.tensor([grad_loss], device=DEV)
    _lib.call("gsr_normal_loss_backward", _lib.stream(d.device), H, W, tan[0], tan[1], nr.ALPHA_MIN, _lib.ptr(d), _lib.ptr(a), _lib.ptr(n),
              None if g is None else g.data_ptr(), *(None if o is None else o.data_ptr() for o in outs))
    return outs


def rel(x, x64):
    x, x64 = np.asarray(x, np.float64), np.asarray(x64, np.float64)
    scale = np.abs(x64).max(initial=0.0)
    return float(np.abs(x - x64).max(initial=0.0) / scale) if scale > 0 else float(np.abs(x).max(initial=0.0))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hw", GPU_SIZES, ids=[f"{h}x{w}" for h, w in GPU_SIZES])
def test_against_float64_within_twice_the_float32_formulation(hw, kind):
    H, W = hw
    x, r64, r32 = reference(H, W, kind)
    d, a, n = (dev(t) for t in x)
    out2, surf = forward(d, a, n)
    gd, ga, gn = backward(d, a, n)
    torch.cuda.synchronize()
    got = dict(loss=out2[0:1].cpu().numpy(), surf=surf.cpu().numpy(), g_depth=gd.cpu().numpy(), g_alpha=ga.cpu().numpy(), g_normals=gn.cpu().numpy())
    for v in got.values():
        assert np.isfinite(v).all()                                   # the NaN the buffers held is gone: zeros are written
    # the decisions: exactly the reference's
    assert float(out2[1]) == np.float32(r64["fraction"]) and r64["fraction"] == r32["fraction"]
    valid = r64["valid"].numpy()
    assert not got["surf"][:, ~valid].any()
    if not valid.any():                # no interior -- or, at 3 x 3, a hole on the one stencil: everything is zero
        assert hw in NO_INTERIOR or (kind == "holes" and hw == (3, 3))
        assert float(out2[0]) == 0.0 and not any(got[k].any() for k in ("surf", "g_depth", "g_alpha", "g_normals"))
        return
    assert hw not in NO_INTERIOR
    # gradients are zero where no valid stencil reaches
    assert not got["g_normals"][:, ~valid].any()
    ratios = {}
    for k, v in got.items():
        w64 = np.asarray(r64[k], np.float64).reshape(v.shape)
        e, e32 = rel(v, w64), rel(np.asarray(r32[k], np.float64).reshape(v.shape), w64)
        ratios[k] = (e, e32)
        assert e <= 2.0 * e32 + 1e-7, (k, e, e32)
    print(f"{H}x{W} {kind}: " + "  ".join(f"{k} {e:.2e}/{e32:.2e}" for k, (e, e32) in ratios.items()))


@pytest.mark.parametrize("hw", [(3, 3), (2 * 8 + 1, 2 * 32 + 1), (96, 160)], ids=["3x3", "17x65", "96x160"])
def test_null_outputs_scaling_and_determinism(hw):
    H, W = hw
    x, _r64, _r32 = reference(H, W, "smooth" if hw == (3, 3) else "holes")      # (the 3 x 3 image's hole leaves no stencil)
    d, a, n = (dev(t) for t in x)
    full = backward(d, a, n)
    out2, surf = forward(d, a, n)
    # two runs are bit-identical
    again = backward(d, a, n)
    out2b, surfb = forward(d, a, n)
    assert all(torch.equal(p, q) for p, q in zip(full, again)) and torch.equal(out2, out2b) and torch.equal(surf, surfb)
    # every NULL combination leaves the other outputs as they are, bit for bit
    for mask in range(1, 7):
        want = tuple(bool(mask & (1 << i)) for i in range(3))
        part = backward(d, a, n, want=want)
        for w, p, f in zip(want, part, full):
            assert (p is None) == (not w) and (p is None or torch.equal(p, f)), (want,)
    out2c, none = forward(d, a, n, surf=False)
    assert none is None and torch.equal(out2c, out2)
    # a power of two scales exactly; NULL is 1
    quarter = backward(d, a, n, grad_loss=0.25)
    one = backward(d, a, n, grad_loss=1.0)
    assert all(torch.equal(q, f * 0.25) for q, f in zip(quarter, full)) and all(torch.equal(o, f) for o, f in zip(one, full))
    assert any(bool(f.any()) for f in full)


def test_the_python_functions_are_the_c_calls():
    H, W = 17, 65
    x, r64, _ = reference(H, W, "holes")
    d, a, n = (dev(t).requires_grad_(True) for t in x)
    L = loss.normal_consistency_loss(d[None], a[None], n, TX, TY)
    out2, surf = forward(d.detach(), a.detach(), n.detach())
    assert torch.equal(L.detach(), out2[0]) and torch.equal(L.valid_fraction, out2[1]) and not L.valid_fraction.requires_grad
    (L * 0.5).backward()
    want = backward(d.detach(), a.detach(), n.detach(), grad_loss=0.5)
    assert torch.equal(d.grad, want[0]) and torch.equal(a.grad, want[1]) and torch.equal(n.grad, want[2])
    s = loss.surface_normals(d, a[None], TX, TY)
    assert torch.equal(s, surf) and not s.requires_grad
    # only the maps that ask receive a gradient
    d2, n2 = d.detach().clone().requires_grad_(True), n.detach().clone()
    loss.normal_consistency_loss(d2, a.detach(), n2, TX, TY).backward()
    assert torch.equal(d2.grad, backward(d.detach(), a.detach(), n.detach())[0]) and n2.grad is None


def test_one_backward_through_a_real_render_is_the_sum_of_the_map_gradients_pushed_through():
    sc = synth.make_scene(P=2000, width=160, height=96, sh_degree=1, s0=0.05, seed=4)
    cam = TorchCamera(sc.camera, DEV)
    bg = torch.zeros(3, device=DEV)
    tx, ty = sc.camera.tanfovx, sc.camera.tanfovy
    names = ("_xyz", "_opacity", "_scaling", "_rotation")

    pc = GaussianParams.from_synthetic(sc, DEV)
    out = render(cam, pc, PipelineParams(), bg, depth="expected", normals=True)
    L = loss.normal_consistency_loss(out["depth"], out["alpha"], out["normals"], tx, ty)
    assert 0.0 < float(L.valid_fraction) <= 1.0 and float(L.detach()) > 0
    L.backward()
    got = {k: getattr(pc, k).grad.cpu().numpy() for k in names}
    for k, g in got.items():
        assert np.isfinite(g).all() and np.abs(g).max() > 0, k

    # the same maps' gradients from the C call, pushed through the existing passes of a second, identical render
    pc2 = GaussianParams.from_synthetic(sc, DEV)
    out2 = render(cam, pc2, PipelineParams(), bg, depth="expected", normals=True)
    assert torch.equal(out2["normals"], out["normals"]) and torch.equal(out2["depth"], out["depth"])
    gd, ga, gn = backward(out2["depth"][0].detach().contiguous(), out2["alpha"][0].detach().contiguous(), out2["normals"].detach().contiguous(),
                          tan=(tx, ty))
    ((out2["depth"][0] * gd).sum() + (out2["alpha"][0] * ga).sum() + (out2["normals"] * gn).sum()).backward()
    for k in names:
        st = grad_rows(got[k], getattr(pc2, k).grad.cpu().numpy())     # float atomics land in another order from run to run: close, not bit-equal
        assert st["p99"] <= F32_P99_MAX and st["max"] <= GRAD_RTOL, (k, st)
