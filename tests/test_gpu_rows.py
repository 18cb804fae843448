"""-m gpu: the row glue (include/gsr_rows.h, gaussian_transformer_amd/rows.py).  gsr_rows_unpack and gsr_rows_grad_pack through
ctypes against tests/rows_ref.py bit for bit (sizes around the 64-row tile, every row width class, aligned and unaligned bases,
guard bands), their refusals, and render_rows against `render_fused(cam, unflatten_gaussians(rows))` per camera: images and radii
equal, the row gradient equal to the per-camera gradients added in camera order under the deterministic reverse pass.
Non-finite values only ever go through unpack and pack, never through the rasterizer."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib, synth
from gaussian_transformer_amd.model import GaussianParams
from gaussian_transformer_amd.render import PipelineParams, TorchCamera, render_fused
from gaussian_transformer_amd.sequence import flatten_gaussians, unflatten_gaussians
from tests import rows_ref as rr

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64
SENTINEL = 0x5A5A5A5A
PS = [1, 63, 64, 65, 1501]
DS = [17, 26, 62]
ORDER = ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"]


def stream():
    return torch.cuda.current_stream().cuda_stream


def up(t):
    """CPU float32 -> device, moved as integers: no value is interpreted on the way."""
    return rr.bits(t).to(DEV).view(torch.float32)


def down_bits(t):
    return rr.bits(t).cpu()


def guarded(numel, offset=0):
    """(store, view): `numel` floats at `offset` floats into a buffer of sentinel words with GUARD more after them."""
    store = torch.full((offset + numel + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    return store, store[offset:offset + numel].view(torch.float32)


def guards_intact(store, numel, offset=0):
    return bool((store[:offset] == SENTINEL).all()) and bool((store[offset + numel:] == SENTINEL).all())


def ptr(t):
    return t.data_ptr() if t.numel() else None


def native_unpack(rows_dev, P, D):
    lib = _lib.load()
    want = rr.unpack_ref(torch.empty((P, D)))            # shapes only
    outs = {k: guarded(want[k].numel()) for k in ORDER}
    K = (D - 14) // 3
    rc = lib.gsr_rows_unpack(stream(), P, D, ptr(rows_dev), *[ptr(outs[k][1]) if (k != "f_rest" or K > 1) else None for k in ORDER])
    return rc, outs


def check_unpack(rows_cpu, rows_dev):
    P, D = rows_cpu.shape
    want = rr.unpack_ref(rows_cpu)
    rc, outs = native_unpack(rows_dev, P, D)
    assert rc == 0, _lib.load().gsr_last_error()
    for k in ORDER:
        store, view = outs[k]
        assert torch.equal(down_bits(view), rr.bits(want[k]).reshape(-1)), k
        assert guards_intact(store, want[k].numel()), k


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("P", PS)
def test_unpack_is_a_bit_copy(P, D):
    rows = rr.planted_rows(P, D, seed=1000 + P + D)
    check_unpack(rows, up(rows))


def test_unpack_and_pack_from_bases_that_are_only_4_byte_aligned():
    """rows / grad_rows one float past a 16-byte boundary: the tile is moved dword by dword."""
    P, D, B = 130, 26, 2
    rows = rr.planted_rows(P, D, seed=5)
    store = torch.zeros((P * D + 1,), device=DEV)
    dev = store[1:].view(P, D)
    dev.copy_(up(rows))
    assert dev.data_ptr() % 16 == 4
    check_unpack(rows, dev)
    arenas = rr.planted_arenas(B, P, D, seed=6)
    got = run_pack(arenas, P, D, out_offset=1)
    assert torch.equal(got, rr.bits(rr.pack_ref(arenas, P, D)))


def run_pack(arenas_cpu, P, D, out_offset=0, expect_rc=0):
    """gsr_rows_grad_pack on device copies of the arenas, arena b starting b % 4 floats into its slot (4-byte alignment is all an
    arena needs).  Returns the bits of grad_rows on the CPU; the guard band behind it is checked."""
    lib = _lib.load()
    B, n = len(arenas_cpu), rr.arena_floats(P, D)
    store = torch.zeros((B, n + 3), device=DEV)
    devs = []
    for b, a in enumerate(arenas_cpu):
        v = store[b, b % 4:b % 4 + n]
        v.copy_(up(a))
        devs.append(v)
    gstore, grad = guarded(P * D, out_offset)
    ptrs = (C.c_void_p * B)(*[v.data_ptr() for v in devs])
    rc = lib.gsr_rows_grad_pack(stream(), P, D, B, ptrs, ptr(grad))
    assert rc == expect_rc, lib.gsr_last_error()
    assert guards_intact(gstore, P * D, out_offset)
    return down_bits(grad).reshape(P, D)


@pytest.mark.parametrize("B", [1, 2, 3, 64])
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("P", PS)
def test_pack_is_the_ordered_sum(P, D, B):
    arenas = rr.planted_arenas(B, P, D, seed=2000 + P + D + B)
    want = rr.pack_ref(arenas, P, D)
    got = run_pack(arenas, P, D)
    assert torch.equal(got, rr.bits(want))
    assert (got[:, D - 3:] == 0).all()                               # flags: +0.0 by bit pattern
    assert (got == -2 ** 31).any()                                   # a -0.0 survived (-0.0 + -0.0 at the shared positions)
    if B == 1:
        off = 0
        for name, col, w in rr.blocks(D):
            assert torch.equal(got[:, col:col + w], rr.bits(arenas[0][off:off + P * w]).reshape(P, w)), name
            off += P * w
    assert torch.equal(run_pack(arenas, P, D), got)                  # run to run


def test_pack_with_nan_and_infinities():
    P, D, B = 257, 26, 3
    arenas = rr.planted_arenas(B, P, D, seed=77, nonfinite=True)
    want = rr.pack_ref(arenas, P, D)
    assert torch.isnan(want).any() and torch.isinf(want).any()
    got = run_pack(arenas, P, D).view(torch.float32)
    assert torch.equal(rr.canonical_nan_bits(got), rr.canonical_nan_bits(want))


def test_empty_input_launches_nothing():
    lib = _lib.load()
    assert lib.gsr_rows_unpack(stream(), 0, 26, None, None, None, None, None, None, None) == 0
    z = torch.zeros(4, device=DEV)
    assert lib.gsr_rows_unpack(stream(), 0, 17, None, None, None, None, None, None, None) == 0
    assert lib.gsr_rows_grad_pack(stream(), 0, 26, 1, (C.c_void_p * 1)(z.data_ptr()), None) == 0
    torch.cuda.synchronize()


def test_refusals_leave_a_message_and_a_usable_device():
    lib = _lib.load()
    P, D, K = 70, 26, 4
    rows = rr.planted_rows(P, D, seed=9)
    dev = up(rows)
    bufs = {k: torch.zeros(v.numel() + 4, device=DEV) for k, v in rr.unpack_ref(rows).items()}
    p = lambda k, off=0: bufs[k].data_ptr() + 4 * off
    arena = torch.zeros(rr.arena_floats(P, D) + P * D, device=DEV)
    grad = torch.zeros(P * D, device=DEV)
    one = (C.c_void_p * 1)(arena.data_ptr())
    many = (C.c_void_p * 65)(*[arena.data_ptr()] * 65)

    def refused(rc, text):
        msg = lib.gsr_last_error().decode()
        assert rc != 0 and text in msg, (rc, msg)

    def unpack(D_=D, rot=None, xyz=None, scaling=None, rest="f_rest"):
        return lib.gsr_rows_unpack(stream(), P, D_, dev.data_ptr(), p("xyz") if xyz is None else xyz, p("f_dc"),
                                   None if rest is None else p(rest), p("opacity"), p("scaling") if scaling is None else scaling,
                                   p("rotation") if rot is None else rot)
    refused(unpack(D_=18), "D=18 is not 3 K + 14")
    refused(unpack(D_=65), "D=65")
    refused(unpack(rot=p("rotation", 1)), "rotation must be 16-byte aligned")
    refused(unpack(rest=None), "f_rest must be NULL if and only if K = 1")
    refused(unpack(xyz=dev.data_ptr() + 4 * (P * D - 1)), "xyz overlaps rows")                  # the last float of rows
    refused(unpack(scaling=dev.data_ptr() - 4 * (3 * P - 1)), "scaling overlaps rows")          # scaling ending in the first float of rows
    refused(lib.gsr_rows_unpack(stream(), -1, D, None, None, None, None, None, None, None), "P=-1 is negative")
    refused(lib.gsr_rows_grad_pack(stream(), P, 18, 1, one, grad.data_ptr()), "D=18 is not 3 K + 14")
    refused(lib.gsr_rows_grad_pack(stream(), P, D, 0, one, grad.data_ptr()), "B=0 not in 1..64")
    refused(lib.gsr_rows_grad_pack(stream(), P, D, 65, many, grad.data_ptr()), "B=65 not in 1..64")
    refused(lib.gsr_rows_grad_pack(stream(), P, D, 1, one, arena.data_ptr() + 4 * (rr.arena_floats(P, D) - 1)), "grad_rows overlaps arenas[0]")
    refused(lib.gsr_rows_grad_pack(stream(), P, D, 1, one, None), "grad_rows is NULL")
    refused(lib.gsr_rows_grad_pack(stream(), P, D, 1, (C.c_void_p * 1)(None), grad.data_ptr()), "arenas[0] is NULL")
    # adjacent is not overlapping: grad_rows right behind the arena is accepted, and the device still works
    assert lib.gsr_rows_grad_pack(stream(), P, D, 1, one, arena.data_ptr() + 4 * rr.arena_floats(P, D)) == 0
    torch.cuda.synchronize()
    for b in bufs.values():
        assert not b.any()                                           # no refused call wrote anything
    check_unpack(rows, dev)


# ---------------------------------------------------------------- end to end ----------------------------------------------------------------

@contextlib.contextmanager
def deterministic_bwd():
    saved = _lib.get_option("deterministic_bwd")
    _lib.set_option("deterministic_bwd", 1)
    try:
        yield
    finally:
        _lib.set_option("deterministic_bwd", saved)


class Case:
    """Rows of a synthetic scene, three cameras of different sizes, fixed image gradients, and per camera what
    render_fused(cam, unflatten_gaussians(rows)) gives: image, radii and (under the deterministic reverse pass) the row gradient."""

    def __init__(self, sh_degree, seed, P=1501):
        from gaussian_transformer_amd import rows as R
        self.R = R
        sc = synth.make_scene(P, 128, 80, sh_degree=sh_degree, seed=seed)
        self.rows = flatten_gaussians(GaussianParams.from_synthetic(sc, DEV, requires_grad=False)).contiguous()
        self.P, self.D = self.rows.shape
        self.K = (self.D - 14) // 3
        self.cams = [TorchCamera(c, DEV) for c in (sc.camera, synth.identity_camera(96, 64), synth.identity_camera(50, 37, tanfovx=0.3))]
        self.pipe, self.bg = PipelineParams(), torch.tensor(sc.bg, device=DEV)
        self.G = [torch.tensor(np.random.default_rng(seed + 100 + b).normal(size=(3, c.image_height, c.image_width)).astype(np.float32), device=DEV)
                  for b, c in enumerate(self.cams)]
        self.images, self.radii, self.g = [], [], []
        with deterministic_bwd():
            for b, cam in enumerate(self.cams):
                leaf = self.rows.clone().requires_grad_()
                out = render_fused(cam, unflatten_gaussians(leaf), self.pipe, self.bg)
                (g,) = torch.autograd.grad(out["render"], leaf, self.G[b])
                self.images.append(out["render"].detach()); self.radii.append(out["radii"]); self.g.append(g)

    def groups(self, g):
        K = self.K
        return dict(features=g[:, :3 * K], rotation=g[:, 3 * K:3 * K + 4], opacity=g[:, 3 * K + 4:3 * K + 5], xyz=g[:, 3 * K + 5:3 * K + 8],
                    scaling=g[:, 3 * K + 8:3 * K + 11])

    def render(self, rows, cams=None, **kw):
        return self.R.render_rows(self.cams if cams is None else cams, rows, self.pipe, self.bg, **kw)


@pytest.fixture(scope="module")
def case26():
    return Case(1, 41)


@pytest.fixture(scope="module")
def case62():
    return Case(3, 43)


def check_forward(cs):
    out = cs.render(cs.rows)
    assert set(out) == {"renders", "radii", "visibility_filter"} and len(out["renders"]) == 3
    assert out["radii"].shape == (3, cs.P) and out["radii"].dtype == torch.int32
    for b, cam in enumerate(cs.cams):
        assert out["renders"][b].shape == (3, cam.image_height, cam.image_width)
        assert torch.equal(out["renders"][b], cs.images[b]) and torch.equal(out["radii"][b], cs.radii[b]), b
        assert float(cs.images[b].abs().max()) > 0
    vis = (torch.stack(cs.radii) > 0).any(0)
    assert out["visibility_filter"].dtype == torch.bool and torch.equal(out["visibility_filter"], vis) and 0 < int(vis.sum())


def check_backward(cs):
    # the comparison means something: every camera's gradient reaches all five parameter groups, and cameras share Gaussians
    for b, g in enumerate(cs.g):
        for name, v in cs.groups(g).items():
            assert bool((v != 0).any()), (b, name)
        assert not g[:, cs.D - 3:].any()
    assert int(((cs.radii[0] > 0) & (cs.radii[2] > 0)).sum()) > 100
    want = (cs.g[0] + cs.g[1]) + cs.g[2]
    leaf = cs.rows.clone().requires_grad_()
    with deterministic_bwd():
        out = cs.render(leaf)
        from gaussian_transformer_amd.rasterizer import composited_mask
        mask = composited_mask()                                             # the last camera's render
        assert mask is not None and mask.shape == (cs.P,) and not bool(((cs.g[2] != 0).any(1) & ~mask).any())
        fns = [im.grad_fn for im in out["renders"]]
        assert fns[0] is not None and all(f is fns[0] for f in fns)          # one node for the B images
        (got,) = torch.autograd.grad(out["renders"], leaf, cs.G)
    assert got.shape == (cs.P, cs.D) and torch.equal(got, want)
    assert (rr.bits(got[:, cs.D - 3:]) == 0).all()


def test_forward_is_render_fused_per_camera_d26(case26):
    check_forward(case26)


def test_forward_is_render_fused_per_camera_d62(case62):
    check_forward(case62)


def test_backward_is_the_ordered_sum_of_the_cameras_d26(case26):
    check_backward(case26)


def test_backward_is_the_ordered_sum_of_the_cameras_d62(case62):
    check_backward(case62)


def test_sh_degree_argument(case62):
    """sh_degree = 1 on 62-column rows: render_fused with active_sh_degree = 1."""
    cs = case62
    g = unflatten_gaussians(cs.rows)
    g.active_sh_degree = 1
    want = render_fused(cs.cams[1], g, cs.pipe, cs.bg)["render"]
    got = cs.render(cs.rows, cams=cs.cams[1:2], sh_degree=1)["renders"][0]
    assert torch.equal(got, want) and not torch.equal(got, cs.images[1])


def test_skipped_camera_runs_no_backward(case26, monkeypatch):
    from gaussian_transformer_amd.rasterizer import get_backend
    cs, be = case26, get_backend()
    calls, real = [], be.backward

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(be, "backward", counted)
    leaf = cs.rows.clone().requires_grad_()
    with deterministic_bwd():
        r = cs.render(leaf)["renders"]
        ((r[0] * cs.G[0]).sum() + (r[2] * cs.G[2]).sum()).backward()
    assert len(calls) == 2
    assert torch.equal(leaf.grad, cs.g[0] + cs.g[2])


def test_callers_gradient_arena_is_ignored_and_restored(case26):
    from gaussian_transformer_amd import rasterizer
    from gaussian_transformer_amd.rasterizer import arena_floats, gradient_arena
    cs = case26
    mine = torch.full((arena_floats(cs.P, cs.K) + 8,), float("nan"), device=DEV)
    leaf = cs.rows.clone().requires_grad_()
    with deterministic_bwd(), gradient_arena(mine):
        out = cs.render(leaf)
        (got,) = torch.autograd.grad(out["renders"], leaf, cs.G)
        assert rasterizer._grad_arena is mine
    assert rasterizer._grad_arena is None
    assert bool(torch.isnan(mine).all())
    assert torch.equal(got, (cs.g[0] + cs.g[1]) + cs.g[2])


def test_non_contiguous_rows_get_their_gradient(case26):
    cs = case26
    base = torch.zeros((cs.P, cs.D + 7), device=DEV)
    base[:, 3:3 + cs.D] = cs.rows
    base.requires_grad_()
    view = base[:, 3:3 + cs.D]
    assert not view.is_contiguous()
    with deterministic_bwd():
        out = cs.render(view, cams=cs.cams[:1])
        assert torch.equal(out["renders"][0], cs.images[0])
        out["renders"][0].backward(cs.G[0])
    assert torch.equal(base.grad[:, 3:3 + cs.D], cs.g[0]) and not base.grad[:, :3].any() and not base.grad[:, 3 + cs.D:].any()


def test_more_cameras_than_one_pack_call_takes():
    cs = Case(1, 47, P=257)
    cam, G = cs.cams[2], cs.G[2]
    want = cs.g[2]
    for _ in range(64):
        want = want + cs.g[2]
    leaf = cs.rows.clone().requires_grad_()
    with deterministic_bwd():
        out = cs.render(leaf, cams=[cam] * 65)
        assert out["radii"].shape == (65, 257)
        (got,) = torch.autograd.grad(out["renders"], leaf, [G] * 65)
    assert bool(cs.g[2].any()) and torch.equal(got, want)


def test_no_grad_keeps_nothing(case26):
    cs = case26
    leaf = cs.rows.clone().requires_grad_()
    graph = cs.render(leaf)
    assert all(im.requires_grad for im in graph["renders"])
    cs.render(cs.rows)                                               # warm: workspace-size caches and binning hints are host state
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        out = cs.render(leaf)
    torch.cuda.synchronize()
    after = torch.cuda.memory_allocated()
    for a, b in zip(out["renders"], graph["renders"]):
        assert a.grad_fn is None and not a.requires_grad and torch.equal(a, b)
    assert torch.equal(out["radii"], graph["radii"])
    # net of what was returned (the allocator hands out 512-byte blocks) nothing stays allocated: no arena (3 x 222 KB here), no workspace
    block = lambda t: -(-t.numel() * t.element_size() // 512) * 512
    returned = sum(block(t) for t in out["renders"]) + block(out["radii"]) + block(out["visibility_filter"])
    assert after - before <= returned
    same = cs.render(cs.rows)                                        # rows without requires_grad, gradients enabled: no graph either
    assert all(im.grad_fn is None for im in same["renders"])


def test_one_coefficient_rows_end_to_end():
    """D = 17 (K = 1: no f_rest buffer, no f_rest block in the arenas), which render_fused does not take: against the same backend calls
    made by hand on unflatten_gaussians(rows) made contiguous, the arenas packed by tests/rows_ref.py."""
    from gaussian_transformer_amd.rasterizer import camera_settings, get_backend
    cs_rows = flatten_gaussians(GaussianParams.from_synthetic(synth.make_scene(300, 128, 80, sh_degree=0, seed=45), DEV, requires_grad=False)).contiguous()
    from gaussian_transformer_amd import rows as R
    P, D = cs_rows.shape
    assert D == 17
    cams = [TorchCamera(c, DEV) for c in (synth.identity_camera(128, 80), synth.identity_camera(50, 37, tanfovx=0.3))]
    pipe, bg = PipelineParams(), torch.zeros(3, device=DEV)
    G = [torch.tensor(np.random.default_rng(145 + b).normal(size=(3, c.image_height, c.image_width)).astype(np.float32), device=DEV)
         for b, c in enumerate(cams)]
    be = get_backend()
    g = unflatten_gaussians(cs_rows)
    xyz, dc, op, sc, rot = (t.contiguous() for t in (g._xyz, g._features_dc, g._opacity, g._scaling, g._rotation))
    empty = xyz.new_empty((0,))
    leaf = cs_rows.clone().requires_grad_()
    with deterministic_bwd():
        out = R.render_rows(cams, leaf, pipe, bg)
        (got,) = torch.autograd.grad(out["renders"], leaf, G)
        arenas = []
        for b, cam in enumerate(cams):
            rs = camera_settings(cam, bg, 1.0, 0, False)
            n, color, radii, geom, binning, img = be.forward(rs, xyz, dc, empty, op, sc, rot, empty, shs_rest=None, raw_params=True)
            assert torch.equal(color, out["renders"][b]) and torch.equal(radii, out["radii"][b]) and float(color.abs().max()) > 0
            gm3, _gm2, gsh, _gc, gop, gsc, grot, _gcov = be.backward(rs, n, G[b], xyz, radii, dc, empty, sc, rot, empty, geom, binning, img,
                                                                     shs_rest=None, raw_params=True)
            arenas.append(torch.cat([t.reshape(-1) for t in (gm3, gsh, gop, gsc, grot)]).cpu())
    want = rr.pack_ref(arenas, P, D)
    assert bool(want.any()) and torch.equal(got.cpu(), want)


def test_together_with_the_stacked_loss(case26):
    from gaussian_transformer_amd.loss import stacked_image_loss
    cs = case26
    cams = [cs.cams[0], TorchCamera(synth.identity_camera(128, 80, tanfovx=0.5), DEV)]
    with torch.no_grad():
        tgt_rows = cs.rows.clone()
        tgt_rows[:, :3] += 0.2                                       # another DC colour
        targets = cs.render(tgt_rows, cams=cams)["renders"]
    leaf = cs.rows.clone().requires_grad_()
    loss = stacked_image_loss(cs.render(leaf, cams=cams)["renders"], targets)
    loss.backward()
    assert leaf.grad.shape == (cs.P, cs.D) and bool(torch.isfinite(leaf.grad).all()) and bool(leaf.grad.any())
    assert float(loss) > 0
