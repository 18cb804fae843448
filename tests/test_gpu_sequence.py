"""-m gpu: the native sequence preparation (include/gsr_sequence.h) -- box sort bit-equal to the restatements of
tests/sequence_ref.py (themselves pinned to the reference by tests/golden/box_sort.npz), multi-camera visibility integer-equal to
the radii of gsr_forward and of the float32 CPU oracle, and the chain up to the token batch."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib, sequence as seq, synth
from gaussian_transformer_amd import GaussianRasterizationSettings, GaussianRasterizer
from gaussian_transformer_amd.model import GaussianParams
from gaussian_transformer_amd.rasterizer import rasterize_gaussians_fused
from gaussian_transformer_amd.render import PipelineParams, TorchCamera, render
from tests import sequence_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "box_sort.npz")


def dev(a, dtype=torch.float32):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def check_box(rows, xyz_col, n):
    """Runs the native sort and demands bit-equal rows, perm and count; returns the three device tensors."""
    want_rows, want_perm, want_count = sr.box_sort_vec(rows, xyz_col, n)
    out, perm, count = seq.box_sort_rows(dev(rows), xyz_col, n)
    assert int(count.item()) == want_count
    assert (perm.cpu().numpy() == want_perm).all()
    assert out.cpu().numpy().tobytes() == want_rows.tobytes()        # bits, so NaN payloads and -0.0 count
    return out, perm, count


# ---------------------------------------------------------------- box sort ----------------------------------------------------------------

@pytest.mark.parametrize("n", [10, 40])
def test_box_sort_reproduces_the_reference_fixture(n):
    z = np.load(GOLDEN)
    out, perm, count = check_box(z["rows"], 17, n)
    last = int(z[f"last_{n}"])
    assert int(count.item()) == last and out[:last].cpu().numpy().tobytes() == z[f"sorted_{n}"].tobytes()
    # the public path: GaussianHandler on the raw parameters, normalisation included
    g = GaussianParams(1)
    for name in ("xyz", "scaling", "features_dc", "features_rest", "rotation", "opacity"):
        setattr(g, "_" + name, dev(z[name]))
    h = seq.GaussianHandler(g, n)
    res, p = h.box_sort(g, return_perm=True)
    assert res.shape == (last, 26) and p.dtype == torch.int64
    # normalisation is exact on this cloud (every axis spans exactly [0, 1]); the scaling columns go through one division
    got = res.cpu().numpy()
    assert got[:, :20].tobytes() == z[f"sorted_{n}"][:, :20].tobytes() and (got[:, 23:] == 0).all()
    np.testing.assert_allclose(got[:, 20:23], z[f"sorted_{n}"][:, 20:23], rtol=0, atol=1e-6)
    assert (z["rows"][p.cpu().numpy()][:, :20] == got[:, :20]).all()


@pytest.mark.parametrize("P", [0, 1, 2, 257, 100_003, 1_000_000])
@pytest.mark.parametrize("n", [1, 2, 10, 40, 128])
def test_box_sort_bit_equal_planted_rows(n, P):
    check_box(sr.planted_rows(P, 26, 17, n, seed=7 * n + P % 1000), 17, n)


@pytest.mark.parametrize("P", [257, 100_003])
@pytest.mark.parametrize("n", [1, 2, 10, 40, 128])
@pytest.mark.parametrize("D,xyz_col", [(3, 0), (26, 0), (26, 23), (62, 0), (62, 53), (62, 59)])
def test_box_sort_row_widths_and_coordinate_columns(D, xyz_col, n, P):
    check_box(sr.planted_rows(P, D, xyz_col, n, seed=D + xyz_col + n), xyz_col, n)


@pytest.mark.parametrize("n", [1, 40, 128])
def test_box_sort_one_box_all_dropped_and_duplicates(n):
    rng = np.random.default_rng(n)
    P = 100_003
    b = sr.boundaries(n)
    rows = rng.normal(size=(P, 26)).astype(np.float32)
    cell = n // 2
    rows[:, 17:20] = (b[cell] + (b[cell + 1] - b[cell]) * rng.random((P, 3)) * 0.5).astype(np.float32)      # every row in one box
    _, perm, count = check_box(rows, 17, n)
    assert int(count.item()) == P and (perm.cpu().numpy() == np.arange(P)).all()
    rows[:, 18] = np.float32(1.0)                                                                             # every row dropped
    out, perm, count = check_box(rows, 17, n)
    assert int(count.item()) == 0 and (out == 0).all() and (perm == -1).all()
    rows[:, 17:20] = rng.random((P, 3), dtype=np.float32)
    rows[P // 2:] = rows[:P - P // 2]                                                                         # half the cloud duplicated
    check_box(rows, 17, n)


def test_single_gaussian_normalises_to_nan_and_is_dropped():
    g = GaussianParams(1)
    g._xyz, g._scaling = dev([[1.0, 2.0, 3.0]]), dev([[-3.0, -3.0, -3.0]])
    g._features_dc, g._features_rest = dev(np.zeros((1, 1, 3))), dev(np.zeros((1, 3, 3)))
    g._rotation, g._opacity = dev([[1.0, 0, 0, 0]]), dev([[0.5]])
    h = seq.GaussianHandler(g, 40)
    res, p = h.box_sort(g, return_perm=True)                       # (x - min) / (max - min) = 0 / 0
    assert res.shape == (0, 26) and p.shape == (0,)


def test_box_sort_is_bitwise_reproducible_and_runs_on_a_second_stream():
    rows = dev(sr.planted_rows(300_007, 26, 17, 40, seed=3))
    a = seq.box_sort_rows(rows, 17, 40)
    b = seq.box_sort_rows(rows, 17, 40)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        c = seq.box_sort_rows(rows, 17, 40)
    side.synchronize()
    for x, y, w in zip(a, b, c):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() == w.cpu().numpy().tobytes()


def guarded(nbytes, pad=4096):
    """A byte buffer with sentinel-filled guard regions either side; returns (whole, payload pointer, check function)."""
    whole = torch.full((nbytes + 2 * pad,), 0xA5, dtype=torch.uint8, device=DEV)

    def intact():
        return bool((whole[:pad] == 0xA5).all()) and bool((whole[pad + nbytes:] == 0xA5).all())
    return whole, whole.data_ptr() + pad, intact


@pytest.mark.parametrize("P,D,n", [(1000, 26, 40), (4097, 3, 1), (333, 62, 128)])
def test_box_sort_writes_inside_its_buffers(P, D, n):
    lib = _lib.load()
    xyz_col = D - 3
    rows_np = sr.planted_rows(P, D, xyz_col, n, seed=P)
    rows = dev(rows_np)
    nb = C.c_size_t()
    _lib.check(lib.gsr_box_sort_workspace(P, n, C.byref(nb)), "workspace")
    assert nb.value >= 12 * P
    bufs = [guarded(4 * P * D), guarded(4 * P), guarded(4), guarded(nb.value)]
    stream = torch.cuda.current_stream(DEV).cuda_stream
    _lib.check(lib.gsr_box_sort(stream, P, D, rows.data_ptr(), xyz_col, n, bufs[0][1], bufs[1][1], bufs[2][1], bufs[3][1], nb.value), "sort")
    torch.cuda.synchronize()
    assert all(b[2]() for b in bufs)
    want_rows, want_perm, want_count = sr.box_sort_vec(rows_np, xyz_col, n)
    assert bufs[0][0][4096:4096 + 4 * P * D].cpu().numpy().tobytes() == want_rows.tobytes()
    assert bufs[1][0][4096:4096 + 4 * P].cpu().numpy().tobytes() == want_perm.tobytes()
    assert bufs[2][0][4096:4100].cpu().numpy().view(np.int32)[0] == want_count
    assert (rows.cpu().numpy().tobytes() == rows_np.tobytes())      # the input is untouched


def test_box_sort_error_paths():
    lib = _lib.load()
    P, D = 100, 26
    rows = dev(sr.planted_rows(P, D, 17, 10, seed=1))
    out, perm, cnt = torch.empty_like(rows), torch.empty(P, dtype=torch.int32, device=DEV), torch.full((1,), 77, dtype=torch.int32, device=DEV)
    nb = C.c_size_t()
    _lib.check(lib.gsr_box_sort_workspace(P, 10, C.byref(nb)), "workspace")
    ws = torch.empty(nb.value, dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream(DEV).cuda_stream
    call = lambda **k: lib.gsr_box_sort(s, k.get("P", P), k.get("D", D), k.get("rows", rows.data_ptr()), k.get("col", 17), k.get("n", 10),
                                        k.get("out", out.data_ptr()), perm.data_ptr(), k.get("cnt", cnt.data_ptr()), ws.data_ptr(), k.get("wsb", nb.value))
    err = lambda: lib.gsr_last_error().decode()
    assert call(out=rows.data_ptr()) == 1 and "must not overlap" in err()
    assert call(n=0) == 1 and call(n=129) == 1 and "n=129 not in 1..128" in err()
    assert call(D=2) == 1 and call(D=65) == 1 and "D=65" in err()
    assert call(col=24) == 1 and "xyz_col=24" in err() and call(col=-1) == 1
    assert call(P=-1) == 1 and call(cnt=None) == 1 and call(rows=None) == 1
    assert call(wsb=nb.value - 1) == 4 and "workspace" in err()
    assert lib.gsr_box_sort_workspace(P, 10, None) == 1 and lib.gsr_box_sort_workspace(P, 200, C.byref(nb)) == 1
    torch.cuda.synchronize()
    assert int(cnt.item()) == 77                                    # nothing was enqueued by the refused calls
    assert call(P=0, rows=None, out=None) == 0 and int(cnt.item()) == 0
    assert call() == 0 and int(cnt.item()) == sr.box_sort_vec(rows.cpu().numpy(), 17, 10)[2]


# ---------------------------------------------------------------- visibility ----------------------------------------------------------------

def forward_radii(cam, means, scales=None, rotations=None, cov=None, mod=1.0, raw=False):
    """radii of one gsr_forward call through the public rasterizer (colours precomputed: they do not enter)."""
    P = means.shape[0]
    tc = TorchCamera(cam, DEV)
    rs = GaussianRasterizationSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=math.tan(cam.FoVx * 0.5),
        tanfovy=math.tan(cam.FoVy * 0.5), bg=torch.zeros(3, device=DEV), scale_modifier=mod, viewmatrix=tc.world_view_transform,
        projmatrix=tc.full_proj_transform, sh_degree=1, campos=tc.camera_center, prefiltered=False, debug=False)
    means2D = torch.zeros((P, 3), device=DEV)
    with torch.no_grad():
        if raw:
            dc, rest = torch.zeros((P, 1, 3), device=DEV), torch.zeros((P, 3, 3), device=DEV)
            _, radii = rasterize_gaussians_fused(means, means2D, dc, rest, torch.zeros((P, 1), device=DEV), scales, rotations, rs)
        else:
            _, radii = GaussianRasterizer(raster_settings=rs)(means3D=means, means2D=means2D, opacities=torch.full((P, 1), 0.5, device=DEV),
                                                              colors_precomp=torch.zeros((P, 3), device=DEV), scales=scales, rotations=rotations,
                                                              cov3D_precomp=cov)
    return radii


def check_visible(cams, means, **kw):
    """radii equal to per-camera gsr_forward calls; visible and counts consistent with them.  Returns radii [B, P]."""
    fw = {k: kw[k] for k in ("scales", "rotations", "cov", "mod", "raw") if k in kw}
    vis, radii, counts = seq.visible_union_tensors(cams, means, kw.get("scales"), kw.get("rotations"), kw.get("cov"), kw.get("mod", 1.0),
                                                   kw.get("raw", False), want_radii=True, want_counts=True)
    assert radii.shape == (len(cams), means.shape[0]) and radii.dtype == torch.int32 and vis.dtype == torch.bool
    for b, cam in enumerate(cams):
        want = forward_radii(cam, means, **fw)
        assert torch.equal(radii[b], want), (b, int((radii[b] != want).sum()))
    assert torch.equal(vis, (radii > 0).any(0)) and torch.equal(counts, (radii > 0).sum(1).to(torch.int32))
    return radii


@pytest.fixture(scope="module")
def tiramisu():
    sc = synth.make_tiramisu_scene(seed=0, copies=3)
    return sc, dev(sc.means3D), dev(sc.scales), dev(sc.rotations)


def test_visible_union_ring_cameras_with_and_without_exact_cull(tiramisu):
    sc, means, scales, rots = tiramisu
    cams = synth.tiramisu_ring_cameras(8)
    try:
        for cull in (0, 1):
            _lib.set_option("exact_tile_cull", cull)
            radii = check_visible(cams, means, scales=scales, rotations=rots)
    finally:
        _lib.set_option("exact_tile_cull", 1)
    assert (radii > 0).any(1).all()                                # every camera sees part of the cloud


def test_visible_union_table_camera_mixed_sizes_and_variants():
    table = synth.make_table_scene(seed=0, copies=2)
    means, scales, rots = dev(table.means3D), dev(table.scales), dev(table.rotations)
    ring = synth.tiramisu_ring_cameras
    mixed = [table.camera, synth.identity_camera(256, 256), synth.identity_camera(1920, 1080, tanfovx=0.9), synth.identity_camera(33, 517, tanfovx=0.2),
             ring(3, 640, 360, centre=table.means3D.mean(0), radius=6.0)[1]]
    check_visible([table.camera], means, scales=scales, rotations=rots)                            # B = 1
    check_visible(mixed, means, scales=scales, rotations=rots)
    check_visible(mixed, means, scales=scales, rotations=rots, mod=0.5)
    check_visible(mixed, means, scales=torch.log(scales), rotations=rots * 3.0, raw=True)           # raw_params = 1
    g = GaussianParams(3)
    g._scaling, g._rotation = torch.log(scales), rots
    check_visible(mixed, means, cov=g.get_covariance(1.0).contiguous())                            # cov3D_precomp


def test_visible_union_behind_every_camera_and_singular_covariance():
    sc = synth.make_scene(4000, 512, 512, sh_degree=0, seed=5, tanfovx=0.5)
    means = sc.means3D.copy()
    means[:500, 2] *= -1                                            # behind every camera below (all look down +z from the origin)
    means[500:600] = (0.0, 0.0, 5.0)
    g = GaussianParams(0)
    g._scaling, g._rotation = torch.log(dev(sc.scales)), dev(sc.rotations)
    cov = g.get_covariance(1.0).contiguous()
    cov[500:600] = torch.tensor([1e12, 1e12, 0, 1e12, 0, 0], device=DEV)     # a = b = c after projection with fx = fy: det == 0 exactly
    cams = [synth.identity_camera(512, 512, tanfovx=0.5), synth.identity_camera(256, 256, tanfovx=0.5), synth.identity_camera(800, 800, tanfovx=0.25)]
    radii = check_visible(cams, dev(means), cov=cov)
    assert (radii[:, :600] == 0).all() and (radii[:, 600:] > 0).any()
    big = cov.clone(); big[500:600] = torch.tensor([1e12, 0, 0, 1e12, 0, 0], device=DEV)           # same size, not singular: visible
    r2 = check_visible(cams, dev(means), cov=big)
    assert (r2[:, 500:600] > 0).all()


def test_visible_union_equals_the_float32_cpu_oracle():
    from oracle import ref
    from tests.helpers import oracle_scene
    sc = synth.make_scene(3000, 256, 256, sh_degree=0, seed=11)
    cams = [sc.camera, synth.identity_camera(200, 120, tanfovx=0.4)]
    _, radii, _ = seq.visible_union_tensors(cams, dev(sc.means3D), dev(sc.scales), dev(sc.rotations), want_radii=True)
    r32 = ref.get("f32")
    for b, cam in enumerate(cams):
        S = oracle_scene(sc, W=cam.image_width, H=cam.image_height, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
                         viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, campos=cam.camera_center)
        want = r32.forward(S)["radii"]
        assert (radii[b].cpu().numpy() == want).all(), b


def test_visible_union_64_cameras_and_chunking_beyond():
    sc = synth.make_scene(20_000, 320, 200, sh_degree=0, seed=2, zmin=-4.0, zmax=8.0)
    means, scales, rots = dev(sc.means3D), dev(sc.scales), dev(sc.rotations)
    centre = np.array([0.0, 0.0, 3.0])
    cams = synth.tiramisu_ring_cameras(64, 320, 200, centre=centre, radius=4.0)
    r64 = check_visible(cams, means, scales=scales, rotations=rots)                                # B = 64, one native call
    more = cams + synth.tiramisu_ring_cameras(7, 200, 320, centre=centre, radius=2.5)              # 71: two native calls
    vis, radii, counts = seq.visible_union_tensors(more, means, scales, rots, want_radii=True, want_counts=True)
    assert torch.equal(radii[:64], r64)
    for b in range(64, 71):
        assert torch.equal(radii[b], forward_radii(more[b], means, scales=scales, rotations=rots))
    assert torch.equal(vis, (radii > 0).any(0)) and torch.equal(counts, (radii > 0).sum(1).to(torch.int32))


def test_visible_union_null_outputs_in_every_combination_and_guards():
    lib = _lib.load()
    sc = synth.make_scene(5003, 256, 256, sh_degree=0, seed=4, zmin=-2.0)
    means, scales, rots = dev(sc.means3D), dev(sc.scales), dev(sc.rotations)
    cams = [sc.camera, synth.identity_camera(100, 300)]
    P, B = means.shape[0], 2
    vis0, radii0, counts0 = seq.visible_union_tensors(cams, means, scales, rots, want_radii=True, want_counts=True)
    view = torch.stack([dev(c.world_view_transform).reshape(16) for c in cams])
    proj = torch.stack([dev(c.full_proj_transform).reshape(16) for c in cams])
    tfx = (C.c_float * B)(*[c.tanfovx for c in cams]); tfy = (C.c_float * B)(*[c.tanfovy for c in cams])
    ws = (C.c_int32 * B)(*[c.image_width for c in cams]); hs = (C.c_int32 * B)(*[c.image_height for c in cams])
    s = torch.cuda.current_stream(DEV).cuda_stream
    for mask in range(8):
        r, v, c = guarded(4 * B * P), guarded(P), guarded(4 * B)
        rc = lib.gsr_visible_union(s, P, B, means.data_ptr(), scales.data_ptr(), 1.0, rots.data_ptr(), None, 0, view.data_ptr(), proj.data_ptr(),
                                   tfx, tfy, ws, hs, r[1] if mask & 1 else None, v[1] if mask & 2 else None, c[1] if mask & 4 else None)
        assert rc == 0, lib.gsr_last_error()
        torch.cuda.synchronize()
        assert r[2]() and v[2]() and c[2]()
        payload = lambda b, n: b[0][4096:4096 + n].cpu().numpy()
        for on, buf, n, want in ((mask & 1, r, 4 * B * P, radii0), (mask & 2, v, P, vis0.to(torch.uint8)), (mask & 4, c, 4 * B, counts0)):
            if on:
                assert payload(buf, n).tobytes() == want.cpu().numpy().tobytes()
            else:
                assert (payload(buf, n) == 0xA5).all()              # an output not asked for is not written
    # a second stream, and the error paths
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        v2, r2, c2 = seq.visible_union_tensors(cams, means, scales, rots, want_radii=True, want_counts=True)
    side.synchronize()
    assert torch.equal(v2, vis0) and torch.equal(r2, radii0) and torch.equal(c2, counts0)
    call = lambda **k: lib.gsr_visible_union(s, k.get("P", P), k.get("B", B), means.data_ptr(), k.get("scales", scales.data_ptr()), 1.0, rots.data_ptr(),
                                             k.get("cov", None), k.get("raw", 0), view.data_ptr(), proj.data_ptr(), tfx, tfy, k.get("ws", ws), hs, None, None, None)
    err = lambda: lib.gsr_last_error().decode()
    assert call(B=0) == 1 and call(B=65) == 1 and "B=65 not in 1..64" in err()
    assert call(P=-1) == 1 and call(scales=None) == 1 and "exactly one of" in err()
    assert call(cov=means.data_ptr()) == 1 and call(ws=(C.c_int32 * B)(0, 5)) == 1 and "camera 0" in err()
    assert call(P=0) == 0 and call() == 0


def test_validation_of_mixed_devices_and_partial_overlap():
    g = lambda *sh, **kw: torch.zeros(*sh, device=DEV, **kw)
    cams = [synth.identity_camera(64, 64)]
    with pytest.raises(_lib.GsrError, match="scales must be on a HIP device"):
        seq.visible_union_tensors(cams, g(4, 3), torch.zeros(4, 3), g(4, 4))
    with pytest.raises(_lib.GsrError, match="rows must be float32, got float64"):
        seq.box_sort_rows(g(5, 26, dtype=torch.float64), 17, 10)
    # rows and out_rows that intersect without being equal are refused, whichever comes first
    lib = _lib.load()
    P, D = 64, 26
    buf = g(2 * P * D)
    perm, cnt = torch.empty(P, dtype=torch.int32, device=DEV), torch.full((1,), 5, dtype=torch.int32, device=DEV)
    nb = C.c_size_t()
    _lib.check(lib.gsr_box_sort_workspace(P, 10, C.byref(nb)), "workspace")
    ws = torch.empty(nb.value, dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream(DEV).cuda_stream
    base = buf.data_ptr()
    for rows_at, out_at, rc in ((0, 4 * D, 1), (4 * D, 0, 1), (0, 4 * (P * D - 1), 1), (0, 4 * P * D, 0), (4 * P * D, 0, 0)):
        got = lib.gsr_box_sort(s, P, D, base + rows_at, 17, 10, base + out_at, perm.data_ptr(), cnt.data_ptr(), ws.data_ptr(), nb.value)
        assert got == rc, (rows_at, out_at, lib.gsr_last_error())
        if rc:
            assert b"must not overlap" in lib.gsr_last_error()


# ---------------------------------------------------------------- end to end ----------------------------------------------------------------

def test_scene_to_token_batch_end_to_end():
    """GaussianHandler.box_sort on a GaussianParams, denormalise, visible_union against render(), fold and batch: every step
    against the same chain in torch / numpy."""
    sc = synth.make_scene(30_011, 400, 300, sh_degree=1, seed=9, zmin=-6.0)      # z < 0.2: behind every camera below
    mk = lambda: GaussianParams.from_synthetic(sc, DEV, requires_grad=False)
    g, g0 = mk(), mk()
    with torch.no_grad():
        handler = seq.GaussianHandler(g, 40)
        rows, perm = handler.box_sort(g, return_perm=True)
        flat0 = seq.flatten_gaussians(handler.normalize(g0)).cpu().numpy()
    want_rows, want_perm, want_count = sr.box_sort_vec(flat0, 17, 40)
    assert rows.shape[0] == want_count < sc.P and rows.cpu().numpy().tobytes() == want_rows[:want_count].tobytes()
    assert (perm.cpu().numpy() == want_perm[:want_count]).all()
    with torch.no_grad():
        scene = handler.denormalize(seq.unflatten_gaussians(rows))                                # train_stacked_transformer.py:73
    assert scene.max_sh_degree == 1 and scene.get_xyz.shape == (want_count, 3)
    cams = [TorchCamera(c, DEV) for c in (sc.camera, synth.identity_camera(200, 150, tanfovx=0.1), synth.identity_camera(640, 360, tanfovx=0.3))]
    vis, radii, counts = seq.visible_union(cams, scene, return_radii=True, return_counts=True)
    want_vis = torch.zeros(want_count, dtype=torch.bool, device=DEV)
    bg = torch.zeros(3, device=DEV)
    with torch.no_grad():
        for b, cam in enumerate(cams):                                                             # :93-96
            pkg = render(cam, scene, PipelineParams(), bg)
            assert torch.equal(pkg["radii"], radii[b])
            want_vis |= pkg["visibility_filter"]
    assert torch.equal(vis, want_vis) and torch.equal(counts, (radii > 0).sum(1).to(torch.int32)) and 0 < int(vis.sum()) < want_count
    assert torch.equal(seq.visible_union(cams, scene), vis)
    flat = seq.flatten_gaussians(scene)
    for stack, dropout, u in ((3, 0.3, 0.5), (8, 0.6, 0.0), (0, 0.0, 0.999)):
        got = seq.make_token_batch(flat, vis, stack, dropout, u)
        want = sr.token_batch(flat.cpu().numpy(), vis.cpu().numpy(), stack, dropout, u)
        for k in want:
            assert got[k].device.type == "cuda" and got[k].cpu().numpy().tobytes() == want[k].tobytes(), (k, stack)
        assert torch.equal(seq.unstack(got["trg_y"], stack).cpu(), torch.tensor(want["trg_y"][0].reshape(-1, 26)))
