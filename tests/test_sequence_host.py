"""CPU tests of the sequence preparation's host side: the numpy restatements (tests/sequence_ref.py) against the reference's own
recorded results (tests/golden/box_sort.npz) and against each other, the token folding and batching, the header / ctypes contract
and validation without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib
from gaussian_transformer_amd.model import GaussianParams
from tests import sequence_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "box_sort.npz")


def seq():
    from gaussian_transformer_amd import sequence
    return sequence


def golden_params(z):
    g = GaussianParams(1)
    for name in ("xyz", "scaling", "features_dc", "features_rest", "rotation", "opacity"):
        setattr(g, "_" + name, torch.tensor(z[name]))
    return g


def test_boundary_table_properties():
    for n in range(1, 257):
        b = sr.boundaries(n)
        assert b.dtype == np.float32 and len(b) == n + 1
        assert b[0] == 0 and b[n] == np.float32(1.0) and (np.diff(b) > 0).all(), n


@pytest.mark.parametrize("n", [10, 40])
def test_restatements_reproduce_the_reference_fixture(n):
    z = np.load(GOLDEN)
    rows, want, last = z["rows"], z[f"sorted_{n}"], int(z[f"last_{n}"])
    assert rows.shape == (2000, 26) and want.shape == (last, 26) and 0 < last < 2000       # the maxima are dropped
    out, perm, count = sr.box_sort_vec(rows, 17, n)
    assert count == last and out[:count].tobytes() == want.tobytes()
    assert (out[count:] == 0).all() and (perm[count:] == -1).all() and (rows[perm[:count]] == want).all()
    lout, lperm, llast = sr.box_sort_loop(rows, 17, n)
    assert llast == last and lout.tobytes() == want.tobytes() and (lperm == perm[:count]).all()


def test_fixture_covers_boundaries_and_dropped_rows():
    z = np.load(GOLDEN)
    xyz = z["rows"][:, 17:20]
    for n in (10, 40):
        b = sr.boundaries(n)
        assert np.isin(xyz, b).sum() > 50 and np.isin(xyz, np.nextafter(b, np.float32(-1))).sum() > 20
    assert (xyz == 1).any(axis=1).sum() == 2000 - int(z["last_10"])


@pytest.mark.parametrize("n", [1, 3, 7, 10, 12])
def test_loop_and_vectorised_restatements_agree_on_planted_rows(n):
    rows = sr.planted_rows(5000, 26, 17, n, seed=n)
    out, perm, count = sr.box_sort_vec(rows, 17, n)
    lout, lperm, llast = sr.box_sort_loop(rows, 17, n)
    assert count == llast and 0 < count < 5000
    assert out[:count].tobytes() == lout.tobytes() and (perm[:count] == lperm).all()


@pytest.mark.parametrize("n", [2, 12, 40, 100, 128])
def test_planted_rows_defeat_a_floor_only_cell(n):
    """The planted boundary cases are strong enough: deciding the cell from floor(c * n) alone changes keys (the mutation the
    GPU test must catch at n = 40, the reference's interval_num).  Powers of two have exact boundaries and are the control; so,
    as it happens, is n = 10, where the float32 product rounds to the right side of every boundary."""
    rows = sr.planted_rows(20000, 26, 17, n, seed=100 + n)
    differ = int((sr.box_keys(rows, 17, n) != sr.box_keys_floor(rows, 17, n)).sum())
    assert (differ == 0) if n in (2, 128) else (differ > 30), differ


def test_normalize_and_flatten_reproduce_the_fixture_rows():
    z = np.load(GOLDEN)
    s = seq()
    g = golden_params(z)
    h = s.GaussianHandler(g, 10)
    assert (h.worldMin.numpy() == z["world_min"]).all() and (h.worldMax.numpy() == z["world_max"]).all()
    assert h.scalingMin.item() == z["scaling_min"] and h.scalingMax.item() == z["scaling_max"] and h.box_num == 1000
    rows = s.flatten_gaussians(h.normalize(g))
    assert rows.shape == (2000, 26) and rows.numpy().tobytes() == z["rows"].tobytes()
    assert s.xyz_column(26) == 17 and s.row_width(4) == 26 and s.row_width(16) == 62 and s.xyz_column(62) == 53
    back = s.unflatten_gaussians(rows)
    assert back.max_sh_degree == 1 and back._xyz.data_ptr() == rows[:, 17:20].data_ptr()          # views, as the reference's
    for name in ("xyz", "scaling", "features_dc", "features_rest", "rotation", "opacity"):
        assert torch.equal(getattr(back, "_" + name), getattr(g, "_" + name)), name
    d = h.denormalize_copy(back)
    np.testing.assert_allclose(d._xyz.numpy(), z["xyz"], atol=1e-6)
    np.testing.assert_allclose(d._scaling.numpy(), z["scaling"], atol=1e-5)
    assert (s.start_gaussian().numpy() == sr.start_gaussian()).all()
    pad = np.zeros(26, np.float32); pad[24] = 1
    assert (s.pad_gaussian().numpy() == pad).all()
    with pytest.raises(_lib.GsrError, match="3 K \\+ 14 columns"):
        s.xyz_column(27)


@pytest.mark.parametrize("stack", [0, 1, 3, 8])
@pytest.mark.parametrize("S", [0, 1, 255, 256, 1000, 1029])
def test_fold_is_a_reshape_view(S, stack):
    s = seq()
    x = torch.arange(S * 5, dtype=torch.float32).reshape(S, 5)
    got = s.fold_tokens(x, stack)
    want = sr.fold_cat(x.numpy(), stack)
    assert tuple(got.shape) == want.shape and (got.numpy() == want).all()
    if got.numel():
        assert got.data_ptr() == x.data_ptr()                        # a view: nothing copied
    back = s.unstack(got, stack)
    assert torch.equal(back, x[:S - S % 2 ** stack]) and (not back.numel() or back.data_ptr() == x.data_ptr())
    assert torch.equal(s.unstack(got[None], stack), back)


@pytest.mark.parametrize("S,stack", [(5000, 3), (777, 0), (4096, 8), (300, 2)])
@pytest.mark.parametrize("dropout", [0.0, 0.3, 0.6])
@pytest.mark.parametrize("u", [0.0, 0.37, 0.9999999999999999])
def test_make_token_batch_restates_the_trainer(S, stack, dropout, u):
    s = seq()
    rng = np.random.default_rng(S + stack)
    rows = rng.normal(size=(S, 26)).astype(np.float32)
    vis = rng.random(S) < 0.7
    want = sr.token_batch(rows, vis, stack, dropout, u)
    got = s.make_token_batch(torch.tensor(rows), torch.tensor(vis), stack, dropout, u)
    assert set(got) == {"src", "trg", "trg_y"}
    for k in want:
        assert tuple(got[k].shape) == want[k].shape and (got[k].numpy() == want[k]).all(), k
    assert got["src"].shape[1] + got["trg_y"].shape[1] == vis.sum() // 2 ** stack
    if got["trg"].shape[1]:
        assert (got["trg"][0, 0].numpy() == np.tile(sr.start_gaussian(), 2 ** stack)).all()
    with pytest.raises(_lib.GsrError, match="u=1.0 not in"):
        s.make_token_batch(torch.tensor(rows), torch.tensor(vis), stack, dropout, 1.0)


def test_header_declares_exactly_what_the_ctypes_stub_binds():
    header = open(os.path.join(ROOT, "include", "gsr_sequence.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decls = dict(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", code, flags=re.S))
    assert set(decls) == {"gsr_box_sort_workspace", "gsr_box_sort", "gsr_visible_union"}
    assert set(_lib.SEQUENCE_SIGNATURES) == set(decls)
    for name, args in decls.items():
        assert len(_lib.SEQUENCE_SIGNATURES[name][1]) == len(args.split(",")), name
    assert not set(_lib.SEQUENCE_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.CHAMFER_SIGNATURES))
    assert "#define GSR_ABI_VERSION 2" in open(os.path.join(ROOT, "include", "gsr.h")).read()   # purely additive
    assert "deviation" in header.lower() and "zero" in header.lower()                           # the dropped rows are documented
    from gaussian_transformer_amd import build
    assert build.SOURCES["sequence.hip"] == build.SOURCES["preprocess.hip"]                      # the radii round identically
    lib = _lib.load()
    for name in decls:
        assert hasattr(lib, name)


def test_validation_names_the_argument_before_any_native_call(monkeypatch):
    s = seq()

    def no_native():
        raise AssertionError("the native library was reached")
    monkeypatch.setattr(_lib, "load", no_native)
    rows = torch.zeros(5, 26)
    with pytest.raises(RuntimeError, match=r"rows must be on a HIP device.*no CPU fallback"):
        s.box_sort_rows(rows, 17, 10)
    with pytest.raises(_lib.GsrError, match="rows must be a torch.Tensor"):
        s.box_sort_rows(rows.numpy(), 17, 10)
    meta = lambda *sh, **kw: torch.empty(*sh, device="meta", **kw)
    with pytest.raises(_lib.GsrError, match="rows must be on a HIP device"):
        s.box_sort_rows(meta(5, 26), 17, 10)
    s._validate_box_sizes(26, 17, 40)
    s._validate_box_sizes(3, 0, 1)
    s._validate_box_sizes(64, 61, 128)
    for D, col, n, msg in ((2, 0, 10, r"D=2 columns, supported: 3..64"), (65, 0, 10, "D=65"), (26, 24, 10, r"xyz_col=24 not in 0..D-3=23"),
                           (26, -1, 10, "xyz_col=-1"), (26, 17, 0, r"interval_num=0 not in 1..128"), (26, 17, 129, "interval_num=129"),
                           (26, 17, 2.5, "interval_num=2.5")):
        with pytest.raises(_lib.GsrError, match=msg):
            s._validate_box_sizes(D, col, n)
    cams = [object()]
    with pytest.raises(_lib.GsrError, match="means3D must be on a HIP device"):
        s.visible_union_tensors(cams, torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 4))
    with pytest.raises(_lib.GsrError, match="at least one camera"):
        s.visible_union_tensors([], torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 4))
    # types, dtypes, shapes and the combination of arguments are checked before the device: CPU tensors reach every message
    g = lambda *sh, **kw: torch.zeros(*sh, **kw)
    with pytest.raises(_lib.GsrError, match="rows must be float32, got float64"):
        s.box_sort_rows(g(5, 26, dtype=torch.float64), 17, 10)
    with pytest.raises(_lib.GsrError, match=r"rows must have shape \[P, D\]"):
        s.box_sort_rows(g(5, 26, 1), 17, 10)
    with pytest.raises(_lib.GsrError, match=r"xyz_col=24 not in"):
        s.box_sort_rows(g(5, 26), 24, 10)
    with pytest.raises(_lib.GsrError, match=r"means3D must have shape \[P, 3\]"):
        s.visible_union_tensors(cams, g(4, 2), g(4, 3), g(4, 4))
    with pytest.raises(_lib.GsrError, match="means3D must be float32, got float16"):
        s.visible_union_tensors(cams, g(4, 3, dtype=torch.float16), g(4, 3), g(4, 4))
    with pytest.raises(_lib.GsrError, match="exactly one of"):
        s.visible_union_tensors(cams, g(4, 3), g(4, 3), g(4, 4), g(4, 6))
    with pytest.raises(_lib.GsrError, match="exactly one of"):
        s.visible_union_tensors(cams, g(4, 3), g(4, 3))
    with pytest.raises(_lib.GsrError, match="exactly one of"):
        s.visible_union_tensors(cams, g(4, 3))
    with pytest.raises(_lib.GsrError, match="raw_params needs scales and rotations"):
        s.visible_union_tensors(cams, g(4, 3), cov3D_precomp=g(4, 6), raw_params=True)
    with pytest.raises(_lib.GsrError, match=r"rotations must have shape \[4, 4\]"):
        s.visible_union_tensors(cams, g(4, 3), g(4, 3), g(4, 3))
    with pytest.raises(_lib.GsrError, match="scales must be float32, got int32"):
        s.visible_union_tensors(cams, g(4, 3), g(4, 3, dtype=torch.int32), g(4, 4))
    with pytest.raises(_lib.GsrError, match="cov3D_precomp must be a torch.Tensor"):
        s.visible_union_tensors(cams, g(4, 3), cov3D_precomp=np.zeros((4, 6), np.float32))
    meta3 = meta(4, 3)
    with pytest.raises(_lib.GsrError, match="means3D must be on a HIP device, got meta"):
        s.visible_union_tensors(cams, meta3, meta(4, 3), meta(4, 4))


def test_camera_matrices_are_staged_in_one_block():
    """numpy cameras: every matrix of the call in one [B, 2, 16] host block (one upload); the halves come back in camera order."""
    from gaussian_transformer_amd import synth
    s = seq()
    cams = synth.tiramisu_ring_cameras(5, 64, 48)
    view, proj = s._camera_matrices(cams, torch.device("cpu"))
    assert view.shape == proj.shape == (5, 16) and view.is_contiguous() and proj.is_contiguous()
    for b, c in enumerate(cams):
        assert (view[b].numpy() == np.asarray(c.world_view_transform, np.float32).reshape(16)).all()
        assert (proj[b].numpy() == np.asarray(c.full_proj_transform, np.float32).reshape(16)).all()
    tc = [type("C", (), dict(world_view_transform=torch.tensor(c.world_view_transform), full_proj_transform=torch.tensor(c.full_proj_transform)))
          for c in cams]
    v2, p2 = s._camera_matrices(tc, torch.device("cpu"))          # tensors already on the target device: stacked there
    assert torch.equal(v2, view) and torch.equal(p2, proj)
