"""CPU tests of the row glue's host side: the torch restatements (tests/rows_ref.py) against sequence.unflatten_gaussians and
autograd through it, the header / ctypes contract, and validation without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib
from gaussian_transformer_amd.sequence import unflatten_gaussians
from tests import rows_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = dict(xyz="_xyz", f_dc="_features_dc", f_rest="_features_rest", opacity="_opacity", scaling="_scaling", rotation="_rotation")


@pytest.mark.parametrize("D", [17, 26, 41, 62])
@pytest.mark.parametrize("P", [1, 65, 300])
def test_unpack_ref_is_unflatten_made_contiguous(P, D):
    rows = rr.planted_rows(P, D, seed=P + D)
    flat = rr.bits(rows).numpy().view(np.uint32)
    for s in rr.SPECIALS:
        assert (flat == s).any(), hex(int(s))                    # NaN payloads, +-inf, -0.0 and denormals are all there
    got = rr.unpack_ref(rows)
    g = unflatten_gaussians(rows)
    assert list(got) == ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"]
    for name, attr in NAMES.items():
        want = getattr(g, attr).contiguous()
        assert got[name].shape == want.shape and got[name].is_contiguous(), name
        assert torch.equal(rr.bits(got[name]), rr.bits(want)) if want.numel() else got[name].numel() == 0, name
    K = (D - 14) // 3
    assert got["f_rest"].shape == (P, K - 1, 3) and g.max_sh_degree == int(round(K ** 0.5)) - 1
    assert sum(v.numel() for v in got.values()) == P * (D - 3) == rr.arena_floats(P, D)          # the flags are in no buffer


@pytest.mark.parametrize("D", [17, 26, 62])
def test_pack_ref_of_one_arena_is_the_arena_bits(D):
    P = 130
    (a,) = rr.planted_arenas(1, P, D, seed=D)
    out = rr.pack_ref([a], P, D)
    off, seen_negzero = 0, 0
    for name, col, w in rr.blocks(D):
        blk = a[off:off + P * w].reshape(P, w)
        assert torch.equal(rr.bits(out[:, col:col + w]), rr.bits(blk)), name
        seen_negzero += int((rr.bits(blk) == -2 ** 31).sum())
        off += P * w
    assert off == a.numel() and seen_negzero >= 10                  # -0.0 went through
    assert (rr.bits(out[:, D - 3:]) == 0).all()                     # flags: +0.0 by bit pattern


@pytest.mark.parametrize("D", [17, 26, 62])
@pytest.mark.parametrize("B", [2, 3, 5])
def test_pack_ref_is_the_ordered_sum_and_what_autograd_gives(B, D):
    P = 97
    arenas = rr.planted_arenas(B, P, D, seed=10 * B + D)
    got = rr.pack_ref(arenas, P, D)
    # the ordered float32 sum, written out independently with numpy
    want = np.zeros((P, D), np.float32)
    off = 0
    for _, col, w in rr.blocks(D):
        acc = arenas[0].numpy()[off:off + P * w].copy()
        for a in arenas[1:]:
            acc = (acc + a.numpy()[off:off + P * w]).astype(np.float32)
        want[:, col:col + w] = acc.reshape(P, w)
        off += P * w
    assert np.array_equal(got.numpy(), want)
    # autograd through unflatten_gaussians, one camera at a time (every column of rows hangs on exactly one parameter: 0 + x is exact),
    # the cameras' results added in order.  Slice backward turns -0.0 into +0.0: equal as values, not as bits.
    rows = torch.randn(P, D, requires_grad=True)
    g = unflatten_gaussians(rows)
    total = None
    for a in arenas:
        outs, gouts, off = [], [], 0
        for name, _, w in rr.blocks(D):
            t = getattr(g, NAMES[name])
            if t.numel():
                outs.append(t)
                gouts.append(a[off:off + P * w].reshape(t.shape))
            off += P * w
        (gr,) = torch.autograd.grad(outs, rows, gouts, retain_graph=True)
        total = gr if total is None else total + gr
    assert torch.equal(total, got)
    # the order matters at all: another order gives other bits somewhere (B >= 3)
    if B >= 3:
        assert not torch.equal(rr.bits(rr.pack_ref(arenas[::-1], P, D)), rr.bits(got))


def test_header_declares_exactly_what_the_ctypes_stub_binds():
    header = open(os.path.join(ROOT, "include", "gsr_rows.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decls = dict(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", code, flags=re.S))
    assert set(decls) == {"gsr_rows_unpack", "gsr_rows_grad_pack"}
    assert set(_lib.ROWS_SIGNATURES) == set(decls)
    for name, args in decls.items():
        assert len(_lib.ROWS_SIGNATURES[name][1]) == len(args.split(",")), name
    others = set(_lib.SIGNATURES) | set(_lib.CHAMFER_SIGNATURES) | set(_lib.SEQUENCE_SIGNATURES) | set(_lib.DENSITY_SIGNATURES)
    assert not set(_lib.ROWS_SIGNATURES) & others
    assert "#define GSR_ABI_VERSION 2" in open(os.path.join(ROOT, "include", "gsr.h")).read()   # purely additive
    assert "#define GSR_ROWS_MAX_B 64" in header and "P (3 K + 11) floats" in header              # the arena layout is stated
    from gaussian_transformer_amd import build, rows
    assert build.SOURCES["rows.hip"] == [] and rows.MAX_B == 64
    lib = _lib.load()
    for name in decls:
        assert hasattr(lib, name)


def test_validation_names_the_argument_before_any_native_call(monkeypatch):
    from gaussian_transformer_amd import rows as R
    from gaussian_transformer_amd.render import PipelineParams

    def no_native(*_a, **_k):
        raise AssertionError("the native library was reached")
    monkeypatch.setattr(_lib, "load", no_native)
    monkeypatch.setattr(R, "get_backend", no_native)
    pipe, bg, cams = PipelineParams(), torch.zeros(3), [object()]
    g = lambda *sh, **kw: torch.zeros(*sh, **kw)
    calls = (lambda x: R.render_rows(cams, x, pipe, bg), "render_rows"), (lambda x: R.unpack_rows(x), "unpack_rows")
    for call, who in calls:
        with pytest.raises(_lib.GsrError, match=f"{who}: rows must be a torch.Tensor, got ndarray"):
            call(np.zeros((5, 26), np.float32))
        with pytest.raises(_lib.GsrError, match=f"{who}: rows must be float32, got float64"):
            call(g(5, 26, dtype=torch.float64))
        with pytest.raises(_lib.GsrError, match=rf"{who}: rows must have shape \[P, D\], got \(5, 26, 1\)"):
            call(g(5, 26, 1))
        for D in (16, 18, 27, 20, 29, 35, 65):                     # 20, 29, 35: 3 K + 14 with K = 2, 5, 7, no square number
            with pytest.raises(_lib.GsrError, match=rf"{who}: rows must have D = 3 K \+ 14 columns.*got D={D}"):
                call(g(5, D))
        for D in (17, 26, 41, 62):
            with pytest.raises(RuntimeError, match=rf"{who}: rows must be on a HIP device, got cpu \(no CPU fallback\)"):
                call(g(5, D))
        with pytest.raises(_lib.GsrError, match=f"{who}: rows must be on a HIP device, got meta"):
            call(torch.empty(5, 26, device="meta"))
    with pytest.raises(_lib.GsrError, match="render_rows: cameras must hold at least one camera"):
        R.render_rows([], g(5, 26), pipe, bg)
    for bad in (2, -1, 1.0):
        with pytest.raises(_lib.GsrError, match="render_rows: sh_degree=.* not in 0..1"):
            R.render_rows(cams, g(5, 26), pipe, bg, sh_degree=bad)


def test_native_refusals_need_no_device():
    """The entry points validate on the host before anything is enqueued: sizes, B, NULL, alignment and overlap are refused with a
    code and a text in gsr_last_error() (pointers are only compared, never followed), and P = 0 is accepted."""
    import ctypes as C
    lib = _lib.load()
    P, D = 10, 26
    base = 1 << 20                                                 # made-up device addresses, 16-byte aligned and far apart
    rows, xyz, dc, rest, op, sc, rot, grad = (base * (i + 1) for i in range(8))
    arenas = (C.c_void_p * 65)(*[base * 16 + 4096 * b for b in range(65)])

    def refused(rc, text):
        msg = lib.gsr_last_error().decode()
        assert rc == 1 and text in msg, (rc, msg)
    refused(lib.gsr_rows_unpack(None, P, 18, rows, xyz, dc, rest, op, sc, rot), "gsr_rows_unpack: D=18 is not 3 K + 14")
    refused(lib.gsr_rows_unpack(None, P, 14, rows, xyz, dc, rest, op, sc, rot), "D=14")
    refused(lib.gsr_rows_unpack(None, P, 65, rows, xyz, dc, rest, op, sc, rot), "D=65")
    refused(lib.gsr_rows_unpack(None, -1, D, rows, xyz, dc, rest, op, sc, rot), "P=-1 is negative")
    refused(lib.gsr_rows_unpack(None, 2 ** 31 - 1, D, rows, xyz, dc, rest, op, sc, rot), "too large")
    refused(lib.gsr_rows_unpack(None, P, D, rows, xyz, dc, None, op, sc, rot), "f_rest must be NULL if and only if K = 1")
    refused(lib.gsr_rows_unpack(None, P, 17, rows, xyz, dc, rest, op, sc, rot), "f_rest must be NULL if and only if K = 1")
    refused(lib.gsr_rows_unpack(None, P, D, rows, None, dc, rest, op, sc, rot), "null pointer")
    refused(lib.gsr_rows_unpack(None, P, D, rows, xyz, dc, rest, op, sc, rot + 4), "rotation must be 16-byte aligned")
    refused(lib.gsr_rows_unpack(None, P, D, rows, xyz, dc, rest, rows + 4 * (P * D - 1), sc, rot), "opacity overlaps rows")
    refused(lib.gsr_rows_unpack(None, P, D, rows, xyz, dc, rows - 4 * (9 * P - 1), op, sc, rot), "f_rest overlaps rows")
    assert lib.gsr_rows_unpack(None, 0, D, None, None, None, rest, None, None, None) == 0
    assert lib.gsr_rows_unpack(None, 0, 17, None, None, None, None, None, None, None) == 0
    assert lib.gsr_rows_unpack(None, 0, D, None, None, None, None, None, None, None) == 0       # P = 0: no pointer is looked at
    refused(lib.gsr_rows_unpack(None, 0, 18, None, None, None, None, None, None, None), "D=18")
    refused(lib.gsr_rows_grad_pack(None, 0, D, 65, None, None), "B=65")
    assert lib.gsr_rows_grad_pack(None, 0, D, 1, None, None) == 0
    refused(lib.gsr_rows_grad_pack(None, P, 18, 1, arenas, grad), "gsr_rows_grad_pack: D=18")
    refused(lib.gsr_rows_grad_pack(None, P, D, 0, arenas, grad), "B=0 not in 1..64")
    refused(lib.gsr_rows_grad_pack(None, P, D, 65, arenas, grad), "B=65 not in 1..64")
    refused(lib.gsr_rows_grad_pack(None, P, D, 1, None, grad), "arenas (host array) required")
    refused(lib.gsr_rows_grad_pack(None, P, D, 1, arenas, None), "grad_rows is NULL")
    refused(lib.gsr_rows_grad_pack(None, P, D, 3, arenas, arenas[2] + 4 * (P * 23 - 1)), "grad_rows overlaps arenas[2]")
    refused(lib.gsr_rows_grad_pack(None, P, D, 3, arenas, arenas[1] - 4 * (P * D - 1)), "grad_rows overlaps arenas[1]")
    refused(lib.gsr_rows_grad_pack(None, P, D, 2, (C.c_void_p * 2)(base, None), grad), "arenas[1] is NULL")
    refused(lib.gsr_rows_grad_pack(None, P, D, 1, (C.c_void_p * 1)(base + 2), grad), "arenas[0] is not 4-byte aligned")
    assert lib.gsr_rows_grad_pack(None, 0, D, 64, arenas, None) == 0
    # the text went where every other entry point's goes: the next refusal elsewhere replaces it
    assert lib.gsr_set_option(b"no_such_option", 1) == 1 and b"no_such_option" in lib.gsr_last_error()


@pytest.mark.parametrize("deg,seed,P", [(1, 41, 1501), (3, 43, 1501), (0, 45, 300), (1, 47, 257)])
def test_seeds_of_the_gpu_cases_meet_their_sanity_condition_on_the_oracle(deg, seed, P):
    """The scenes tests/test_gpu_rows.py renders (seeds 41, 43, 45, 47), on the float32 CPU oracle through render() and autograd:
    under each of the three cameras the row gradient reaches all five parameter column groups and leaves the flags at zero, and
    every pair of cameras sees common Gaussians -- the condition that gives the ordered-sum comparison on the GPU its meaning."""
    from gaussian_transformer_amd import rasterizer, synth
    from gaussian_transformer_amd.model import GaussianParams
    from gaussian_transformer_amd.render import PipelineParams, TorchCamera, render
    from gaussian_transformer_amd.sequence import flatten_gaussians
    from tests.oracle_backend import OracleBackend
    sc = synth.make_scene(P, 128, 80, sh_degree=deg, seed=seed)
    rows = flatten_gaussians(GaussianParams.from_synthetic(sc, "cpu", requires_grad=False)).requires_grad_()
    D = int(rows.shape[1])
    K = (D - 14) // 3
    assert K == (deg + 1) ** 2
    cams = [sc.camera, synth.identity_camera(96, 64), synth.identity_camera(50, 37, tanfovx=0.3)]
    prev = rasterizer._set_backend_for_tests(OracleBackend())
    try:
        seen = []
        for b, cam in enumerate(cams):
            out = render(TorchCamera(cam, "cpu"), unflatten_gaussians(rows), PipelineParams(), torch.tensor(sc.bg))
            G = torch.tensor(np.random.default_rng(seed + 100 + b).normal(size=tuple(out["render"].shape)).astype(np.float32))
            (g,) = torch.autograd.grad(out["render"], rows, G)
            groups = dict(features=g[:, :3 * K], rotation=g[:, 3 * K:3 * K + 4], opacity=g[:, 3 * K + 4:3 * K + 5],
                          xyz=g[:, 3 * K + 5:3 * K + 8], scaling=g[:, 3 * K + 8:3 * K + 11])
            for name, v in groups.items():
                assert int((v != 0).any(1).sum()) > 50, (b, name)
            assert not g[:, 3 * K + 11:].any()
            seen.append(out["radii"] > 0)
        for i in range(3):
            for j in range(i + 1, 3):
                assert int((seen[i] & seen[j]).sum()) > 100, (i, j)
    finally:
        rasterizer._set_backend_for_tests(prev)
