"""include/gsr_absgrad.h without a device: the header against the ctypes table, the refusals that are decided before the HIP runtime is
asked for anything, the collector (AbsGrad, collect_absgrad) on HipBackend.backward with the library stood in for, and the `absgrad=`
keyword of the density statistics on CPU tensors against the formula written out in torch."""
import contextlib
import ctypes as C
import os
import re
import types

import pytest
import torch

from gaussian_transformer_amd import _lib, rasterizer
from gaussian_transformer_amd.densify import DensityController
from gaussian_transformer_amd.rasterizer import GaussianRasterizationSettings
from tests import density_ref
from tests.test_density_host import make_controller

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, WORKSPACE = 0, 1, 4
SENTINEL = "gsr_set_option: unknown option 'sentinel'"
BIG = 1 << 40
A = 1 << 20                        # made-up device addresses, only compared, never followed


def test_header_declares_exactly_what_the_ctypes_stub_binds():
    header = open(os.path.join(ROOT, "include", "gsr_absgrad.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decls = dict(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", code, flags=re.S))
    assert set(decls) == {"gsr_absgrad_workspace_bytes", "gsr_absgrad_backward"} == set(_lib.ABSGRAD_SIGNATURES)
    for name, args in decls.items():
        assert len(_lib.ABSGRAD_SIGNATURES[name][1]) == len(args.split(",")), name
    others = (_lib.SIGNATURES, _lib.CHAMFER_SIGNATURES, _lib.SEQUENCE_SIGNATURES, _lib.ROWS_SIGNATURES, _lib.DENSITY_SIGNATURES,
              _lib.MCMC_SIGNATURES, _lib.DEPTH_SIGNATURES, _lib.FEATURES_SIGNATURES, _lib.POSE_SIGNATURES, _lib.CONTRIB_SIGNATURES)
    assert not any(set(_lib.ABSGRAD_SIGNATURES) & set(t) for t in others)
    assert "#define GSR_ABI_VERSION 2" in open(os.path.join(ROOT, "include", "gsr.h")).read()   # purely additive
    low = header.lower()
    assert "only the colour image's loss enters" in low and "deterministic_bwd" in low and "raw_params" in low and "+0.0" in low
    from gaussian_transformer_amd import build
    assert build.SOURCES["absgrad.hip"] == build.SOURCES["depth_maps.hip"]
    lib = _lib.load()
    for name in decls:
        assert hasattr(lib, name)


def acc_rows(P):
    return max(P, 1) + max(P, 1) // 32 + 1024


@pytest.mark.parametrize("P", [0, 1, 31, 32, 1000, 123457])
def test_workspace_bytes(P):
    want = 2 * ((8 * acc_rows(P) + 255) // 256 * 256)
    assert _lib.workspace_bytes("gsr_absgrad_workspace_bytes", P) == want


def bwd(**kw):
    a = dict(P=10, W=32, H=32, R=100, bg=5 * A, dL=6 * A, geom=A, geom_n=BIG, binning=2 * A, binning_n=BIG, img=3 * A, img_n=BIG,
             ws=4 * A, ws_n=BIG, accumulate=0, out=7 * A, signed=None)
    a.update(kw)
    return lambda L: L.gsr_absgrad_backward(None, a["P"], a["W"], a["H"], a["R"], a["bg"], a["dL"], a["geom"], a["geom_n"], a["binning"],
                                            a["binning_n"], a["img"], a["img_n"], a["ws"], a["ws_n"], a["accumulate"], a["out"], a["signed"])


B = "gsr_absgrad_backward: "
MISSING = B + "missing input, workspace or output buffer"
CASES = [
    (bwd(P=-1), INVALID, B + "bad sizes"),
    (bwd(W=0), INVALID, B + "bad sizes"),
    (bwd(H=-3), INVALID, B + "bad sizes"),
    (bwd(R=-1), INVALID, B + "bad sizes"),
    (bwd(W=65536 * 16), INVALID, "image too large"),
    (bwd(P=0, out=None, geom=None, ws=None, bg=None), OK, SENTINEL),             # nothing to do: nothing is looked at
    (bwd(bg=None), INVALID, MISSING),
    (bwd(dL=None), INVALID, MISSING),
    (bwd(geom=None), INVALID, MISSING),
    (bwd(img=None), INVALID, MISSING),
    (bwd(ws=None), INVALID, MISSING),
    (bwd(out=None), INVALID, MISSING),
    (bwd(binning=None), INVALID, B + "binning workspace missing"),
    (bwd(ws_n=2 * 8448 - 1), WORKSPACE, re.compile(r"absgrad workspace 16895 < 16896")),   # P = 10: 1035 rows of 8 bytes, rounded up to 256, twice
    (bwd(P=1 << 28), INVALID, B + "P too large for the 28-bit accumulator row index"),
    (bwd(R=0, binning=None, accumulate=1), OK, SENTINEL),                        # nothing was composited and nothing is to be cleared
    # the order: sizes, pointers, the binning workspace, the workspace's size
    (bwd(W=0, out=None, ws_n=0), INVALID, B + "bad sizes"),
    (bwd(out=None, binning=None, ws_n=0), INVALID, MISSING),
    (bwd(binning=None, ws_n=0), INVALID, B + "binning workspace missing"),
    # (R == 0 with accumulate = 0 clears the output, and the workspaces of the forward pass are checked by view_geom, which asks the
    # HIP runtime for two temporary sizes: tests/test_gpu_absgrad_cabi.py)
]


@pytest.mark.parametrize("k", range(len(CASES)), ids=[f"{k:02d}" for k in range(len(CASES))])
def test_return_code_and_message(k):
    call, rc, text = CASES[k]
    lib = _lib.load()
    assert lib.gsr_set_option(b"sentinel", 0) == INVALID and lib.gsr_last_error().decode() == SENTINEL
    got, said = call(lib), lib.gsr_last_error().decode()
    assert got == rc
    assert said == text if isinstance(text, str) else text.fullmatch(said), said


def test_deterministic_bwd_is_refused_by_name():
    lib = _lib.load()
    was = _lib.get_option("deterministic_bwd")
    try:
        _lib.set_option("deterministic_bwd", 1)
        assert bwd()(lib) == INVALID
        said = lib.gsr_last_error().decode()
        assert said.startswith(B + "not available while the option deterministic_bwd is on") and "float atomics" in said
        assert bwd(ws_n=0)(lib) == INVALID                                       # before the workspace's size
        assert bwd(binning=None)(lib) == INVALID and lib.gsr_last_error().decode() == B + "binning workspace missing"      # after the pointers
    finally:
        _lib.set_option("deterministic_bwd", was)
    n = C.c_size_t(0)
    assert lib.gsr_absgrad_workspace_bytes(-1, C.byref(n)) == INVALID and lib.gsr_last_error().decode() == "gsr_absgrad_workspace_bytes: bad argument"
    assert lib.gsr_absgrad_workspace_bytes(5, None) == INVALID


# ---- the collector on HipBackend.backward, the library stood in for ----
class _Buf(rasterizer.AbsGrad):
    def __init__(self, P):                     # CPU tensors: the library never sees them here
        self.P, self.device, self.grad, self.views = P, torch.device("cpu"), torch.zeros((P, 2)), 0


@pytest.fixture
def backend(monkeypatch):
    calls = []
    be = object.__new__(rasterizer.HipBackend)
    be.lib = types.SimpleNamespace(gsr_backward=lambda *a: calls.append(("gsr_backward", a)) or 0)
    be._ws_cache, be._announced, be._bin_hint, be._arena_claims = {}, {}, {}, {}
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: types.SimpleNamespace(cuda_stream=77))
    monkeypatch.setattr(_lib, "workspace", lambda sizer, dev, *sizes: calls.append((sizer, sizes)) or torch.empty(16, dtype=torch.uint8))
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append((name, a)))
    return be, calls


def run_backward(be, P=6, W=8, H=4):
    rs = GaussianRasterizationSettings(H, W, 0.5, 0.5, torch.tensor([0.2, 0.5, 0.9]), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False, False)
    e = torch.empty(0)
    u8 = torch.zeros(32, dtype=torch.uint8)
    dL = torch.ones((3, H, W))
    out = be.backward(rs, 11, dL, torch.zeros((P, 3)), torch.ones(P, dtype=torch.int32), torch.zeros((P, 1, 3)), e, torch.ones((P, 3)),
                      torch.ones((P, 4)), e, u8, u8.clone(), u8.clone())
    return out, dL


def test_the_collector_adds_once_per_reverse_pass_and_nothing_runs_without_it(backend):
    be, calls = backend
    run_backward(be)
    assert [c[0] for c in calls] == ["gsr_backward_workspace_bytes", "gsr_backward"]
    del calls[:]
    buf = _Buf(6)
    with rasterizer.collect_absgrad(buf) as got:
        assert got is buf and rasterizer._absgrad_buf is buf
        run_backward(be)
        run_backward(be)
    assert rasterizer._absgrad_buf is None and buf.views == 2
    names = [c[0] for c in calls]
    assert names == ["gsr_backward_workspace_bytes", "gsr_backward", "gsr_absgrad_workspace_bytes", "gsr_absgrad_backward"] * 2
    a = calls[3][1]
    # stream P W H R bg dL geom n binning n img n ws n accumulate absgrad signed_sum
    assert a[:5] == (77, 6, 8, 4, 11) and a[8] == a[10] == a[12] == 32 and a[14] == 16 and a[15] == 1
    assert a[16] == buf.grad.data_ptr() and a[17] is None and a[5] is not None and a[6] is not None
    assert calls[2][1] == (6,)
    del calls[:]
    run_backward(be)
    assert [c[0] for c in calls] == ["gsr_backward_workspace_bytes", "gsr_backward"] and buf.views == 2
    assert buf.zero_() is buf and buf.views == 0


def test_the_collector_refuses_another_P_another_device_and_nesting(backend):
    be, calls = backend
    buf = _Buf(7)
    with rasterizer.collect_absgrad(buf):
        with pytest.raises(_lib.GsrError, match="collect_absgrad: the collector holds 7 Gaussians on cpu, the render has 6 on cpu"):
            run_backward(be)
        with pytest.raises(_lib.GsrError, match="collectors do not nest"):
            with rasterizer.collect_absgrad(_Buf(6)):
                pass
        assert rasterizer._absgrad_buf is buf                  # the refused one changed nothing
        buf.device = torch.device("meta")
        with pytest.raises(_lib.GsrError, match="holds 7 Gaussians on meta, the render has 6 on cpu"):
            run_backward(be, P=6)
    assert rasterizer._absgrad_buf is None and buf.views == 0
    assert "gsr_absgrad_backward" not in [c[0] for c in calls]


# ---- the density statistics ----
def _views(P, seed=3):
    gen = torch.Generator().manual_seed(seed)
    grad = torch.randn((P, 3), generator=gen) * 1e-3
    absg = torch.rand((P, 2), generator=gen) * torch.exp(8 * torch.rand((P, 1), generator=gen) - 8)
    radii = torch.randint(-1, 40, (P,), generator=gen, dtype=torch.int32).clamp_min(0)
    return grad, absg, radii, radii > 0


@pytest.mark.parametrize("form", ["AbsGrad", "tensor"])
def test_record_with_absgrad_is_the_formula_bit_for_bit(form):
    P = 257
    d = density_ref.build_inputs(P, 3)
    grad, absg, radii, vis = _views(P)
    vs = torch.zeros((P, 3)); vs.grad = grad
    buf = _Buf(P); buf.grad.copy_(absg)
    arg = buf if form == "AbsGrad" else absg
    with torch.no_grad():
        # without the keyword: what it returned before
        plain = make_controller(density_ref.clone_inputs(d))
        start = [t.clone() for t in (plain.model.xyz_gradient_accum, plain.model.denom, plain.model.max_radii2D)]
        plain.record(vs, vis, radii)
        want = start[0].clone(); want[vis] += torch.norm(grad[vis, :2], dim=-1, keepdim=True)
        assert torch.equal(plain.model.xyz_gradient_accum, want)
        # with it: the same statement on the absgrad rows; visibility, denom and max_radii2D as before
        ctl = make_controller(density_ref.clone_inputs(d))
        ctl.record(vs, vis, radii, absgrad=arg)
        want = start[0].clone(); want[vis] += torch.norm(absg[vis, :2], dim=-1, keepdim=True)
        assert torch.equal(ctl.model.xyz_gradient_accum, want) and not torch.equal(want, plain.model.xyz_gradient_accum)
        assert torch.equal(ctl.model.denom, plain.model.denom) and torch.equal(ctl.model.max_radii2D, plain.model.max_radii2D)
        den = start[1].clone(); den[vis] += 1
        mx = start[2].clone(); mx[vis] = torch.max(mx[vis], radii[vis].float())
        assert torch.equal(ctl.model.denom, den) and torch.equal(ctl.model.max_radii2D, mx)
        # after_backward hands it on; GaussianParams.add_densification_stats takes it too
        other = make_controller(density_ref.clone_inputs(d))
        other.after_backward(1, vs, vis, radii, 1.0, absgrad=arg)
        assert torch.equal(other.model.xyz_gradient_accum, ctl.model.xyz_gradient_accum)
        third = make_controller(density_ref.clone_inputs(d))
        third.model.add_densification_stats(vs, vis, absgrad=arg)
        assert torch.equal(third.model.xyz_gradient_accum, ctl.model.xyz_gradient_accum)
        with pytest.raises(ValueError, match=r"absgrad must be a rasterizer.AbsGrad or a \[257, 2\] tensor"):
            ctl.record(vs, vis, radii, absgrad=absg[:5])
    assert isinstance(ctl, DensityController)
