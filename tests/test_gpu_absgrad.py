"""-m gpu: absgrad (include/gsr_absgrad.h) -- gsr_absgrad_backward through ctypes on the workspaces of a render, and the public
collector (AbsGrad, collect_absgrad) around GaussianRasterizer / render / render_fused / render_rows and the density controllers.

Scenes: the five of tests/depth_ref.py, tests/test_gpu_depth.py's REPLICA (one Gaussian over all 272 tiles: replica rows) and
depth_ref.LARGE (more than 6144 tiles: the other forward route, empty tiles), all on the background (0.2, 0.5, 0.9) under
dL_dcolor ~ N(0,1); SCENES[2] also under the sign pattern of an L1 loss.  The reference is tests/absgrad_ref.py's float32 and float64
walks of the oracle's lists (LARGE: the float32 walk only), computed once per scene and shared.

1. Against the reference, helpers.grad_rows on the [P,2] rows -- the project's gates for every other gradient, as they stand:
   device against the float32 walk: fail fraction <= F32_FAIL_FRAC_MAX, p99 <= F32_P99_MAX; device against the float64 walk: fail
   fraction <= 2 x the float32 walk's + 1e-3, p99 <= max(GRAD_RTOL, 2 x its p99).
2. The signed output against dL_dmeans2D[:, :2] of the same render's gsr_backward (device against device, every decision shared), by
   the same gates; absgrad >= |signed_sum| (1 - 1e-5) on every row; and on every scene with P >= 64 the median of
   ||absgrad|| / ||dL/dmeans2D|| over the rows with a gradient exceeds 1.3 (the reference's medians: 1.7 .. 8.9) -- an implementation
   that returns the signed gradient fails here.
3. Exactness where there is nothing to decide: +0.0 rows, accumulate = 1, zero inputs.
4. Every forward route of tests/test_gpu_depth_routes.FWD_ROUTES passes gate 1; `det` is refused by name.
5. The collector: views add; maps add nothing; the two density controllers agree; nothing new without a collector.

Observed on an MI355X, default route (fail fraction / p99 through grad_rows; the float32 walk's own figures against the float64 walk
in brackets; the last column is the median of ||absgrad|| / ||dL/dmeans2D||):
    scene      device vs float32 walk   device vs float64 walk (float32 walk)        signed vs gsr_backward   ratio
    SCENES[0]  0 / 1.8e-7               0 / 2.5e-7        (0 / 1.5e-7)               0 / 3.0e-8               1.70
    SCENES[1]  0 / 3.9e-7               0 / 3.3e-6        (0 / 3.3e-6)               0 / 8.2e-7               2.01
    SCENES[2]  0 / 5.3e-7               0 / 4.4e-6        (0 / 4.5e-6)               0 / 1.2e-6               2.94
    SCENES[3]  0 / 5.5e-7               3.35e-4 / 1.1e-5  (3.35e-4 / 1.1e-5)         0 / 1.5e-6               2.68
    SCENES[4]  0 / 9.3e-7               0 / 5.3e-6        (0 / 5.2e-6)               0 / 4.1e-6               3.08
    REPLICA    0 / 2.4e-7               0 / 6.4e-6        (0 / 6.4e-6)               0 / 9.0e-7               8.89
    LARGE      0 / 4.2e-7               -                                            0 / 2.9e-6               52.3
    SCENES[2], L1 sign pattern: 0 / 5.1e-7 and 0 / 4.3e-6 (0 / 4.2e-6).
The largest single-row error against the float32 walk is 2.8e-6 (SCENES[4]); on SCENES[3] the device misses the same one row in 2981
against float64 that the float32 walk misses (one borderline decision).  The 36 route cases stay inside the same figures; the two
controllers' statistics are bit-equal; views add to within 1.5e-7 of a row.
"""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib, synth
from gaussian_transformer_amd.densify import DensityController, FusedDensityController
from gaussian_transformer_amd.model import GaussianParams
from gaussian_transformer_amd.rasterizer import AbsGrad, GaussianRasterizer, collect_absgrad
from gaussian_transformer_amd.render import PipelineParams, TorchCamera, render, render_fused
from gaussian_transformer_amd.rows import render_rows
from gaussian_transformer_amd.sequence import flatten_gaussians
from tests import absgrad_ref as ar
from tests import density_ref
from tests import depth_ref as dr
from tests.helpers import F32_FAIL_FRAC_MAX, F32_P99_MAX, GRAD_RTOL, grad_rows
from tests.test_density_host import make_controller
from tests.test_gpu_depth import CONFIGS, IDS, REPLICA, tensors
from tests.test_gpu_depth_routes import FWD_ROUTES, options

pytestmark = pytest.mark.gpu
DEV = "cuda"
ptr = _lib.ptr


def absgrad_call(fn, rs, dL, accumulate=0, out=None, signed=True, signed_out=None):
    """gsr_absgrad_backward on the workspaces the render behind the autograd node `fn` left.  Returns (absgrad, signed_sum or None)."""
    geom, binning, img = fn.saved_tensors[7:10]
    P = int(fn.saved_tensors[1].shape[0])
    H, W = int(rs.image_height), int(rs.image_width)
    ws = _lib.workspace("gsr_absgrad_workspace_bytes", DEV, P)
    a = torch.full((P, 2), float("nan"), device=DEV) if out is None else out
    s = (torch.full((P, 2), float("nan"), device=DEV) if signed_out is None else signed_out) if signed else None
    g = torch.as_tensor(dL, device=DEV).contiguous()
    _lib.call("gsr_absgrad_backward", _lib.stream(torch.device(DEV)), P, W, H, int(fn.num_rendered), ptr(rs.bg), ptr(g), ptr(geom), geom.numel(),
              ptr(binning), binning.numel(), ptr(img), img.numel(), ptr(ws), ws.numel(), accumulate, ptr(a), ptr(s))
    return a, s


def device_run(S, dL, **opts):
    """One render of S, the absgrad call with signed sums on its workspaces, then the same render's gsr_backward."""
    with options(**opts):
        rs, inp = tensors(S)
        color, radii = GaussianRasterizer(rs)(**inp)
        a, s = absgrad_call(color.grad_fn, rs, dL)
        color.backward(torch.as_tensor(dL, device=DEV))
    return dict(abs=a.cpu().numpy(), signed=s.cpu().numpy(), m2d=inp["means2D"].grad[:, :2].cpu().numpy(), radii=radii.cpu().numpy())


@functools.lru_cache(maxsize=None)
def default_run(cfg, kind="normal"):
    S, dL, _w32, _w64 = ar.walks(cfg, kind, cfg != ar.LARGE)
    return device_run(S, dL)


def gate1(got, w32, w64, tag):
    st32 = grad_rows(got, w32["abs"])
    print(f"{tag}: device vs float32 walk: fail {st32['fail_frac']:.2e} p99 {st32['p99']:.2e} max {st32['max']:.2e} rows {st32['rows']}")
    assert st32["rows"] > 0 and st32["fail_frac"] <= F32_FAIL_FRAC_MAX and st32["p99"] <= F32_P99_MAX, st32
    if w64 is not None:
        st64, base = grad_rows(got, w64["abs"]), grad_rows(w32["abs"], w64["abs"])
        print(f"{tag}: device vs float64 walk: fail {st64['fail_frac']:.2e} p99 {st64['p99']:.2e} (float32 walk: {base['fail_frac']:.2e} {base['p99']:.2e})")
        assert st64["fail_frac"] <= 2.0 * base["fail_frac"] + 1e-3 and st64["p99"] <= max(GRAD_RTOL, 2.0 * base["p99"]), (st64, base)


ALL = CONFIGS + (ar.LARGE,)
ALL_IDS = IDS + [ar.LARGE]


# ---- 1. against the reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ALL, ids=ALL_IDS)
def test_against_the_reference(cfg):
    S, dL, w32, w64 = ar.walks(cfg, "normal", cfg != ar.LARGE)
    if cfg == ar.LARGE:
        assert ((S.W + 15) // 16) * ((S.H + 15) // 16) > 6144
    gate1(default_run(cfg)["abs"], w32, w64, str(cfg))


def test_against_the_reference_under_an_l1_sign_pattern():
    S, dL, w32, w64 = ar.walks(dr.SCENES[2], "l1")
    gate1(default_run(dr.SCENES[2], "l1")["abs"], w32, w64, "l1")


# ---- 2. the signed output ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ALL, ids=ALL_IDS)
def test_signed_sums_are_the_same_renders_means2D_gradient(cfg):
    r = default_run(cfg)
    st = grad_rows(r["signed"], r["m2d"])
    ratio = ar.ratio_median(r["abs"], r["m2d"])
    print(f"{cfg}: signed vs gsr_backward: fail {st['fail_frac']:.2e} p99 {st['p99']:.2e} max {st['max']:.2e}; median ratio {ratio:.2f}")
    assert st["rows"] > 0 and st["fail_frac"] <= F32_FAIL_FRAC_MAX and st["p99"] <= F32_P99_MAX, st
    assert (r["abs"] >= np.abs(r["signed"]) * (1 - 1e-5)).all()
    P = r["abs"].shape[0]
    if P >= 64:
        assert ratio > 1.3, ratio


# ---- 3. exactness where there is nothing to decide ---------------------------------------------------------------------------------------
def test_rows_without_a_gradient_are_exact_zeros():
    """SCENES[2] with every 50th Gaussian mirrored to behind the camera (culled: radii 0), and SCENES[3], 19 of whose Gaussians are
    blended nowhere.  The outputs were prefilled with NaN: every element was written, and a row without a gradient holds +0.0."""
    S, dL, _w32, _w64 = ar.walks(dr.SCENES[2])
    m = np.array(S.means3D, np.float32).reshape(-1, 3).copy()
    m[::50] *= -1.0
    r = device_run(dataclasses.replace(S, means3D=m), dL)
    culled = r["radii"] <= 0
    assert culled[::50].all() and culled.sum() == 10
    for k in ("abs", "signed"):
        assert np.isfinite(r[k]).all(), k
        assert (r[k][culled] == 0).all() and (r[k][~culled] != 0).any(), k
        assert not np.signbit(r[k][r[k] == 0]).any(), k
    r = default_run(dr.SCENES[3])
    never = (r["abs"] == 0).all(axis=1)
    assert never.any() and (r["radii"][never] > 0).all() and (r["m2d"][never] == 0).all()
    for k in ("abs", "signed"):
        assert np.isfinite(r[k]).all() and not np.signbit(r[k][r[k] == 0]).any(), k
    assert (r["abs"] >= 0).all() and (r["signed"][never] == 0).all()


def test_accumulate_adds_once_and_leaves_other_rows_alone():
    """known + g with ONE rounding.  Two walks differ in the order of their float atomics, so g itself is reproducible only to a few
    ulp of g; the known tensor is therefore taken in [K, 2K) with K = 16 x the largest element of g (a power of two): an ulp of
    known + g is then at least 16 ulp of any g, and what the gate sees is the add.  On the one-splat scene every sum has two terms and
    is reproducible: there the result is torch's known + g bit for bit, for any known."""
    for cfg, exact in ((dr.SCENES[2], False), (dr.SCENES[0], True)):
        S, dL, _w32, _w64 = ar.walks(cfg)
        if not exact:                       # every 50th Gaussian behind the camera: rows without a gradient
            m = np.array(S.means3D, np.float32).reshape(-1, 3).copy()
            m[::50] *= -1.0
            S = dataclasses.replace(S, means3D=m)
        with options():
            rs, inp = tensors(S)
            color, radii = GaussianRasterizer(rs)(**inp)
            fn = color.grad_fn
            a0, s0 = absgrad_call(fn, rs, dL)
            K = 2.0 ** np.ceil(np.log2(16.0 * float(a0.max())))
            gen = torch.Generator().manual_seed(3)
            known = ((1.0 + torch.rand(a0.shape, generator=gen)) * (K if not exact else 0.37)).to(DEV)
            sknown = -known.clone()
            no_grad = (radii <= 0)
            assert exact or int(no_grad.sum()) == 10
            if no_grad.any():
                known[no_grad] = torch.tensor([float("nan"), -0.0], device=DEV)
            before = known.clone()
            a1, s1 = absgrad_call(fn, rs, dL, accumulate=1, out=known.clone(), signed_out=sknown.clone())
        for got, base, g in ((a1, before, a0), (s1, sknown, s0)):
            want = base + g
            has = ~no_grad if base is before else torch.ones_like(no_grad)
            if exact:
                assert torch.equal(got[has], want[has])
            else:
                inf = torch.full_like(want, float("inf"))
                ulp = torch.maximum(torch.nextafter(want, inf) - want, want - torch.nextafter(want, -inf))
                assert (torch.abs(got - want)[has] <= ulp[has]).all()
            assert (g[has] != 0).any()
        assert torch.equal(a1[no_grad].view(torch.int32), before[no_grad].view(torch.int32))      # NaN and -0.0 as they were
        assert torch.equal(s1[no_grad], sknown[no_grad])


def test_zero_gradient_and_zero_background_give_zeros():
    S = ar.scene(dr.SCENES[2])
    with options():
        rs, inp = tensors(S)
        rs = rs._replace(bg=torch.zeros(3, device=DEV))
        color, _ = GaussianRasterizer(rs)(**inp)
        a, s = absgrad_call(color.grad_fn, rs, np.zeros((3, S.H, S.W), np.float32))
    assert not a.view(torch.int32).any() and not s.view(torch.int32).any()


# ---- 4. routes -----------------------------------------------------------------------------------------------------------------------------
ROUTE_CASES = [(r, c) for c in (dr.SCENES[4], REPLICA) for r in FWD_ROUTES if r not in ("default", "det")]


@pytest.mark.parametrize("route,cfg", ROUTE_CASES, ids=[f"{r}-{'P4000' if c != REPLICA else c}" for r, c in ROUTE_CASES])
def test_every_forward_route_passes_the_reference_gates(route, cfg):
    S, dL, w32, w64 = ar.walks(cfg)
    gate1(device_run(S, dL, **FWD_ROUTES[route])["abs"], w32, w64, f"{route} {cfg}")


def test_deterministic_bwd_is_refused_by_name_and_the_device_stays_usable():
    S, dL, w32, w64 = ar.walks(dr.SCENES[1])
    with options(**FWD_ROUTES["det"]):
        rs, inp = tensors(S)
        color, _ = GaussianRasterizer(rs)(**inp)
        out = torch.full((int(inp["means3D"].shape[0]), 2), 7.0, device=DEV)
        with pytest.raises(_lib.GsrError, match="deterministic_bwd"):
            absgrad_call(color.grad_fn, rs, dL, out=out)
        assert (out == 7.0).all()
        buf = AbsGrad(int(inp["means3D"].shape[0]), DEV)
        with collect_absgrad(buf), pytest.raises(_lib.GsrError, match="deterministic_bwd"):
            color.backward(torch.as_tensor(dL, device=DEV))
        assert buf.views == 0 and not buf.grad.any()
    gate1(device_run(S, dL)["abs"], w32, w64, "after the refusal")


# ---- 5. the collector ----------------------------------------------------------------------------------------------------------------------
def same_rows(a, b, tag):
    st = grad_rows(a.cpu().numpy(), b.cpu().numpy())
    print(f"{tag}: {st}")
    assert st["rows"] > 0 and st["fail_frac"] <= F32_FAIL_FRAC_MAX and st["p99"] <= F32_P99_MAX, (tag, st)


def test_render_render_fused_and_render_rows_add_their_views():
    sc = synth.make_scene(P=300, width=80, height=48, sh_degree=1, s0=0.06, seed=5)
    pipe, bg = PipelineParams(), torch.tensor(ar.BG, device=DEV)
    cams = [TorchCamera(sc.camera, DEV), TorchCamera(synth.identity_camera(50, 37, tanfovx=0.3), DEV)]
    gen = torch.Generator().manual_seed(1)
    targets = [torch.rand((3, int(c.image_height), int(c.image_width)), generator=gen).to(DEV) for c in cams]

    def step(which, cam_ids, buf):
        pc = GaussianParams.from_synthetic(sc, DEV, requires_grad=True)
        with collect_absgrad(buf):
            if which == "render_rows":
                rows = flatten_gaussians(pc).detach().contiguous().requires_grad_(True)
                imgs = render_rows([cams[i] for i in cam_ids], rows, pipe, bg)["renders"]
            else:
                fn = render if which == "render" else render_fused
                imgs = [fn(cams[i], pc, pipe, bg)["render"] for i in cam_ids]
            sum((img - targets[i]).abs().mean() for img, i in zip(imgs, cam_ids)).backward()
        return buf

    for which in ("render", "render_fused", "render_rows"):
        both = step(which, (0, 1), AbsGrad(300, DEV))
        one, two = step(which, (0,), AbsGrad(300, DEV)), step(which, (1,), AbsGrad(300, DEV))
        assert (both.views, one.views, two.views) == (2, 1, 1), which
        assert one.grad.any() and two.grad.any() and not torch.equal(one.grad, two.grad)
        same_rows(both.grad, one.grad + two.grad, which)
        assert both.zero_() is both and both.views == 0 and not both.grad.any()


def test_map_losses_add_nothing():
    S, dL, _w32, _w64 = ar.walks(dr.SCENES[2])
    P = int(np.asarray(S.means3D).shape[0])
    gen = torch.Generator().manual_seed(2)
    F = torch.randn((P, 5), generator=gen).to(DEV).requires_grad_(True)
    gC = torch.as_tensor(dL, device=DEV)
    bufs = []
    for with_maps in (False, True):
        rs, inp = tensors(S)
        buf = AbsGrad(P, DEV)
        with options(), collect_absgrad(buf):
            color, _radii, depth, alpha, feat = GaussianRasterizer(rs)(depth="expected", features=F, **inp)
            loss = (color * gC).sum()
            if with_maps:
                loss = loss + (depth * 0.3).sum() + (alpha * alpha).sum() + (feat * feat).sum()
            loss.backward()
        assert buf.views == 1
        bufs.append(buf.grad.clone())
    same_rows(bufs[1], bufs[0], "colour + maps against colour alone")
    same_rows(bufs[0], torch.as_tensor(default_run(dr.SCENES[2])["abs"], device=DEV), "the collector against the direct call")
    # a map loss alone: the colour pass runs on a zero gradient and adds zeros
    rs, inp = tensors(S)
    buf = AbsGrad(P, DEV)
    with options(), collect_absgrad(buf):
        out = GaussianRasterizer(rs)(depth="expected", **inp)
        out[2].sum().backward()
    assert not buf.grad.any()


def test_the_two_density_controllers_agree_bit_for_bit():
    P = 257
    d = density_ref.build_inputs(P, 3)
    a, b = (make_controller(density_ref.clone_inputs(d, DEV), cls=cls) for cls in (DensityController, FusedDensityController))
    gen = torch.Generator().manual_seed(4)
    buf = AbsGrad(P, DEV)
    buf.grad.copy_(torch.rand((P, 2), generator=gen) * torch.exp(8 * torch.rand((P, 1), generator=gen) - 8))
    radii = torch.randint(-1, 40, (P,), generator=gen, dtype=torch.int32).clamp_min(0).to(DEV)
    vis = radii > 0
    vs = torch.zeros((P, 3), device=DEV)
    vs.grad = torch.full((P, 3), float("nan"), device=DEV)           # not looked at
    with torch.no_grad():
        a.record(vs, vis, radii, absgrad=buf)
        b.record(vs, vis, radii, absgrad=buf)
        for x, y in ((a.model.xyz_gradient_accum, b.model.xyz_gradient_accum), (a.model.denom, b.model.denom), (a.model.max_radii2D, b.model.max_radii2D)):
            assert torch.equal(x, y)
        assert vis.any() and torch.isfinite(a.model.xyz_gradient_accum).all()
        b.record(vs, vis, radii, absgrad=buf.grad)                  # a tensor is taken as well
        a.after_backward(1, vs, vis, radii, 1.0, absgrad=buf.grad)
        assert torch.equal(a.model.xyz_gradient_accum, b.model.xyz_gradient_accum)


def test_without_a_collector_nothing_new_runs(monkeypatch):
    """Under deterministic_bwd the reverse pass is reproducible to the bit: two renders without a collector give the same gradients,
    the library is never asked for absgrad, and a collector that is left again leaves nothing behind."""
    S, dL, _w32, _w64 = ar.walks(dr.SCENES[3])
    called = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (called.append(name), real(name, *a))[1])

    def grads():
        with options(deterministic_bwd=1):
            rs, inp = tensors(S)
            color, _ = GaussianRasterizer(rs)(**inp)
            color.backward(torch.as_tensor(dL, device=DEV))
        return {k: v.grad.clone() for k, v in inp.items() if v is not None and v.grad is not None}
    g0 = grads()
    with collect_absgrad(AbsGrad(3, DEV)):
        pass
    g1 = grads()
    assert len(g0) >= 5 and g0.keys() == g1.keys() and all(torch.equal(g0[k], g1[k]) for k in g0)
    assert not [n for n in called if "absgrad" in n]
