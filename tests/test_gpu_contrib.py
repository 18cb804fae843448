"""-m gpu: the per-Gaussian blend-weight statistics (include/gsr_contrib.h) through the public API -- ContributionStats and
collect_contribution around GaussianRasterizer / render / render_fused / render_rows -> ctypes -> C ABI -> csrc/contrib_stats.hip.

Scenes: the five of tests/depth_ref.py and tests/test_gpu_depth.py's REPLICA (one Gaussian over all 272 tiles: 69 632 pixels into one
16-byte row), against tests/contrib_ref.py's float32 and float64 walks of the oracle's lists; depth_ref.LARGE (more than 6144 tiles:
the forward pass's other launch, and empty tiles) against the float32 walk only.

1. Against the reference, every visible Gaussian (contrib_ref.gates; the Gaussians the reference flags are held to the wider bound,
   not exempt):
       |count - count32| <= slack_count
       |sum - sum64|     <= slack_weight + count 2^-32 + rel_sum sum64
       |max - max64|     <= rel_max max64 where slack_count == 0; elsewhere max <= min(0.99, opacity) (1 + 2^-23)
   rel_sum, rel_max = 2 x (the float32 walk's own largest relative error of that field against the float64 walk on that scene) + 2e-6,
   from the two walks and never from the device (contrib_ref.rel_of).  LARGE has no float64 walk: its sum and max are held to the
   float32 walk's, with the largest rel_sum and rel_max of the six scenes (its lists, at most 23 entries, are shorter than SCENES[3]'s
   and SCENES[4]'s, whose sums set those figures); both sides then carry a float32 error of that kind.
   The tolerances and the device's measured largest relative error on clean rows (slack_count == 0), per scene, on an MI355X; no gate
   was missed on any Gaussian of any scene, and the counts equal the float32 walk's on every Gaussian of the six scenes (on LARGE
   one count differs, inside its slack):
       scene      rel_sum   device sum    rel_max   device max
       SCENES[0]  2.08e-6   4.8e-8        2.07e-6   3.2e-8
       SCENES[1]  8.10e-6   3.0e-6        7.53e-6   2.8e-6
       SCENES[2]  1.17e-5   4.8e-6        1.56e-5   6.8e-6
       SCENES[3]  2.05e-5   9.2e-6        4.07e-5   1.9e-5
       SCENES[4]  2.45e-5   2.1e-4 (*)    2.40e-5   1.1e-5
       REPLICA    1.79e-5   7.9e-6        1.49e-5   6.6e-6
       LARGE      2.45e-5   3.1e-7        4.07e-5   2.4e-7      (against the float32 walk)
   (*) on a row whose sum is of the order of 1e-5: pixels with T near 1e-4 add weights of about 1e-6 each, and each term loses up to
   2^-32 = 2.3e-10 to the truncation -- the gate's count 2^-32 term, which that row stays inside.
2. Exact gates, byte for byte -- between two device runs there is no decision to differ on: run to run; views A then B against B then
   A and against the per-view rows added in Python integers; every forward route of tests/test_gpu_depth_routes.py named in ROUTES
   against the default route; gsr_contrib_read against numpy.
3. Device self-consistency, sharing every decision: weight_sum against dL_dcolors[:, 0] of the same render's gsr_backward under a
   gradient of ones in channel 0 (helpers.grad_rows at GRAD_RTOL); the total against the alpha map; per-row invariants.
4. The collector: render, render_fused and render_rows under no_grad, the refusals, and nothing new without a collector.
"""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib, synth
from gaussian_transformer_amd.model import GaussianParams
from gaussian_transformer_amd.rasterizer import ContributionStats, GaussianRasterizer, collect_contribution
from gaussian_transformer_amd.render import PipelineParams, TorchCamera, render, render_fused
from gaussian_transformer_amd.rows import render_rows
from gaussian_transformer_amd.sequence import flatten_gaussians
from tests import contrib_ref as cr
from tests import depth_ref as dr
from tests.helpers import GRAD_RTOL, grad_rows, oracle_scene
from tests.test_gpu_depth import CONFIGS, IDS, REPLICA, scene, tensors
from tests.test_gpu_depth_routes import ALL_DEFAULTS, FWD_ROUTES, options

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROW = np.dtype([("sum_q32", "<u8"), ("max_bits", "<u4"), ("count", "<u4")])
ROUTES = ("default", "walk", "pair256", "cpp2", "npx1", "seg64", "noseg", "det", "lists1", "sort1", "nocull")
assert set(ROUTES) <= set(FWD_ROUTES) and "deterministic_bwd" in ALL_DEFAULTS


def as_rows(stats):
    return stats.rows.cpu().numpy().view(ROW).reshape(stats.P).copy()


def collect(S, settings=(None,), stats=None):
    """The rows after one no_grad render of S per entry of `settings` (None: S's own; else the scale_modifier of that view)."""
    rs, inp = tensors(S, grad=False)
    st = ContributionStats(int(inp["means3D"].shape[0]), DEV) if stats is None else stats
    with collect_contribution(st), torch.no_grad():
        for mod in settings:
            GaussianRasterizer(rs if mod is None else rs._replace(scale_modifier=mod))(**inp)
    return st


@functools.lru_cache(maxsize=None)
def default_rows(cfg):
    with options():
        return as_rows(collect(scene(cfg)))


def floats_of(rows):
    return rows["sum_q32"].astype(np.float64) * 2.0 ** -32, rows["max_bits"].view(np.float32).astype(np.float64), rows["count"].astype(np.int64)


# ---- 1. against the reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_against_the_reference(cfg):
    S, a32, a64 = cr.walks(cfg)
    rel = cr.rel_of(a32, a64)
    rows = default_rows(cfg)
    st = cr.gates(*floats_of(rows), a32, a64, rel, opacity=S.opacities)
    print(cfg, "rel", rel, st)
    assert st["visible"] > 0
    assert (st["bad_count"], st["bad_sum"], st["bad_max"]) == (0, 0, 0), st
    assert not rows[a32["radii"] == 0].view(np.uint8).any()


@functools.lru_cache(maxsize=None)
def large_scene():
    return oracle_scene(synth.make_scene(**dr.LARGE))


def test_the_large_image_against_the_float32_walk():
    S = large_scene()
    assert ((S.W + 15) // 16) * ((S.H + 15) // 16) > 6144
    a32 = cr.walk(S, "f32")
    rels = [cr.rel_of(*cr.walks(cfg)[1:]) for cfg in CONFIGS]
    rel = (max(r[0] for r in rels), max(r[1] for r in rels))
    with options():
        rows = as_rows(collect(S))
        again = as_rows(collect(S))
    st = cr.gates(*floats_of(rows), a32, a32, rel, opacity=S.opacities)
    print("large: rel", rel, st)
    assert st["visible"] > 100 and (st["bad_count"], st["bad_sum"], st["bad_max"]) == (0, 0, 0), st
    np.testing.assert_array_equal(rows, again)


# ---- 2. exact gates ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_rows_equal_from_run_to_run(cfg):
    with options():
        np.testing.assert_array_equal(as_rows(collect(scene(cfg))), default_rows(cfg))


def add_rows(a, b):
    out = np.zeros(len(a), ROW)
    out["sum_q32"] = [(int(x) + int(y)) % 2 ** 64 for x, y in zip(a["sum_q32"], b["sum_q32"])]
    out["max_bits"] = np.maximum(a["max_bits"], b["max_bits"])
    out["count"] = [(int(x) + int(y)) % 2 ** 32 for x, y in zip(a["count"], b["count"])]
    return out


@pytest.mark.parametrize("cfg", (dr.SCENES[3], dr.SCENES[4], REPLICA), ids=["P3000", "P4000", REPLICA])
def test_the_order_of_the_views_does_not_matter(cfg):
    """View B: the same Gaussians 1.3 times as large."""
    S = scene(cfg)
    with options():
        a, b = as_rows(collect(S, (None,))), as_rows(collect(S, (1.3,)))
        ab, ba = collect(S, (None, 1.3)), collect(S, (1.3, None))
    assert not np.array_equal(a, b) and (ab.views, ab.pixels_added) == (2, 2 * S.W * S.H)
    np.testing.assert_array_equal(as_rows(ab), as_rows(ba))
    np.testing.assert_array_equal(as_rows(ab), add_rows(a, b))
    np.testing.assert_array_equal(a, default_rows(cfg))


ROUTE_CASES = [(r, c) for c in (dr.SCENES[4], REPLICA) for r in ROUTES if r != "default"]


@pytest.mark.parametrize("route,cfg", ROUTE_CASES, ids=[f"{r}-{'P4000' if c != REPLICA else c}" for r, c in ROUTE_CASES])
def test_rows_identical_on_every_forward_route(route, cfg):
    """The depth map is bit-equal across these routes (tests/test_gpu_depth_routes.py) and the statistics are integer functions of the
    same weights.  `det` also shows that the call is not refused while deterministic_bwd is on."""
    with options(**FWD_ROUTES[route]):
        got = as_rows(collect(scene(cfg)))
    np.testing.assert_array_equal(got, default_rows(cfg))


@pytest.mark.parametrize("cfg", (dr.SCENES[4], REPLICA), ids=["P4000", REPLICA])
def test_read_against_numpy(cfg):
    with options():
        st = collect(scene(cfg), (None, 1.3, None))
    rows = as_rows(st)
    w_sum, w_max, n_pix = (t.cpu().numpy() for t in st.read())
    assert (w_sum.dtype, w_max.dtype, n_pix.dtype) == (np.float32, np.float32, np.int32)
    np.testing.assert_array_equal(w_sum, (rows["sum_q32"].astype(np.float64) * 2.0 ** -32).astype(np.float32))
    np.testing.assert_array_equal(w_max.view(np.uint32), rows["max_bits"])
    np.testing.assert_array_equal(n_pix, rows["count"].astype(np.int32))
    np.testing.assert_array_equal(as_rows(st), rows)                    # reading changes nothing
    st.reset()
    assert (st.views, st.pixels_added) == (0, 0) and not as_rows(st).view(np.uint8).any()


# ---- 3. device self-consistency ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_against_the_same_renders_backward_pass_and_alpha_map(cfg):
    S = scene(cfg)
    P = int(np.asarray(S.means3D).shape[0])
    col = np.zeros((P, 3), np.float32); col[:, 0] = 1.0
    Sp = dataclasses.replace(S, shs=None, colors_precomp=col, bg=np.zeros(3, np.float32), sh_degree=0)
    rs, inp = tensors(Sp)
    st = ContributionStats(P, DEV)
    with options():
        with collect_contribution(st):
            color, radii, _depth, alpha = GaussianRasterizer(rs)(depth="expected", **inp)
        color[0].sum().backward()
    rows = as_rows(st)
    assert st.views == 1
    w_sum = st.read()[0].cpu().numpy()
    g = inp["colors_precomp"].grad[:, 0].cpu().numpy()
    rep = grad_rows(w_sum[:, None], g[:, None], rtol=GRAD_RTOL)
    print(cfg, "weight_sum against dL_dcolors[:, 0]:", rep)
    assert rep["rows"] > 0 and rep["fail_frac"] == 0.0, rep
    # the total against the alpha map: sum over pixels of 1 - final_T
    pairs = sum(int(c) for c in rows["count"])
    total = sum(int(q) for q in rows["sum_q32"]) * 2.0 ** -32
    want = float(alpha.detach().double().sum())
    print(cfg, "pairs", pairs, "total", total, "alpha map", want)
    assert abs(total - want) <= pairs * 2.0 ** -32 + 1e-6 * want
    # per row, in integers: floor(max 2^32) <= sum_q32 <= count floor(max 2^32); the three fields are empty together
    qmax = [int(float(m) * 2.0 ** 32) for m in rows["max_bits"].view(np.float32)]
    for q, s, c in zip(qmax, rows["sum_q32"], rows["count"]):
        assert q <= int(s) <= int(c) * q
        assert (int(c) == 0) == (int(s) == 0) == (q == 0)
    assert rows["count"].any() and not rows[radii.cpu().numpy() == 0].view(np.uint8).any()
    np.testing.assert_array_equal(rows, default_rows(cfg))             # the records do not know the colour


# ---- 4. the collector ----------------------------------------------------------------------------------------------------------------------
def test_render_render_fused_and_render_rows_each_add_their_views():
    sc = synth.make_scene(P=300, width=80, height=48, sh_degree=1, s0=0.06, seed=5)
    pc = GaussianParams.from_synthetic(sc, DEV, requires_grad=False)
    cam, cam2 = TorchCamera(sc.camera, DEV), TorchCamera(synth.identity_camera(50, 37, tanfovx=0.3), DEV)
    pipe, bg = PipelineParams(), torch.zeros(3, device=DEV)
    st = ContributionStats(300, DEV)
    seen = {}
    with torch.no_grad():
        for name, fn in (("render", lambda: render(cam, pc, pipe, bg)), ("render_fused", lambda: render_fused(cam, pc, pipe, bg)),
                         ("render_rows", lambda: render_rows([cam, cam2], flatten_gaussians(pc).contiguous(), pipe, bg))):
            st.reset()
            with collect_contribution(st):
                out = fn()
            views = 2 if name == "render_rows" else 1
            assert (st.views, st.pixels_added) == (views, 80 * 48 + (50 * 37 if views == 2 else 0)), name
            seen[name] = as_rows(st)
            assert seen[name]["count"].any(), name
            if views == 1:
                vis = out["radii"].cpu().numpy() > 0
                assert not seen[name][~vis].view(np.uint8).any(), name
        # outside the context nothing is added
        render(cam, pc, pipe, bg)
        assert st.views == 2
    # the fused entry point forms the same activations on the device: nearly every count is the other path's
    assert (seen["render"]["count"] == seen["render_fused"]["count"]).mean() > 0.9
    assert (seen["render_rows"]["count"] >= seen["render_fused"]["count"]).all()


def test_collector_refusals_and_no_collector():
    S = scene(dr.SCENES[1])
    rs, inp = tensors(S, grad=False)
    P = int(inp["means3D"].shape[0])
    with torch.no_grad():
        color0, radii0 = GaussianRasterizer(rs)(**inp)
        st = ContributionStats(P, DEV)
        with collect_contribution(st):
            color1, radii1 = GaussianRasterizer(rs)(**inp)
        assert torch.equal(color0, color1) and torch.equal(radii0, radii1) and st.views == 1
        before = as_rows(st)
        with collect_contribution(ContributionStats(P + 1, DEV)) as other:
            with pytest.raises(_lib.GsrError, match=f"holds {P + 1} Gaussians"):
                GaussianRasterizer(rs)(**inp)
        assert other.views == 0 and not as_rows(other).view(np.uint8).any()
        st.pixels_added = 2 ** 32 - S.W * S.H                            # one pixel short of room for another view
        with collect_contribution(st):
            with pytest.raises(_lib.GsrError, match="would pass the 4294967295"):
                GaussianRasterizer(rs)(**inp)
        np.testing.assert_array_equal(as_rows(st), before)
        st.pixels_added = 2 ** 32 - 1 - S.W * S.H
        with collect_contribution(st):
            GaussianRasterizer(rs)(**inp)
        assert (st.views, st.pixels_added) == (2, 2 ** 32 - 1)
        color2, _ = GaussianRasterizer(rs)(**inp)                       # the device is as usable as before
        assert torch.equal(color2, color0)
