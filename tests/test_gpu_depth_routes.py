"""-m gpu: the depth and alpha maps (include/gsr_depth.h) on every route the forward pass can take, the reverse side under
accumulate = 1 on every mechanism by which gsr_backward writes its outputs, and workspaces that held something else before.

csrc/depth_maps.hip builds no lists and runs no per-Gaussian stage: it re-reads what gsr_forward left on the device (ranges, point_list,
the 12-float records, the reachability bytes contrib[4][R], n_contrib, final_T, the touched marks, the replica-row flags).  What is left
there depends on the forward kernel, its instrumentation, the waves per workgroup, the checkpoints, the list builder, the tile culling and
the image size.  The machinery is tests/test_gpu_depth.py's (scene, reference, render_maps, check_grads, assert_sums_agree, final_T_of,
map_grads) and the oracle is used through the colour trick of tests/depth_ref.py; the oracle's side is cached once per (scene, mode).

Scenes (figures: float32 oracle on the CPU, the reference's tile rule; the device's exact culling can only shorten a list):
  SCENES[4]  P = 4000, 64 x 64: 16 tiles, lists of 368 .. 687 entries, 2644 pixels with T_final < 1e-3 (they stop before the end of
             their list): the pair kernel, several checkpoints per half tile, the stop path
  SCENES[3]  P = 3000, 96 x 80: 30 tiles, lists of 128 .. 227: longer than one 64-entry staging batch, shorter than a 256-entry segment
  SCENES[1]  P = 64, 40 x 24: 6 ragged tiles, lists of 4 .. 31: nothing reaches the pair threshold
  REPLICA    P = 201, 272 x 256: 272 tiles, lists of 1 .. 12, one Gaussian with replica accumulator rows (>= 256 tiles)
  SH16       SCENES[2]'s Gaussians with max_sh_degree = 3 (M = 16 SH rows), 64 x 48: 12 tiles, lists of 61 .. 83
  LARGE      depth_ref.LARGE, P = 600, 1616 x 1008: 6363 tiles (> 6144), 5 of them empty, 67452 pairs, longest list 23.  The reference
             alone (float64 against float32 oracle, tests/test_depth_ref_host.py): 2 pixels over tolerance of the 16 the cap
             max(3, MAX_CERTIFIED_FRAC * pixels) allows
The same on an MI355X with exact tile culling (the default): SCENES[4] lists of 337 .. 506 (6758 pairs, 32 of 64 checkpoint slots at
256 entries per segment, all 64 at 64), SCENES[3] 115 .. 173 (4359 pairs; 114 of 128 slots at 64), SCENES[1] 4 .. 21, REPLICA 1 .. 11,
LARGE 29399 pairs, longest list 16, 65 empty tiles.  With culling off the lists are the oracle's.

Forward routes.  Every route sets every option of ALL_DEFAULTS; the line says what differs and which kernel of composite_fwd.hip's
FWD_KERNELS then runs on an image of at most 6144 tiles (make_plan, launch_composite_fwd):
  default        composite_fwd_pair_kernel<0>: lists > 64 by two waves, one per 8x8 block (fwd_unit_pair: each wave writes its own
                 block's reachability byte and stops when its block is done); shorter ones by wave 0 alone (fwd_unit<2, 0, true>)
  walk           fwd_pair_long 0: composite_fwd_walk_kernel<0>, one wave per half tile, the written-out walk
  pair256        fwd_pair_long 256: the pair kernel; two waves only for lists > 256 (SCENES[4]), every other half tile takes its
                 w == 0 branch (SCENES[3], SCENES[1], REPLICA)
  cpp2           asm_walk 0: composite_fwd_kernel<2, 0>, the C++ walk
  npx1, npx4     fwd_blocks_per_wave = bwd_blocks_per_wave = 1 / 4, persistent_bwd 0, segment_entries 0: composite_fwd_kernel<1, 0> /
                 <4, 0> (one wave per block writes one byte per entry; one wave per tile writes all four)
  wpb2, wpb4     composite_waves_per_block 2 / 4: on these images the pair kernel is launched as workgroups of two waves whatever this
                 option says -- the route pins that
  walk_wpb2, walk_wpb4  the same with fwd_pair_long 0: composite_fwd_walk_kernel<0> with 2 / 4 waves per workgroup
                 (unit = workgroup * wpb + wave), with checkpoints on SCENES[4]'s lists; LARGE (below) runs 4 waves without any
  count1         count_lanes 1: composite_fwd_kernel<2, 1>, the lane-counting C++ walk (no written-out walk, so no pair kernel)
  count2         count_lanes 2: composite_fwd_pair_kernel<2>, the wave timeline
  seg64          persistent_bwd 1, segment_entries 64: checkpoints every 64 entries (drawn through the pair's LDS words)
  noseg          persistent_bwd 0, segment_entries 0: no checkpoints, no half-tile lengths filed
  det            deterministic_bwd 1: no checkpoints either; forward maps only (gsr_depth_backward refuses, tested in test_gpu_depth.py)
  lists1         tile_lists 1, depth_buckets 2: depth_order.hip + tile_lists.hip
  sort2          tile_lists 0, two_level_sort 1: key emission, two rocPRIM sorts, range detection
  sort1          tile_lists 0, two_level_sort 0, depth_buckets 0: one global sort on tile << 32 | depth
  nocull         exact_tile_cull 0: the reference's tile rule; records carry tau = 0 and every reachability byte reads 1
  nocull_lists1  the same through tile_lists 1
Evidence that a route ran, where the library offers any: the list lengths read back (gsr_debug_read_binning) against the pair
threshold; gsr_debug_read_segments' summary[0] (entries per segment the forward pass used) and [2] (checkpoint slots handed out) for
seg64, noseg and det; the forward lane counter "staged" for count1; num_rendered for the two nocull routes.  walk, cpp2, npx1, npx4,
wpb2, wpb4, walk_wpb2, walk_wpb4, count2 and the three list builders have no route indicator: the library does not report which
kernel it launched.
Per route: radii, alpha map (= 1 - final_T of that render), depth map and n_contrib equal the default route's bit for bit; so does the
colour, except on the (route, scene) pairs of the table COLOUR_EQUALS, where the checkpoints fall at other entries and the colour
equals, bit for bit, that of the route the table names (the operation that differs is the sum of the per-segment colours); the maps
pass the oracle certificate; the DA gradients pass check_grads and agree with the default route's sums.

Reverse routes (tests/test_gpu_grad_outputs.py's ROUTES, imported): classic, persistent, persistent_c, fill, dense_late, dense_early --
the three mechanisms by which gsr_backward writes the buffers gsr_depth_backward(accumulate = 1) then adds into.  SCENES[4] and REPLICA
have M = 4 SH rows (a dense route falls back to the streaming kernel); SH16 takes the dense kernel ("pergauss_path" bit 0, read between
the colour pass and the map pass).  LARGE runs the defaults there: composite_bwd_lpt_kernel.

Bars: bit-equality; one float32 addition, 2^-24 (|a| + |b|); the constants of tests/helpers.py through the helpers of
tests/test_gpu_depth.py.  Every cap on excluded pixels is max(3, MAX_CERTIFIED_FRAC * pixels).
"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib, synth
from tests import depth_ref as dr
from tests.helpers import MAX_CERTIFIED_FRAC, assert_image_certified, oracle_scene
from tests.test_gpu_depth import (REPLICA, assert_sums_agree, check_grads, final_T_of, map_grads, reference, render_maps, scene, tensors)
from tests.test_gpu_grad_outputs import DEFAULTS as BWD_DEFAULTS, GUARD, ROUTES as BWD_ROUTES, _carve

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ("expected", "inverse")
SH16, LARGE = "sh16", "large"

ALL_DEFAULTS = dict(BWD_DEFAULTS, fwd_pair_long=-1, count_lanes=0, tile_lists=2, depth_buckets=1, two_level_sort=1, exact_tile_cull=1)
FWD_ROUTES = {
    "default": dict(),
    "walk": dict(fwd_pair_long=0),
    "pair256": dict(fwd_pair_long=256),
    "cpp2": dict(asm_walk=0),
    "npx1": dict(fwd_blocks_per_wave=1, bwd_blocks_per_wave=1, persistent_bwd=0, segment_entries=0),
    "npx4": dict(fwd_blocks_per_wave=4, bwd_blocks_per_wave=4, persistent_bwd=0, segment_entries=0),
    "wpb2": dict(composite_waves_per_block=2),
    "wpb4": dict(composite_waves_per_block=4),
    "walk_wpb2": dict(fwd_pair_long=0, composite_waves_per_block=2),
    "walk_wpb4": dict(fwd_pair_long=0, composite_waves_per_block=4),
    "count1": dict(count_lanes=1),
    "count2": dict(count_lanes=2),
    "seg64": dict(persistent_bwd=1, segment_entries=64),
    "noseg": dict(persistent_bwd=0, segment_entries=0),
    "det": dict(deterministic_bwd=1),
    "lists1": dict(tile_lists=1, depth_buckets=2),
    "sort2": dict(tile_lists=0, two_level_sort=1),
    "sort1": dict(tile_lists=0, two_level_sort=0, depth_buckets=0),
    "nocull": dict(exact_tile_cull=0),
    "nocull_lists1": dict(exact_tile_cull=0, tile_lists=1),
}
PAIR_LONG_DEFAULT = 64          # GSR_PAIR_LONG_DEFAULT of csrc/gsr_api.hip
SCENE_IDS = {dr.SCENES[1]: "P64", dr.SCENES[3]: "P3000", dr.SCENES[4]: "P4000", REPLICA: REPLICA}


@contextlib.contextmanager
def options(**kw):
    """Every option a route of this module depends on, set explicitly; all of them, and the device's adaptive depth map, restored."""
    kw = dict(ALL_DEFAULTS, **kw)
    saved = {k: _lib.get_option(k) for k in set(kw) | {"depth_log_map"}}
    try:
        for k, v in kw.items():
            _lib.set_option(k, v)
        yield
    finally:
        for k, v in saved.items():
            _lib.set_option(k, v)


def tiles_of(S):
    return ((S.W + 15) // 16) * ((S.H + 15) // 16)


def left_behind(out, S):
    """What the forward call behind `out` (a 4-tuple of a render whose graph is alive) left in its workspaces, through the debug readers."""
    fn = out[2].grad_fn
    binning, img = fn.saved_tensors[8], fn.saved_tensors[9]
    n = int(fn.num_rendered)
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    pl = np.zeros(max(n, 1), np.uint32); ranges = np.zeros((tiles_of(S), 2), np.uint32)
    _lib.check(lib.gsr_debug_read_binning(stream, n, S.W, S.H, binning.data_ptr() if n else None, img.data_ptr(), None, pl.ctypes.data,
                                          ranges.ctypes.data), "read binning")
    fT = np.zeros((S.H, S.W), np.float32); nc = np.zeros((S.H, S.W), np.uint32)
    _lib.check(lib.gsr_debug_read_image_state(stream, S.W, S.H, img.data_ptr(), fT.ctypes.data, nc.ctypes.data), "read image")
    seg = np.zeros(8, np.uint32)
    _lib.check(lib.gsr_debug_read_segments(stream, S.W, S.H, img.data_ptr(), seg.ctypes.data), "read segments")
    r = ranges.astype(np.int64)
    return dict(n=n, ranges=r, lengths=r[:, 1] - r[:, 0], final_T=fT, n_contrib=nc, seg=seg)


def run_route(S, mode, kw, grads=True):
    """Forward maps (graph kept: evidence is read from its workspaces) and, in a second render, the gradients of the DA loss."""
    with options(**kw):
        if kw.get("count_lanes") == 1:
            _lib.read_lane_counters()                      # reading resets: what follows is this render's alone
        h = render_maps(S, mode)
        counters = _lib.read_lane_counters() if kw.get("count_lanes") == 1 else None      # read and discarded but for "staged"
        left = left_behind(h["out"], S)
        alpha_from_T = np.float32(1.0) - final_T_of(h["out"], S)
        g = None
        if grads:
            gD, gA = map_grads(S, "DA")
            g = render_maps(S, mode, gD=gD, gA=gA)
            for k in ("color", "radii", "depth", "alpha"):
                np.testing.assert_array_equal(g[k], h[k])
        if counters is not None:
            _lib.read_lane_counters()
    return dict(color=h["color"], radii=h["radii"], depth=h["depth"], alpha=h["alpha"], left=left, alpha_from_T=alpha_from_T, counters=counters,
                grads=None if g is None else g["grads"], g=g)


@functools.lru_cache(maxsize=None)
def default_run(cfg, mode):
    r = run_route(scene(cfg), mode, {})
    r.pop("g")                                              # the tensors of the render are not kept
    return r


# Colour.  One operation of the colour pass does depend on the route: at a checkpoint fwd_unit / fwd_unit_pair (composite_fwd.hip)
# restart the colour sums, and a pixel's colour is the sum of its per-segment sums.  A route that places the checkpoints at other
# entries than the default route adds the same terms in another grouping, and its colour differs from the default route's in the
# last bits.  T is never restarted: alpha, depth and n_contrib do not depend on the grouping.
# COLOUR_EQUALS[(route, scene)] names the route whose colour a route's must equal bit for bit ON THAT SCENE where that is not
# "default"; the test also asserts that a listed route's colour does differ from the default route's, so an entry cannot outlive
# its reason.  Why each entry (default: one checkpoint per half tile at entry 256 on SCENES[4], none on the other scenes):
#   SCENES[4]  npx1, npx4, noseg, det take no checkpoint at all: one grouping (noseg is compared with npx1, the others with noseg);
#              seg64 takes the checkpoints at 64 and 128 and then has used its band's two slots: as seg64_walk, the same options
#              through the one-wave-per-half-tile kernel (defined for this comparison only);
#              nocull, nocull_lists1: the lists are longer (368 .. 687 against 337 .. 506), so entry 256 is another Gaussian and the
#              lists past 512 take a second checkpoint: the two builders against each other
#   SCENES[3]  seg64 takes checkpoints at 64 and 128 where the default (lists <= 173 < 256) takes none: as seg64_walk
COLOUR_EQUALS = {
    ("npx1", "P4000"): "noseg", ("npx4", "P4000"): "noseg", ("det", "P4000"): "noseg", ("noseg", "P4000"): "npx1",
    ("seg64", "P4000"): "seg64_walk", ("nocull", "P4000"): "nocull_lists1", ("nocull_lists1", "P4000"): "nocull",
    ("seg64", "P3000"): "seg64_walk",
}
AUX_ROUTES = {"seg64_walk": dict(persistent_bwd=1, segment_entries=64, fwd_pair_long=0)}
SEG_BANDS, SEG_MAXCK = 32, 7     # GSR_SEG_BANDS, GSR_SEG_MAXCK of csrc/gsr_internal.h


def band_can_overdraw(lengths, seg):
    """Whether the checkpoints of a render can depend on the order its waves ran in.  A half tile draws its slots from its band's
    share of the pool (`slot < share` in fwd_unit and fwd_unit_pair, composite_fwd.hip) and goes without once the share is used up;
    who goes without is decided by arrival only where several half tiles share a band and together want more than the share.  (A
    band of one half tile that wants more, as seg64 on SCENES[4], always gets its first `share` checkpoints.)  From the summary of
    gsr_debug_read_segments: seg[0] entries per segment, seg[3] slots in the pool, seg[4] half tiles; unit = 2 tile + half."""
    seg_len, pool, units = int(seg[0]), int(seg[3]), int(seg[4])
    if seg_len == 0:
        return False
    band_units, share = -(-units // SEG_BANDS), pool // SEG_BANDS
    want = np.clip((np.repeat(np.asarray(lengths, np.int64), 2) - 1) // seg_len, 0, SEG_MAXCK)      # boundaries inside the list
    assert len(want) == units
    band = np.arange(units) // band_units
    wanted = np.bincount(band, weights=want, minlength=SEG_BANDS)
    return bool(((np.bincount(band, minlength=SEG_BANDS) > 1) & (wanted > share)).any())


@functools.lru_cache(maxsize=None)
def colour_of(route, cfg, mode):
    with options(**{**FWD_ROUTES, **AUX_ROUTES}[route]):
        return render_maps(scene(cfg), mode)["color"]


def certify(S, t32, depth, alpha):
    """The certificate of test_maps_against_the_oracle: same helper, same cap."""
    img = np.stack([depth[0] / t32["vmax"], alpha[0], np.zeros((S.H, S.W), np.float32)])
    st = assert_image_certified(img, t32["fwd"]["color"], t32["fwd"]["state"].decision_margin())
    assert st["over"] <= max(3, MAX_CERTIFIED_FRAC * st["pixels"]), st
    return st


# ---- 1. forward routes ---------------------------------------------------------------------------------------------------------------
ROUTE_CASES = [(r, c) for c in (dr.SCENES[4], dr.SCENES[3], REPLICA) for r in FWD_ROUTES if r != "default"] + \
              [(r, dr.SCENES[1]) for r in ("walk", "pair256", "cpp2")]


@pytest.mark.parametrize("route,cfg", ROUTE_CASES, ids=[f"{r}-{SCENE_IDS[c]}" for r, c in ROUTE_CASES])
def test_maps_on_every_forward_route(route, cfg):
    kw = FWD_ROUTES[route]
    S = scene(cfg)
    for mode in MODES:
        R = reference(cfg, mode)
        base = default_run(cfg, mode)
        got = run_route(S, mode, kw, grads=route != "det")
        lengths, seg = got["left"]["lengths"], got["left"]["seg"]
        longest = int(lengths.max())
        print(route, SCENE_IDS[cfg], mode, "num_rendered", got["left"]["n"], "lists", int(lengths.min()), "..", longest, "segments", seg[:6].tolist())
        # -- evidence that the route ran
        if cfg == dr.SCENES[4]:
            assert longest > 256                                        # past every pair threshold used here: two waves per half tile
        elif cfg == dr.SCENES[3]:
            assert PAIR_LONG_DEFAULT < longest <= 256                   # the pair kernel's two waves at the default, its w == 0 branch at 256
        else:
            assert longest <= PAIR_LONG_DEFAULT                         # nothing reaches the pair threshold: fwd_unit<2> by wave 0
        if route == "seg64":
            assert seg[0] == 64
            # checkpoints were taken wherever a list passes a boundary.  REPLICA's lists end at 11 entries: none is taken there, and
            # seg[0] == 64 is all the evidence the library offers of this route on that scene
            assert (seg[2] > 0) == (longest > 64), seg
        if route in ("noseg", "det"):
            assert seg[0] == 0, seg
        if route == "count1":
            assert got["counters"]["fwd"]["staged"] > 0
        if kw.get("exact_tile_cull", 1) == 0:
            assert got["left"]["n"] > base["left"]["n"]
        else:
            assert got["left"]["n"] == base["left"]["n"]
            np.testing.assert_array_equal(lengths, base["left"]["lengths"])
            np.testing.assert_array_equal(got["left"]["n_contrib"], base["left"]["n_contrib"])      # one convention for the last contributor
        # -- colour and radii, bit for bit: the default route's, or that of the route COLOUR_EQUALS names for this route and scene
        assert not band_can_overdraw(lengths, seg), seg                 # the checkpoints are a function of the lists, not of the waves' order
        equals = COLOUR_EQUALS.get((route, SCENE_IDS[cfg]), "default")
        if equals == "default":
            np.testing.assert_array_equal(got["color"], base["color"])
        else:
            np.testing.assert_array_equal(got["color"], colour_of(equals, cfg, mode), err_msg=f"{route} against {equals}")
            assert not np.array_equal(got["color"], base["color"]), f"{route} groups its colour sums as the default route does: drop the entry"
        np.testing.assert_array_equal(got["radii"], base["radii"])
        # -- alpha: 1 - final_T of this render, and the default route's
        np.testing.assert_array_equal(got["alpha"][0], got["alpha_from_T"])
        np.testing.assert_array_equal(got["alpha"], base["alpha"])
        # -- depth: every forward variant takes the same decisions and the depth walk's arithmetic does not depend on the route
        np.testing.assert_array_equal(got["depth"], base["depth"])
        # -- the oracle certificate
        np.testing.assert_array_equal(got["radii"], R["t32"]["radii"])
        certify(S, R["t32"], got["depth"], got["alpha"])
        # -- gradients: the helpers' gates, and the default route's sums (float atomics only reorder)
        if got["grads"] is not None:
            check_grads(R, got["g"], "DA")
            assert_sums_agree(got["grads"], base["grads"])


def test_the_default_route_itself():
    """What the other routes are compared with: the default route against the oracle on the four scenes, with its evidence."""
    for cfg in (dr.SCENES[4], dr.SCENES[3], dr.SCENES[1], REPLICA):
        S = scene(cfg)
        for mode in MODES:
            R, base = reference(cfg, mode), default_run(cfg, mode)
            np.testing.assert_array_equal(base["alpha"][0], base["alpha_from_T"])
            certify(S, R["t32"], base["depth"], base["alpha"])
            assert base["left"]["seg"][0] == 256                        # small image: checkpoints every 256 entries
            assert (base["left"]["seg"][2] > 0) == (int(base["left"]["lengths"].max()) > 256)
            assert base["left"]["n"] == int(base["left"]["lengths"].sum()) > 0


# ---- 2. the large image ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def extra_scene(name):
    if name == LARGE:
        return oracle_scene(synth.make_scene(**dr.LARGE))
    assert name == SH16
    P, W, H, s0, seed = dr.SCENES[2]
    return oracle_scene(synth.make_scene(P=P, width=W, height=H, sh_degree=1, max_sh_degree=3, s0=s0, seed=seed))


LARGE_WHICH = {"expected": "DA", "inverse": "D"}


@functools.lru_cache(maxsize=None)
def large_reference(mode):
    """test_gpu_depth.reference for LARGE, with the gradients of the one loss its mode is tested with."""
    S = extra_scene(LARGE)
    t32 = dr.trick_forward(S, mode, "f32", scale="vmax")
    r64 = dr.ref.get("f64")
    f64 = r64.forward(t32["scene"], nthreads=r64.max_threads())
    which = LARGE_WHICH[mode]
    gD, gA = map_grads(S, which)
    grads = {which: (dr.trick_backward(t32, S, mode, gD, gA, "f32"), dr.trick_backward(dict(t32, fwd=f64), S, mode, gD, gA, "f64"))}
    return dict(S=S, Sp=t32["scene"], t32=t32, f64=f64, grads=grads)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,kw", [("defaults", dict()), ("wpb4", dict(composite_waves_per_block=4)), ("no_lpt", dict(bwd_lpt=0))],
                         ids=["defaults", "wpb4", "no_lpt"])
def test_large_image(name, kw, mode):
    """More than 6144 tiles: no pair kernel (composite_fwd_walk_kernel<0>, with wpb4 four waves per workgroup); the forward pass files
    half-tile lengths under lpt_span (summary[0] = 512) unless bwd_lpt is off."""
    R = large_reference(mode)
    S, which = R["S"], LARGE_WHICH[mode]
    assert tiles_of(S) > 6144
    gD, gA = map_grads(S, which)
    with options(**kw):
        h = render_maps(S, mode)
        left = left_behind(h["out"], S)
        alpha_from_T = np.float32(1.0) - final_T_of(h["out"], S)
        g = render_maps(S, mode, gD=gD, gA=gA)
    print(name, mode, "num_rendered", left["n"], "longest", int(left["lengths"].max()), "empty", int((left["lengths"] == 0).sum()), "segments", left["seg"][:6].tolist())
    assert left["seg"][0] == (0 if name == "no_lpt" else 512)
    np.testing.assert_array_equal(h["radii"], R["t32"]["radii"])
    np.testing.assert_array_equal(h["alpha"][0], alpha_from_T)
    for k in ("color", "depth", "alpha"):
        np.testing.assert_array_equal(g[k], h[k])
    certify(S, R["t32"], h["depth"], h["alpha"])
    empty = np.nonzero(left["lengths"] == 0)[0]
    ref_ranges = np.asarray(R["t32"]["base_fwd"]["state"].binning()["ranges"], np.int64)
    ref_empty = np.nonzero(ref_ranges[:, 1] == ref_ranges[:, 0])[0]
    assert len(ref_empty) > 0 and np.isin(ref_empty, empty).all()      # (measured: 65 on the device, whose exact culling only shortens a list, 5 in the oracle)
    gridx = (S.W + 15) // 16
    for t in empty:
        ys, xs = slice(16 * (t // gridx), 16 * (t // gridx) + 16), slice(16 * (t % gridx), 16 * (t % gridx) + 16)
        assert not h["depth"][0, ys, xs].any() and not h["alpha"][0, ys, xs].any(), int(t)
    check_grads(R, g, which)


# ---- 3. reverse routes under accumulate = 1 --------------------------------------------------------------------------------------------
REVERSE = ("classic", "persistent", "persistent_c", "fill", "dense_late", "dense_early")


def colour_grad(S):
    return (np.random.default_rng(3).normal(size=(3, S.H, S.W)) / (S.H * S.W)).astype(np.float32)


def scene_of(cfg):
    return extra_scene(cfg) if cfg in (SH16, LARGE) else scene(cfg)


@functools.lru_cache(maxsize=None)
def sum_of_separate_graphs(cfg, mode):
    """The colour graph's gradients plus the map graph's, each on the default route: what one graph with the three losses must give."""
    S = scene_of(cfg)
    gD, gA = map_grads(S, "DA")
    with options():
        colour = render_maps(S, mode, gC=colour_grad(S))["grads"]
        maps = render_maps(S, mode, gD=gD, gA=gA)["grads"]
    return {k: (None if colour[k] is None and maps[k] is None else (0 if colour[k] is None else colour[k]) + (0 if maps[k] is None else maps[k]))
            for k in colour}


@pytest.mark.parametrize("route", REVERSE)
@pytest.mark.parametrize("cfg,mode", [(dr.SCENES[4], "expected"), (REPLICA, "inverse"), (SH16, "expected")], ids=["P4000", REPLICA, SH16])
def test_combined_losses_on_every_reverse_route(cfg, mode, route):
    from gaussian_transformer_amd.rasterizer import get_backend
    S = scene_of(cfg)
    want = sum_of_separate_graphs(cfg, mode)
    gD, gA = map_grads(S, "DA")
    be = get_backend()
    path_between = []

    def spy(*a, **k):                                       # the map pass runs the streaming per-Gaussian kernel and files its own path
        path_between.append(_lib.get_option("pergauss_path"))
        return type(be).depth_backward(be, *a, **k)
    be.depth_backward = spy
    try:
        with options(**BWD_ROUTES[route]):
            h = render_maps(S, mode, gC=colour_grad(S), gD=gD, gA=gA)
    finally:
        del be.depth_backward
    assert len(path_between) == 1
    dense = route in ("dense_late", "dense_early") and cfg == SH16
    assert (path_between[0] & 1) == (1 if dense else 0), (route, path_between)
    assert want["shs"] is not None and np.abs(want["means3D"]).max() > 0
    assert_sums_agree(h["grads"], want)


def test_combined_losses_on_the_large_image():
    """The defaults on more than 6144 tiles: composite_bwd_lpt_kernel writes what the map pass adds into."""
    S = extra_scene(LARGE)
    gD, gA = map_grads(S, "DA")
    with options():
        h = render_maps(S, "expected", gC=colour_grad(S), gD=gD, gA=gA)
    assert_sums_agree(h["grads"], sum_of_separate_graphs(LARGE, "expected"))


# ---- 4. workspaces that held something else: straight through the C ABI, every buffer the test's own ----------------------------------
GUARD_BYTES = 4096
OUT_SHAPES = lambda P: dict(means3D=(P, 3), means2D=(P, 3), opacity=(P, 1), scales=(P, 3), rots=(P, 4))
OUT_KEYS = dict(means3D="means3D", means2D="means2D", opacity="opacities", scales="scales", rots="rotations")


class _Raw:
    """gsr_forward, gsr_depth_forward and gsr_depth_backward through ctypes (after _Raw of tests/test_gpu_inflight.py)."""

    def __init__(self, S):
        from gaussian_transformer_amd.rasterizer import get_backend
        self.be = get_backend()
        self.lib = self.be.lib
        self.S = S
        self.rs, self.x = tensors(S, grad=False)
        self.P, self.M, self.W, self.H = int(self.x["means3D"].shape[0]), int(self.x["shs"].shape[1]), S.W, S.H
        self.sizes = self.be._sizes(self.P, self.W, self.H)
        self.ws_bytes = _lib.workspace_bytes("gsr_depth_workspace_bytes", self.P)

    @staticmethod
    def stream():
        return torch.cuda.current_stream().cuda_stream

    def forward(self, fill=None):
        """fill: the byte the binning workspace, and GUARD_BYTES behind it, hold when the library is given it (None: torch.empty)."""
        x, rs = self.x, self.rs
        color = torch.empty((3, self.H, self.W), device=DEV)
        radii = torch.empty((self.P,), dtype=torch.int32, device=DEV)
        geom = torch.empty((self.sizes[0],), dtype=torch.uint8, device=DEV)
        img = torch.empty((self.sizes[1],), dtype=torch.uint8, device=DEV)
        held = []

        def alloc(_user, nbytes):
            try:
                n = max(int(nbytes), 1)
                t = torch.empty((n,), dtype=torch.uint8, device=DEV) if fill is None else torch.full((n + GUARD_BYTES,), fill, dtype=torch.uint8, device=DEV)
                held.append((t, n))
                return t.data_ptr()
            except Exception:
                return None
        cb = _lib.ALLOC_FN(alloc)
        n = C.c_int64(0)
        p = _lib.ptr
        rc = self.lib.gsr_forward(self.stream(), self.P, int(rs.sh_degree), self.M, self.W, self.H, p(rs.bg), p(x["means3D"]), p(x["shs"]), None,
                                  p(x["opacities"]), p(x["scales"]), float(rs.scale_modifier), p(x["rotations"]), None, p(rs.viewmatrix), p(rs.projmatrix),
                                  p(rs.campos), float(rs.tanfovx), float(rs.tanfovy), 0, 0, color.data_ptr(), radii.data_ptr(), geom.data_ptr(), geom.numel(),
                                  cb, None, img.data_ptr(), img.numel(), C.byref(n), None, 0)
        _lib.check(rc, "gsr_forward")
        assert len(held) == 1 and n.value > 0
        return dict(n=int(n.value), color=color, radii=radii, geom=geom, img=img, store=held[0][0], bin_bytes=held[0][1], fill=fill)

    def guard_intact(self, f):
        return f["fill"] is None or bool((f["store"][f["bin_bytes"]:] == f["fill"]).all())

    def depth_forward(self, f, mode, depth=True, alpha=True):
        d = torch.full((self.H, self.W), float("nan"), device=DEV) if depth else None
        a = torch.full((self.H, self.W), float("nan"), device=DEV) if alpha else None
        rc = self.lib.gsr_depth_forward(self.stream(), self.P, self.W, self.H, f["n"], dr.MODES[mode],
                                        f["geom"].data_ptr(), f["geom"].numel(), f["store"].data_ptr(), f["bin_bytes"], f["img"].data_ptr(), f["img"].numel(),
                                        None if d is None else d.data_ptr(), None if a is None else a.data_ptr())
        _lib.check(rc, "gsr_depth_forward")
        return d, a

    def depth_backward(self, f, mode, outs, accumulate=0, ws=None):
        """outs: dict of the five gradient tensors (OUT_SHAPES); ws: the workspace, torch.empty when None."""
        x, rs = self.x, self.rs
        gD, gA = (torch.tensor(g, device=DEV) for g in map_grads(self.S, "DA"))
        if ws is None:
            ws = torch.empty((self.ws_bytes,), dtype=torch.uint8, device=DEV)
        p = _lib.ptr
        rc = self.lib.gsr_depth_backward(self.stream(), self.P, self.W, self.H, f["n"], dr.MODES[mode], p(x["means3D"]), f["radii"].data_ptr(), p(x["scales"]),
                                         float(rs.scale_modifier), p(x["rotations"]), None, p(rs.viewmatrix), p(rs.projmatrix), p(rs.campos),
                                         float(rs.tanfovx), float(rs.tanfovy), gD.data_ptr(), gA.data_ptr(), f["geom"].data_ptr(), f["geom"].numel(),
                                         f["store"].data_ptr(), f["bin_bytes"], f["img"].data_ptr(), f["img"].numel(), ws.data_ptr(), self.ws_bytes,
                                         int(accumulate), outs["means2D"].data_ptr(), outs["opacity"].data_ptr(), outs["means3D"].data_ptr(), None,
                                         outs["scales"].data_ptr(), outs["rots"].data_ptr())
        _lib.check(rc, "gsr_depth_backward")
        torch.cuda.synchronize()
        return outs

    def fresh_outputs(self):
        return {k: torch.empty(s, device=DEV) for k, s in OUT_SHAPES(self.P).items()}

    def idle(self, f):
        """Gaussians without a gradient: culled, or left out of the composited mask."""
        return ((f["radii"] <= 0) | ~self.be.composited_mask(f["geom"], self.P)).cpu().numpy()


def as_grads(outs):
    return {OUT_KEYS[k]: v.cpu().numpy().astype(np.float64) for k, v in outs.items()}


RAW_CASES = [(dr.SCENES[4], "expected"), (REPLICA, "inverse")]
RAW_IDS = ["P4000", REPLICA]


@pytest.mark.parametrize("cfg,mode", RAW_CASES, ids=RAW_IDS)
def test_binning_workspace_that_held_a_constant_byte(cfg, mode):
    """The binning workspace arrives filled with 0x00, 0x01 or 0xFF, a guard zone of the same byte behind it.  At the defaults the pair
    kernel leaves the tails of contrib unwritten (each wave stops staging when its block is done), so the depth walks meet those
    bytes: pos >= blk_last[q] must skip them, and the id is checked before the gather.  Maps bit-equal across the fills, the gradients
    equal up to the order of the float atomics, the guard untouched."""
    raw = _Raw(scene(cfg))
    runs = []
    with options():
        for fill in (0x00, 0x01, 0xFF):
            f = raw.forward(fill)
            d, a = raw.depth_forward(f, mode)
            g = raw.depth_backward(f, mode, raw.fresh_outputs())
            assert raw.guard_intact(f), hex(fill)
            runs.append((f["color"].cpu().numpy(), d.cpu().numpy(), a.cpu().numpy(), as_grads(g)))
        h = render_maps(scene(cfg), mode)                  # and the public API's render of the same scene
    for other in runs[1:]:
        for i in range(3):
            np.testing.assert_array_equal(other[i], runs[0][i])
        assert_sums_agree(other[3], runs[0][3])
    np.testing.assert_array_equal(runs[0][1], h["depth"][0]); np.testing.assert_array_equal(runs[0][2], h["alpha"][0])
    assert not np.isnan(runs[0][1]).any() and np.abs(runs[0][3]["means3D"]).max() > 0


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("cfg,mode", RAW_CASES, ids=RAW_IDS)
def test_depth_workspace_that_held_nan(cfg, mode, accumulate):
    """gsr_depth_backward's workspace filled with 0xFF bytes (every float a NaN), 0xFF guard bytes behind it: only the rows that can be
    added into are cleared, and nothing else may be read.  Against a zero-filled workspace."""
    raw = _Raw(scene(cfg))
    with options():
        f = raw.forward()
        got = []
        for byte in (0x00, 0xFF):
            ws = torch.full((raw.ws_bytes + GUARD_BYTES,), byte, dtype=torch.uint8, device=DEV)
            outs = raw.fresh_outputs()
            if accumulate:
                for v in outs.values():
                    v.zero_()
            g = as_grads(raw.depth_backward(f, mode, outs, accumulate=accumulate, ws=ws))
            assert bool((ws[raw.ws_bytes:] == byte).all()), "written behind the workspace"
            got.append(g)
    for k, v in got[1].items():
        assert not np.isnan(v).any(), k
    assert_sums_agree(got[1], got[0])
    assert np.abs(got[0]["means3D"]).max() > 0


@pytest.mark.parametrize("cfg,mode", RAW_CASES, ids=RAW_IDS)
def test_gradient_outputs_between_guards(cfg, mode):
    """accumulate = 0 into outputs carved from one NaN tensor: every element written, exact zeros for every Gaussian that was culled or
    that the composited mask leaves out, guards still NaN.  accumulate = 1 into the same outputs holding a known finite pattern: rows
    outside the composited mask bit-unchanged, every other element pattern + gradient within one float32 addition.  The gradient is the
    accumulate = 0 call's; the two calls sum with float atomics in their own order, so their gradients differ by a few 2^-24 of sums
    that stay below 0.1 here (asserted): with 1 <= |pattern| < 2 the bound 2^-24 (|pattern| + |g|) >= 6e-8 lies an order of magnitude
    above that, and a row that is skipped, added twice or added elsewhere misses it by |g|."""
    raw = _Raw(scene(cfg))
    P = raw.P
    rng = np.random.default_rng(17)
    with options():
        f = raw.forward()
        idle = raw.idle(f)
        store, v, inside = _carve(OUT_SHAPES(P), {})
        raw.depth_backward(f, mode, v, accumulate=0)
        host = store.cpu().numpy()
        g = {k: x.cpu().numpy() for k, x in v.items()}
        pattern = {k: ((1.0 + rng.random(x.shape)) * rng.choice([-1.0, 1.0], size=x.shape)).astype(np.float32) for k, x in g.items()}
        for k, x in v.items():
            x.copy_(torch.tensor(pattern[k], device=DEV))
        raw.depth_backward(f, mode, v, accumulate=1)
        host1 = store.cpu().numpy()
        added = {k: x.cpu().numpy() for k, x in v.items()}
    nan = np.isnan(host)
    assert not nan[inside].any(), {k: int(np.isnan(x).sum()) for k, x in g.items()}
    assert nan[~inside].all() and np.isnan(host1[~inside]).all(), "written outside an output"
    assert not np.isnan(host1[inside]).any()
    print(SCENE_IDS[cfg], mode, "Gaussians without a gradient", int(idle.sum()), "of", P, "largest |g|", max(float(np.abs(x).max()) for x in g.values()))
    assert idle.sum() < P and inside.sum() == 14 * P and GUARD >= 64
    assert idle.any() or cfg == REPLICA                    # measured: 14 of SCENES[4]'s 4000 are never composited, none of REPLICA's 201
    for k, x in g.items():
        assert not np.any(x[idle]), (k, "non-zero row of a Gaussian without a gradient")
        assert np.array_equal(added[k][idle], pattern[k][idle]), (k, "a row outside the composited mask was touched")
        a, b = pattern[k][~idle].astype(np.float64), x[~idle].astype(np.float64)
        assert np.abs(b).max() < 0.1                       # measured: 0.029 (SCENES[4]), 0.0045 (REPLICA)
        err = np.abs(added[k][~idle].astype(np.float64) - (a + b))
        assert (err <= 2.0 ** -24 * (np.abs(a) + np.abs(b))).all(), (k, float(err.max()))
    assert max(np.abs(x).max() for x in g.values()) > 0


@pytest.mark.parametrize("cfg,mode", RAW_CASES, ids=RAW_IDS)
def test_forward_call_with_null_outputs(cfg, mode):
    raw = _Raw(scene(cfg))
    with options():
        f = raw.forward()
        d, a = raw.depth_forward(f, mode)
        d_only, none = raw.depth_forward(f, mode, alpha=False)
        assert none is None
        none, a_only = raw.depth_forward(f, mode, depth=False)
        assert none is None
        before = [f[k].clone() for k in ("geom", "store", "img")]
        assert raw.depth_forward(f, mode, depth=False, alpha=False) == (None, None)      # returns 0 ...
        torch.cuda.synchronize()
        for k, b in zip(("geom", "store", "img"), before):                                # ... and touches nothing
            assert torch.equal(f[k], b), k
    assert torch.equal(d_only, d) and torch.equal(a_only, a)
    assert not bool(torch.isnan(d).any()) and not bool(torch.isnan(a).any()) and bool(a.any())
