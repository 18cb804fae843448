"""Reference for the per-Gaussian blend-weight statistics (include/gsr_contrib.h): the oracle's own lists, walked again.

walk(S, precision) runs the oracle's forward pass on S and re-composites every tile from state.geom()["xy"], ["conic_o"] and
state.binning(), 256 pixels at a time, with the operation order of helpers.recomposite_pixel, in float32 or in float64 (the oracle of
that precision supplies the lists).  Per Gaussian it returns, over the (pixel, entry) pairs that blend:
    sum    of w = alpha T            (accumulated in float64 whatever the walk's precision)
    max    of w
    count  of pairs

Beside these, two slacks from the same walk: how far a correct float32 implementation may legitimately differ, because a decision
it takes lies within `margin` (helpers.MARGIN_CERT; margins as recomposite_pixel defines them) of its threshold and may fall the other
way under another rounding of the exponent.  For Gaussian g,
    slack_count[g]  = number of pixels in which g passes -- or borderline-passes -- its own power and alpha tests AND
                        * g's own power, alpha or T decision is borderline, or
                        * an earlier decision in that pixel was borderline (it shifts every later T), or
                        * the pixel stopped on a borderline T decision: another implementation may go on blending there, so the walk
                          continues in that pixel as a "ghost" (T kept as it was at the stop);
    slack_weight[g] = sum of min(alpha, 0.99) over the same pixels (w <= alpha: a bound on what those pixels can add or withhold).

fault: a planted error an implementation could have, for tests/test_contrib_ref_host.py to show that the gates catch it --
    "count_stop"  the entry that triggers the stop (T (1 - alpha) < 1e-4) is counted, summed and offered to the max;
    "alpha_only"  the weights are summed (and maximised) as alpha in place of alpha T.
"""
import functools

import numpy as np

from oracle import ref
from tests.helpers import MARGIN_CERT

ALPHA_MIN, ALPHA_MAX, T_MIN = 1.0 / 255.0, 0.99, 1e-4


def walk(S, precision="f32", margin=MARGIN_CERT, fault=None, fwd=None):
    """dict(sum, max [P] float64, count [P] int64, slack_count [P] int64, slack_weight [P] float64, radii, num_rendered, fwd).
    fwd: the forward result of ref.get(precision) on S, if the caller has it already."""
    assert fault in (None, "count_stop", "alpha_only")
    r = ref.get(precision)
    f = fwd if fwd is not None else r.forward(S, nthreads=r.max_threads())
    st = f["state"]
    geom, binn = st.geom(), st.binning()
    dt = np.float32 if precision == "f32" else np.float64
    xy, co = geom["xy"].astype(dt), geom["conic_o"].astype(dt)
    vals, ranges = binn["vals"], binn["ranges"]
    P = xy.shape[0]
    s = np.zeros(P); mx = np.zeros(P); cnt = np.zeros(P, np.int64)
    slack = np.zeros(P, np.int64); slackw = np.zeros(P)
    gridx, gridy = (S.W + 15) // 16, (S.H + 15) // 16
    amin, amax, tmin, half, one = dt(ALPHA_MIN), dt(ALPHA_MAX), dt(T_MIN), dt(0.5), dt(1.0)
    for tile in range(gridx * gridy):
        r0, r1 = int(ranges[tile][0]), int(ranges[tile][1])
        if r1 <= r0:
            continue
        tx, ty = tile % gridx, tile // gridx
        yy, xx = np.meshgrid(np.arange(16) + ty * 16, np.arange(16) + tx * 16, indexing="ij")
        inside = ((xx < S.W) & (yy < S.H)).ravel()
        px, py = xx.ravel().astype(dt), yy.ravel().astype(dt)
        T = np.ones(256, dt)
        alive = inside.copy()
        ghost = np.zeros(256, bool)        # stopped on a borderline T decision: another implementation may still be blending here
        taint = np.zeros(256, bool)        # a borderline decision was met earlier in this pixel
        for j in range(r0, r1):
            if not alive.any() and not ghost.any():
                break
            g = int(vals[j])
            dx, dy = xy[g, 0] - px, xy[g, 1] - py
            power = -half * (co[g, 0] * dx * dx + co[g, 2] * dy * dy) - co[g, 1] * dx * dy
            with np.errstate(over="ignore"):
                araw = co[g, 3] * np.exp(power)
            skipP = power > 0
            alpha = np.minimum(araw, amax)
            skipA = alpha < amin
            cand = alive & ~skipP & ~skipA
            Tn = T * (one - alpha)
            stop = cand & (Tn < tmin)
            blend = cand & ~stop
            w = alpha if fault == "alpha_only" else alpha * T
            counted = cand if fault == "count_stop" else blend
            if counted.any():
                wb = w[counted].astype(np.float64)
                s[g] += wb.sum(); mx[g] = max(mx[g], wb.max()); cnt[g] += int(counted.sum())
            # margins, as recomposite_pixel records them
            with np.errstate(invalid="ignore"):
                mP = np.where(araw >= amin * half, np.abs(power), np.inf)
                mA = np.where(~skipP, np.abs((alpha - amin) / amin), np.inf)
                mT = np.where(~skipP & ~skipA, np.abs((Tn - tmin) / tmin), np.inf)
            walked = alive | ghost
            ownPA = (mP < margin) | (mA < margin)
            passes = (~skipP & ~skipA) | ownPA
            ownT = cand & (mT < margin)
            unc = walked & passes & (taint | ghost | ownPA | ownT)
            if unc.any():
                slack[g] += int(unc.sum())
                slackw[g] += float(np.minimum(alpha[unc], amax).astype(np.float64).sum())
            taint |= walked & (ownPA | ownT)
            ghost |= stop & (mT < margin)
            T = np.where(blend, Tn, T)
            alive &= ~stop
    return dict(sum=s, max=mx, count=cnt, slack_count=slack, slack_weight=slackw, radii=np.asarray(f["radii"]),
                num_rendered=int(f["num_rendered"]), fwd=f)


def visible(a, b=None):
    """The Gaussians either walk blends at all."""
    v = a["count"] > 0
    return v if b is None else v | (b["count"] > 0)


def own_error(a32, a64):
    """(sum, max): the float32 walk's largest relative error against the float64 walk over the clean visible rows (slack_count == 0)."""
    clean = visible(a32, a64) & (a32["slack_count"] == 0)
    if not clean.any():
        return 0.0, 0.0
    es = np.abs(a32["sum"] - a64["sum"])[clean] / np.maximum(a64["sum"][clean], 1e-30)
    em = np.abs(a32["max"] - a64["max"])[clean] / np.maximum(a64["max"][clean], 1e-30)
    return float(es.max()), float(em.max())


REL_FLOOR = 2e-6


def rel_of(a32, a64):
    """(rel_sum, rel_max): the relative tolerances of the device gates on one scene, each twice the float32 walk's own largest relative
    error of that field against the float64 walk (the device's exp2-based exponent and its reciprocal are not libm's), plus a floor
    of 2e-6 (on the one-Gaussian scene the float32 walk's own error is below one float32 ulp).  From the two walks alone, never from
    the device."""
    es, em = own_error(a32, a64)
    return 2.0 * es + REL_FLOOR, 2.0 * em + REL_FLOOR


def gates(got_sum, got_max, got_count, a32, a64, rel, opacity=None):
    """The three gates of tests/test_gpu_contrib.py on every visible Gaussian, as counts of violations (and the largest relative
    errors on clean rows): `got_*` against the float32 walk's count and the float64 walk's sum and max.
        |count - count32| <= slack_count
        |sum - sum64| <= slack_weight + count 2^-32 + rel_sum sum64
        |max - max64| <= rel_max max64 on clean rows; elsewhere max <= min(0.99, opacity) (1 + 2^-23)"""
    got_sum, got_max, got_count = (np.asarray(x, np.float64) for x in (got_sum, got_max, got_count))
    rel_sum, rel_max = rel
    vis = visible(a32, a64) | (got_count > 0)
    sl, sw = a32["slack_count"], a32["slack_weight"]
    clean = vis & (sl == 0)
    bad_count = vis & (np.abs(got_count - a32["count"]) > sl)
    bad_sum = vis & (np.abs(got_sum - a64["sum"]) > sw + got_count * 2.0 ** -32 + rel_sum * a64["sum"])
    bad_max = clean & (np.abs(got_max - a64["max"]) > rel_max * a64["max"])
    if opacity is not None:
        cap = np.minimum(ALPHA_MAX, np.asarray(opacity, np.float64).reshape(-1)) * (1.0 + 2.0 ** -23)
        bad_max = bad_max | (vis & ~clean & (got_max > cap))
    es = (np.abs(got_sum - a64["sum"])[clean] / np.maximum(a64["sum"][clean], 1e-30)).max() if clean.any() else 0.0
    em = (np.abs(got_max - a64["max"])[clean] / np.maximum(a64["max"][clean], 1e-30)).max() if clean.any() else 0.0
    return dict(visible=int(vis.sum()), flagged=int((vis & (sl > 0)).sum()), bad_count=int(bad_count.sum()), bad_sum=int(bad_sum.sum()),
                bad_max=int(bad_max.sum()), err_sum=float(es), err_max=float(em), count_differs=int((vis & (got_count != a32["count"])).sum()))


@functools.lru_cache(maxsize=None)
def walks(cfg):
    """(S, float32 walk, float64 walk) of one of tests/test_gpu_depth.py's scenes (depth_ref.SCENES[k] or "replica"), computed once."""
    from tests.test_gpu_depth import scene
    S = scene(cfg)
    return S, walk(S, "f32"), walk(S, "f64")
