"""Reference for absgrad (include/gsr_absgrad.h): the oracle's own lists, walked forwards and then backwards, tile by tile.

walk(S, dL, precision) runs the oracle's forward pass on S and re-composites every tile from state.geom()["xy"], ["conic_o"], ["rgb"]
and state.binning(), 256 pixels at a time, in float32 or in float64 (the oracle of that precision supplies the lists).  The forward
sweep takes the decisions (power > 0, alpha < 1/255, the stop on T (1 - alpha) < 1e-4) and keeps, per entry, alpha, the alpha before the
0.99 cap, T in front of the entry and the blend mask; the reverse sweep is the header's definition as it is written there:

    u_i         = sum_ch gC[ch] rgb_g[ch]
    S_i         = sum_{j behind i, blended} u_j alpha_j T_j
    dL/dalpha_i = u_i T_i - S_i / (1 - alpha_i) - (sum_ch gC[ch] bg[ch]) T_final / (1 - alpha_i)
    s           = opacity_g G dL/dalpha_i                (the alpha before the cap: the cap is straight-through)
    d           = centre_g - pixel
    t_x = -0.5 W s (conA d_x + conB d_y),   t_y = -0.5 H s (conB d_x + conC d_y)

Returned per Gaussian, [P,2] float64 each (the terms are formed in the walk's precision and summed in float64):
    signed = (sum t_x, sum t_y)        -- the oracle's dL_dmeans2D[:, :2]
    abs    = (sum |t_x|, sum |t_y|)    -- absgrad

fault: a planted error an implementation could have, for tests/test_absgrad_ref_host.py to show that the gates catch it --
    "signed"          |sum t| in place of sum |t|;
    "abs_after_tile"  the absolute value taken after a tile's sum (a kernel that takes it after its wave reduction does the like);
    "no_bg"           the background term of dL/dalpha dropped.
"""
import dataclasses
import functools

import numpy as np

from oracle import ref

ALPHA_MIN, ALPHA_MAX, T_MIN = 1.0 / 255.0, 0.99, 1e-4
BG = (0.2, 0.5, 0.9)        # every test's background: the background term is live
FAULTS = ("signed", "abs_after_tile", "no_bg")


def walk(S, dL, precision="f32", fault=None, fwd=None):
    """dict(signed, abs [P,2] float64, radii, num_rendered, fwd).  dL: [3,H,W].  fwd: the forward result of ref.get(precision) on S,
    if the caller has it already."""
    assert fault in (None,) + FAULTS
    r = ref.get(precision)
    f = fwd if fwd is not None else r.forward(S, nthreads=r.max_threads())
    st = f["state"]
    geom, binn = st.geom(), st.binning()
    dt = np.float32 if precision == "f32" else np.float64
    xy, co, rgb = geom["xy"].astype(dt), geom["conic_o"].astype(dt), geom["rgb"].astype(dt)
    vals, ranges = binn["vals"], binn["ranges"]
    P = xy.shape[0]
    W, H = int(S.W), int(S.H)
    gC_all = np.asarray(dL, dt).reshape(3, H, W)
    bg = np.asarray(S.bg, dt).reshape(3)
    signed = np.zeros((P, 2)); absum = np.zeros((P, 2))
    gridx, gridy = (W + 15) // 16, (H + 15) // 16
    amin, amax, tmin, half, one = dt(ALPHA_MIN), dt(ALPHA_MAX), dt(T_MIN), dt(0.5), dt(1.0)
    kx, ky = dt(-0.5) * dt(W), dt(-0.5) * dt(H)
    for tile in range(gridx * gridy):
        r0, r1 = int(ranges[tile][0]), int(ranges[tile][1])
        if r1 <= r0:
            continue
        tx, ty = tile % gridx, tile // gridx
        yy, xx = np.meshgrid(np.arange(16) + ty * 16, np.arange(16) + tx * 16, indexing="ij")
        inside = ((xx < W) & (yy < H)).ravel()
        xi, yi = np.minimum(xx, W - 1).ravel(), np.minimum(yy, H - 1).ravel()
        gC = np.where(inside[None, :], gC_all[:, yi, xi], dt(0.0))      # [3,256]
        px, py = xx.ravel().astype(dt), yy.ravel().astype(dt)
        # forward sweep: the decisions
        T = np.ones(256, dt)
        alive = inside.copy()
        kept = []
        for j in range(r0, r1):
            if not alive.any():
                break
            g = int(vals[j])
            dx, dy = xy[g, 0] - px, xy[g, 1] - py
            power = -half * (co[g, 0] * dx * dx + co[g, 2] * dy * dy) - co[g, 1] * dx * dy
            with np.errstate(over="ignore"):
                araw = co[g, 3] * np.exp(power)
            alpha = np.minimum(araw, amax)
            cand = alive & ~(power > 0) & ~(alpha < amin)
            Tn = T * (one - alpha)
            stop = cand & (Tn < tmin)
            blend = cand & ~stop
            if blend.any():
                kept.append((g, dx, dy, araw, alpha, T, blend))
            T = np.where(blend, Tn, T)
            alive &= ~stop
        T_final = T
        gbg = (gC[0] * bg[0] + gC[1] * bg[1] + gC[2] * bg[2]) * T_final
        if fault == "no_bg":
            gbg = np.zeros(256, dt)
        # reverse sweep: the definition
        Ssum = np.zeros(256, dt)
        for g, dx, dy, araw, alpha, Ti, blend in reversed(kept):
            u = gC[0] * rgb[g, 0] + gC[1] * rgb[g, 1] + gC[2] * rgb[g, 2]
            om = one - alpha
            dLda = u * Ti - Ssum / om - gbg / om
            with np.errstate(over="ignore", invalid="ignore"):      # a skipped pixel's exp may be inf: selected away below
                s = araw * dLda
                t_x = np.where(blend, kx * s * (co[g, 0] * dx + co[g, 1] * dy), dt(0.0)).astype(np.float64)
                t_y = np.where(blend, ky * s * (co[g, 1] * dx + co[g, 2] * dy), dt(0.0)).astype(np.float64)
            sx, sy = t_x.sum(), t_y.sum()
            signed[g, 0] += sx; signed[g, 1] += sy
            if fault == "abs_after_tile":
                absum[g, 0] += abs(sx); absum[g, 1] += abs(sy)
            else:
                absum[g, 0] += np.abs(t_x).sum(); absum[g, 1] += np.abs(t_y).sum()
            Ssum = np.where(blend, Ssum + u * alpha * Ti, Ssum)
    if fault == "signed":
        absum = np.abs(signed)
    return dict(signed=signed, abs=absum, radii=np.asarray(f["radii"]), num_rendered=int(f["num_rendered"]), fwd=f)


def upstream(S, kind="normal", seed=5):
    """dL_dcolor [3,H,W] float32: "normal" ~ N(0,1); "l1" the gradient of a mean absolute error, +-1 / (3 H W) in a random pattern."""
    rng = np.random.default_rng(seed)
    g = rng.normal(size=(3, S.H, S.W))
    if kind == "l1":
        g = np.sign(g) / (3.0 * S.H * S.W)
    return g.astype(np.float32)


LARGE = "large"


@functools.lru_cache(maxsize=None)
def scene(cfg):
    """One of tests/test_gpu_depth.py's scenes (depth_ref.SCENES[k] or "replica") or "large" (depth_ref.LARGE), on the background BG."""
    from gaussian_transformer_amd import synth
    from tests import depth_ref
    from tests.helpers import oracle_scene
    from tests.test_gpu_depth import scene as depth_scene
    S = oracle_scene(synth.make_scene(**depth_ref.LARGE)) if cfg == LARGE else depth_scene(cfg)
    return dataclasses.replace(S, bg=np.array(BG, np.float32))


@functools.lru_cache(maxsize=None)
def walks(cfg, kind="normal", want64=True):
    """(S, dL, float32 walk, float64 walk or None) of a scene, computed once and shared."""
    S = scene(cfg)
    dL = upstream(S, kind)
    return S, dL, walk(S, dL, "f32"), (walk(S, dL, "f64") if want64 else None)


def ratio_median(absgrad, signed):
    """median over the rows with a gradient of ||absgrad|| / ||signed||"""
    a, s = np.linalg.norm(np.asarray(absgrad, np.float64), axis=1), np.linalg.norm(np.asarray(signed, np.float64), axis=1)
    ok = s > 0
    return float(np.median(a[ok] / s[ok])) if ok.any() else float("nan")
