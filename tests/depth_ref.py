"""Reference for the depth and alpha maps (include/gsr_depth.h): the oracle, untouched, used through the colour trick.

Depth blends exactly like a colour channel: rendering the scene S a second time with colors_precomp = (v, 1, 0), a zero background
and no SH gives  channel 0 = sum v alpha T (the depth map),  channel 1 = sum alpha T = 1 - T_final (the alpha map).  Its backward
pass under dL = (gD, gA, 0) gives every gradient of  L = <gD, depth> + <gA, alpha>  directly, except that v depends on the mean:
dL_dcolors[:, 0] is dL/dv, and  dL/dmeans3D += dL/dv * dv/dz * (m[2], m[6], m[10])  with the view matrix m in gsr.h's layout.

`scale`: the colour is (v / scale, 1, 0) and dL = (gD * scale, gA, 0) -- the same loss, with channel 0 of the oracle's image the depth
map divided by a constant, so that the image helpers of tests/helpers.py (absolute RGB tolerance) can be applied to it as they are.

Besides the trick: depth_alpha_pixels() re-composites pixels one by one from the oracle's lists with helpers.recomposite_pixel, which
takes arbitrary values per Gaussian -- an independent statement of the same maps -- and three planted faults an implementation of
the maps could have.
"""
import dataclasses

import numpy as np

from oracle import ref
from tests.helpers import recomposite_pixel

MODES = {"expected": 0, "inverse": 1}

# (P, W, H, s0, seed): make_scene(P, W, H, sh_degree=1, s0, seed); float32 against float64 oracle, both modes, pixels over 1e-4 vmax: 0 0 0 1 0
SCENES = ((1, 16, 16, 0.3, 0), (64, 40, 24, 0.05, 1), (500, 64, 48, 0.05, 2), (3000, 96, 80, 0.03, 3), (4000, 64, 64, 0.08, 4))

# The large image, under a name of its own (other modules index SCENES): more than 6144 tiles, so the forward pass has no pair kernel
# and files half-tile lengths for the length-ordered reverse kernel.  make_scene(**LARGE): 101 x 63 = 6363 tiles, 5 of them with an
# empty range, 67452 pairs, longest list 23.  float32 against float64 oracle through helpers.assert_image_certified, both modes: 2
# pixels over tolerance, 0 uncertified, against the cap max(3, MAX_CERTIFIED_FRAC * pixels) = 16
# (tests/test_depth_ref_host.py::test_the_large_scene_certifies_itself).
LARGE = dict(P=600, width=1616, height=1008, sh_degree=1, s0=0.05, seed=7)


def values(z, radii, mode):
    """v per Gaussian (float64): z or 1 / z; 0 for a culled Gaussian, whose stored depth means nothing."""
    z = np.asarray(z, np.float64)
    ok = np.asarray(radii) > 0
    v = np.zeros_like(z)
    v[ok] = z[ok] if MODES[mode] == 0 else 1.0 / z[ok]
    return v


def vmax_of(v, radii):
    ok = np.asarray(radii) > 0
    return max(1.0, float(np.abs(v[ok]).max())) if ok.any() else 1.0


def trick_scene(S, v, scale=1.0):
    P = int(np.asarray(S.means3D).shape[0])
    col = np.zeros((P, 3), np.float64)
    col[:, 0] = np.asarray(v, np.float64) / scale
    col[:, 1] = 1.0
    return dataclasses.replace(S, shs=None, colors_precomp=col, bg=np.zeros(3), sh_degree=0)


def trick_forward(S, mode, precision="f32", scale=None, nthreads=0):
    """Runs the oracle on S (for the depths) and on S'.  Returns dict(depth[H,W], alpha[H,W], v[P], vmax, scale, radii, fwd = the S'
    forward result (its "color" is [depth / scale, alpha, 0]), scene = S')."""
    r = ref.get(precision)
    nt = nthreads or r.max_threads()
    f = r.forward(S, nthreads=nt)
    v = values(f["state"].geom()["depth"], f["radii"], mode)
    vm = vmax_of(v, f["radii"])
    sc = vm if scale == "vmax" else float(scale or 1.0)
    Sp = trick_scene(S, v, sc)
    fp = r.forward(Sp, nthreads=nt)
    return dict(depth=np.asarray(fp["color"][0], np.float64) * sc, alpha=np.asarray(fp["color"][1], np.float64), v=v, vmax=vm, scale=sc,
                radii=f["radii"], fwd=fp, scene=Sp, base_fwd=f)


def trick_backward(t, S, mode, gD, gA, precision="f32", nthreads=0):
    """Gradients of <gD, depth> + <gA, alpha> from the S' backward pass of trick_forward's result t (same precision).  gD / gA: [H,W] or
    None.  Returns the oracle's gradient dict with dL_dmeans3D completed by the dL/dv term, and dL_dv."""
    r = ref.get(precision)
    nt = nthreads or r.max_threads()
    H, W = S.H, S.W
    dL = np.zeros((3, H, W), np.float64)
    if gD is not None:
        dL[0] = np.asarray(gD, np.float64) * t["scale"]
    if gA is not None:
        dL[1] = np.asarray(gA, np.float64)
    g = r.backward(t["fwd"], dL, nthreads=nt)
    dv = np.asarray(g["dL_dcolors"][:, 0], np.float64) / t["scale"]
    m = np.asarray(S.viewmatrix, np.float64).reshape(16)
    p = np.asarray(S.means3D, np.float64).reshape(-1, 3)
    z = m[2] * p[:, 0] + m[6] * p[:, 1] + m[10] * p[:, 2] + m[14]
    ok = np.asarray(t["radii"]) > 0
    dvdz = np.zeros_like(z)
    dvdz[ok] = 1.0 if MODES[mode] == 0 else -1.0 / (z[ok] * z[ok])
    out = {k: (None if a is None else np.asarray(a, np.float64)) for k, a in g.items()}
    out["dL_dmeans3D"] = out["dL_dmeans3D"] + (dv * dvdz)[:, None] * np.array([m[2], m[6], m[10]])[None, :]
    out["dL_dv"] = dv
    out["dL_dcolors"] = None          # the maps have no colour gradient
    return out


# ---- the independent statement: pixel by pixel from the oracle's lists ----
def _faulty_walk(geom, vals, r0, r1, x, y, v32, blend_stop=False, alpha_whole_list=False):
    """One pixel in float32, the walk of helpers.recomposite_pixel restated with a planted fault: blend_stop blends the entry that
    triggered the stop before stopping; alpha_whole_list goes on summing alpha T behind the stop.  Returns (depth, alpha)."""
    f32 = np.float32
    xy, co = geom["xy"], geom["conic_o"]
    Tr = f32(1.0); D = f32(0.0); A = f32(0.0)
    stopped = False
    for j in range(int(r0), int(r1)):
        k = int(vals[j])
        dx = f32(xy[k, 0] - f32(x)); dy = f32(xy[k, 1] - f32(y))
        power = f32(f32(-0.5) * f32(f32(co[k, 0] * dx * dx) + f32(co[k, 2] * dy * dy)) - f32(f32(co[k, 1] * dx) * dy))
        if power > 0:
            continue
        alpha = min(f32(co[k, 3] * np.exp(power, dtype=np.float32)), f32(0.99))
        if alpha < f32(1.0 / 255.0):
            continue
        Tn = f32(Tr * f32(f32(1.0) - alpha))
        w = f32(alpha * Tr)
        if stopped:                       # only alpha_whole_list gets here
            A = f32(A + w); Tr = Tn
            continue
        if Tn < f32(1e-4):
            if blend_stop:
                D = f32(D + v32[k] * w); A = f32(A + w)
            if not alpha_whole_list:
                break
            stopped = True
            if blend_stop:
                Tr = Tn
            continue
        D = f32(D + v32[k] * w); A = f32(A + w); Tr = Tn
    return float(D), float(A)


def _pixel(geom, vals, r0, r1, x, y, v32, fault=None):
    """(depth, alpha) of one pixel in float32.  No fault: through helpers.recomposite_pixel with the per-Gaussian 'colour' (v, 1, 0)."""
    if fault == "blend_stop":
        return _faulty_walk(geom, vals, r0, r1, x, y, v32, blend_stop=True)
    if fault == "alpha_whole_list":
        return _faulty_walk(geom, vals, r0, r1, x, y, v32, alpha_whole_list=True)
    g = dict(geom)
    rgb = np.zeros((len(v32), 3), np.float32)
    rgb[:, 0] = v32; rgb[:, 1] = 1.0
    g["rgb"] = rgb
    c, _ = recomposite_pixel(g, vals, r0, r1, x, y, np.zeros(3, np.float32))
    d, a = float(c[0]), float(c[1])
    if fault == "normalised":
        d = d / a if a > 0 else 0.0
    return d, a


def depth_alpha_pixels(S, mode, fault=None, precision="f32", step=1):
    """(depth[H,W], alpha[H,W], vmax) re-composited pixel by pixel (float32 walk) from the lists of the oracle's run on S.
    step > 1: only the pixels of every step-th row and column (from 0) are walked; the others read NaN."""
    r = ref.get(precision)
    f = r.forward(S, nthreads=r.max_threads())
    st = f["state"]
    geom, binn = st.geom(), st.binning()
    v = values(geom["depth"], f["radii"], mode)
    v32 = v.astype(np.float32)
    D = np.full((S.H, S.W), np.nan); A = np.full((S.H, S.W), np.nan)
    gridx = (S.W + 15) // 16
    for y in range(0, S.H, step):
        for x in range(0, S.W, step):
            r0, r1 = binn["ranges"][(y // 16) * gridx + (x // 16)]
            D[y, x], A[y, x] = _pixel(geom, binn["vals"], r0, r1, x, y, v32, fault) if r1 > r0 else (0.0, 0.0)
    return D, A, vmax_of(v, f["radii"])
