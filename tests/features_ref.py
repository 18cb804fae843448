"""Reference for the N-channel feature maps (include/gsr_features.h): the oracle, untouched, used through the colour trick.

A feature blends exactly like a colour channel.  The channels of F [P,C] are taken in triples, the last one padded with zeros: rendering
the scene a second time with colors_precomp = F[:, 3k:3k+3] / fmax, a zero background and no SH gives the channels 3k..3k+2 of the map
divided by fmax, and its backward pass under dL = G[3k:3k+3] * fmax gives every gradient of <G[3k:3k+3], map[3k:3k+3]>; the geometry
gradients of the triples are added, and dL_dcolors / fmax of triple k is dL/dF[:, 3k:3k+3].  fmax = max(1, max |F|) over radii > 0, so
that the image helpers of tests/helpers.py (absolute RGB tolerance) apply as they are.  The oracle copies colors_precomp through without
clamping: negative features are legitimate, and used.

features(): the test matrices.  Uniform in (-2, 2), with one entry of column 0 -- the first Gaussian with radii > 0 -- set to 2: fmax is
then 2 for every leading block of columns F[:, :C], so a triple's oracle runs are the same whatever C it is part of, and
tests/test_gpu_features.py computes each (scene, triple) once and shares it among the channel counts.

Besides the trick: feature_pixels() re-composites pixels one by one from the oracle's lists with helpers.recomposite_pixel, which takes
arbitrary values per Gaussian -- an independent statement of the same map -- and three planted faults an implementation could have.

Self-certification (tests/test_features_ref_host.py): float32 oracle against float64 oracle through helpers.assert_image_certified,
pixels over RGB_ATOL / uncertified in every triple of C = 4, 17 (and 64 on SCENES[3]; every count of EDGE_CHANNELS on SCENES[1]), seed 0
of features():  depth_ref.SCENES[0..4]: 0/0 0/0 0/0 1/0 0/0, the replica scene (272 x 256): 0/0, against the cap max(3, 1e-5 pixels) = 3
per triple.  Gradients: inside assert_parity's gates everywhere; what the seeds of map_grad() are chosen by is said there and at
GRAD_SEEDS.
"""
import dataclasses
import functools

import numpy as np

from gaussian_transformer_amd import synth
from oracle import ref
from tests import depth_ref
from tests.helpers import MAX_CERTIFIED_FRAC, assert_image_certified, assert_parity, build_report, oracle_scene, recomposite_pixel

FMAX = 2.0
GEOMETRY_KEYS = ("dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dscales", "dL_drots", "dL_dcov3D")


def features(radii, C, seed=0):
    """F [P,C] float32, uniform in (-2, 2) -- negative values included -- with max |F| over radii > 0 equal to FMAX in column 0."""
    P = len(radii)
    F = np.random.default_rng(1000 + seed).uniform(-1.999, 1.999, size=(P, 64)).astype(np.float32)[:, :C].copy()
    vis = np.flatnonzero(np.asarray(radii) > 0)
    if len(vis):
        F[vis[0], 0] = FMAX
    return F


def map_grad(S, C, seed=11):
    """Random upstream gradient [C,H,W] of scale 1 / (H W), |normal|; the leading channels do not depend on C.  Non-negative (the
    features carry the signs): with a random sign per pixel as well, every Gaussian's gradient is a sum that cancels over its pixels,
    and on depth_ref.SCENES[1] -- 63 gradient rows, so that the gates' p99 is the worst row -- the float32 oracle's own dL/dopacity
    then lies 9e-5 to 1e-3 of a row's magnitude from the float64 oracle's at some channel count (seeds 11..30): no float32 evaluation
    can be held to 1e-4 of another there.  With this form and seed the float32 oracle stays within half the gate (F32_P99_MAX / 2) of
    the float64 one at every channel count, which tests/test_features_ref_host.py asserts."""
    return np.abs(np.random.default_rng(seed).normal(size=(64, S.H, S.W)) / (S.H * S.W)).astype(np.float32)[:C].copy()


def fmax_of(F, radii):
    ok = np.asarray(radii) > 0
    return max(1.0, float(np.abs(np.asarray(F, np.float64)[ok]).max())) if ok.any() and np.asarray(F).size else 1.0


def triples(C):
    return [(k, 3 * k, min(3 * k + 3, C)) for k in range((C + 2) // 3)]


def pad3(a, lo, hi):
    """Columns (or leading planes) lo..hi of `a` as three, zero-padded."""
    a = np.asarray(a, np.float64)
    out = np.zeros((3,) + a.shape[1:], np.float64) if a.ndim == 3 else np.zeros((a.shape[0], 3), np.float64)
    if a.ndim == 3:
        out[:hi - lo] = a[lo:hi]
    else:
        out[:, :hi - lo] = a[:, lo:hi]
    return out


def trick_scene(S, F3, fmax):
    return dataclasses.replace(S, shs=None, colors_precomp=np.asarray(F3, np.float64) / fmax, bg=np.zeros(3), sh_degree=0)


def triple_forward(S, F, lo, hi, fmax, precision="f32", nthreads=0):
    """The oracle's forward result on the trick scene of one triple; its "color" is map[lo:hi] / fmax, zero-padded to three channels."""
    r = ref.get(precision)
    Sp = trick_scene(S, pad3(F, lo, hi), fmax)
    return Sp, r.forward(Sp, nthreads=nthreads or r.max_threads())


def triple_backward(fwd, G, lo, hi, fmax, precision="f32", nthreads=0):
    """The oracle's gradients of <G[lo:hi], map[lo:hi]> from that triple's forward result, dL_dcolors turned into dL/dF[:, lo:hi]."""
    r = ref.get(precision)
    g = r.backward(fwd, pad3(G, lo, hi) * fmax, nthreads=nthreads or r.max_threads())
    out = {k: (None if g.get(k) is None else np.asarray(g[k], np.float64)) for k in GEOMETRY_KEYS}
    out["dL_dfeatures"] = np.asarray(g["dL_dcolors"], np.float64)[:, :hi - lo] / fmax
    return out


def add_triples(parts, C):
    """The gradients of the whole map from those of its triples (in triples(C)'s order)."""
    out = {k: (None if parts[0][k] is None else sum(p[k] for p in parts)) for k in GEOMETRY_KEYS}
    out["dL_dfeatures"] = np.concatenate([p["dL_dfeatures"] for p in parts], axis=1)
    assert out["dL_dfeatures"].shape[1] == C
    return out


def trick_forward(S, F, precision="f32", nthreads=0):
    """dict(map [C,H,W] float64, fmax, radii, fwd = the per-triple forward results, scenes = their trick scenes)."""
    r = ref.get(precision)
    nt = nthreads or r.max_threads()
    base = r.forward(S, nthreads=nt)
    C = int(np.asarray(F).shape[1])
    fm = fmax_of(F, base["radii"])
    scenes, fwds = zip(*[triple_forward(S, F, lo, hi, fm, precision, nt) for _k, lo, hi in triples(C)])
    fmap = np.concatenate([np.asarray(f["color"], np.float64)[:hi - lo] for f, (_k, lo, hi) in zip(fwds, triples(C))]) * fm
    return dict(map=fmap, fmax=fm, radii=base["radii"], fwd=list(fwds), scenes=list(scenes), base_fwd=base, C=C)


def trick_backward(t, G, precision="f32", nthreads=0):
    """Gradients of <G, map> from the backward passes of trick_forward's result t (same precision), triples added."""
    C = t["C"]
    return add_triples([triple_backward(f, G, lo, hi, t["fmax"], precision, nthreads) for f, (_k, lo, hi) in zip(t["fwd"], triples(C))], C)


# ---- the scenes of tests/test_gpu_features.py and their oracle runs, computed once per (scene, triple) ----
REPLICA = "replica"            # tests/test_gpu_depth.py's: 272 x 256 pixels, 200 Gaussians and one that covers all 272 tiles (replica rows)
CONFIGS = depth_ref.SCENES + (REPLICA,)
IDS = [f"P{c[0]}" for c in depth_ref.SCENES] + [REPLICA]
EDGE_CHANNELS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64)      # around the kernels' chunks of 4, 8 and 16, and around multiples of 16
SCENE_CHANNELS = (4, 17)                                                       # every scene: one chunk of 4; one channel above a chunk of 16
# map_grad's seed per scene, 11 where none is named.  On a scene with fewer than 500 gradient rows a single row beyond GRAD_RTOL is more
# than the gates' failing fraction (2e-3), so there the float32 oracle's own worst row must stay well inside it: on the replica scene
# (201 rows) seed 11 leaves one dL/dscales row of the float32 oracle 1.5e-3 from the float64 one at C = 17, seed 17 none beyond 1.8e-4
# (tests/test_features_ref_host.py asserts GRAD_RTOL / 2)
GRAD_SEEDS = {REPLICA: 17}


@functools.lru_cache(maxsize=None)
def scene(cfg, cov=False):
    if cfg == REPLICA:
        sc = synth.make_scene(P=201, width=272, height=256, sh_degree=1, s0=0.05, seed=0)
        sc.scales[0] = np.array([8.0, 8.0, 8.0], np.float32)
        sc.opacities[0] = 0.6
    else:
        P, W, H, s0, seed = cfg
        sc = synth.make_scene(P=P, width=W, height=H, sh_degree=1, s0=s0, seed=seed)
    S = oracle_scene(sc)
    if cov:             # the same Gaussians given as packed 3D covariances (xx xy xz yy yz zz) of R S S^T R^T
        q = np.asarray(S.rotations, np.float64); s = np.asarray(S.scales, np.float64)
        r, x, y, z = q.T
        R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                      2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
        Mm = R * s[:, None, :]
        Sg = Mm @ Mm.transpose(0, 2, 1)
        cov6 = np.stack([Sg[:, 0, 0], Sg[:, 0, 1], Sg[:, 0, 2], Sg[:, 1, 1], Sg[:, 1, 2], Sg[:, 2, 2]], 1).astype(np.float32)
        S = dataclasses.replace(S, scales=None, rotations=None, cov3D_precomp=cov6)
    return S


class Reference:
    """The oracle's side of one scene for every channel count: features(radii, 64), map_grad(S, 64) and, per triple (first channel,
    channels in it), the float32 and float64 forward and backward results -- run when first asked for, kept, never changed."""

    def __init__(self, cfg, cov=False):
        self.S = scene(cfg, cov)
        r32 = ref.get("f32")
        self.base = r32.forward(self.S, nthreads=r32.max_threads())
        self.radii = self.base["radii"]
        self.F = features(self.radii, 64)
        self.G = map_grad(self.S, 64, GRAD_SEEDS.get(cfg, 11))
        self.fmax = fmax_of(self.F, self.radii)
        self._triples = {}

    def triple(self, lo, hi):
        t = self._triples.get((lo, hi))
        if t is None:
            Sp, f32 = triple_forward(self.S, self.F, lo, hi, self.fmax, "f32")
            _, f64 = triple_forward(self.S, self.F, lo, hi, self.fmax, "f64")
            t = self._triples[(lo, hi)] = dict(Sp=Sp, f32=f32, f64=f64, g32=triple_backward(f32, self.G, lo, hi, self.fmax, "f32"),
                                               g64=triple_backward(f64, self.G, lo, hi, self.fmax, "f64"))
        return t

    def of(self, C):
        """dict(F, G, fmax, triples = [(lo, hi, triple)], g32, g64 = the summed gradients) for the leading C channels."""
        ts = [(lo, hi, self.triple(lo, hi)) for _k, lo, hi in triples(C)]
        assert fmax_of(self.F[:, :C], self.radii) == self.fmax
        return dict(F=self.F[:, :C].copy(), G=self.G[:C].copy(), fmax=self.fmax, triples=ts, g32=add_triples([t["g32"] for _l, _h, t in ts], C),
                    g64=add_triples([t["g64"] for _l, _h, t in ts], C))


@functools.lru_cache(maxsize=None)
def reference(cfg, cov=False):
    return Reference(cfg, cov)


def triple_image(fmap, lo, hi, fmax):
    """Channels lo..hi of a [C,H,W] map as the three-channel image the oracle's trick render of that triple produces."""
    return pad3(np.asarray(fmap, np.float64), lo, hi) / fmax


GRAD_NAMES = (("means3D", "dL_dmeans3D"), ("means2D", "dL_dmeans2D"), ("opacities", "dL_dopacity"), ("scales", "dL_dscales"),
              ("rotations", "dL_drots"), ("cov3D_precomp", "dL_dcov3D"), ("features", "dL_dfeatures"))


def check_against(R, C, fmap, grads=None, radii=None):
    """The project's gates on a [C,H,W] map and (grads: dict by API name, or None) its gradients against the oracle runs of
    R = reference(...): every triple's image through assert_image_certified within the cap, the gradients -- dL/dF held as dL_dcolors
    is -- through build_report / assert_parity.  Returns the (pixels over tolerance, uncertified) counts per triple."""
    o = R.of(C)
    counts = []
    for lo, hi, t in o["triples"]:
        st = assert_image_certified(triple_image(fmap, lo, hi, o["fmax"]), t["f32"]["color"], t["f32"]["state"].decision_margin())
        assert st["over"] <= max(3, MAX_CERTIFIED_FRAC * st["pixels"]), (lo, hi, st)
        counts.append((st["over"], st["uncertified"]))
    if grads is not None:
        H, G32, G64 = {}, {}, {}
        for hk, rk in GRAD_NAMES:
            if grads.get(hk) is None or o["g32"].get(rk) is None:
                continue
            H[hk] = np.asarray(grads[hk], np.float64)
            G32[hk] = o["g32"][rk].reshape(H[hk].shape); G64[hk] = o["g64"][rk].reshape(H[hk].shape)
        assert {"means3D", "means2D", "opacities"} <= set(H) and ({"scales", "rotations"} <= set(H) or "cov3D_precomp" in H)
        lo, hi, t = o["triples"][0]
        rep = build_report(t["Sp"], t["f32"], t["f64"], triple_image(fmap, lo, hi, o["fmax"]), H, G32, G64,
                           radii_equal=radii is None or bool(np.array_equal(radii, R.radii)))
        print(C, {k: (rep["grads_vs_f32"][k]["p99"], rep["grads_vs_f32"][k]["fail_frac"], rep["grads"][k]["p99"], rep["grads_f32_oracle"][k]["p99"]) for k in H})
        assert_parity(rep)
    return counts


# ---- the independent statement: pixel by pixel from the oracle's lists ----
def _walk_without_last(geom, vals, r0, r1, x, y, F32):
    """One pixel in float32, the walk of helpers.recomposite_pixel restated for a C-vector with a planted fault: the last entry the
    pixel blends is left out."""
    f32 = np.float32
    xy, co = geom["xy"], geom["conic_o"]
    Tr = f32(1.0)
    terms = []
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
        if Tn < f32(1e-4):
            break
        terms.append(F32[k] * f32(alpha * Tr))
        Tr = Tn
    out = np.zeros(F32.shape[1], np.float32)
    for t in terms[:-1]:
        out = (out + t).astype(np.float32)
    return out


def _pixel(geom, vals, r0, r1, x, y, F32, fault=None):
    """The C values of one pixel in float32.  No fault: through helpers.recomposite_pixel, three channels at a time, background 0."""
    if fault == "missed_last":
        return _walk_without_last(geom, vals, r0, r1, x, y, F32)
    C = F32.shape[1]
    out = np.zeros(C, np.float32)
    g = dict(geom)
    bg = np.full(3, 0.25 if fault == "background" else 0.0, np.float32)
    for _k, lo, hi in triples(C):
        g["rgb"] = pad3(F32, lo, hi).astype(np.float32)
        c, _ = recomposite_pixel(g, vals, r0, r1, x, y, bg)
        out[lo:hi] = c[:hi - lo]
    if fault == "normalised":
        g["rgb"] = np.ones((F32.shape[0], 3), np.float32)
        a, _ = recomposite_pixel(g, vals, r0, r1, x, y, np.zeros(3, np.float32))
        out = out / a[0] if a[0] > 0 else out * 0
    return out


def feature_pixels(S, F, fault=None, precision="f32", step=1):
    """map [C,H,W] re-composited pixel by pixel (float32 walk) from the lists of the oracle's run on S.  step > 1: only the pixels of
    every step-th row and column (from 0) are walked; the others read NaN.  fault: None, "background" (a background term T_final * 0.25
    added), "normalised" (divided by the accumulated alpha) or "missed_last" (the pixel's last contributor left out)."""
    r = ref.get(precision)
    f = r.forward(S, nthreads=r.max_threads())
    st = f["state"]
    geom, binn = st.geom(), st.binning()
    F32 = np.asarray(F, np.float32)
    C = F32.shape[1]
    out = np.full((C, S.H, S.W), np.nan)
    gridx = (S.W + 15) // 16
    for y in range(0, S.H, step):
        for x in range(0, S.W, step):
            r0, r1 = binn["ranges"][(y // 16) * gridx + (x // 16)]
            out[:, y, x] = _pixel(geom, binn["vals"], r0, r1, x, y, F32, fault) if r1 > r0 else (0.25 if fault == "background" else 0.0)
    return out
