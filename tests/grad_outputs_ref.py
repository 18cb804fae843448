"""Scenes for the gradient-output tests (tests/test_gpu_grad_outputs.py; certified on the CPU by tests/test_grad_outputs_host.py).

gsr_backward promises that every element of every gradient output is written exactly once: zeros for the Gaussians the frame culled
(radii == 0) and for those in view that no pixel composited.  synth.make_scene puts every mean inside the frustum, so its scenes have
next to none of either class; planted_scene() replants disjoint random subsets of one of them:
  * P // 8 behind the camera (z negated) and P // 8 far outside the frustum (x = 40 z): culled;
  * max(4, P // 32) as an opaque wall close to the camera over the left half of the image: what lies behind it is in view, binned,
    and never composited (the pixels stop at the wall).
classes() sorts the Gaussians of an oracle run into the three classes the tests rely on.
"""
import dataclasses
import functools

import numpy as np

from gaussian_transformer_amd import synth
from tests.helpers import GRAD_KEYS, oracle_runs, oracle_scene

FORMS = ("sh", "colors_cov")
MAX_TILES_PERSISTENT = 6144          # GSR_PERSISTENT_MAX_TILES (csrc/gsr_internal.h): above, make_plan leaves the persistent kernel
FILL_CHUNK = 256                     # GSR_SEG_FILL_CHUNK: Gaussians per zero-fill unit
BANDS = 32                           # GSR_SEG_BANDS: unit lists; with more chunks than bands a band holds several


def cov6_of(scales, rotations):
    """Packed 3D covariances (xx xy xz yy yz zz) of R S S^T R^T, float32 (as tests/test_gpu_depth.py::scene packs them)."""
    q = np.asarray(rotations, np.float64); s = np.asarray(scales, np.float64)
    r, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    Mm = R * s[:, None, :]
    Sg = Mm @ Mm.transpose(0, 2, 1)
    return np.stack([Sg[:, 0, 0], Sg[:, 0, 1], Sg[:, 0, 2], Sg[:, 1, 1], Sg[:, 1, 2], Sg[:, 2, 2]], 1).astype(np.float32)


def planted_synth(P, W, H, sh_degree, max_sh_degree, seed, s0=0.05, wall_n=None):
    """The SyntheticScene (scales, rotations, SH) with the three subsets replanted; below 8 Gaussians the plain scene.
    s0, wall_n: the recipe's constants (median scale of the plain scene; Gaussians in the wall, max(4, P // 32) unless given)."""
    sc = synth.make_scene(P=P, width=W, height=H, sh_degree=sh_degree, max_sh_degree=max_sh_degree, s0=s0, seed=seed)
    if P < 8:
        return sc
    rng = np.random.default_rng(seed + 7919)
    order = rng.permutation(P)
    nb, nf, nw = P // 8, P // 8, max(4, P // 32) if wall_n is None else wall_n
    behind, far, wall = order[:nb], order[nb:nb + nf], order[nb + nf:nb + nf + nw]
    sc.means3D[behind, 2] *= -1.0
    sc.means3D[far, 0] = 40.0 * sc.means3D[far, 2]
    sc.means3D[wall] = np.stack([rng.uniform(-0.55, 0.0, nw), rng.uniform(-0.5, 0.5, nw), np.ones(nw)], 1).astype(np.float32)
    sc.scales[wall] = np.array([0.25, 0.25, 0.01], np.float32)
    sc.rotations[wall] = np.array([1.0, 0.0, 0.0, 0.0], np.float32)
    sc.opacities[wall] = 0.99
    return sc


def planted_scene(P, W, H, sh_degree, max_sh_degree, seed, form, **recipe):
    """(oracle Scene, upstream gradient) of the planted scene.  form "sh": scales + rotations + SH; "colors_cov": colors_precomp
    (uniform in [0, 1]) + the packed cov3D_precomp of the same Gaussians."""
    assert form in FORMS
    sc = planted_synth(P, W, H, sh_degree, max_sh_degree, seed, **recipe)
    S = oracle_scene(sc)
    if form == "colors_cov":
        colors = np.random.default_rng(seed + 104729).uniform(0.0, 1.0, (P, 3)).astype(np.float32)
        S = dataclasses.replace(S, shs=None, sh_degree=0, colors_precomp=colors, scales=None, rotations=None,
                                cov3D_precomp=cov6_of(sc.scales, sc.rotations))
    return S, sc.dL_dimage


# name -> (P, W, H, sh_degree, max_sh_degree, seed, form[, recipe constants]); "r0" is "main" with every mean moved 1000 units behind the camera
SCENES = {
    "main": (1501, 250, 131, 3, 3, 5, "sh"),
    "main_cc": (1501, 250, 131, 3, 3, 5, "colors_cov"),
    "m4": (1501, 250, 131, 1, 1, 5, "sh"),
    "m9": (1501, 250, 131, 2, 2, 5, "sh"),
    # (seed 5 with active degree 2: two of the 421 rows of the float32 oracle's own dL_dopacity miss the row bar against float64 --
    # cancelling sums -- and a gate of 2e-3 over 421 rows admits none; seed 4 has no such row, see the host test)
    "m16_deg2": (1501, 250, 131, 2, 3, 4, "sh"),
    "p1": (1, 40, 24, 3, 3, 3, "sh"),
    "p63": (63, 40, 24, 3, 3, 3, "sh"),
    "p64": (64, 40, 24, 3, 3, 3, "sh"),
    "p65": (65, 40, 24, 3, 3, 3, "sh"),
    "p257": (257, 100, 52, 3, 3, 7, "sh"),
    "p4099": (4099, 250, 131, 3, 3, 6, "sh"),
    # 250 x 131 pixels give at most a few thousand Gaussians a gradient, and a wall of P // 32 = 512 splats (3 sigma = 0.75 of the 1.15 the
    # frustum is wide at their depth) hides nearly all of them: fewer in the wall, smaller Gaussians, for P / 8 with a gradient
    "p16411": (16411, 250, 131, 3, 3, 7, "sh", dict(s0=0.03, wall_n=64)),
    "large": (1501, 1552, 1040, 3, 3, 4, "sh"),
    "r0": (1501, 250, 131, 3, 3, 5, "sh"),
}
# The render_fused case: degree 1 of max 3, planted_synth(*SPLIT), scale modifier SPLIT_SCALE_MODIFIER.  It compares two renders whose inputs differ
# by the rounding of the activations (torch's against the kernels') in max norm, at 1e-4: one discrete decision of the compositing walk
# taken the other way moves a gradient by more than that (at 250 x 131, seed 5, the float32 oracle's smallest decision margin is 5e-7 and
# one-ulp changes of its inputs move its dL_dmeans2D by 3.5e-4 of the largest element), so the scene is chosen for the oracle's margins:
# rounding_sensitivity() below, asserted by the host test.
SPLIT = (1501, 100, 52, 1, 3, 6)
SPLIT_SCALE_MODIFIER = 0.9


@functools.lru_cache(maxsize=None)
def scene(name):
    cfg = SCENES[name]
    S, dL = planted_scene(*cfg[:7], **(cfg[7] if len(cfg) > 7 else {}))
    if name == "r0":
        m = np.array(S.means3D, np.float32, copy=True)
        m[:, 2] -= 1000.0
        S = dataclasses.replace(S, means3D=m)
    return S, dL


@functools.lru_cache(maxsize=None)
def oracles(name):
    """(float32 forward, float32 backward, float64 forward, float64 backward) of the oracle: computed once per scene, shared, left alone."""
    S, dL = scene(name)
    return oracle_runs(S, dL)


def rows_with_gradient(grads):
    """bool [P]: the rows in which any gradient tensor of an oracle backward() result is non-zero."""
    has = None
    for _, rk in GRAD_KEYS:
        g = grads.get(rk)
        if g is None:
            continue
        nz = np.abs(np.asarray(g).reshape(len(g), -1)).max(axis=1) > 0
        has = nz if has is None else has | nz
    return has


def classes(fwd, grads):
    """dict(culled, idle, grad) of bool [P]: radii == 0; in view without any gradient; with a gradient (always in view)."""
    has = rows_with_gradient(grads)
    seen = np.asarray(fwd["radii"]) > 0
    assert not (has & ~seen).any(), "a culled Gaussian has a gradient"
    return dict(culled=~seen, idle=seen & ~has, grad=has)


def api_gradients(S):
    """The gradient tensors gsr_backward writes for S, by their API names."""
    return ({"means3D", "means2D", "opacities"} | ({"shs"} if S.shs is not None else {"colors_precomp"}) |
            ({"scales", "rotations"} if S.scales is not None else {"cov3D_precomp"}))


def tiles(S):
    return ((S.W + 15) // 16) * ((S.H + 15) // 16)


def fill_chunks(P):
    return (P + FILL_CHUNK - 1) // FILL_CHUNK


def _one_ulp(a, rng):
    """Every element of a float32 array moved to its lower neighbour, left alone, or moved to its upper neighbour, at random."""
    a = np.asarray(a, np.float32)
    k = rng.integers(-1, 2, a.shape)
    up, down = np.nextafter(a, np.float32(np.inf)), np.nextafter(a, np.float32(-np.inf))
    return np.where(k > 0, up, np.where(k < 0, down, a)).astype(np.float32)


def rounding_sensitivity(sc, scale_modifier=1.0, trials=25, seed=0):
    """How far the float32 oracle's gradients move (helpers.grad_err, the largest over the tensors and the trials) when opacities, scales and
    rotations change by at most one ulp each -- what an activation evaluated by another implementation does to them -- and the oracle's
    smallest decision margin over the image.  Returns (largest grad_err, smallest margin, float32 forward, float32 backward)."""
    from oracle import ref
    from tests.helpers import grad_err
    r32 = ref.get("f32")
    nt = r32.max_threads()
    rng = np.random.default_rng(seed)
    S = oracle_scene(sc, scale_modifier=scale_modifier)
    f0 = r32.forward(S, nthreads=nt); g0 = r32.backward(f0, sc.dL_dimage, nthreads=nt)
    keys = [rk for hk, rk in GRAD_KEYS if hk in api_gradients(S)]
    worst = 0.0
    for _ in range(trials):
        S1 = dataclasses.replace(S, opacities=np.minimum(_one_ulp(sc.opacities, rng), np.float32(1.0)), scales=_one_ulp(sc.scales, rng),
                                 rotations=_one_ulp(sc.rotations, rng))
        f1 = r32.forward(S1, nthreads=nt); g1 = r32.backward(f1, sc.dL_dimage, nthreads=nt)
        worst = max(worst, max(grad_err(g1[k], g0[k]) for k in keys))
    return worst, float(f0["state"].decision_margin().min()), f0, g0
