"""Seeded inputs shared by the edge tests of the loss, Adam and kNN kernels (tests/test_gpu_*_edges.py) and by the CPU check of
their float64 references (tests/test_aux_references.py).  Everything is generated in numpy and returned as float32."""
import numpy as np

# ---------------------------------------------------------------------------------------------
# L1 + SSIM: input families
# ---------------------------------------------------------------------------------------------
FAMILY_SHAPE = (3, 50, 37)             # several 16x16 tiles per axis, neither extent a multiple of 16

# H, W in {1, 2, 10, 11, 12, 15, 16, 17, 26, 27, 31, 32, 33} (tile 16, window 11, halo 5, staged 26: the off-by-one places), paired so
# that every value occurs on each axis; C cycles through 1..4
_EDGE = [1, 2, 10, 11, 12, 15, 16, 17, 26, 27, 31, 32, 33]
EDGE_SHAPES = [(1 + i % 4, h, _EDGE[(i + 5) % len(_EDGE)]) for i, h in enumerate(_EDGE)] + [(2, 1, 1), (4, 11, 11), (1, 16, 16)]


def _box_blur(a, times=6):
    for _ in range(times):                                   # 3x3 box with wrap-around, a few times: a smooth random field
        a = sum(np.roll(np.roll(a, dy, 1), dx, 2) for dy in (-1, 0, 1) for dx in (-1, 0, 1)) / 9.0
    return a


def smooth_pair(shape, seed=0):
    """Low-pass noise scaled to [0.2, 0.9] against the same field shifted by a pixel plus 1 % noise: high local correlation and a
    variance that is small against the squared mean (s11 - m1*m1 cancels)."""
    rng = np.random.default_rng(seed)
    f = _box_blur(rng.uniform(0, 1, shape))
    lo, hi = f.min(), f.max()
    f = 0.2 + 0.7 * (f - lo) / (hi - lo) if hi > lo else np.full(shape, 0.55)
    gt = np.roll(f, 1, axis=2) + 0.01 * rng.uniform(-1, 1, shape)
    return f.astype(np.float32), gt.astype(np.float32)


def flat_one_pixel(shape, y, x, seed=0, level=0.3, bright=1.0):
    """Both images flat (slightly different constants) except for one bright pixel of the image, in every channel."""
    img = np.full(shape, level, dtype=np.float32)
    gt = np.full(shape, level + 0.05, dtype=np.float32)
    img[:, min(y, shape[1] - 1), min(x, shape[2] - 1)] = bright
    return img, gt


def loss_families(shape=FAMILY_SHAPE):
    """name -> (image, target): the regimes the loss kernel meets in training and that uniform noise never produces."""
    C, H, W = shape
    rng = np.random.default_rng(12)
    out = {}
    out["smooth"] = smooth_pair(shape, 1)
    out["flat_equal"] = (np.full(shape, 0.5, np.float32), np.full(shape, 0.5, np.float32))
    out["flat_different"] = (np.full(shape, 0.25, np.float32), np.full(shape, 0.75, np.float32))
    out["flat_vs_noise"] = (np.full(shape, 0.4, np.float32), rng.uniform(0, 1, shape).astype(np.float32))
    out["noise_vs_flat"] = (rng.uniform(0, 1, shape).astype(np.float32), np.full(shape, 0.4, np.float32))
    out["flat_black"] = (np.zeros(shape, np.float32), np.zeros(shape, np.float32) + np.float32(0.1))
    for name, (y, x) in dict(corner=(0, 0), seam_x15=(H // 2, 15), seam_x16=(H // 2, 16), seam_y15=(15, W // 2), seam_y16=(16, W // 2),
                             interior=(H // 2 + 3, W // 2 + 2)).items():
        out["pixel_" + name] = flat_one_pixel(shape, y, x)
    target = smooth_pair(shape, 2)[1]
    out["converged_1e-3"] = ((target + 1e-3 * rng.uniform(-1, 1, shape)).astype(np.float32), target)
    out["converged_1e-6"] = ((target + 1e-6 * rng.uniform(-1, 1, shape)).astype(np.float32), target)
    out["converged_exact"] = (target.copy(), target)
    out["out_of_range"] = (rng.uniform(-0.5, 2.5, shape).astype(np.float32), rng.uniform(0, 1, shape).astype(np.float32))
    hot = smooth_pair(shape, 3)
    hot[0].reshape(-1)[rng.choice(hot[0].size, 5, replace=False)] = 50.0
    out["pixels_at_50"] = hot
    return out


# families in which image == target everywhere: the true gradient is 0 (SSIM has its maximum there, sign(0) = 0)
ALL_EQUAL = ("flat_equal", "converged_exact")


# ---------------------------------------------------------------------------------------------
# Adam: the gradient schedule of tests/test_gpu_optim.py, for any list of lengths
# ---------------------------------------------------------------------------------------------
ADAM_STEPS = 12
ADAM_LR_CHANGE_AFTER = 7               # 0-based step after which group 0's learning rate changes
ADAM_LR_CHANGED = 0.00005


def adam_params(lengths, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n).astype(np.float32) for n in lengths]


def adam_grads(lengths, step, seed=1):
    """Gradients of 0-based `step`: the scale changes by decades between steps, one step has exact zeros in every third element."""
    rng = np.random.default_rng([seed, step])
    out = []
    for n in lengths:
        g = (rng.standard_normal(n) * 10.0 ** (-(step % 4))).astype(np.float32)
        if step == 5:
            g[::3] = 0.0
        out.append(g)
    return out


# ---------------------------------------------------------------------------------------------
# kNN: clouds
# ---------------------------------------------------------------------------------------------
def cloud(kind, n, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        p = rng.uniform(-1, 1, (n, 3))
    elif kind == "clustered":           # as in tests/test_gpu_knn.py: 50 tight clusters and 100 far outliers
        c = rng.normal(0, 5, (50, 3)); p = c[rng.integers(0, 50, n)] + rng.normal(0, 0.05, (n, 3)); p[:100] = rng.normal(0, 200, (100, 3))
    elif kind == "sfm_like":
        p = rng.normal(0, 1, (n, 3)) * np.array([5.0, 5.0, 1.0]) + np.array([0.4, 1.0, 6.2])
    elif kind == "duplicates":          # a third of the points occur twice or more
        p = rng.uniform(-1, 1, (n, 3)); p[: n // 3] = p[rng.integers(n // 3, n, n // 3)]
    elif kind == "identical":
        p = np.tile(np.array([[0.3, -1.7, 2.5]]), (n, 1))
    elif kind == "collinear":           # spacing 1e-3 along a skew direction, in shuffled order
        t = rng.permutation(n)[:, None] * 1e-3
        p = np.array([[1.0, 2.0, -0.5]]) + t * np.array([[0.6, 0.0, 0.8]])
    elif kind == "grid":                # planar square grid (n must be a square): every point has 4 nearest neighbours at the same distance
        s = int(round(n ** 0.5)); assert s * s == n
        i, j = np.meshgrid(np.arange(s), np.arange(s), indexing="ij")
        p = np.stack([i.ravel() * 0.01, j.ravel() * 0.01, np.zeros(n)], 1)[rng.permutation(n)]
    else:
        raise ValueError(kind)
    return p.astype(np.float32)
