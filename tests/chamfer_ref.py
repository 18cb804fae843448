"""Float64 NumPy reference of the Chamfer distance (include/gsr_chamfer.h) and the error bounds its tests assert.  Helper, not collected.

dist_bound(ref, D) = (D + 3) * 2^-24 * ref + D * 2^-149.  Derivation, u = 2^-24, float32 inputs: fl(a - b) carries one rounding,
its square two more relative errors (3u per term); summing D non-negative terms in any order adds at most (D - 1)u; so <= (D + 2)u
to first order, with or without FMA contraction (a contracted step only drops a rounding).  +1u absorbs the second-order terms; the
absolute term covers subnormal results.  All terms are non-negative, so there is no cancellation and the bound is relative to the
distance itself.  This holds for the difference form only, not for |a|^2 + |b|^2 - 2ab.

backward_bound: a float32 sum of k terms in unknown order, each term carrying <= 4 roundings, is within (k + 4) * 2^-24 * sum|terms|
of the exact sum."""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149


def dist_bound(ref, D):
    return (D + 3) * U * np.asarray(ref, dtype=np.float64) + D * TINY


def pair_dist(a, b, dtype=np.float64):
    """[n, m] matrix of sum_k (a[i,k] - b[j,k])^2, evaluated in `dtype`, k ascending (no FMA)."""
    a = np.asarray(a, dtype=dtype); b = np.asarray(b, dtype=dtype)
    d = np.zeros((a.shape[0], b.shape[0]), dtype=dtype)
    for k in range(a.shape[1]):
        t = a[:, k, None] - b[None, :, k]
        t *= t
        d += t
    return d


def _one_batch(a, b, rows=256):
    n, m = a.shape[0], b.shape[0]
    starts = list(range(0, n, rows))

    def work(s):
        d = pair_dist(a[s:s + rows], b)
        return s, d.min(axis=1), d.argmin(axis=1), d.min(axis=0), d.argmin(axis=0) + s
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        parts = list(ex.map(work, starts))
    d1 = np.empty(n); i1 = np.empty(n, dtype=np.int64)
    d2 = np.full(m, np.inf); i2 = np.zeros(m, dtype=np.int64)
    first = True
    for s, rmin, rarg, cmin, carg in parts:            # ascending s: a strict < keeps the first minimum
        d1[s:s + rows] = rmin; i1[s:s + rows] = rarg
        better = np.ones(m, dtype=bool) if first else cmin < d2
        d2[better] = cmin[better]; i2[better] = carg[better]
        first = False
    return d1, i1, d2, i2


def chamfer_ref(x1, x2):
    """x1 [B,N,D], x2 [B,M,D] -> dist1 [B,N], idx1 [B,N], dist2 [B,M], idx2 [B,M]; float64 brute force, first minimum."""
    x1 = np.asarray(x1, dtype=np.float64); x2 = np.asarray(x2, dtype=np.float64)
    out = [_one_batch(x1[b], x2[b]) for b in range(x1.shape[0])]
    return tuple(np.stack([o[k] for o in out]) for k in range(4))


def dist_to(x1, x2, idx):
    """Float64 distance from every row of x1 to the row idx[...] of x2: [B,N]."""
    x1 = np.asarray(x1, dtype=np.float64); x2 = np.asarray(x2, dtype=np.float64)
    sel = np.take_along_axis(x2, np.asarray(idx, dtype=np.int64)[:, :, None], axis=1)
    return ((x1 - sel) ** 2).sum(-1)


def backward_ref(x1, x2, idx1, idx2, g1, g2):
    """The backward formula of include/gsr_chamfer.h for GIVEN index arrays, in float64.  g1 / g2 may be None (= zeros).
    Returns (dx1, dx2, abs1, abs2, k1, k2): gradients, per-element sums of |terms|, per-row numbers of terms."""
    x1 = np.asarray(x1, dtype=np.float64); x2 = np.asarray(x2, dtype=np.float64)
    B, N, D = x1.shape; M = x2.shape[1]
    dx1 = np.zeros_like(x1); dx2 = np.zeros_like(x2); a1 = np.zeros_like(x1); a2 = np.zeros_like(x2)
    k1 = np.zeros((B, N), dtype=np.int64); k2 = np.zeros((B, M), dtype=np.int64)
    for b in range(B):
        for (xa, xb, idx, g, da, db, aa, ab, ka, kb) in ((x1[b], x2[b], idx1[b], None if g1 is None else g1[b], dx1[b], dx2[b], a1[b], a2[b], k1[b], k2[b]),
                                                         (x2[b], x1[b], idx2[b], None if g2 is None else g2[b], dx2[b], dx1[b], a2[b], a1[b], k2[b], k1[b])):
            if g is None:
                continue
            j = np.asarray(idx, dtype=np.int64)
            t = 2.0 * np.asarray(g, dtype=np.float64)[:, None] * (xa - xb[j])
            da += t; aa += np.abs(t); ka += 1
            np.add.at(db, j, -t); np.add.at(ab, j, np.abs(t)); np.add.at(kb, j, 1)
    return dx1, dx2, a1, a2, k1, k2


def backward_bound(abs_terms, k):
    return (np.asarray(k, dtype=np.float64)[..., None] + 4) * U * abs_terms


def make_cloud(kind, B, N, M, D, seed):
    """The three clouds of the tests, float32: 'normal'; 'dup' = near-duplicates (sigma 1e-3 around shared centres);
    'wide' = wide dynamic range (every coordinate scaled by 10^U(-3, 3))."""
    rng = np.random.default_rng(seed)
    if kind == "normal":
        x1, x2 = rng.normal(size=(B, N, D)), rng.normal(size=(B, M, D))
    elif kind == "dup":
        K = max(1, min(N, M) // 4)
        c = rng.normal(size=(B, K, D))
        x1 = np.stack([c[b][rng.integers(0, K, N)] for b in range(B)]) + 1e-3 * rng.normal(size=(B, N, D))
        x2 = np.stack([c[b][rng.integers(0, K, M)] for b in range(B)]) + 1e-3 * rng.normal(size=(B, M, D))
    elif kind == "wide":
        x1 = rng.normal(size=(B, N, D)) * 10.0 ** rng.uniform(-3, 3, size=(B, N, D))
        x2 = rng.normal(size=(B, M, D)) * 10.0 ** rng.uniform(-3, 3, size=(B, M, D))
    else:
        raise ValueError(kind)
    return x1.astype(np.float32), x2.astype(np.float32)


def make_integer_cloud(N, M, D, seed, dups=50):
    """Coordinates from the integers -8..8 (every float32 operation exact), `dups` target rows repeated further down."""
    rng = np.random.default_rng(seed)
    x1 = rng.integers(-8, 9, size=(1, N, D)).astype(np.float32)
    x2 = rng.integers(-8, 9, size=(1, M, D)).astype(np.float32)
    src = rng.choice(M // 2, size=dups, replace=False)
    x2[0, src + M // 2] = x2[0, src]
    return x1, x2
