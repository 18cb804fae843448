"""Torch restatements of include/gsr_rows.h on CPU tensors: what gsr_rows_unpack and gsr_rows_grad_pack must produce, bit for bit.
Their own proof: tests/test_rows_host.py (against sequence.unflatten_gaussians and autograd through it)."""
import numpy as np
import torch


def blocks(D: int):
    """(name, first column, width) of the parameter column groups of a D-column row, in the ORDER they sit in a gradient arena."""
    K = (D - 14) // 3
    assert D == 3 * K + 14 and 1 <= K <= 16, D
    return [("xyz", 3 * K + 5, 3), ("f_dc", 0, 3), ("f_rest", 3, 3 * (K - 1)), ("opacity", 3 * K + 4, 1), ("scaling", 3 * K + 8, 3),
            ("rotation", 3 * K, 4)]


def arena_floats(P: int, D: int) -> int:
    return P * sum(w for _, _, w in blocks(D))          # P (3 K + 11)


def unpack_ref(rows: torch.Tensor) -> dict:
    """The six dense buffers of gsr_rows_unpack, as a dict in the function's argument order; f_rest is [P, 0, 3] at K = 1."""
    P, D = rows.shape
    K = (D - 14) // 3
    shape = dict(xyz=(P, 3), f_dc=(P, 1, 3), f_rest=(P, K - 1, 3), opacity=(P, 1), scaling=(P, 3), rotation=(P, 4))
    return {name: rows[:, col:col + w].clone().reshape(shape[name]) for name, col, w in blocks(D)}


def pack_ref(arenas, P: int, D: int) -> torch.Tensor:
    """grad_rows [P, D] of gsr_rows_grad_pack: every block summed over the arenas in order, starting from the first arena's own
    values; flag columns +0.0."""
    out = torch.zeros((P, D), dtype=torch.float32)
    off = 0
    for _, col, w in blocks(D):
        tot = arenas[0][off:off + P * w].clone()
        for a in arenas[1:]:
            tot = tot + a[off:off + P * w]
        out[:, col:col + w] = tot.reshape(P, w)
        off += P * w
    return out


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def canonical_nan_bits(t: torch.Tensor) -> torch.Tensor:
    """Bit patterns with every NaN replaced by one pattern (an addition may hand back any of its NaN operands' payloads)."""
    b = bits(t).clone()
    b[torch.isnan(t.contiguous())] = 0x7fc00000
    return b


SPECIALS = np.array([0x7fc00000, 0x7fa12345, 0xffc00001, 0x7f800000, 0xff800000, 0x80000000, 0x00000001, 0x807fffff, 0x00400000],
                    dtype=np.uint32)        # NaNs with payloads (quiet, signalling, negative), +-inf, -0.0, denormals


def planted_rows(P: int, D: int, seed: int) -> torch.Tensor:
    """Random rows with NaN payloads, infinities, -0.0 and denormals planted: every special in every column when P allows, and in
    the first and the last row."""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(P, D)).astype(np.float32).view(np.uint32)
    n = max(1, (P * D) // 7)
    a.reshape(-1)[rng.choice(P * D, n, replace=False)] = rng.choice(SPECIALS, n)
    for c in range(D):
        a[(c * 5) % P, c] = SPECIALS[c % len(SPECIALS)]
        a[P - 1 - (c * 3) % P, c] = SPECIALS[(c + 4) % len(SPECIALS)]
    return torch.from_numpy(a.view(np.float32).copy())


def planted_arenas(B: int, P: int, D: int, seed: int, nonfinite: bool = False):
    """B finite random arenas with -0.0 planted in every block of every arena: at shared positions (so that -0.0 + -0.0 occurs),
    at positions of the first arena alone, and in the first and last entry of a block.  With `nonfinite`, NaN and infinities too."""
    rng = np.random.default_rng(seed)
    n = arena_floats(P, D)
    out = []
    for b in range(B):
        a = (rng.normal(size=n) * 10.0 ** rng.integers(-3, 3, size=n)).astype(np.float32)
        off = 0
        for _, _, w in blocks(D):
            m = P * w
            if m:
                a[off] = -0.0                       # shared by every arena
                a[off + m - 1] = -0.0
                a[off + (7 * b + 3) % m] = -0.0     # this arena alone (mostly)
                if nonfinite:
                    a[off + (11 * b + 5) % m] = [np.nan, np.inf, -np.inf][b % 3]
            off += m
        out.append(torch.from_numpy(a))
    return out
