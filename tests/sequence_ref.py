"""numpy restatements of the reference's sequence preparation, the yardsticks of tests/test_sequence_host.py and
tests/test_gpu_sequence.py.  Pinned to the reference itself by tests/golden/box_sort.npz (scripts/make_box_sort_golden.py)."""
import numpy as np


def boundaries(n: int) -> np.ndarray:
    """b_k = float32(double(1.0 / n) * k): what torch.FloatTensor([interval_size * x, ...]) holds (model/box_sort.py:53,59-60)."""
    interval_size = 1.0 / n
    return np.array([interval_size * k for k in range(n + 1)], dtype=np.float32)


def box_sort_loop(rows: np.ndarray, xyz_col: int, n: int):
    """model/box_sort.py:52-67, literally: one pass over all rows per box.  Returns (sorted rows [last], perm [last], last).
    O(n^3 P): small n only."""
    interval_size = 1.0 / n
    xyz = rows[:, xyz_col:xyz_col + 3]
    out, perm = [], []
    for i in range(n ** 3):
        x = i % n
        y = (i // n) % n
        z = i // n ** 2
        lo = np.array([interval_size * x, interval_size * y, interval_size * z], dtype=np.float32)
        hi = np.array([interval_size * (x + 1), interval_size * (y + 1), interval_size * (z + 1)], dtype=np.float32)
        mask = np.all(np.concatenate([xyz >= lo, xyz < hi], -1), -1)
        if mask.sum() == 0:
            continue
        out.append(rows[mask])
        perm.append(np.nonzero(mask)[0])
    if not out:
        return rows[:0].copy(), np.zeros(0, np.int64), 0
    out, perm = np.concatenate(out), np.concatenate(perm)
    return out, perm, len(perm)


def box_keys(rows: np.ndarray, xyz_col: int, n: int) -> np.ndarray:
    """Box of every row, n^3 for a row that lies in none (a coordinate < b_0, >= b_n or NaN)."""
    b = boundaries(n)
    xyz = rows[:, xyz_col:xyz_col + 3]
    with np.errstate(invalid="ignore"):
        valid = np.all((xyz >= b[0]) & (xyz < b[n]), axis=1)
    cell = np.searchsorted(b, np.where(np.isnan(xyz), np.float32(0), xyz), side="right").astype(np.int64) - 1     # b_a <= c < b_{a+1}
    key = cell[:, 0] + n * cell[:, 1] + n * n * cell[:, 2]
    return np.where(valid, key, n ** 3)


def box_sort_vec(rows: np.ndarray, xyz_col: int, n: int):
    """The same result by searchsorted on the boundary table and a stable argsort.  Returns what the native call writes:
    (out_rows [P, D] with a zero tail, perm [P] int32 with -1 in the tail, count)."""
    P = rows.shape[0]
    key = box_keys(rows, xyz_col, n)
    order = np.argsort(key, kind="stable")
    count = int((key < n ** 3).sum())
    out = np.zeros_like(rows)
    out[:count] = rows[order[:count]]
    perm = np.full(P, -1, np.int32)
    perm[:count] = order[:count]
    return out, perm, count


def box_keys_floor(rows: np.ndarray, xyz_col: int, n: int) -> np.ndarray:
    """The shortcut a kernel must NOT take: the cell from floor(c * n) in float32 alone (mutation check)."""
    xyz = rows[:, xyz_col:xyz_col + 3]
    with np.errstate(invalid="ignore"):
        valid = np.all((xyz >= 0) & (xyz < 1), axis=1)
        cell = np.clip(np.nan_to_num((xyz * np.float32(n)).astype(np.float32)).astype(np.int64), 0, n - 1)
    return np.where(valid, cell[:, 0] + n * cell[:, 1] + n * n * cell[:, 2], n ** 3)


def planted_rows(P: int, D: int, xyz_col: int, n: int, seed: int) -> np.ndarray:
    """Random rows in [0, 1) with the hard cases planted: coordinates exactly on boundaries and one ulp either side, NaN, -0.0,
    1.0, values just above 1, negatives, and the second half of the cloud a copy of part of the first (heavy duplicates)."""
    rng = np.random.default_rng(seed)
    rows = rng.random((P, D), dtype=np.float32)
    rows[:, :xyz_col] = rng.normal(size=(P, xyz_col)).astype(np.float32)
    b = boundaries(n)
    edge = np.concatenate([b, np.nextafter(b, np.float32(-np.inf)), np.nextafter(b, np.float32(np.inf)),
                           np.array([np.nan, -0.0, 1.0, 1.0000001, 1.5, -1e-30, -0.25, np.inf, -np.inf, 0.99999994], np.float32)]).astype(np.float32)
    k = min(P, 3 * P // 10)
    where = rng.choice(P, size=k, replace=False)
    rows[where, xyz_col + rng.integers(0, 3, size=k)] = edge[rng.integers(0, len(edge), size=k)]
    if P >= 4:
        rows[P // 2:] = rows[rng.integers(0, P // 2, size=P - P // 2)]
    return rows


def fold_cat(x: np.ndarray, stack: int) -> np.ndarray:
    """train_stacked_transformer.py:99-101, literally."""
    x = x[:(x.shape[0] // (2 ** stack)) * (2 ** stack)]
    for _ in range(stack):
        x = np.concatenate([x[0::2], x[1::2]], 1)
    return x


def start_gaussian() -> np.ndarray:
    """train_stacked_transformer.py:29-32."""
    s = np.zeros(26, np.float32)
    s[20:23] = -5
    s[16:17] = -5
    s[23] = 1
    return s


def token_batch(gaussian_list: np.ndarray, visibility_filter: np.ndarray, stack: int, dropout: float, u: float):
    """train_stacked_transformer.py:98-117, literally, with np.random.random() replaced by `u`.  26-column rows."""
    seen_gaussians = gaussian_list[visibility_filter]
    seen_gaussians = fold_cat(seen_gaussians, stack)
    mid = seen_gaussians.shape[0] // 2
    low = int(mid - mid * dropout)
    high = int(mid + mid * dropout)
    offset = int((u * 0.8 + 0.1) * (low + (seen_gaussians.shape[0] - high)) - (seen_gaussians.shape[0] - high))
    low -= offset
    high -= offset
    tgt_count = high - low
    src_count = seen_gaussians.shape[0] - tgt_count
    src_gaussians = np.zeros((1, src_count, 26 * 2 ** stack), np.float32)
    tgt_gaussians = np.zeros((1, tgt_count + 1, 26 * 2 ** stack), np.float32)
    src_gaussians[0] = np.concatenate([seen_gaussians[:low], seen_gaussians[high:]])
    tgt_gaussians[0, 0] = np.tile(start_gaussian(), 2 ** stack)
    tgt_gaussians[0, 1:] = seen_gaussians[low:high]
    return {"src": src_gaussians, "trg": tgt_gaussians[:, :-1], "trg_y": tgt_gaussians[:, 1:]}
