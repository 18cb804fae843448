"""From a splat scene to token sequences (include/gsr_sequence.h, csrc/sequence.hip).

Restates the data path in front of the reference's transformer:

    model/box_sort.py                     flattenGaussians / unflattenGaussians / GaussianHandler (normalize, box_sort, denormalize)
    train_stacked_transformer.py:72-73    handler = GaussianHandler(gaussians, 40); gaussians = handler.denormalize(unflatten(handler.box_sort(gaussians)))
    train_stacked_transformer.py:91-98    visibility_filter |= render(cam, ...)["visibility_filter"] for every camera of the batch
    train_stacked_transformer.py:99-117   fold 2**STACK consecutive rows into one token, split into src / trg / trg_y

The two steps that are pathological there are native here: `box_sort_rows` (one stable sort instead of a 64 000-iteration Python
loop) and `visible_union_tensors` (one pass over the Gaussians instead of batch_size full renders whose images are thrown away).
Everything else is torch slicing.  There is no CPU fallback: tensors that are not float32 on a HIP device raise GsrError.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from .model import GaussianParams

MAX_N = 128          # GSR_BOX_MAX_N
MAX_D = 64           # GSR_BOX_MAX_D
MAX_B = 64           # GSR_VISIBLE_MAX_B: cameras per native call (larger sets are chunked here)


# ---------------------------------------------------------------- row layout ----------------------------------------------------------------

def row_width(n_sh: int) -> int:
    """Columns of a flattened Gaussian with n_sh SH coefficients: features 3 n_sh, rotation 4, opacity 1, xyz 3, scaling 3, flags 3."""
    return 3 * n_sh + 14


def xyz_column(D: int) -> int:
    """First coordinate column of a D-column row (17 for the reference's 26 columns)."""
    if D < 17 or (D - 14) % 3:
        raise _lib.GsrError(f"rows must have 3 K + 14 columns for K >= 1 SH coefficients, got D={D}")
    return D - 9


def flatten_gaussians(g) -> torch.Tensor:
    """model/box_sort.py:6-15 on a GaussianParams: [P, 3 K + 14] rows (26 columns for the reference's SH degree 1)."""
    features = g.get_features
    features = features.reshape((features.shape[0], features.shape[1] * features.shape[2]))
    flags = torch.zeros((g._scaling.shape[0], 3), device=features.device, dtype=features.dtype)
    return torch.cat((features, g._rotation, g._opacity, g._xyz, g._scaling, flags), dim=1)


def unflatten_gaussians(x: torch.Tensor) -> GaussianParams:
    """model/box_sort.py:17-27: the parameters are views of `x`; the SH degree follows from the row width."""
    if x.dim() != 2:
        raise _lib.GsrError(f"unflatten_gaussians: x must have shape [P, D], got {tuple(x.shape)}")
    c = xyz_column(int(x.shape[1]))
    K = (c - 5) // 3
    deg = int(round(math.sqrt(K))) - 1
    if (deg + 1) ** 2 != K:
        raise _lib.GsrError(f"unflatten_gaussians: D={x.shape[1]} holds K={K} SH coefficients, not a square number")
    g = GaussianParams(deg)
    features = x[:, :3 * K].reshape((x.shape[0], K, 3))
    g._features_dc = features[:, 0:1, :]
    g._features_rest = features[:, 1:, :]
    g._rotation = x[:, c - 5:c - 1]
    g._opacity = x[:, c - 1:c]
    g._xyz = x[:, c:c + 3]
    g._scaling = x[:, c + 3:c + 6]
    return g


def start_gaussian(D: int = 26, device=None) -> torch.Tensor:
    """START_GAUSSIAN of train_stacked_transformer.py:29-32: opacity and scaling -5, first flag 1."""
    c = xyz_column(D)
    t = torch.zeros(D, dtype=torch.float32, device=device)
    t[c + 3:c + 6] = -5
    t[c - 1] = -5
    t[c + 6] = 1
    return t


def pad_gaussian(D: int = 26, device=None) -> torch.Tensor:
    """PAD_GAUSSIAN of train_stacked_transformer.py:33-34: second flag 1."""
    t = torch.zeros(D, dtype=torch.float32, device=device)
    t[xyz_column(D) + 7] = 1
    return t


# ---------------------------------------------------------------- box sort ----------------------------------------------------------------

def _validate_box(rows, xyz_col, interval_num) -> None:
    _lib.require_tensor("box_sort_rows", "rows", rows)
    if rows.dim() != 2:
        raise _lib.GsrError(f"box_sort_rows: rows must have shape [P, D], got {tuple(rows.shape)}")
    _validate_box_sizes(int(rows.shape[1]), xyz_col, interval_num)
    _lib.require_hip("box_sort_rows", "rows", rows)


def _validate_box_sizes(D: int, xyz_col, interval_num) -> None:
    if not 3 <= D <= MAX_D:
        raise _lib.GsrError(f"box_sort_rows: rows has D={D} columns, supported: 3..{MAX_D}")
    if not isinstance(xyz_col, int) or not 0 <= xyz_col <= D - 3:
        raise _lib.GsrError(f"box_sort_rows: xyz_col={xyz_col!r} not in 0..D-3={D - 3}")
    if not isinstance(interval_num, int) or not 1 <= interval_num <= MAX_N:
        raise _lib.GsrError(f"box_sort_rows: interval_num={interval_num!r} not in 1..{MAX_N}")


def box_sort_rows(rows: torch.Tensor, xyz_col: int, interval_num: int):
    """Native box sort of float32 rows [P, D] on a HIP device whose columns xyz_col .. xyz_col+2 are normalised coordinates.

    Returns (out_rows [P, D], perm [P] int32, count [1] int32), all on the device, enqueued on the current stream without any
    host synchronisation.  Rows [0, count) are the reference's result: ordered by box ax + n ay + n^2 az, inside a box by
    original index; perm names their original rows.  Rows with a coordinate < 0, >= 1 or NaN belong to no box (the reference
    drops them silently): out_rows is zero and perm -1 in [count, P)."""
    _validate_box(rows, xyz_col, interval_num)
    rows = rows.detach().contiguous()
    P, D = int(rows.shape[0]), int(rows.shape[1])
    dev = rows.device
    out_rows = torch.empty_like(rows)
    perm = torch.empty((P,), dtype=torch.int32, device=dev)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    ptr = _lib.ptr
    with torch.cuda.device(dev):
        ws = _lib.workspace("gsr_box_sort_workspace", dev, P, interval_num)
        _lib.call("gsr_box_sort", _lib.stream(dev), P, D, ptr(rows), xyz_col, interval_num, ptr(out_rows), ptr(perm), ptr(count),
                  ptr(ws), ws.numel())
    return out_rows, perm, count


class GaussianHandler:
    """The interface of the reference's `GaussianHandler` (model/box_sort.py:30-82) on this repository's GaussianParams.

    The handler remembers two affine maps fixed at construction: positions, per axis, from [min, max] of the cloud to [0, 1],
    and raw (log) scalings, with one pair of extrema over all three columns, to [0, 1].  `normalize` / `denormalize` apply them
    and their inverses IN PLACE, as the reference does (train_stacked_transformer.py:73 relies on it); `denormalize_copy` leaves
    its argument alone.  Plain torch: elementwise, run once."""

    def __init__(self, gaussians, interval_num: int = 10) -> None:
        self.interval_num = interval_num
        self.box_num = interval_num ** 3
        xyz, scaling = gaussians.get_xyz, gaussians._scaling
        self.worldMin, self.worldMax = xyz.amin(0), xyz.amax(0)
        self.scalingMin, self.scalingMax = scaling.amin(), scaling.amax()

    def _maps(self):
        return ((self.worldMin, self.worldMax - self.worldMin), (self.scalingMin, self.scalingMax - self.scalingMin))

    def normalize(self, gaussians):
        (x0, xs), (s0, ss) = self._maps()
        gaussians._xyz = (gaussians.get_xyz - x0) / xs
        gaussians._scaling = (gaussians._scaling - s0) / ss
        return gaussians

    def denormalize(self, gaussians):
        (x0, xs), (s0, ss) = self._maps()
        gaussians._xyz = gaussians.get_xyz * xs + x0
        gaussians._scaling = gaussians._scaling * ss + s0
        return gaussians

    def denormalize_copy(self, gaussians):
        """A new GaussianParams in world units sharing the other tensors with `gaussians`.  Its SH degree is that of `gaussians`
        (the reference hard-codes degree 3 here whatever the input holds; not reproduced)."""
        g = GaussianParams(gaussians.max_sh_degree)
        g.active_sh_degree = gaussians.active_sh_degree
        for name in ("_features_dc", "_features_rest", "_opacity", "_rotation", "_xyz", "_scaling"):
            setattr(g, name, getattr(gaussians, name))
        return self.denormalize(g)

    def box_sort(self, gaussians, return_perm: bool = False):
        """Normalises `gaussians` (in place, as the reference), flattens them and orders the rows by box.

        Returns the sorted rows [count, D]: ONLY the rows that lie in a box.  A Gaussian that attains the maximum on an axis has
        the normalised coordinate 1.0 and lies in none, so count < P for any real scene; the reference returns P rows whose tail
        is uninitialised memory instead.  Reading `count` is this method's one host synchronisation (`box_sort_rows` has none);
        it is meant to run once per scene, and allocates its workspace per call.
        With return_perm, also the int64 original indices [count] of the returned rows."""
        with torch.no_grad():
            rows = flatten_gaussians(self.normalize(gaussians))
            out_rows, perm, count = box_sort_rows(rows, xyz_column(int(rows.shape[1])), self.interval_num)
            n = int(count.item())
            return (out_rows[:n], perm[:n].long()) if return_perm else out_rows[:n]


# ---------------------------------------------------------------- visibility ----------------------------------------------------------------

def _validate_visible(means3D, scales, rotations, cov3D_precomp, raw_params, n_cameras) -> None:
    """Types, dtypes, shapes and the combination of arguments first (checkable on any tensors), devices last."""
    who = "visible_union"
    if n_cameras < 1:
        raise _lib.GsrError(f"{who}: cameras must hold at least one camera")
    _lib.require_tensor(who, "means3D", means3D)
    if means3D.dim() != 2 or means3D.shape[1] != 3:
        raise _lib.GsrError(f"{who}: means3D must have shape [P, 3], got {tuple(means3D.shape)}")
    P = int(means3D.shape[0])
    if (cov3D_precomp is None) == (scales is None and rotations is None) or (cov3D_precomp is None and (scales is None or rotations is None)):
        raise _lib.GsrError(f"{who}: exactly one of (scales, rotations) / cov3D_precomp must be given")
    if raw_params and cov3D_precomp is not None:
        raise _lib.GsrError(f"{who}: raw_params needs scales and rotations, not cov3D_precomp")
    given = [(n, t, w) for n, t, w in (("scales", scales, 3), ("rotations", rotations, 4), ("cov3D_precomp", cov3D_precomp, 6)) if t is not None]
    for name, t, w in given:
        _lib.require_tensor(who, name, t)
        if tuple(t.shape) != (P, w):
            raise _lib.GsrError(f"{who}: {name} must have shape [{P}, {w}], got {tuple(t.shape)}")
    _lib.require_hip(who, "means3D", means3D)
    for name, t, _ in given:
        _lib.require_hip(who, name, t)
        if t.device != means3D.device:
            raise _lib.GsrError(f"{who}: {name} is on {t.device} but means3D on {means3D.device}")


def _camera_matrices(cameras, dev):
    """[B, 16] view and projection matrices on `dev`.  Matrices that are tensors on `dev` already (TorchCamera) are stacked there,
    nothing crosses the bus; otherwise (numpy cameras, tensors elsewhere) all 2 B matrices go up in ONE host-to-device copy."""
    mats = [m for cam in cameras for m in (cam.world_view_transform, cam.full_proj_transform)]
    if all(isinstance(m, torch.Tensor) and m.device == dev for m in mats):
        both = torch.stack([m.to(torch.float32).reshape(16) for m in mats])
    else:
        host = np.stack([np.asarray(m.detach().cpu() if isinstance(m, torch.Tensor) else m, dtype=np.float32).reshape(16) for m in mats])
        both = torch.from_numpy(host).to(dev)
    both = both.reshape(len(cameras), 2, 16)
    return both[:, 0].contiguous(), both[:, 1].contiguous()


def visible_union_tensors(cameras, means3D, scales=None, rotations=None, cov3D_precomp=None, scale_modifier: float = 1.0,
                          raw_params: bool = False, want_radii: bool = False, want_visible: bool = True, want_counts: bool = False):
    """The native call on tensors.  Returns (visible [P] bool or None, radii [B, P] int32 or None, counts [B] int32 or None);
    radii[b] is bit for bit what the rasterizer returns for cameras[b] with the same inputs.  Any number of cameras: the native
    call takes 64 at a time.  Nothing is read back.  With camera matrices that are tensors on the Gaussians' device (TorchCamera)
    the host never waits for the device; cameras holding numpy matrices cost one blocking upload of all their matrices per call."""
    cameras = list(cameras)
    _validate_visible(means3D, scales, rotations, cov3D_precomp, raw_params, len(cameras))
    dev, ptr = means3D.device, _lib.ptr
    P, B = int(means3D.shape[0]), len(cameras)
    c = lambda t: None if t is None else t.detach().contiguous()
    means3D, scales, rotations, cov3D_precomp = c(means3D), c(scales), c(rotations), c(cov3D_precomp)
    view, proj = _camera_matrices(cameras, dev)
    radii = torch.empty((B, P), dtype=torch.int32, device=dev) if want_radii else None
    counts = torch.empty((B,), dtype=torch.int32, device=dev) if want_counts else None
    visible = None
    with torch.cuda.device(dev):
        stream = _lib.stream(dev)
        for b0 in range(0, B, MAX_B):
            nb = min(MAX_B, B - b0)
            chunk = cameras[b0:b0 + nb]
            tfx = (C.c_float * nb)(*[math.tan(cam.FoVx * 0.5) for cam in chunk])
            tfy = (C.c_float * nb)(*[math.tan(cam.FoVy * 0.5) for cam in chunk])
            ws_ = (C.c_int32 * nb)(*[int(cam.image_width) for cam in chunk])
            hs_ = (C.c_int32 * nb)(*[int(cam.image_height) for cam in chunk])
            vis = torch.empty((P,), dtype=torch.uint8, device=dev) if want_visible else None
            _lib.call("gsr_visible_union", stream, P, nb, ptr(means3D), ptr(scales), float(scale_modifier), ptr(rotations),
                      ptr(cov3D_precomp), 1 if raw_params else 0, ptr(view[b0:]), ptr(proj[b0:]), tfx, tfy, ws_, hs_,
                      ptr(radii[b0:]) if want_radii else None, ptr(vis), ptr(counts[b0:]) if want_counts else None)
            if want_visible:
                visible = vis if visible is None else visible | vis
    return (visible.bool() if want_visible else None), radii, counts


def visible_union(cameras, gaussians, scaling_modifier: float = 1.0, return_radii: bool = False, return_counts: bool = False):
    """`visibility_filter` of train_stacked_transformer.py:91-96 without rendering: the OR over `cameras` of render()'s
    `radii > 0`, for the camera objects render() takes (image_width / image_height, FoVx / FoVy, world_view_transform,
    full_proj_transform) and a GaussianParams.  Returns visible [P] bool; with return_radii also radii [B, P] int32 (row b equals
    render(cameras[b], ...)["radii"]), with return_counts also counts [B] int32 (visible Gaussians per camera), in that order."""
    with torch.no_grad():
        visible, radii, counts = visible_union_tensors(cameras, gaussians.get_xyz, gaussians.get_scaling, gaussians.get_rotation,
                                                       scale_modifier=scaling_modifier, want_radii=return_radii, want_counts=return_counts)
    out = (visible,) + ((radii,) if return_radii else ()) + ((counts,) if return_counts else ())
    return out[0] if len(out) == 1 else out


# ---------------------------------------------------------------- tokens ----------------------------------------------------------------

def fold_tokens(rows: torch.Tensor, stack: int) -> torch.Tensor:
    """train_stacked_transformer.py:99-101: `stack` rounds of cat([x[0::2], x[1::2]], 1) put 2**stack consecutive rows side by
    side, which is a reshape of the truncated rows: a view when `rows` is contiguous, no copy."""
    if rows.dim() != 2 or stack < 0:
        raise _lib.GsrError(f"fold_tokens: rows must have shape [S, D] and stack be >= 0, got {tuple(rows.shape)}, stack={stack}")
    S, D = rows.shape
    k = 2 ** stack
    return rows[:S - S % k].reshape(-1, D * k)


def unstack(x: torch.Tensor, stack: int) -> torch.Tensor:
    """Inverse of fold_tokens: [..., T, D 2**stack] tokens back to [T 2**stack, D] rows."""
    k = 2 ** stack
    if x.shape[-1] % k:
        raise _lib.GsrError(f"unstack: last dimension {x.shape[-1]} is not a multiple of 2**stack={k}")
    return x.reshape(-1, x.shape[-1] // k)


def make_token_batch(flat_rows: torch.Tensor, visible: torch.Tensor, stack: int, dropout: float, u: float) -> dict:
    """train_stacked_transformer.py:98-117: the visible rows folded into tokens, a window of about 2 * dropout of them around a
    random centre cut out as the target, the rest the source.  `u` in [0, 1) is the one random draw (np.random.random() there).
    Returns {"src" [1, S, W], "trg" [1, T, W], "trg_y" [1, T, W]} on the device of flat_rows; trg starts with the START row and
    is trg_y shifted by one."""
    if not 0.0 <= u < 1.0:
        raise _lib.GsrError(f"make_token_batch: u={u!r} not in [0, 1)")
    D = int(flat_rows.shape[1])
    seen = fold_tokens(flat_rows[visible], stack)
    T = int(seen.shape[0])
    mid = T // 2
    low = int(mid - mid * dropout)
    high = int(mid + mid * dropout)
    offset = int((u * 0.8 + 0.1) * (low + (T - high)) - (T - high))
    low -= offset
    high -= offset
    src = torch.cat([seen[:low], seen[high:]])[None]
    start = start_gaussian(D, device=flat_rows.device).repeat(2 ** stack)[None]
    tgt = torch.cat([start, seen[low:high]])[None]
    return {"src": src, "trg": tgt[:, :-1], "trg_y": tgt[:, 1:]}
