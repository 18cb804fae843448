"""Render B cameras straight from flat Gaussian rows (include/gsr_rows.h, csrc/rows.hip).

Every network-side call site of the reference renders `unflattenGaussians(rows)`, the rows being the transformer's or the
autoencoder's output (train_stacked_transformer.py:200-212 and :279, train_transformer.py:185-186, train_autoencoder.py:155,166-168).
Through `sequence.unflatten_gaussians` + `render_fused` that costs six contiguous() copies per camera on the way in and, on the way
back, a chain of slice / reshape nodes per camera and parameter, each allocating and zero-filling a [P, D] tensor, summed in whatever
order the autograd engine picks.  Here:

    unpack_rows(rows)                 one launch: the six dense raw-parameter buffers of gsr_forward's fused form
    render_rows(cameras, rows, ...)   one autograd node for all B cameras: one unpack, B forward calls; in backward B backward calls
                                      into B arenas and ONE launch that packs and sums them, in camera order, into dL/drows [P, D]

The rasterizer calls are exactly those of `rasterizer._RasterizeGaussiansFused`.  There is no CPU fallback: rows that are not
float32 on a HIP device raise GsrError.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .model import GaussianParams
from .rasterizer import _remember_forward, arena_floats, camera_settings, get_backend, gradient_arena

MAX_B = 64           # GSR_ROWS_MAX_B: arenas per native pack call (larger camera sets are packed in chunks and added in order)
_ALIGN = 16          # floats: every unpacked buffer starts on a 64-byte boundary


def _check_rows(who: str, rows) -> int:
    """Type, dtype, rank and width (checkable on any tensor; callers check the device last).  Returns K, the SH coefficients per row."""
    _lib.require_tensor(who, "rows", rows)
    if rows.dim() != 2:
        raise _lib.GsrError(f"{who}: rows must have shape [P, D], got {tuple(rows.shape)}")
    D = int(rows.shape[1])
    K = (D - 14) // 3
    if D < 17 or (D - 14) % 3 or K not in (1, 4, 9, 16):
        raise _lib.GsrError(f"{who}: rows must have D = 3 K + 14 columns for K in (1, 4, 9, 16) SH coefficients (17, 26, 41 or 62), got D={D}")
    return K


def _unpack(rows: torch.Tensor, K: int):
    """rows: contiguous, detached, validated.  Returns (xyz, f_dc, f_rest or None, opacity, scaling, rotation), slices of one
    allocation, written by one launch on the current stream."""
    P, dev, ptr = int(rows.shape[0]), rows.device, _lib.ptr
    shapes = [(P, 3), (P, 1, 3), (P, K - 1, 3), (P, 1), (P, 3), (P, 4)]
    offs, total = [], 0
    for s in shapes:
        offs.append(total)
        total += -(-math.prod(s) // _ALIGN) * _ALIGN
    with torch.cuda.device(dev):
        store = torch.empty((max(total, 1),), dtype=torch.float32, device=dev)
        xyz, dc, rest, op, sc, rot = (store[o:o + math.prod(s)].view(s) for o, s in zip(offs, shapes))
        _lib.call("gsr_rows_unpack", _lib.stream(dev), P, int(rows.shape[1]), ptr(rows), ptr(xyz), ptr(dc), ptr(rest), ptr(op), ptr(sc),
                  ptr(rot))                  # K == 1: rest is empty, NULL
    return xyz, dc, (rest if K > 1 else None), op, sc, rot


def unpack_rows(rows: torch.Tensor) -> GaussianParams:
    """The raw parameters of float32 rows [P, 3 K + 14] on a HIP device as a GaussianParams with contiguous tensors and no gradient:
    what `unflatten_gaussians(rows)` holds as strided views, bit for bit, written by one launch into one allocation (each tensor
    on a 64-byte boundary).  The SH degree follows from the row width, as there."""
    K = _check_rows("unpack_rows", rows)
    _lib.require_hip("unpack_rows", "rows", rows)
    xyz, dc, rest, op, sc, rot = _unpack(rows.detach().contiguous(), K)
    g = GaussianParams(int(round(math.sqrt(K))) - 1)
    g._xyz, g._features_dc, g._opacity, g._scaling, g._rotation = xyz, dc, op, sc, rot
    g._features_rest = rest if rest is not None else xyz.new_empty((xyz.shape[0], 0, 3))
    return g


def _forward_all(settings, rows: torch.Tensor, K: int):
    """One unpack, then one fused forward call per camera.  Returns (unpacked buffers, per-camera (num_rendered, radii, geom,
    binning, img), images)."""
    be = get_backend()
    xyz, dc, rest, op, sc, rot = bufs = _unpack(rows, K)
    empty = xyz.new_empty((0,))
    states, images = [], []
    for rs in settings:
        n, color, radii, geom, binning, img = be.forward(rs, xyz, dc, empty, op, sc, rot, empty, shs_rest=rest, raw_params=True)
        states.append((n, radii, geom, binning, img))
        images.append(color)
    if states:
        _remember_forward(states[-1][2], int(xyz.shape[0]))       # an argument-less composited_mask() means the last camera's render, as after render_fused
    return bufs, states, images


def _pack(arenas, P: int, D: int, dev) -> torch.Tensor:
    """dL/drows [P, D] from the cameras' arenas, summed in order: one launch per MAX_B arenas, chunk results added in order."""
    total = None
    stream = _lib.stream(dev)
    for b0 in range(0, len(arenas), MAX_B):
        chunk = arenas[b0:b0 + MAX_B]
        out = torch.empty((P, D), dtype=torch.float32, device=dev)
        _lib.call("gsr_rows_grad_pack", stream, P, D, len(chunk), _lib.ptr_array([_lib.ptr(a) for a in chunk]), _lib.ptr(out))
        total = out if total is None else total + out
    return total


class _RenderRows(torch.autograd.Function):
    """rows [P, D] -> B images (and the radii [B, P]); `rows` is the only differentiable input."""

    @staticmethod
    def forward(ctx, rows, K, settings):
        rc = rows.detach().contiguous()
        (xyz, dc, rest, _op, sc, rot), states, images = _forward_all(settings, rc, K)
        ctx.settings, ctx.K, ctx.D = settings, K, int(rows.shape[1])
        ctx.num_rendered = [s[0] for s in states]
        ctx.save_for_backward(xyz, dc, sc, rot, *([rest] if rest is not None else []), *[t for s in states for t in s[1:]])
        radii = torch.stack([s[1] for s in states])
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)      # an image the loss does not use arrives as None: its backward call does not run
        return (*images, radii)

    @staticmethod
    def backward(ctx, *grads):
        be = get_backend()
        settings, K, D = ctx.settings, ctx.K, ctx.D
        B = len(settings)
        saved = ctx.saved_tensors
        xyz, dc, sc, rot = saved[:4]
        rest = saved[4] if K > 1 else None
        per_cam = saved[4 + (K > 1):]
        P, dev = int(xyz.shape[0]), xyz.device
        live = [b for b in range(B) if grads[b] is not None]
        if not live or P == 0:
            return (torch.zeros((P, D), dtype=torch.float32, device=dev) if live else None), None, None
        empty = xyz.new_empty((0,))
        n = arena_floats(P, K)
        pad = (-3 * P) % 4                    # dL/df_dc sits 3 P floats into an arena: 16-byte aligned with the arena `pad` floats into its slot
        slot = -(-(pad + n) // 4) * 4
        with torch.cuda.device(dev):
            store = torch.empty((len(live), slot), dtype=torch.float32, device=dev)
            arenas = []
            for i, b in enumerate(live):
                radii, geom, binning, img = per_cam[4 * b:4 * b + 4]
                arena = store[i, pad:pad + n]
                with gradient_arena(arena):   # this call's own arena, whatever arena the caller has active (restored on exit)
                    be.backward(settings[b], ctx.num_rendered[b], grads[b], xyz, radii, dc, empty, sc, rot, empty, geom, binning, img,
                                shs_rest=rest, raw_params=True)
                arenas.append(arena)
            return _pack(arenas, P, D, dev), None, None


def render_rows(cameras, rows: torch.Tensor, pipe, bg: torch.Tensor, scaling_modifier: float = 1.0, sh_degree=None, features=None) -> dict:
    """Renders float32 rows [P, 3 K + 14] (K in 1, 4, 9, 16) on a HIP device under every camera of `cameras` (the objects render()
    takes; they may differ in size).  Returns {"renders": list of B images [3, H_b, W_b], "radii": [B, P] int32,
    "visibility_filter": [P] bool, the OR over the cameras of radii > 0}.

    Images and radii are those of `render_fused(cam, unflatten_gaussians(rows), pipe, bg, scaling_modifier)` per camera, bit for bit:
    the same rasterizer calls on the same bits.  `sh_degree`: the active SH degree, None for the one the row width implies.
    With gradients enabled and rows.requires_grad, the images hang on ONE autograd node whose backward runs the rasterizer's backward
    for every camera whose image received a gradient, in camera order, each into an arena of its own, and then sums the arenas in
    that order into dL/drows with one launch (flag columns +0.0): no per-parameter autograd nodes, and an order of summation that
    does not depend on the autograd engine.  Under torch.no_grad() (target and prompt renders) nothing is kept.
    Non-contiguous rows are copied once; the gradient still reaches the caller's tensor.
    No camera gradient: the cameras' tensors are constants here even when they require grad (the raw-parameter path has none,
    include/gsr_pose.h).
    `rasterizer.composited_mask()` without an argument refers to the LAST camera's render afterwards (while the images' graph is
    alive: a no_grad call keeps no workspace); composited_mask(image) does not know the images of this function and returns None.
    `features`: refused -- the raw-parameter path has no feature maps (include/gsr_features.h); render() takes the keyword."""
    who = "render_rows"
    if features is not None:
        raise _lib.GsrError(f"{who}: no feature maps on the raw-parameter path (include/gsr_features.h has no raw_params form): use render(features=...)")
    K = _check_rows(who, rows)
    cameras = list(cameras)
    if len(cameras) < 1:
        raise _lib.GsrError(f"{who}: cameras must hold at least one camera")
    deg = int(round(math.sqrt(K))) - 1
    if sh_degree is None:
        sh_degree = deg
    if not isinstance(sh_degree, int) or not 0 <= sh_degree <= deg:
        raise _lib.GsrError(f"{who}: sh_degree={sh_degree!r} not in 0..{deg}, the degree D={int(rows.shape[1])} columns hold")
    _lib.require_hip(who, "rows", rows)
    settings = tuple(camera_settings(cam, bg, scaling_modifier, sh_degree, pipe.debug) for cam in cameras)
    if torch.is_grad_enabled() and rows.requires_grad:
        *images, radii = _RenderRows.apply(rows, K, settings)
    else:
        _, states, images = _forward_all(settings, rows.detach().contiguous(), K)
        radii = torch.stack([s[1] for s in states])
    return {"renders": list(images), "radii": radii, "visibility_filter": (radii > 0).any(dim=0)}
