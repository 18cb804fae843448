"""`chamfer_distance.ChamferDistance` on HIP (include/gsr_chamfer.h, csrc/chamfer.hip).

The reference's newest training script imports `from chamfer_distance import ChamferDistance`
(train_stacked_transformer.py:24), builds one module (:184) and calls it every optimisation step (:193-196):

    dist1, dist2, idx1, idx2 = self.chd(pred.unsqueeze(0), tgt.unsqueeze(0))
    chamfer = dist1.mean() + dist2.mean()

on rows of 26 floats, then back-propagates (:245).  Squared Euclidean distance over ALL features of the last dimension
(1..64), nearest row of the other set and its index, both ways; the lowest index wins a tie.  No CPU fallback."""
from __future__ import annotations

import torch

from . import _lib

MAX_D = 64


def _validate(xyz1, xyz2) -> None:
    """Everything that can be said without the native library; raises _lib.GsrError naming the argument."""
    for name, t in (("xyz1", xyz1), ("xyz2", xyz2)):
        if not isinstance(t, torch.Tensor):
            raise _lib.GsrError(f"ChamferDistance: {name} must be a torch.Tensor, got {type(t).__name__}")
        _lib.require_hip("ChamferDistance", name, t)
        if t.dim() != 3:
            raise _lib.GsrError(f"ChamferDistance: {name} must have shape [B, N, D], got {tuple(t.shape)}")
        if not t.is_floating_point():
            raise _lib.GsrError(f"ChamferDistance: {name} must be a floating-point tensor, got {t.dtype}")
    if xyz2.device != xyz1.device:
        raise _lib.GsrError(f"ChamferDistance: xyz2 is on {xyz2.device} but xyz1 on {xyz1.device}")
    _validate_shapes(tuple(xyz1.shape), tuple(xyz2.shape))


def _validate_shapes(s1, s2) -> None:
    if s2[0] != s1[0]:
        raise _lib.GsrError(f"ChamferDistance: xyz2 has batch size B={s2[0]} but xyz1 has B={s1[0]}")
    if s2[2] != s1[2]:
        raise _lib.GsrError(f"ChamferDistance: xyz2 has D={s2[2]} features per row but xyz1 has D={s1[2]}")
    if not 1 <= s1[2] <= MAX_D:
        raise _lib.GsrError(f"ChamferDistance: xyz1 has D={s1[2]} features per row, supported: 1..{MAX_D}")


class ChamferDistanceFunction(torch.autograd.Function):
    """float32 tensors on one HIP device in, (dist1 [B,N], dist2 [B,M], idx1 [B,N] int32, idx2 [B,M] int32) out."""

    @staticmethod
    def forward(ctx, xyz1, xyz2):
        _validate(xyz1, xyz2)
        if xyz1.dtype != torch.float32 or xyz2.dtype != torch.float32:
            raise _lib.GsrError("ChamferDistanceFunction: xyz1 and xyz2 must be float32 (ChamferDistance casts for you)")
        ptr = _lib.ptr
        x1, x2 = xyz1.detach().contiguous(), xyz2.detach().contiguous()
        (B, N, D), M = x1.shape, int(x2.shape[1])
        dev = x1.device
        dist1 = torch.empty((B, N), dtype=torch.float32, device=dev)
        dist2 = torch.empty((B, M), dtype=torch.float32, device=dev)
        idx1 = torch.empty((B, N), dtype=torch.int32, device=dev)
        idx2 = torch.empty((B, M), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            ws = _lib.workspace("gsr_chamfer_workspace", dev, B, N, M)
            _lib.call("gsr_chamfer_forward", _lib.stream(dev), B, N, M, D, ptr(x1), ptr(x2), ptr(dist1), ptr(dist2), ptr(idx1), ptr(idx2),
                      ptr(ws), ws.numel())
        ctx.save_for_backward(x1, x2, idx1, idx2)
        ctx.mark_non_differentiable(idx1, idx2)
        ctx.set_materialize_grads(False)          # an unused dist arrives as None and goes down as NULL (= zeros)
        return dist1, dist2, idx1, idx2

    @staticmethod
    def backward(ctx, g1, g2, _gi1, _gi2):
        x1, x2, idx1, idx2 = ctx.saved_tensors
        (B, N, D), M = x1.shape, int(x2.shape[1])
        dev, ptr = x1.device, _lib.ptr
        g1 = None if g1 is None else g1.to(torch.float32).contiguous()
        g2 = None if g2 is None else g2.to(torch.float32).contiguous()
        dx1 = torch.empty_like(x1) if ctx.needs_input_grad[0] else None      # fully written by the call
        dx2 = torch.empty_like(x2) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(dev):
            _lib.call("gsr_chamfer_backward", _lib.stream(dev), B, N, M, D, ptr(x1), ptr(x2), ptr(idx1), ptr(idx2), ptr(g1), ptr(g2),
                      ptr(dx1), ptr(dx2))
        return dx1, dx2


class ChamferDistance(torch.nn.Module):
    """Drop-in for the reference's `ChamferDistance()`: forward(xyz1 [B,N,D], xyz2 [B,M,D]) -> (dist1, dist2, idx1, idx2).

    Inputs may be non-contiguous, non-leaf and float16 / bfloat16 / float64: they are cast to float32 here, outside the autograd
    function, so that autograd casts the gradient back; dist1 / dist2 are float32."""

    def forward(self, xyz1, xyz2):
        _validate(xyz1, xyz2)
        return ChamferDistanceFunction.apply(xyz1.to(torch.float32), xyz2.to(torch.float32))
