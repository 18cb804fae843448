"""Adam over the Gaussian parameter groups through ONE HIP launch (include/gsr_optim.h, csrc/adam.hip).

A torch.optim.Optimizer with the state layout of torch.optim.Adam ("step", "exp_avg", "exp_avg_sq" per tensor), so the
optimiser-state surgery of densify.py -- and anything else written against the reference's optimiser
(scene/gaussian_model.py:155-164: six one-tensor groups, eps 1e-15) -- works on it unchanged.  No weight decay, no
amsgrad, like the reference's.  There is no CPU fallback: parameters must be float32 tensors on a HIP device.

HipSparseAdam is the opt-in variant whose step takes the iteration's visibility mask and skips the Gaussians no view saw.
"""
from __future__ import annotations

import torch

from . import _lib


class HipAdam(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))

    @torch.no_grad()
    def step(self, closure=None):
        return self._step(closure, None)

    def _step(self, closure, visibility):
        """One step of every tensor that has a gradient; visibility None: gsr_adam_step, else gsr_adam_step_masked with that mask
        (checked by HipSparseAdam.step).  Every tensor is checked before any state changes and before anything is launched."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        name, ptr = type(self).__name__, _lib.ptr
        by_hyper = {}
        keep = []                                   # tensors that must outlive the launch call
        for g in self.param_groups:
            for p in g["params"]:
                if p.grad is None:
                    continue
                if p.dtype != torch.float32 or p.device.type != "cuda" or not p.is_contiguous():
                    raise _lib.GsrError(f"{name} needs contiguous float32 parameters on a HIP device (no CPU fallback)")
                if visibility is not None and (p.device != visibility.device or p.dim() == 0 or p.shape[0] != visibility.shape[0]):
                    who = g.get("name")
                    raise _lib.GsrError(f"{name}: parameter {who + ' ' if who else ''}of shape {tuple(p.shape)} on {p.device} does not have the "
                                        f"{visibility.shape[0]} rows of visibility on {visibility.device}")
        for g in self.param_groups:
            for p in g["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p)
                    st["exp_avg_sq"] = torch.zeros_like(p)
                st["step"] = int(st["step"]) + 1
                grad = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                keep.append(grad)
                key = (p.device, tuple(g["betas"]), float(g["eps"]))
                by_hyper.setdefault(key, []).append(
                    _lib.AdamGroup(ptr(p), ptr(grad), ptr(st["exp_avg"]), ptr(st["exp_avg_sq"]), p.numel(), float(g["lr"]), st["step"]))
        if visibility is not None:
            kind = _lib.ADAM_MASK_RADII if visibility.dtype == torch.int32 else _lib.ADAM_MASK_BYTES
            P, mask = int(visibility.shape[0]), ptr(visibility)
        for (dev, betas, eps), groups in by_hyper.items():
            with torch.cuda.device(dev):
                stream = _lib.stream(dev)
                for i in range(0, len(groups), _lib.ADAM_MAX_GROUPS):
                    chunk = groups[i:i + _lib.ADAM_MAX_GROUPS]
                    arr = (_lib.AdamGroup * len(chunk))(*chunk)
                    if visibility is None:
                        _lib.call("gsr_adam_step", stream, len(chunk), arr, betas[0], betas[1], eps)
                    else:
                        _lib.call("gsr_adam_step_masked", stream, len(chunk), arr, betas[0], betas[1], eps, P, mask, kind)
        return loss


class HipSparseAdam(HipAdam):
    """HipAdam whose step takes the per-Gaussian visibility of the iteration and leaves alone every row no view saw
    (gsr_adam_step_masked, include/gsr_optim.h): `optimizer.step(visibility=radii)`.  A visible row gets HipAdam's update bit for
    bit; an invisible one keeps parameter and moments bit for bit -- it neither decays its moments nor coasts on its momentum, which
    is where this differs from dense Adam on a zero gradient.  `step` stays one count per tensor and advances on every call.
    Same state layout as HipAdam, so densify.py works on it unchanged."""

    @torch.no_grad()
    def step(self, closure=None, *, visibility=None):
        """visibility: None (exactly HipAdam.step) or a contiguous 1-D tensor of P entries on the parameters' device: torch.bool /
        torch.uint8 (visible iff != 0) or torch.int32 (the rasterizer's radii, visible iff > 0).  Every tensor that has a gradient
        must have P rows; tensors without one are skipped first, so the step right after a densification does nothing."""
        if visibility is not None:
            if not isinstance(visibility, torch.Tensor) or visibility.dtype not in (torch.bool, torch.uint8, torch.int32):
                raise _lib.GsrError("HipSparseAdam: visibility must be a torch.bool, torch.uint8 or torch.int32 tensor, got "
                                    f"{getattr(visibility, 'dtype', type(visibility).__name__)}")
            if visibility.dim() != 1 or not visibility.is_contiguous():
                raise _lib.GsrError(f"HipSparseAdam: visibility must be 1-D and contiguous, got shape {tuple(visibility.shape)}")
            if visibility.device.type != "cuda":
                raise _lib.GsrError("HipSparseAdam: visibility must be on a HIP device (no CPU fallback)")
        return self._step(closure, visibility)
