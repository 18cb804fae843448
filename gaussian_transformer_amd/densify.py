"""Adaptive density control and the optimiser state that follows it.

Restates the behaviour of the reference's scene/gaussian_model.py: training_setup :149-167 (six Adam groups, eps 1e-15),
update_learning_rate :169-175 with utils/general_utils.py:29-61 (log-linear decay of the position rate),
reset_opacity :210-213, the optimiser-state surgery :258-322, densify_and_split :349-371, densify_and_clone :373-387,
densify_and_prune :389-403 -- and of train.py:113-123, which drives it.  Everything is torch index arithmetic on the
device that holds the Gaussians; no kernel of its own is needed.  FusedDensityController, at the end, is the same
controller with the statistics and the clone / split / prune on the HIP path (include/gsr_density.h): opt-in, and held to
DensityController, which stays the oracle.

One deliberate extension: `densify_and_split` draws its samples from a caller-supplied torch.Generator, so
data-parallel ranks that seed it identically split identically (the reference uses the global RNG).

MCMCController / FusedMCMCController, after them, are a second strategy that is not in the reference (Kheradmand et al. 2024,
include/gsr_mcmc.h): a fixed budget, relocation of dead Gaussians, growth to a count the host knows in advance, position noise
and two regularisers -- in torch index arithmetic (the oracle) and on the HIP path.  Opt-in as well.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Dict, Optional

import numpy as np
import torch

from . import _lib
from .model import GaussianParams, absgrad_rows, inverse_sigmoid

GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")          # order of training_setup :155-162
_ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
         "rotation": "_rotation"}


@dataclass
class OptimizationParams:          # arguments/__init__.py:71-90 (this fork's defaults)
    iterations: int = 30_000
    position_lr_init: float = 0.00016
    position_lr_final: float = 0.0000016
    position_lr_delay_mult: float = 0.01
    position_lr_max_steps: int = 30_000
    feature_lr: float = 0.0025
    opacity_lr: float = 0.05
    scaling_lr: float = 0.005
    rotation_lr: float = 0.001
    percent_dense: float = 0.01
    lambda_dssim: float = 0.2
    densification_interval: int = 500
    opacity_reset_interval: int = 3000
    densify_from_iter: int = 100
    densify_until_iter: int = 10_000
    densify_grad_threshold: float = 0.0002
    random_background: bool = False


def expon_lr(lr_init: float, lr_final: float, lr_delay_steps: int = 0, lr_delay_mult: float = 1.0,
             max_steps: int = 1_000_000) -> Callable[[int], float]:
    """Log-linear interpolation lr_init -> lr_final over max_steps, optionally eased in (utils/general_utils.py:29-61)."""
    def at(step: int) -> float:
        if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
            return 0.0
        delay = 1.0
        if lr_delay_steps > 0:
            delay = lr_delay_mult + (1.0 - lr_delay_mult) * math.sin(0.5 * math.pi * min(max(step / lr_delay_steps, 0.0), 1.0))
        t = min(max(step / max_steps, 0.0), 1.0)
        return delay * math.exp(math.log(lr_init) * (1.0 - t) + math.log(lr_final) * t)
    return at


def quaternion_to_rotation(q: torch.Tensor) -> torch.Tensor:
    """[P,4] (r,x,y,z), any norm -> [P,3,3] (utils/general_utils.py:78-99)."""
    q = q / torch.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])[:, None]
    r, x, y, z = q.unbind(dim=1)
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
            2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
            2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, dim=1).view(-1, 3, 3)


class DensityController:
    """Owns the Adam optimiser of a GaussianParams and keeps it consistent while Gaussians are cloned, split and pruned."""

    def __init__(self, model: GaussianParams, opt: Optional[OptimizationParams] = None, spatial_lr_scale: float = 1.0,
                 fused_adam: bool = False, adam: str = "torch"):
        """adam: "torch" (torch.optim.Adam; fused_adam=True for its fused kernels), "hip" (optim.HipAdam, one launch) or
        "hip_sparse" (optim.HipSparseAdam: `optimizer.step(visibility=radii)` skips the Gaussians the view did not see)."""
        if adam not in ("torch", "hip", "hip_sparse"):
            raise ValueError(f"adam must be 'torch', 'hip' or 'hip_sparse', got {adam!r}")
        self.model = model
        self.opt = opt or OptimizationParams()
        self.spatial_lr_scale = spatial_lr_scale
        o = self.opt
        self._zero_statistics(model._xyz.shape[0], model._xyz.device)
        lrs = {"xyz": o.position_lr_init * spatial_lr_scale, "f_dc": o.feature_lr, "f_rest": o.feature_lr / 20.0,
               "opacity": o.opacity_lr, "scaling": o.scaling_lr, "rotation": o.rotation_lr}
        for n in GROUPS:           # the optimiser must own leaf tensors it can replace
            setattr(model, _ATTR[n], torch.nn.Parameter(getattr(model, _ATTR[n]).detach().clone().requires_grad_(True)))
        groups = [{"params": [getattr(model, _ATTR[n])], "lr": lrs[n], "name": n} for n in GROUPS]
        if adam == "hip":
            from .optim import HipAdam
            self.optimizer = HipAdam(groups, lr=0.0, eps=1e-15)
        elif adam == "hip_sparse":
            from .optim import HipSparseAdam
            self.optimizer = HipSparseAdam(groups, lr=0.0, eps=1e-15)
        else:
            self.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15, **({"fused": True} if fused_adam else {}))
        self._xyz_lr = expon_lr(o.position_lr_init * spatial_lr_scale, o.position_lr_final * spatial_lr_scale,
                                lr_delay_mult=o.position_lr_delay_mult, max_steps=o.position_lr_max_steps)

    # ---- learning rate ----
    def update_learning_rate(self, iteration: int) -> float:
        lr = self._xyz_lr(iteration)
        for g in self.optimizer.param_groups:
            if g["name"] == "xyz":
                g["lr"] = lr
        return lr

    # ---- optimiser-state surgery: every change of the Gaussian set is one row map applied to parameter and moments ----
    def _install(self, new: Dict[str, torch.Tensor], states: Dict[str, Optional[tuple]]) -> None:
        """The one place a group gets a new tensor: the optimiser state of every group in `new` moves from the old parameter to the new
        Parameter -- with the moments states[name] = (exp_avg, exp_avg_sq), or its own where that is None -- which group and model take."""
        for g in self.optimizer.param_groups:
            name = g["name"]
            if name not in new:
                continue
            state = self.optimizer.state.pop(g["params"][0], None)
            p = torch.nn.Parameter(new[name].requires_grad_(True))
            if state is not None:
                if states[name] is not None:
                    state["exp_avg"], state["exp_avg_sq"] = states[name]
                self.optimizer.state[p] = state
            g["params"][0] = p
            setattr(self.model, _ATTR[name], p)

    def _remap(self, param_fn: Callable[[str, torch.Tensor], torch.Tensor],
               moment_fn: Callable[[str, torch.Tensor], torch.Tensor], only: Optional[str] = None) -> None:
        for g in self.optimizer.param_groups:                       # group by group: one group's old and new tensors live at a time
            name, old = g["name"], g["params"][0]
            if only is not None and name != only:
                continue
            state = self.optimizer.state.get(old, None)
            new = param_fn(name, old.detach())
            moments = (moment_fn(name, state["exp_avg"]), moment_fn(name, state["exp_avg_sq"])) if state is not None else None
            self._install({name: new}, {name: moments})

    def _zero_statistics(self, P: int, dev) -> None:
        m = self.model
        m.xyz_gradient_accum = torch.zeros((P, 1), device=dev)
        m.denom = torch.zeros((P, 1), device=dev)
        m.max_radii2D = torch.zeros((P,), device=dev)

    def prune_points(self, mask: torch.Tensor) -> None:
        """Removes the Gaussians where `mask` is True (:287-301)."""
        keep = ~mask
        self._remap(lambda n, p: p[keep], lambda n, m: m[keep])
        m = self.model
        m.xyz_gradient_accum = m.xyz_gradient_accum[keep]
        m.denom = m.denom[keep]
        m.max_radii2D = m.max_radii2D[keep]

    # ---- pruning by measured contribution (rasterizer.ContributionStats: blend weights collected over many views) ----
    def _contribution(self, stats):
        w_sum, w_max, n_pix = stats.read()
        P = self.model._xyz.shape[0]
        if w_sum.shape[0] != P:
            raise ValueError(f"the contribution statistics hold {w_sum.shape[0]} Gaussians, the model {P}")
        dev = self.model._xyz.device
        return w_sum.to(dev), w_max.to(dev), n_pix.to(dev)

    def prune_by_max_weight(self, stats, threshold: float = 0.01) -> int:
        """Removes the Gaussians whose largest blend weight alpha T over every collected view is below `threshold` (RadSplat's "max
        ray contribution"), those never blended in any of the views among them.  Returns how many were removed."""
        _, w_max, n_pix = self._contribution(stats)
        mask = (w_max < threshold) | (n_pix == 0)
        self.prune_points(mask)
        return int(mask.sum())

    def prune_by_weight_sum(self, stats, fraction: float, volume_power: float = 0.0) -> int:
        """Removes the round(fraction P) Gaussians with the lowest score weight_sum * (product of the activated scales)^volume_power
        (LightGaussian's global significance; volume_power = 0: the summed blend weight alone).  Equal scores go by index, the
        lower index first.  Returns how many were removed."""
        if not 0.0 <= fraction <= 1.0:
            raise ValueError(f"fraction must lie in [0, 1], got {fraction}")
        w_sum, _, _ = self._contribution(stats)
        score = w_sum.to(torch.float64)
        if volume_power != 0.0:
            score = score * self.model.get_scaling.detach().to(torch.float64).prod(dim=1).pow(volume_power)
        P = score.shape[0]
        k = int(round(fraction * P))
        mask = torch.zeros((P,), dtype=torch.bool, device=score.device)
        mask[torch.sort(score, stable=True).indices[:k]] = True
        self.prune_points(mask)
        return k

    def append_points(self, new: Dict[str, torch.Tensor]) -> None:
        """Appends Gaussians with zero Adam moments and resets the densification statistics (:303-347)."""
        self._remap(lambda n, p: torch.cat((p, new[n]), dim=0), lambda n, m: torch.cat((m, torch.zeros_like(new[n])), dim=0))
        self._zero_statistics(self.model._xyz.shape[0], self.model._xyz.device)

    def replace_tensor(self, name: str, tensor: torch.Tensor) -> None:
        """New values for one group, its Adam moments zeroed (:258-271)."""
        self._remap(lambda n, p: tensor, lambda n, m: torch.zeros_like(tensor), only=name)

    # ---- statistics (train.py:113-116) ----
    def record(self, viewspace_points: torch.Tensor, visibility: torch.Tensor, radii: torch.Tensor, absgrad=None) -> None:
        """absgrad: a rasterizer.AbsGrad or a [P,2] tensor; its rows take the place of viewspace_points.grad[:, :2] in the norm
        (visibility, denom and max_radii2D as before).  AbsGS and gsplat raise densify_grad_threshold with it (0.0002 -> about
        0.0008); the default stays."""
        m = self.model
        m.max_radii2D[visibility] = torch.max(m.max_radii2D[visibility], radii[visibility].to(m.max_radii2D.dtype))
        m.add_densification_stats(viewspace_points, visibility, absgrad=absgrad)

    # ---- densification ----
    def _selected(self, grads: torch.Tensor, threshold: float, extent: float, large: bool) -> torch.Tensor:
        size = self.model.get_scaling.max(dim=1).values
        cut = self.opt.percent_dense * extent
        return (grads >= threshold) & ((size > cut) if large else (size <= cut))

    def densify_and_clone(self, grads: torch.Tensor, threshold: float, extent: float) -> int:
        """Small Gaussians with a large view-space gradient are duplicated in place (:373-387)."""
        m = self.model
        sel = self._selected(grads.norm(dim=-1), threshold, extent, large=False)
        self.append_points({n: getattr(m, _ATTR[n]).detach()[sel] for n in GROUPS})
        return int(sel.sum())

    def densify_and_split(self, grads: torch.Tensor, threshold: float, extent: float, N: int = 2,
                          generator: Optional[torch.Generator] = None, normal_fn: Optional[Callable] = None) -> int:
        """Large Gaussians with a large gradient are replaced by N samples of themselves, 1.6x smaller (:349-371).
        normal_fn(stds) -> samples ~ N(0, stds^2) replaces torch.normal when given (e.g. drawn on the host, so that the
        result does not depend on which device's generator the model sits on)."""
        m = self.model
        P = m._xyz.shape[0]
        padded = torch.zeros((P,), device=m._xyz.device)
        padded[:grads.shape[0]] = grads.squeeze()                    # clones appended just before have no statistics yet
        sel = self._selected(padded, threshold, extent, large=True)
        scale = m.get_scaling.detach()[sel]
        stds = scale.repeat(N, 1)
        samples = normal_fn(stds) if normal_fn is not None else torch.normal(mean=torch.zeros_like(stds), std=stds, generator=generator)
        R = quaternion_to_rotation(m._rotation.detach()[sel]).repeat(N, 1, 1)
        new = {
            "xyz": torch.bmm(R, samples.unsqueeze(-1)).squeeze(-1) + m._xyz.detach()[sel].repeat(N, 1),
            "scaling": torch.log(scale.repeat(N, 1) / (0.8 * N)),
            "rotation": m._rotation.detach()[sel].repeat(N, 1),
            "f_dc": m._features_dc.detach()[sel].repeat(N, 1, 1),
            "f_rest": m._features_rest.detach()[sel].repeat(N, 1, 1),
            "opacity": m._opacity.detach()[sel].repeat(N, 1),
        }
        n_sel = int(sel.sum())
        self.append_points(new)
        self.prune_points(torch.cat((sel, torch.zeros(N * n_sel, dtype=torch.bool, device=sel.device))))
        return n_sel

    def densify_and_prune(self, max_grad: float, min_opacity: float, extent: float, max_screen_size: Optional[float],
                          generator: Optional[torch.Generator] = None, normal_fn: Optional[Callable] = None) -> Dict[str, int]:
        """:389-403.  Returns how many Gaussians were cloned / split / pruned."""
        m = self.model
        grads = m.xyz_gradient_accum / m.denom
        grads[grads.isnan()] = 0.0
        cloned = self.densify_and_clone(grads, max_grad, extent)
        split = self.densify_and_split(grads, max_grad, extent, generator=generator, normal_fn=normal_fn)
        prune = (m.get_opacity.detach() < min_opacity).squeeze(-1)
        if max_screen_size:
            prune = prune | (m.max_radii2D > max_screen_size) | (m.get_scaling.detach().max(dim=1).values > 0.1 * extent)
        self.prune_points(prune)
        return {"cloned": cloned, "split": split, "pruned": int(prune.sum())}

    def reset_opacity(self) -> None:
        """Opacity clamped to at most 0.01, its Adam moments zeroed (:210-213)."""
        o = self.model.get_opacity.detach()
        self.replace_tensor("opacity", inverse_sigmoid(torch.min(o, torch.full_like(o, 0.01))))

    # ---- the schedule of train.py:69-73, 113-123 ----
    def after_backward(self, iteration: int, viewspace_points: torch.Tensor, visibility: torch.Tensor, radii: torch.Tensor,
                       extent: float, white_background: bool = False, generator: Optional[torch.Generator] = None, absgrad=None):
        """Call after loss.backward() and before optimizer.step(), with torch.no_grad().  absgrad: as record()."""
        o = self.opt
        out = None
        if iteration < o.densify_until_iter:
            self.record(viewspace_points, visibility, radii, absgrad=absgrad)
            if iteration > o.densify_from_iter and iteration % o.densification_interval == 0:
                size_threshold = 20 if iteration > o.opacity_reset_interval else None
                out = self.densify_and_prune(o.densify_grad_threshold, 0.005, extent, size_threshold, generator=generator)
            if iteration % o.opacity_reset_interval == 0 or (white_background and iteration == o.densify_from_iter):
                self.reset_opacity()
        return out


class _FusedGroups:
    """What the two controllers on the HIP path share: the check of a tensor that crosses the boundary, the groups' current tensors,
    a workspace kept across calls, the tensors of a new state and the group table of an apply entry point (csrc/group_table.h)."""

    def _device_f32(self, name: str, t) -> torch.Tensor:
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise _lib.GsrError(f"{type(self).__name__}: {name} must be on a HIP device (no CPU fallback)")
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.GsrError(f"{type(self).__name__}: {name} must be contiguous float32, got {t.dtype}")
        return t

    def _olds(self) -> Dict[str, torch.Tensor]:
        olds = {g["name"]: g["params"][0].detach() for g in self.optimizer.param_groups}
        for n in GROUPS:
            self._device_f32(n, olds[n])
        return olds

    def _workspace(self, key: str, dev, sizer: str, *sizes) -> torch.Tensor:
        """As many bytes as `sizer` asks for, kept across calls under `key` (not _lib.workspace()) and regrown when too small or on
        another device.  Call it inside torch.cuda.device(dev)."""
        need = _lib.workspace_bytes(sizer, *sizes)
        ws = self._kept.get(key)
        if ws is None or ws.numel() < need or ws.device != dev:
            ws = self._kept[key] = torch.empty(need, dtype=torch.uint8, device=dev)
        return ws

    def _moments(self, g):
        """(exp_avg, exp_avg_sq) of a group, each checked, or None where the optimiser holds none yet"""
        state = self.optimizer.state.get(g["params"][0], None)
        if state is None or "exp_avg" not in state:
            return None
        return self._device_f32(g["name"] + " exp_avg", state["exp_avg"]), self._device_f32(g["name"] + " exp_avg_sq", state["exp_avg_sq"])

    def _allocate(self, P_new: int, dev):
        """({group: [P_new, ...] tensor}, {group: two such tensors for the moments, or None where the group has none})"""
        new, states = {}, {}
        for g in self.optimizer.param_groups:
            shape = (P_new,) + tuple(g["params"][0].shape[1:])
            new[g["name"]] = torch.empty(shape, device=dev)
            states[g["name"]] = (torch.empty(shape, device=dev), torch.empty(shape, device=dev)) if self._moments(g) else None
        return new, states

    def _group_table(self, struct, roles, olds, new=None, states=None):
        """(ctypes array of `struct`, its length) over the groups of positive width: in place (new None: dst == src) or into the
        tensors of new / states."""
        ptr, descs = _lib.ptr, []
        for g in self.optimizer.param_groups:
            n, old = g["name"], olds[g["name"]]
            sm = self._moments(g) or (None, None)
            width = old[0].numel() if old.shape[0] else 0
            if width:
                dst, dm = (old, sm) if new is None else (new[n], states[n] or (None, None))
                descs.append(struct(ptr(old), ptr(sm[0]), ptr(sm[1]), ptr(dst), ptr(dm[0]), ptr(dm[1]), width, roles[n]))
        return (struct * len(descs))(*descs), len(descs)


_ROLE = {**dict.fromkeys(GROUPS, _lib.DENSITY_COPY), "xyz": _lib.DENSITY_XYZ, "scaling": _lib.DENSITY_SCALING}


class FusedDensityController(_FusedGroups, DensityController):
    """DensityController with `record` and `densify_and_prune` on the device (include/gsr_density.h, csrc/density.hip):
    record is one launch without a host wait; densify_and_prune decides every Gaussian once, waits once for the four counts,
    and writes the new parameters and Adam moments in one launch instead of rebuilding them four times.  Same constructor,
    same public methods, same results: copied rows bit for bit, the split children to float32 rounding of the same formula
    on the same samples.  No CPU fallback."""

    SPLIT_N = 2                        # densify_and_split's N (:349)

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._counts = None            # pinned host words {n_clone, n_split, n_pruned, P_new}
        self._kept = {}                # _workspace()

    def record(self, viewspace_points: torch.Tensor, visibility: Optional[torch.Tensor], radii: torch.Tensor, absgrad=None) -> None:
        """train.py:113-116 in one launch.  viewspace_points.grad is taken as it comes: [P, >= 2] float32 with unit column
        stride and any row stride (a view into a gradient arena).  visibility None: radii > 0.  absgrad: a rasterizer.AbsGrad or a
        [P,2] tensor whose rows take the place of viewspace_points.grad (which is then not looked at), as DensityController.record."""
        m = self.model
        grad = viewspace_points.grad if absgrad is None else absgrad_rows(absgrad, m._xyz.shape[0])
        if grad is None:
            raise _lib.GsrError("FusedDensityController.record: viewspace_points has no gradient")
        if grad.device.type != "cuda":
            raise _lib.GsrError("FusedDensityController.record: the gradient must be on a HIP device (no CPU fallback)")
        P = m._xyz.shape[0]
        if grad.dtype != torch.float32 or grad.dim() != 2 or grad.shape[0] != P or grad.shape[1] < 2 or (P > 1 and grad.stride(0) < 2) or \
                grad.stride(1) != 1:
            grad = grad[:, :2].to(torch.float32).contiguous()
        accum, denom, mx = (self._device_f32(n, t) for n, t in (("xyz_gradient_accum", m.xyz_gradient_accum), ("denom", m.denom),
                                                                ("max_radii2D", m.max_radii2D)))
        radii = radii if radii.dtype == torch.int32 and radii.is_contiguous() else radii.to(torch.int32).contiguous()
        if visibility is not None:
            visibility = visibility if visibility.dtype in (torch.bool, torch.uint8) and visibility.is_contiguous() else (visibility != 0).contiguous()
            if visibility.shape[0] != P:
                raise _lib.GsrError(f"FusedDensityController.record: visibility has {visibility.shape[0]} rows, the model {P}")
        if radii.shape[0] != P or radii.device != grad.device or (visibility is not None and visibility.device != grad.device):
            raise _lib.GsrError("FusedDensityController.record: radii / visibility must have P rows on the gradient's device")
        if P == 0:
            return
        ptr = _lib.ptr
        with torch.cuda.device(grad.device):
            # grad.data_ptr(), not ptr(grad): the one strided tensor that crosses the boundary, handed over with its row stride
            _lib.call("gsr_density_record", _lib.stream(grad.device), P, grad.data_ptr(), max(int(grad.stride(0)), 2), ptr(radii),
                      ptr(visibility), ptr(accum), ptr(denom), ptr(mx))

    def densify_and_prune(self, max_grad: float, min_opacity: float, extent: float, max_screen_size: Optional[float],
                          generator: Optional[torch.Generator] = None, normal_fn: Optional[Callable] = None) -> Dict[str, int]:
        """:389-403 as plan -> one wait for the counts -> samples -> allocate -> apply -> install."""
        m = self.model
        N = self.SPLIT_N
        olds = self._olds()
        accum, denom = self._device_f32("xyz_gradient_accum", m.xyz_gradient_accum), self._device_f32("denom", m.denom)
        dev = olds["xyz"].device
        P = olds["xyz"].shape[0]
        if P == 0:
            self._zero_statistics(0, dev)
            return {"cloned": 0, "split": 0, "pruned": 0}
        f32 = lambda v: float(np.float32(v))       # torch compares a float32 tensor with float32(number)
        ptr = _lib.ptr
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)        # the object, not only _lib.stream(dev): it is waited for below
            ws = self._workspace("plan", dev, "gsr_densify_plan_workspace", P, N)
            if self._counts is None:
                self._counts = torch.zeros(4, dtype=torch.int32).pin_memory()
            # 1. plan
            _lib.call("gsr_densify_plan", _lib.stream(dev), P, ptr(olds["opacity"]), ptr(olds["scaling"]), ptr(accum), ptr(denom),
                      f32(max_grad), f32(min_opacity), f32(self.opt.percent_dense * extent),
                      f32(0.1 * extent) if max_screen_size else -1.0, N, ptr(self._counts), ptr(ws), ws.numel())
            # 2. the only host wait of the call
            stream.synchronize()
            n_clone, n_split, n_pruned, P_new = (int(v) for v in self._counts.tolist())
            # 3. the samples of the split, drawn as densify_and_split draws them (torch.normal(0, stds) is randn * stds)
            ones = torch.ones((N * n_split, 3), device=dev)
            noise = normal_fn(ones) if normal_fn is not None else torch.normal(mean=torch.zeros_like(ones), std=ones, generator=generator)
            noise = noise.to(device=dev, dtype=torch.float32).contiguous()
            # 4. the new tensors
            new, states = self._allocate(P_new, dev)
            arr, k = self._group_table(_lib.DensityGroup, _ROLE, olds, new, states)
            # 5. apply
            if P_new:
                _lib.call("gsr_densify_apply", _lib.stream(dev), P, N, n_split, P_new, k, arr, ptr(olds["scaling"]),
                          ptr(olds["rotation"]), ptr(noise), ptr(ws), ws.numel())
        # 6. install, 7. statistics of the new set
        self._install(new, states)
        self._zero_statistics(P_new, dev)
        return {"cloned": n_clone, "split": n_split, "pruned": n_pruned}


# ---- MCMC density control (include/gsr_mcmc.h): a fixed budget, relocation, growth, noise, two regularisers ----

@dataclass
class MCMCParams:
    """Kheradmand et al. 2024, "3D Gaussian Splatting as Markov Chain Monte Carlo"; cap_max is the budget of Gaussians."""
    cap_max: int
    min_opacity: float = 0.005
    noise_lr: float = 5e5
    refine_start: int = 500
    refine_stop: int = 25_000
    refine_every: int = 100
    grow_factor_percent: int = 105
    opacity_reg: float = 0.01
    scale_reg: float = 0.01
    n_max: int = 51
    gate_k: float = 100.0
    gate_t: float = 0.005


def _binomial_table(n_max: int) -> torch.Tensor:
    """[n_max + 1, n_max] float64: row N, column k holds C(N, k + 1) (0 beyond N); exact in double up to C(51, .)."""
    return torch.tensor([[float(math.comb(N, k + 1)) for k in range(n_max)] for N in range(n_max + 1)], dtype=torch.float64)


class MCMCController(DensityController):
    """The rule of include/gsr_mcmc.h in torch index arithmetic, on the CPU or the device that holds the Gaussians: int64 cumsum,
    searchsorted, bincount, the correction in float64.  The oracle of FusedMCMCController.  It keeps none of the gradient
    statistics: P changes only in grow(), to a number the host computes from P alone.

    Deviation from the published code, on purpose: every row whose parameters were replaced -- sources, relocated rows, appended
    rows -- starts with zero Adam moments (the published code leaves a relocated row the dead Gaussian's moments)."""

    def __init__(self, model: GaussianParams, mcmc: MCMCParams, opt: Optional[OptimizationParams] = None, spatial_lr_scale: float = 1.0,
                 fused_adam: bool = False, adam: str = "torch"):
        super().__init__(model, opt, spatial_lr_scale=spatial_lr_scale, fused_adam=fused_adam, adam=adam)
        if not 1 <= mcmc.n_max <= _lib.MCMC_N_MAX:
            raise ValueError(f"n_max must lie in 1..{_lib.MCMC_N_MAX}, got {mcmc.n_max}")
        if not 0.0 < mcmc.min_opacity < 1.0:
            raise ValueError(f"min_opacity must lie in (0, 1), got {mcmc.min_opacity}")
        self.mcmc = mcmc
        m = mcmc.min_opacity
        self.dead_logit = float(np.float32(math.log(m / (1.0 - m))))      # L: the comparison is on the logit
        self._last = {}                                                    # counts of the last relocate / grow

    # ---- helpers ----
    def _param(self, name: str) -> torch.Tensor:
        return next(g["params"][0] for g in self.optimizer.param_groups if g["name"] == name)

    def _xyz_lr_now(self) -> float:
        return float(next(g["lr"] for g in self.optimizer.param_groups if g["name"] == "xyz"))

    def grown_size(self, P: int) -> int:
        """P after a growth step: min(cap_max, floor(1.05 P)) in integer arithmetic, never below P."""
        return max(P, min(int(self.mcmc.cap_max), (P * int(self.mcmc.grow_factor_percent)) // 100))

    def record(self, *args, **kwargs) -> None:
        """The rule reads only parameters: no statistics."""

    def counts(self, which: str = "relocate") -> Dict[str, int]:
        """{"n_dead", "n_draws", "n_sources", "P_new"} of the last relocate() or grow()."""
        return dict(self._last[which])

    def _uniforms(self, n: int, generator, u, dev) -> torch.Tensor:
        if u is None:
            u = torch.rand(n, generator=generator, device=dev, dtype=torch.float32)
        if u.dtype != torch.float32 or u.dim() != 1 or u.shape[0] < n:
            raise ValueError(f"u must be float32 [>= {n}], got {u.dtype} {tuple(u.shape)}")
        return u.to(dev).contiguous()

    def _draws(self, u: torch.Tensor, n_grow: Optional[int]):
        """(dead [P] bool, src [n] int64, c [P] int64, total) -- n = n_dead for relocation (n_grow None), n_grow for growth."""
        op = self._param("opacity").detach().reshape(-1)
        P = op.shape[0]
        dead = op <= self.dead_logit
        w = torch.floor(torch.sigmoid(op.double()) * float(1 << 20) + 0.5).to(torch.int64)
        w[dead] = 0
        cdf = torch.cumsum(w, dim=0)
        total = int(cdf[-1]) if P else 0
        n = int(dead.sum()) if n_grow is None else n_grow
        if total == 0:
            return dead, None, torch.zeros(P, dtype=torch.int64, device=op.device), 0
        t = torch.floor(u[:n].double() * float(total)).to(torch.int64).clamp_(max=total - 1)
        src = torch.searchsorted(cdf, t, right=True)               # the smallest i with C_i > t
        return dead, src, torch.bincount(src, minlength=P), total

    def _correction(self, rows: torch.Tensor, c: torch.Tensor):
        """New opacity logits [S, 1] and log scales [S, 3] of the sources `rows` drawn c times, float64 rounded once."""
        mc = self.mcmc
        lg = self._param("opacity").detach().reshape(-1)[rows].double()
        N = torch.clamp(c + 1, max=mc.n_max)
        o, q = torch.sigmoid(lg), torch.sigmoid(-lg)                # q = 1 - o without the cancellation
        lq = torch.log(q) / N
        x = -torch.expm1(lq)
        k = torch.arange(mc.n_max, device=lg.device, dtype=torch.float64)
        sign = 1.0 - 2.0 * (k % 2)
        terms = _binomial_table(mc.n_max).to(lg.device)[N] * sign * torch.pow(x[:, None], k + 1.0) / torch.sqrt(k + 1.0)
        D = terms.sum(dim=1)
        new_sc = (self._param("scaling").detach()[rows].double() + torch.log(o / D)[:, None]).float()
        oc = x.clamp(min=mc.min_opacity, max=1.0 - 2.0 ** -23)
        rest = torch.where(oc == x, torch.exp(lq), 1.0 - oc)
        return torch.log(oc / rest).float()[:, None], new_sc

    # ---- the two changes of the set ----
    def relocate(self, generator: Optional[torch.Generator] = None, u: Optional[torch.Tensor] = None) -> None:
        """Every dead Gaussian becomes a copy of a live one drawn by opacity; the sources are corrected.  P is unchanged.
        Always consumes P uniforms of `generator`, whatever the number of dead rows."""
        P, dev = self._param("xyz").shape[0], self._param("xyz").device
        u = self._uniforms(P, generator, u, dev)
        dead, src, c, total = self._draws(u, None)
        n_dead = int(dead.sum()) if P else 0
        if total == 0 or n_dead == 0:
            self._last["relocate"] = {"n_dead": n_dead, "n_draws": n_dead if total else 0, "n_sources": 0, "P_new": P}
            return
        srcs = (c > 0).nonzero().reshape(-1)
        dest = dead.nonzero().reshape(-1)
        new = dict(zip(("opacity", "scaling"), self._correction(srcs, c[srcs])))

        def param_fn(n, p):
            p = p.clone()
            if n in new:
                p[srcs] = new[n]
            p[dest] = p[src]
            return p

        def moment_fn(n, m):
            m = m.clone()
            m[srcs] = 0
            m[dest] = 0
            return m
        self._remap(param_fn, moment_fn)
        self._last["relocate"] = {"n_dead": n_dead, "n_draws": n_dead, "n_sources": int(srcs.shape[0]), "P_new": P}

    def grow(self, generator: Optional[torch.Generator] = None, u: Optional[torch.Tensor] = None) -> int:
        """Appends min(cap_max, floor(1.05 P)) - P copies of live Gaussians drawn by opacity; returns the new P."""
        P, dev = self._param("xyz").shape[0], self._param("xyz").device
        P_new = self.grown_size(P)
        n = P_new - P
        if n == 0:
            self._last["grow"] = {"n_dead": 0, "n_draws": 0, "n_sources": 0, "P_new": P}
            return P
        u = self._uniforms(n, generator, u, dev)
        dead, src, c, total = self._draws(u, n)
        if total == 0:                                              # nothing to draw from: plain copies (include/gsr_mcmc.h)
            src, srcs, new = torch.arange(n, device=dev) % P, torch.zeros(0, dtype=torch.int64, device=dev), {}
        else:
            srcs = (c > 0).nonzero().reshape(-1)
            new = dict(zip(("opacity", "scaling"), self._correction(srcs, c[srcs])))

        def param_fn(name, p):
            p = p.clone()
            if name in new:
                p[srcs] = new[name]
            return torch.cat((p, p[src]), dim=0)

        def moment_fn(name, m):
            m = m.clone()
            m[srcs] = 0
            return torch.cat((m, torch.zeros((n,) + tuple(m.shape[1:]), dtype=m.dtype, device=m.device)), dim=0)
        self._remap(param_fn, moment_fn)
        self._zero_statistics(P_new, dev)
        self._last["grow"] = {"n_dead": int(dead.sum()), "n_draws": n if total else 0, "n_sources": int(srcs.shape[0]), "P_new": P_new}
        return P_new

    # ---- every iteration ----
    def add_noise(self, generator: Optional[torch.Generator] = None, noise: Optional[torch.Tensor] = None) -> None:
        """xyz += (R S S R^T noise) * gate(opacity) * noise_lr * (current xyz learning rate), in place."""
        mc = self.mcmc
        xyz = self._param("xyz")
        P, dev = xyz.shape[0], xyz.device
        if noise is None:
            noise = torch.randn((P, 3), generator=generator, device=dev, dtype=torch.float32)
        if P == 0:
            return
        with torch.no_grad():
            o = torch.sigmoid(self._param("opacity").detach())
            f = 1.0 / (1.0 + torch.exp(mc.gate_k * (o - mc.gate_t)))
            RS = quaternion_to_rotation(self._param("rotation").detach()) * torch.exp(self._param("scaling").detach())[:, None, :]
            cov = torch.bmm(RS, RS.transpose(1, 2))
            xyz.add_(torch.bmm(cov, noise.to(dev)[:, :, None]).squeeze(-1) * f * float(np.float32(mc.noise_lr * self._xyz_lr_now())))

    def regularize(self):
        """Adds the gradients of opacity_reg * mean sigmoid(opacity) + scale_reg * mean exp(scaling) into the parameters' .grad;
        returns the two terms (0-d tensors on the parameters' device)."""
        mc = self.mcmc
        op, sc = self._param("opacity"), self._param("scaling")
        P = op.shape[0]
        with torch.no_grad():
            for p in (op, sc):
                if p.grad is None:
                    p.grad = torch.zeros_like(p)
            if P == 0:
                z = torch.zeros((), dtype=torch.float64, device=op.device)
                return z, z.clone()
            s, e = torch.sigmoid(op.detach()), torch.exp(sc.detach())
            op.grad.add_(float(np.float32(mc.opacity_reg / P)) * (s * (1.0 - s)))
            sc.grad.add_(float(np.float32(mc.scale_reg / (3.0 * P))) * e)
            return mc.opacity_reg * s.double().mean(), mc.scale_reg * e.double().mean()

    # ---- the schedule ----
    def after_backward(self, iteration: int, *args, **kwargs):
        """Call after loss.backward() and before optimizer.step(): the regularisers' gradients.  Returns the two terms."""
        return self.regularize()

    def after_step(self, iteration: int, generator: Optional[torch.Generator] = None) -> None:
        """Call after optimizer.step(): noise every iteration; relocation then growth every refine_every iterations inside
        [refine_start, refine_stop)."""
        mc = self.mcmc
        self.add_noise(generator=generator)
        if mc.refine_start <= iteration < mc.refine_stop and iteration % mc.refine_every == 0:
            self.relocate(generator=generator)
            self.grow(generator=generator)


_MCMC_ROLE = {**dict.fromkeys(GROUPS, _lib.MCMC_COPY), "opacity": _lib.MCMC_OPACITY, "scaling": _lib.MCMC_SCALING}


class FusedMCMCController(_FusedGroups, MCMCController):
    """MCMCController on the HIP path (include/gsr_mcmc.h, csrc/mcmc.hip).  relocate, add_noise and regularize enqueue their kernels
    and return: no host wait.  grow allocates the new rows -- their number is known on the host -- and installs them through
    _install, as _remap does, also without a wait.  counts() is the one method that synchronises.  Same results as MCMCController: indices, counts
    and copied rows bit for bit, the corrected opacity and scaling to one float32 ulp.  No CPU fallback."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._kept = {}                # _workspace()
        self._pinned = {}              # which -> pinned host words {n_dead, n_draws, n_sources, P_new}
        self._issued = {}              # which -> device the last plan ran on

    def counts(self, which: str = "relocate") -> Dict[str, int]:
        """Waits for the device, then {"n_dead", "n_draws", "n_sources", "P_new"} of the last relocate() or grow()."""
        if which in self._last:        # decided on the host (nothing to do): no plan ran
            return dict(self._last[which])
        torch.cuda.current_stream(self._issued[which]).synchronize()
        return dict(zip(("n_dead", "n_draws", "n_sources", "P_new"), (int(v) for v in self._pinned[which].tolist())))

    def _plan_and_apply(self, which: str, mode: int, olds, P: int, n: int, u: torch.Tensor, dev, new=None, states=None) -> None:
        """gsr_mcmc_plan, then gsr_mcmc_apply in place (new None) or into new / states: two calls enqueued, nothing waited for."""
        ptr = _lib.ptr
        with torch.cuda.device(dev):
            ws = self._workspace("plan", dev, "gsr_mcmc_plan_workspace", P, n)
            if which not in self._pinned:
                self._pinned[which] = torch.zeros(4, dtype=torch.int32).pin_memory()
            _lib.call("gsr_mcmc_plan", _lib.stream(dev), mode, P, ptr(olds["opacity"]), ptr(olds["scaling"]), self.dead_logit, float(self.mcmc.min_opacity),
                      int(self.mcmc.n_max), n, ptr(u), ptr(self._pinned[which]), ptr(ws), ws.numel())
            self._last.pop(which, None)
            self._issued[which] = dev
            arr, k = self._group_table(_lib.McmcGroup, _MCMC_ROLE, olds, new, states)
            _lib.call("gsr_mcmc_apply", _lib.stream(dev), mode, P, n, k, arr, ptr(ws), ws.numel())

    def relocate(self, generator: Optional[torch.Generator] = None, u: Optional[torch.Tensor] = None) -> None:
        olds = self._olds()
        P, dev = olds["xyz"].shape[0], olds["xyz"].device
        u = self._device_f32("u", self._uniforms(P, generator, u, dev))
        if P == 0:
            self._last["relocate"] = {"n_dead": 0, "n_draws": 0, "n_sources": 0, "P_new": 0}
            return
        self._plan_and_apply("relocate", _lib.MCMC_RELOCATE, olds, P, 0, u, dev)

    def grow(self, generator: Optional[torch.Generator] = None, u: Optional[torch.Tensor] = None) -> int:
        olds = self._olds()
        P, dev = olds["xyz"].shape[0], olds["xyz"].device
        P_new = self.grown_size(P)
        n = P_new - P
        if n == 0:
            self._last["grow"] = {"n_dead": 0, "n_draws": 0, "n_sources": 0, "P_new": P}
            return P
        u = self._device_f32("u", self._uniforms(n, generator, u, dev))
        new, states = self._allocate(P_new, dev)
        self._plan_and_apply("grow", _lib.MCMC_GROW, olds, P, n, u, dev, new, states)
        self._install(new, states)
        self._zero_statistics(P_new, dev)
        return P_new

    def add_noise(self, generator: Optional[torch.Generator] = None, noise: Optional[torch.Tensor] = None) -> None:
        olds = self._olds()
        P, dev = olds["xyz"].shape[0], olds["xyz"].device
        if noise is None:
            noise = torch.randn((P, 3), generator=generator, device=dev, dtype=torch.float32)
        noise = self._device_f32("noise", noise)
        if tuple(noise.shape) != (P, 3):
            raise _lib.GsrError(f"FusedMCMCController.add_noise: noise must be [{P}, 3], got {tuple(noise.shape)}")
        if P == 0:
            return
        ptr, mc = _lib.ptr, self.mcmc
        with torch.cuda.device(dev):
            _lib.call("gsr_mcmc_noise", _lib.stream(dev), P, ptr(olds["opacity"]), ptr(olds["scaling"]), ptr(olds["rotation"]), ptr(noise),
                      ptr(olds["xyz"]), float(mc.gate_k), float(mc.gate_t), float(np.float32(mc.noise_lr * self._xyz_lr_now())))

    def regularize(self):
        """As MCMCController.regularize, one entry point.  The .grad tensors are taken as they come: float32, unit column stride,
        any row stride (views into a gradient arena)."""
        mc = self.mcmc
        op, sc = self._param("opacity"), self._param("scaling")
        self._device_f32("opacity", op.detach()); self._device_f32("scaling", sc.detach())
        P, dev = op.shape[0], op.device
        for p in (op, sc):
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        means = torch.zeros(2, dtype=torch.float64, device=dev)
        if P == 0:
            return means[0], means[1]
        strides = []
        for name, p, width in (("opacity", op, 1), ("scaling", sc, 3)):
            g = p.grad
            if g.device != dev or g.dtype != torch.float32 or tuple(g.shape) != tuple(p.shape) or (width > 1 and g.stride(1) != 1) or \
                    (P > 1 and g.stride(0) < width):
                raise _lib.GsrError(f"FusedMCMCController.regularize: {name}.grad must be float32 [{P}, {width}] on the parameters' device with "
                                    f"unit column stride, got {g.dtype} {tuple(g.shape)} strides {g.stride()}")
            strides.append(max(int(g.stride(0)), width))
        with torch.cuda.device(dev):
            ws = self._workspace("regularize", dev, "gsr_mcmc_regularize_workspace", P)
            # .data_ptr(), not ptr(): the strided tensors that cross the boundary, handed over with their row strides
            _lib.call("gsr_mcmc_regularize", _lib.stream(dev), P, _lib.ptr(op.detach()), _lib.ptr(sc.detach()), op.grad.data_ptr(), strides[0],
                      sc.grad.data_ptr(), strides[1], float(mc.opacity_reg), float(mc.scale_reg), _lib.ptr(means), _lib.ptr(ws), ws.numel())
        return mc.opacity_reg * means[0], mc.scale_reg * means[1]
