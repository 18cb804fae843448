"""GaussianRasterizationSettings / GaussianRasterizer: the reference's rasterizer API on HIP.

Drop-in for the names the reference imports at gaussian_renderer/__init__.py:14 and uses at
:36-49 (settings), :51 (constructor), :85-93 (keyword-only forward returning (color, radii)).
Same field order, argument meaning, validation messages and gradient order as the absent
upstream package; the native layer underneath is libgsr_hip.so through ctypes
(_lib.py) instead of pybind11/CUDA.
"""
from __future__ import annotations

import ctypes as C
import math
import weakref
from typing import NamedTuple, Optional

import torch
from torch import nn

from . import _lib
from ._lib import ptr


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


def _f32c(t: torch.Tensor, name: str, device) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise _lib.GsrError(f"{name} must be float32, got {t.dtype}")
    if t.device != device:
        t = t.to(device)
    return t.contiguous()


def camera_settings(cam, bg, scale_modifier, sh_degree, debug) -> GaussianRasterizationSettings:
    """The settings of one render from a camera object (image_height / image_width, FoVx / FoVy, world_view_transform,
    full_proj_transform, camera_center), as the reference builds them (gaussian_renderer/__init__.py:32-49)."""
    return GaussianRasterizationSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width),
        tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5), bg=bg, scale_modifier=scale_modifier,
        viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=sh_degree,
        campos=cam.camera_center, prefiltered=False, debug=bool(debug))


def _camera(rs: GaussianRasterizationSettings, dev):
    return _f32c(rs.viewmatrix, "viewmatrix", dev), _f32c(rs.projmatrix, "projmatrix", dev), _f32c(rs.campos, "campos", dev)


def _arena_fits(arena: torch.Tensor, dev, P: int, M: int, has_sr: bool) -> bool:
    return arena.device == dev and arena.dtype == torch.float32 and arena.is_contiguous() and arena.numel() >= arena_floats(P, M, has_sr)


def _usable_arena(dev, P: int, M: int, has_sr: bool):
    """The gradient arena a reverse pass carves its outputs from (None: none is set), refused if it cannot hold them."""
    arena = _grad_arena
    if arena is not None and not _arena_fits(arena, dev, P, M, has_sr):
        raise _lib.GsrError("gradient arena must be a contiguous float32 tensor on the render device with "
                            f"at least {arena_floats(P, M, has_sr)} elements")
    return arena


class HipBackend:
    """Calls the C ABI.  The only backend the product ever constructs."""

    name = "hip"

    def __init__(self):
        self.lib = _lib.load()
        self._ws_cache = {}
        self._announced = {}         # device index -> (geom pointer, P, M, gradient tensors) of a forward(announce_backward=True)
        self._bin_hint = {}          # (P, W, H) -> bytes of binning workspace the last forward pass of that shape asked for
        self._arena_claims = {}      # geom pointer -> (weak reference to geom, first byte, end byte) of the gradient arena a render in flight owns

    def _claim_arena(self, arena, geom):
        """A gradient arena entered around a forward call belongs to that render until its backward call: a second render in flight
        whose forward call is given the same memory would have its gradient views alias the first one's (the later backward call
        overwrites the earlier one's gradients, and autograd then adds a tensor to itself): refused, not summed wrongly."""
        lo, hi = arena.data_ptr(), arena.data_ptr() + 4 * arena.numel()
        for key, (ref_, a, b) in list(self._arena_claims.items()):
            if ref_() is None:                   # that render's graph is gone: it never ran backward, and never will
                del self._arena_claims[key]
            elif a < hi and lo < b:
                raise _lib.GsrError("gradient arena is still owned by another render in flight (its forward call was given the same "
                                    "memory and its backward call has not run): one arena per render between forward and backward -- "
                                    "render the other cameras into a scratch arena and add")
        self._arena_claims[geom.data_ptr()] = (weakref.ref(geom), lo, hi)

    def _release_arena(self, geom):
        """The arena claimed for the render that owns `geom` is the caller's again: its backward call has run, or its forward call failed."""
        self._arena_claims.pop(geom.data_ptr(), None)

    def _sizes(self, P, W, H):
        key = (P, W, H)
        v = self._ws_cache.get(key)
        if v is None:
            g, i, b = C.c_size_t(), C.c_size_t(), C.c_size_t()
            _lib.call("gsr_workspace_sizes", P, W, H, C.byref(g), C.byref(i), C.byref(b))       # three outputs: not a workspace() sizer
            v = (g.value, i.value, b.value)
            if len(self._ws_cache) > 64:
                self._ws_cache.clear()
            self._ws_cache[key] = v
        return v

    def _gradient_outputs(self, dev, P, M, Mrest, has_sr, has_colors, has_cov, arena):
        """The tensors gsr_backward writes (include/gsr.h): carved from the gradient arena when one is set."""
        f32 = dict(dtype=torch.float32, device=dev)
        off = [0]

        def out(shape):
            n = 1
            for d in shape:
                n *= d
            if arena is None or n == 0:
                return torch.empty(shape, **f32)
            v = arena[off[0]:off[0] + n].view(shape)
            off[0] += n
            return v
        g_means3D = out((P, 3))
        g_sh = out((P, M, 3)) if M > 0 else torch.empty((0,), **f32)
        g_sh_rest = out((P, Mrest, 3)) if Mrest > 0 else None
        g_opacity = out((P, 1))
        g_scales = out((P, 3)) if has_sr else torch.empty((0,), **f32)
        g_rots = out((P, 4)) if has_sr else torch.empty((0,), **f32)
        g_means2D = torch.empty((P, 3), **f32)
        # gradients of the inputs that were not given are not written at all (36 B per Gaussian less to store)
        g_colors = torch.empty((P, 3), **f32) if has_colors else None
        g_cov3D = torch.empty((P, 6), **f32) if has_cov else None
        return g_means3D, g_means2D, g_sh, g_colors, g_opacity, g_scales, g_rots, g_cov3D, g_sh_rest

    def forward(self, rs: GaussianRasterizationSettings, means3D, shs, colors_precomp, opacities, scales, rotations,
                cov3D_precomp, shs_rest=None, raw_params=False, announce_backward=False):
        """announce_backward: a backward() call for this render will follow.  Its gradient tensors are created now and announced
        to the library (gsr_backward_prefill), which writes their zeros beside this forward pass where that pays; backward() picks
        them up.  With a gradient arena they are its slices if the arena is set around this call as well as around backward() (the
        same one: anything else makes backward() carve and fill as before).  The fused form (shs_rest given) announces nothing --
        its backward() carves and fills by itself -- but a gradient arena set around the call is claimed for it all the same
        (_claim_arena), so that no second render in flight is given the same memory."""
        dev = means3D.device
        if dev.type != "cuda":
            raise _lib.GsrError(f"the HIP rasterizer needs tensors on a HIP device, got {dev} (no CPU fallback)")
        P, H, W = int(means3D.shape[0]), int(rs.image_height), int(rs.image_width)
        M = int(shs.shape[1]) if shs.numel() else 0
        if shs_rest is not None:
            M += int(shs_rest.shape[1])
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream      # _lib.stream(dev), inline: the hot path (profiles/host/bindings_refactor.txt)
            gb, ib, _ = self._sizes(P, W, H)
            u8 = dict(dtype=torch.uint8, device=dev)
            color = torch.empty((3, H, W), dtype=torch.float32, device=dev)
            radii = torch.empty((P,), dtype=torch.int32, device=dev)
            geom = torch.empty((gb,), **u8)
            img = torch.empty((ib,), **u8)
            holder = []
            # The library asks for the binning workspace in the middle of the forward pass, once the device has counted the pairs,
            # with the GPU waiting for the kernels that follow: torch.empty() there is host time on the critical path.  A buffer
            # of the size this shape needed last time (+5 %) is set aside beforehand; the callback hands it over if it is enough.
            key = (P, W, H)
            hint = self._bin_hint.get(key, 0)
            spare = torch.empty((int(hint * 1.05) + 4096,), **u8) if hint else None
            asked = [0]

            def alloc(_user, nbytes):
                try:
                    asked[0] = int(nbytes)
                    if spare is not None and not holder and nbytes <= spare.numel():
                        holder.append(spare)
                        return spare.data_ptr()
                    t = torch.empty((max(int(nbytes), 1),), **u8)
                    holder.append(t)
                    return t.data_ptr()
                except Exception:        # allocation failure surfaces as GSR_ERR_ALLOC
                    return None
            cb = _lib.ALLOC_FN(alloc)
            n = C.c_int64(0)
            bg = _f32c(rs.bg, "bg", dev)
            vm, pm, cp = _camera(rs, dev)
            grads = None
            arena = _grad_arena            # set around the forward call too: the announced tensors are its slices (and get zeroed now)
            if arena is not None and not _arena_fits(arena, dev, P, M, scales.numel() > 0):
                announce_backward = False  # backward() raises the error
            claimed = arena is not None and announce_backward and P > 0
            if claimed:
                self._claim_arena(arena, geom)          # may refuse: before anything announced earlier is let go
            stale = self._announced.pop(dev.index, None)      # kept allocated until gsr_forward has ordered its fill (include/gsr.h)
            try:
                if announce_backward and shs_rest is None and P > 0:
                    grads = self._gradient_outputs(dev, P, M, 0, scales.numel() > 0, colors_precomp.numel() > 0, cov3D_precomp.numel() > 0, arena)
                    g_means3D, g_means2D, g_sh, g_colors, g_opacity, g_scales, g_rots, g_cov3D, _ = grads
                    _lib.call("gsr_backward_prefill", P, M, ptr(g_means2D), ptr(g_opacity), ptr(g_colors), ptr(g_means3D), ptr(g_cov3D),
                              ptr(g_sh), ptr(g_scales), ptr(g_rots), None)
                # not _lib.call: the return code is needed before `stale` is dropped, the announcement withdrawn and the claim released
                rc = self.lib.gsr_forward(
                    stream, P, int(rs.sh_degree), M, W, H, ptr(bg), ptr(means3D), ptr(shs), ptr(colors_precomp),
                    ptr(opacities), ptr(scales), float(rs.scale_modifier), ptr(rotations), ptr(cov3D_precomp),
                    ptr(vm), ptr(pm), ptr(cp), float(rs.tanfovx), float(rs.tanfovy), int(bool(rs.prefiltered)),
                    int(bool(rs.debug)), color.data_ptr(), ptr(radii), geom.data_ptr(), gb, cb, None, img.data_ptr(), ib,      # allocated above: dense
                    C.byref(n), ptr(shs_rest), int(bool(raw_params)))          # n: num_rendered, the call's one output word
            except BaseException:
                if claimed:
                    self._release_arena(geom)           # no render came of it: nothing waits for a backward call
                raise
            if rc != 0 and grads is not None:
                self.lib.gsr_backward_prefill(0, 0, None, None, None, None, None, None, None, None, None)
            if rc != 0 and claimed:
                self._release_arena(geom)
            del stale
            _lib.check(rc, "gsr_forward")
            if grads is not None:
                # one render per device: the next forward() drops it
                self._announced[dev.index] = (geom.data_ptr(), P, M, grads, None if arena is None else (arena.data_ptr(), arena.numel()))
            if asked[0]:
                self._bin_hint[key] = asked[0]
                if len(self._bin_hint) > 64:
                    self._bin_hint.pop(next(iter(self._bin_hint)))
            binning = holder[0] if holder else torch.empty((0,), **u8)
            if _contrib_stats is not None:     # collect_contribution: this view's blend weights, from the workspaces just filled
                _contrib_stats._add_view(dev, stream, P, W, H, int(n.value), geom, binning, img)
        return int(n.value), color, radii, geom, binning, img

    def backward(self, rs, num_rendered, dL_dpix, means3D, radii, shs, colors_precomp, scales, rotations,
                 cov3D_precomp, geom, binning, img, shs_rest=None, raw_params=False, return_ws=False):
        """return_ws: the workspace tensor this call allocated is returned as one more element, so that the caller can keep it alive
        and hand it to pose_backward (include/gsr_pose.h: its accumulator rows, unmodified, on the same stream)."""
        dev = means3D.device
        P, H, W = int(means3D.shape[0]), int(rs.image_height), int(rs.image_width)
        M = int(shs.shape[1]) if shs.numel() else 0
        Mrest = int(shs_rest.shape[1]) if shs_rest is not None else 0
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream      # _lib.stream(dev), inline, as in forward()
            # depends on the pair count while the deterministic mode is on
            bwd_ws = _lib.workspace("gsr_backward_workspace_bytes", dev, P, int(num_rendered))
            has_sr = scales.numel() > 0
            arena = _usable_arena(dev, P, M + Mrest, has_sr)
            self._release_arena(geom)      # the arena claimed at forward time is the caller's again after this call
            ann = self._announced.pop(dev.index, None)
            if ann is not None and ann[:3] == (geom.data_ptr(), P, M) and Mrest == 0 and \
                    ann[4] == (None if arena is None else (arena.data_ptr(), arena.numel())):
                grads = ann[3]                       # created (and, where it pays, zero-filled) by the forward pass
            else:
                grads = self._gradient_outputs(dev, P, M, Mrest, has_sr, colors_precomp.numel() > 0, cov3D_precomp.numel() > 0, arena)
            g_means3D, g_means2D, g_sh, g_colors, g_opacity, g_scales, g_rots, g_cov3D, g_sh_rest = grads
            bg = _f32c(rs.bg, "bg", dev)
            vm, pm, cp = _camera(rs, dev)
            dL = _f32c(dL_dpix, "grad of rendered image", dev)
            # not _lib.call: the return code is in hand before the announced tensors (`ann`) are dropped and before the check raises
            rc = self.lib.gsr_backward(
                stream, P, int(rs.sh_degree), M + Mrest, int(num_rendered), W, H, ptr(bg), ptr(means3D), ptr(radii),
                ptr(shs), ptr(colors_precomp), ptr(scales), float(rs.scale_modifier), ptr(rotations),
                ptr(cov3D_precomp), ptr(vm), ptr(pm), ptr(cp), float(rs.tanfovx), float(rs.tanfovy), ptr(dL),
                ptr(geom), geom.numel(), ptr(binning), binning.numel(), ptr(img), img.numel(), ptr(bwd_ws),
                bwd_ws.numel(), ptr(g_means2D), ptr(g_opacity), ptr(g_colors), ptr(g_means3D), ptr(g_cov3D),
                ptr(g_sh), ptr(g_scales), ptr(g_rots), int(bool(rs.debug)), ptr(shs_rest), int(bool(raw_params)),
                ptr(g_sh_rest))
            del ann
            _lib.check(rc, "gsr_backward")
            if _absgrad_buf is not None:       # collect_absgrad: this pass's sums of |dL/dmeans2D| per pixel, from the same dL_dpix and workspaces
                _absgrad_buf._add_view(dev, stream, P, W, H, int(num_rendered), bg, dL, geom, binning, img)
        out = (g_means3D, g_means2D, g_sh, g_colors, g_opacity, g_scales, g_rots, g_cov3D)
        if shs_rest is not None:
            out = out + (g_sh_rest,)
        return out + (bwd_ws,) if return_ws else out

    def depth_forward(self, rs, P, num_rendered, mode, geom, binning, img):
        """(depth, alpha), [H,W] each, of the render whose gsr_forward filled the three workspaces (include/gsr_depth.h)."""
        dev = geom.device
        H, W = int(rs.image_height), int(rs.image_width)
        depth = torch.empty((H, W), dtype=torch.float32, device=dev)
        alpha = torch.empty((H, W), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.call("gsr_depth_forward", _lib.stream(dev), P, W, H, int(num_rendered), int(mode),
                      ptr(geom), geom.numel(), ptr(binning), binning.numel(), ptr(img), img.numel(), ptr(depth), ptr(alpha))
        return depth, alpha

    def arena_fill_in_flight(self, geom):
        """True when the render that owns `geom` announced gradient tensors that are slices of a gradient arena: the library may be
        zero-filling them on its second stream, and only gsr_backward joins that fill.  A map gradient alone must then not write
        into the arena by itself: _RasterizeGaussiansDepth runs the colour pass (zero gradient) first and adds to its tensors."""
        ann = self._announced.get(geom.device.index)
        return ann is not None and ann[0] == geom.data_ptr() and ann[4] is not None

    def _map_outputs(self, dev, P, has_sr, has_cov, geom, into, sh_floats):
        """The six tensors a map's reverse pass (depth_backward, features_backward) writes or adds into: `into` itself, or new ones --
        slices of the gradient arena when one is set, whose SH slice (sh_floats = 3 M per Gaussian) is then zeroed: the maps have no SH
        gradient."""
        if into is not None:
            return into
        M = sh_floats // 3
        arena = _usable_arena(dev, P, M, has_sr)
        self._release_arena(geom)
        g_means3D, g_means2D, g_sh, _c, g_opacity, g_scales, g_rots, g_cov3D, _r = self._gradient_outputs(
            dev, P, M if arena is not None else 0, 0, has_sr, False, has_cov, arena)
        if arena is not None and g_sh.numel():
            g_sh.zero_()
        return g_means3D, g_means2D, g_opacity, g_scales, g_rots, g_cov3D

    def features_forward(self, rs, P, num_rendered, features, geom, binning, img):
        """The [C,H,W] map of `features` [P,C] over the render whose gsr_forward filled the three workspaces (include/gsr_features.h)."""
        dev = geom.device
        H, W, Cn = int(rs.image_height), int(rs.image_width), int(features.shape[1])
        out = torch.empty((Cn, H, W), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.call("gsr_features_forward", _lib.stream(dev), P, Cn, W, H, int(num_rendered), ptr(features),
                      ptr(geom), geom.numel(), ptr(binning), binning.numel(), ptr(img), img.numel(), ptr(out))
        return out

    def features_backward(self, rs, num_rendered, features, dL_dout, means3D, radii, scales, rotations, cov3D_precomp,
                          geom, binning, img, into=None, sh_floats=0, want_features_grad=True):
        """Gradients of a feature map (include/gsr_features.h).  into: as depth_backward -- None: new tensors, accumulate = 0; the six
        tensors earlier passes of the same render wrote: added to, accumulate = 1.  Returns that tuple followed by dL/dfeatures
        [P,C], or None for it when want_features_grad is off (the library then forms none of its sums)."""
        dev = means3D.device
        P, H, W, Cn = int(means3D.shape[0]), int(rs.image_height), int(rs.image_width), int(features.shape[1])
        has_sr, has_cov = scales.numel() > 0, cov3D_precomp.numel() > 0
        with torch.cuda.device(dev):
            g_means3D, g_means2D, g_opacity, g_scales, g_rots, g_cov3D = self._map_outputs(dev, P, has_sr, has_cov, geom, into, sh_floats)
            g_feat = torch.empty((P, Cn), dtype=torch.float32, device=dev) if want_features_grad else None
            ws = _lib.workspace("gsr_features_workspace_bytes", dev, P, Cn)
            vm, pm, cp = _camera(rs, dev)
            gF = _f32c(dL_dout, "grad of the feature map", dev)
            _lib.call(
                "gsr_features_backward", _lib.stream(dev), P, Cn, W, H, int(num_rendered), ptr(means3D), ptr(radii), ptr(scales),
                float(rs.scale_modifier), ptr(rotations), ptr(cov3D_precomp), ptr(vm), ptr(pm), ptr(cp), float(rs.tanfovx), float(rs.tanfovy),
                ptr(features), ptr(gF), ptr(geom), geom.numel(), ptr(binning), binning.numel(), ptr(img), img.numel(),
                ptr(ws), ws.numel(), 0 if into is None else 1,
                ptr(g_means2D), ptr(g_opacity), ptr(g_means3D), ptr(g_cov3D), ptr(g_scales), ptr(g_rots), ptr(g_feat))
        return g_means3D, g_means2D, g_opacity, g_scales, g_rots, g_cov3D, g_feat

    def depth_backward(self, rs, num_rendered, mode, dL_ddepth, dL_dalpha, means3D, radii, scales, rotations, cov3D_precomp,
                       geom, binning, img, into=None, sh_floats=0, return_ws=False):
        """Gradients of the depth and alpha maps (include/gsr_depth.h).  into = None: new tensors (slices of the gradient arena when one
        is set; the arena's SH slice, sh_floats = 3 M per Gaussian, is then zeroed: the maps have no SH gradient), accumulate = 0.
        into = (g_means3D, g_means2D, g_opacity, g_scales, g_rots, g_cov3D) as HipBackend.backward of the same render just wrote
        them: added to, accumulate = 1.  Returns that tuple; with return_ws, followed by the workspace tensor this call allocated (for
        pose_backward, as HipBackend.backward)."""
        dev = means3D.device
        P, H, W = int(means3D.shape[0]), int(rs.image_height), int(rs.image_width)
        has_sr, has_cov = scales.numel() > 0, cov3D_precomp.numel() > 0
        with torch.cuda.device(dev):
            g_means3D, g_means2D, g_opacity, g_scales, g_rots, g_cov3D = self._map_outputs(dev, P, has_sr, has_cov, geom, into, sh_floats)
            ws = _lib.workspace("gsr_depth_workspace_bytes", dev, P)
            vm, pm, cp = _camera(rs, dev)
            gD = None if dL_ddepth is None else _f32c(dL_ddepth, "grad of the depth map", dev)
            gA = None if dL_dalpha is None else _f32c(dL_dalpha, "grad of the alpha map", dev)
            _lib.call(
                "gsr_depth_backward", _lib.stream(dev), P, W, H, int(num_rendered), int(mode), ptr(means3D), ptr(radii), ptr(scales),
                float(rs.scale_modifier), ptr(rotations), ptr(cov3D_precomp), ptr(vm), ptr(pm), ptr(cp), float(rs.tanfovx), float(rs.tanfovy),
                ptr(gD), ptr(gA), ptr(geom), geom.numel(), ptr(binning), binning.numel(), ptr(img), img.numel(),
                ptr(ws), ws.numel(), 0 if into is None else 1,
                ptr(g_means2D), ptr(g_opacity), ptr(g_means3D), ptr(g_cov3D), ptr(g_scales), ptr(g_rots))
        out = (g_means3D, g_means2D, g_opacity, g_scales, g_rots, g_cov3D)
        return out + (ws,) if return_ws else out

    def pose_backward(self, rs, kind, num_rendered, means3D, radii, shs, colors_precomp, scales, rotations, cov3D_precomp, geom, acc_ws,
                      want=(True, True, True)):
        """(dL/dviewmatrix [4,4], dL/dprojmatrix [4,4], dL/dcampos [3]) of the loss whose reverse pass -- backward() for kind 0,
        depth_backward() for kind 1 (expected depth) or 2 (inverse depth) -- was given `acc_ws` and ran last on this stream
        (include/gsr_pose.h).  want: which of the three are computed; the others are None (NULL to the library)."""
        dev = means3D.device
        P, H, W = int(means3D.shape[0]), int(rs.image_height), int(rs.image_width)
        M = int(shs.shape[1]) if shs.numel() else 0
        if not any(want):
            return None, None, None
        f32 = dict(dtype=torch.float32, device=dev)
        g_view = torch.empty((4, 4), **f32) if want[0] else None
        g_proj = torch.empty((4, 4), **f32) if want[1] else None
        g_campos = torch.empty((3,), **f32) if want[2] else None
        with torch.cuda.device(dev):
            ws = _lib.workspace("gsr_pose_workspace_bytes", dev, P)
            vm, pm, cp = _camera(rs, dev)
            colour = int(kind) == _lib.POSE_COLOR
            _lib.call(
                "gsr_pose_backward", _lib.stream(dev), int(kind), P, int(rs.sh_degree), M, W, H, int(num_rendered),
                ptr(means3D), ptr(radii), ptr(shs) if colour else None, ptr(colors_precomp) if colour else None,
                ptr(scales), float(rs.scale_modifier), ptr(rotations), ptr(cov3D_precomp), ptr(vm), ptr(pm), ptr(cp),
                float(rs.tanfovx), float(rs.tanfovy), ptr(geom), geom.numel(), ptr(acc_ws), acc_ws.numel(), ptr(ws), ws.numel(),
                ptr(g_view), ptr(g_proj), ptr(g_campos))
        return g_view, g_proj, g_campos

    def composited_mask(self, geom, P):
        """bool [P]: the Gaussians the forward pass that filled `geom` composited at all (include/gsr.h gsr_composited_mask): a
        superset of those that can receive a gradient, usually far smaller than radii > 0."""
        dev = geom.device
        out = torch.empty((P,), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.call("gsr_composited_mask", _lib.stream(dev), P, ptr(geom), geom.numel(), ptr(out))
        return out.bool()

    def gaussian_normals_forward(self, viewmatrix, means3D, scales, rotations):
        """(normals [P,3], axis [P] int32): every Gaussian's shortest axis in view space, facing the camera, and the code of the two
        decisions behind it (include/gsr_normals.h)."""
        dev = means3D.device
        _lib.require_hip("gaussian_normals", "means3D", means3D)
        P = int(means3D.shape[0])
        normals = torch.empty((P, 3), dtype=torch.float32, device=dev)
        axis = torch.empty((P,), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.call("gsr_gaussian_normals_forward", _lib.stream(dev), P, ptr(means3D), ptr(scales), ptr(rotations), ptr(viewmatrix),
                      ptr(normals), ptr(axis))
        return normals, axis

    def gaussian_normals_backward(self, viewmatrix, rotations, axis, dL_dnormals):
        """dL/drotations [P,4] of gaussian_normals_forward's normals; scales and means receive none (include/gsr_normals.h)."""
        dev = rotations.device
        P = int(rotations.shape[0])
        g_rots = torch.empty((P, 4), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.call("gsr_gaussian_normals_backward", _lib.stream(dev), P, ptr(rotations), ptr(viewmatrix), ptr(axis),
                      ptr(_f32c(dL_dnormals, "grad of the normals", dev)), ptr(g_rots))
        return g_rots

    def mark_visible(self, positions, viewmatrix, projmatrix):
        dev = positions.device
        if dev.type != "cuda":
            raise _lib.GsrError(f"the HIP rasterizer needs tensors on a HIP device, got {dev} (no CPU fallback)")
        P = int(positions.shape[0])
        out = torch.empty((P,), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            pos = _f32c(positions, "positions", dev); vm = _f32c(viewmatrix, "viewmatrix", dev)
            pm = _f32c(projmatrix, "projmatrix", dev)
            _lib.call("gsr_mark_visible", _lib.stream(dev), P, ptr(pos), ptr(vm), ptr(pm), ptr(out))
        return out.bool()


_backend = None
_last_forward = None    # (weak reference to the geometry workspace, P) of the most recent forward pass, for composited_mask()
_grad_arena = None      # optional flat float32 tensor the backward pass carves its parameter gradients from


def _remember_forward(geom, P):
    """composited_mask() without arguments refers to the most recent forward pass; a weak reference, so that the workspace (hundreds
    of MB at 5 M Gaussians) is released with its autograd graph instead of living on until the next render."""
    global _last_forward
    _last_forward = (weakref.ref(geom), P)


class gradient_arena:
    """Context manager: while active, gsr_backward writes dL/d{means3D, shs, opacities, scales, rotations}
    straight into consecutive slices of `flat` (59 floats per Gaussian at M = 16, in that order), so a
    data-parallel step can all-reduce `flat` without a packing copy.  The returned gradient tensors are
    views of `flat`.  Entered around the forward call as well, it lets the library zero those slices beside the forward pass already
    (gsr_backward_prefill): `flat` then belongs to that render from its forward call until its backward call.  ONE arena around the
    forward calls of several renders that are all still waiting for their backward calls is not supported -- their gradient views
    would be the same memory -- and the second such forward call raises GsrError; give every render in flight an arena of its own
    (the other cameras into a scratch arena, then add_, as bench.py does).  The refusal is decided at forward time, from the arena
    set around the forward calls alone, whatever arena -- or none -- the backward calls later run under: the claim ends with the
    owner's backward call, with a forward call that fails, or when the owner's autograd graph is freed, so a render with gradients
    whose image is kept but never run backward holds its arena for as long as that image lives.  An arena entered around backward
    calls only is never claimed and is overwritten by each of them in turn: consume or add it before the next one."""

    def __init__(self, flat: torch.Tensor):
        self.flat = flat

    def __enter__(self):
        global _grad_arena
        self.prev, _grad_arena = _grad_arena, self.flat
        return self.flat

    def __exit__(self, *exc):
        global _grad_arena
        _grad_arena = self.prev
        return False


def arena_floats(P: int, M: int, has_scale_rot: bool = True) -> int:
    return P * (3 + 3 * M + 1 + (7 if has_scale_rot else 0))


_contrib_stats = None   # the ContributionStats every forward pass adds its view to (collect_contribution), or None


class ContributionStats:
    """Per-Gaussian blend-weight statistics over many renders (include/gsr_contrib.h): for each of P Gaussians the sum of its blend
    weights alpha T over every pixel it was blended into, the largest of them, and the number of those pixels.  `rows` is the native
    accumulator, uint8 [P,16] on `device` (sum_q32 uint64 | max_bits uint32 | count uint32), all zero = nothing collected; `views`
    and `pixels_added` count what was added.  The sums are integers: they do not depend on the order of the views."""

    def __init__(self, P: int, device):
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.P, self.device = int(P), dev
        self.rows = torch.zeros((self.P, _lib.CONTRIB_ROW_BYTES), dtype=torch.uint8, device=dev)
        self.views = 0
        self.pixels_added = 0

    def reset(self) -> None:
        self.rows.zero_()
        self.views = 0
        self.pixels_added = 0

    def _add_view(self, dev, stream, P, W, H, num_rendered, geom, binning, img) -> None:
        if P != self.P or dev != self.device:
            raise _lib.GsrError(f"collect_contribution: the collector holds {self.P} Gaussians on {self.device}, "
                                f"the render has {P} on {dev}")
        if self.pixels_added + W * H > _lib.CONTRIB_MAX_PIXELS:
            raise _lib.GsrError(f"collect_contribution: {self.pixels_added} pixels collected, {W * H} more would pass the "
                                f"{_lib.CONTRIB_MAX_PIXELS} a row's count can hold (include/gsr_contrib.h): read and reset the collector")
        _lib.call("gsr_contrib_accumulate", stream, P, W, H, num_rendered, ptr(geom), geom.numel(), ptr(binning), binning.numel(),
                  ptr(img), img.numel(), ptr(self.rows))
        self.views += 1
        self.pixels_added += W * H

    def read(self):
        """(weight_sum float32 [P], weight_max float32 [P], pixel_count int32 [P]) of what has been collected so far."""
        w_sum = torch.empty((self.P,), dtype=torch.float32, device=self.device)
        w_max = torch.empty((self.P,), dtype=torch.float32, device=self.device)
        n_pix = torch.empty((self.P,), dtype=torch.int32, device=self.device)
        if self.P:
            with torch.cuda.device(self.device):
                _lib.call("gsr_contrib_read", _lib.stream(self.device), self.P, ptr(self.rows), ptr(w_sum), ptr(w_max), ptr(n_pix))
        return w_sum, w_max, n_pix


class collect_contribution:
    """Context manager: while active, every forward pass of the native backend -- render, render_fused, render_rows, with or without an
    autograd graph -- ends with one gsr_contrib_accumulate of its view into `stats`.  A render of another P or on another device
    raises GsrError, as does a view that would take `stats.pixels_added` past 2^32 - 1.  Outside it nothing new runs."""

    def __init__(self, stats: ContributionStats):
        self.stats = stats

    def __enter__(self):
        global _contrib_stats
        self.prev, _contrib_stats = _contrib_stats, self.stats
        return self.stats

    def __exit__(self, *exc):
        global _contrib_stats
        _contrib_stats = self.prev
        return False


_absgrad_buf = None     # the AbsGrad every colour reverse pass adds its view to (collect_absgrad), or None


class AbsGrad:
    """Per-Gaussian sums of |dL/dmeans2D| over the pixels of many reverse passes (include/gsr_absgrad.h): `grad` is float32 [P,2] on
    `device`, zeroed; `views` counts the reverse passes added.  The absolute value is taken per (pixel, Gaussian) pair, so a splat
    whose per-pixel gradients cancel in viewspace_points.grad still shows here (AbsGS; gsplat's absgrad).  Only the colour image's
    loss enters: depth, alpha and feature-map losses of the same graph add nothing.  Hand it to DensityController.record,
    after_backward or FusedDensityController.record as `absgrad=`; AbsGS and gsplat raise densify_grad_threshold with it
    (0.0002 -> about 0.0008), since the sums are larger than the signed ones."""

    def __init__(self, P: int, device):
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.P, self.device = int(P), dev
        self.grad = torch.zeros((self.P, 2), dtype=torch.float32, device=dev)
        self.views = 0

    def zero_(self) -> "AbsGrad":
        self.grad.zero_()
        self.views = 0
        return self

    def _add_view(self, dev, stream, P, W, H, num_rendered, bg, dL_dpix, geom, binning, img) -> None:
        if P != self.P or dev != self.device:
            raise _lib.GsrError(f"collect_absgrad: the collector holds {self.P} Gaussians on {self.device}, "
                                f"the render has {P} on {dev}")
        ws = _lib.workspace("gsr_absgrad_workspace_bytes", dev, P)
        _lib.call("gsr_absgrad_backward", stream, P, W, H, num_rendered, ptr(bg), ptr(dL_dpix), ptr(geom), geom.numel(),
                  ptr(binning), binning.numel(), ptr(img), img.numel(), ptr(ws), ws.numel(), 1, ptr(self.grad), None)
        self.views += 1


class collect_absgrad:
    """Context manager: while active, every colour reverse pass of the native backend (HipBackend.backward: GaussianRasterizer with or
    without depth=, features= or a differentiable camera, render, render_fused, render_rows -- each camera's pass adds its view) is
    followed, on the same stream, by one gsr_absgrad_backward(accumulate = 1) of that pass's dL_dpix and workspaces into `buf`.  It
    must be active when backward() runs, not (only) around the forward call.  A render of another P or on another device raises
    GsrError, as does entering a second collector inside one.  Outside it nothing new runs."""

    def __init__(self, buf: AbsGrad):
        self.buf = buf

    def __enter__(self):
        global _absgrad_buf
        if _absgrad_buf is not None:
            raise _lib.GsrError("collect_absgrad: a collector is active already (collectors do not nest)")
        _absgrad_buf = self.buf
        return self.buf

    def __exit__(self, *exc):
        global _absgrad_buf
        _absgrad_buf = None
        return False


def get_backend():
    global _backend
    if _backend is None:
        _backend = HipBackend()      # raises if libgsr_hip.so is missing: no fallback
    return _backend


def _set_backend_for_tests(backend):
    """Test hook: tests/ inject an oracle-backed stand-in to exercise the host logic (argument
    validation, autograd plumbing, the gloo data-parallel path) on machines without a GPU.
    Product code never calls this."""
    global _backend
    prev = _backend
    _backend = backend
    return prev


def _dump(path, *objs):
    try:
        torch.save(tuple(o.detach().cpu() if isinstance(o, torch.Tensor) else o for o in objs), path)
    except Exception:
        pass


def composited_mask(image: Optional[torch.Tensor] = None):
    """bool [P]: which Gaussians a forward pass composited at all.  Every Gaussian with a non-zero gradient is among them; a
    data-parallel trainer can restrict its gradient exchange to the union of the ranks' masks
    (dist.GradientExchange.launch(visible=...)).  `image`: the colour tensor a GaussianRasterizer call returned -- the mask of THAT
    render, whatever was rendered since (several cameras per step, several devices per process).  Without it: the most recent
    forward pass of this process, while its autograd graph is alive.  None if the backend does not track it or the render is gone."""
    be = get_backend()
    if not hasattr(be, "composited_mask"):
        return None
    if image is not None:
        fn = image.grad_fn
        if fn is None or not hasattr(fn, "saved_tensors") or not hasattr(fn, "gsr_geom_index"):
            return None
        saved = fn.saved_tensors
        return be.composited_mask(saved[fn.gsr_geom_index], int(saved[fn.gsr_means_index].shape[0]))
    if _last_forward is None:
        return None
    ref_, P = _last_forward
    geom = ref_()
    return None if geom is None else be.composited_mask(geom, P)


_INPUT_NAMES = ("shs", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp")      # of GaussianRasterizer.forward, after means3D


def _gaussian_inputs(means3D, tensors, names):
    """means3D and the tensors after it as the backend takes them: float32, dense, on means3D's device."""
    if means3D.dim() != 2 or means3D.shape[1] != 3:
        raise _lib.GsrError("means3D must have dimensions (num_points, 3)")
    dev = means3D.device
    return [_f32c(means3D, "means3D", dev)] + [_f32c(t, n, dev) for t, n in zip(tensors, names)]


def _announce(ctx, be):
    """The keyword that tells be.forward that a backward call will follow, for backends that announce (the tests' stand-ins take no
    such keyword)."""
    return {"announce_backward": True} if any(ctx.needs_input_grad) and hasattr(be, "_announced") else {}


def _keep(ctx, saved, geom_index, means_index, radii):
    """What every render leaves behind for its backward call and for composited_mask()."""
    _remember_forward(saved[geom_index], int(saved[means_index].shape[0]))
    ctx.save_for_backward(*saved)
    ctx.gsr_geom_index, ctx.gsr_means_index = geom_index, means_index        # composited_mask(image) finds the workspace through image.grad_fn
    ctx.mark_non_differentiable(radii)
    ctx.set_materialize_grads(False)      # no zero tensor for the int32 radii output on every backward (a 4 P byte fill)


def _zero_colour_grad(rs, dev):
    """Materialisation is off (_keep): an unused colour output arrives as None, and the colour pass takes this in its place."""
    return torch.zeros((3, int(rs.image_height), int(rs.image_width)), dtype=torch.float32, device=dev)


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
        be = get_backend()
        args = _gaussian_inputs(means3D, (sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp), _INPUT_NAMES)
        means3D_c, sh_c, colors_c, opac_c, scales_c, rots_c, cov_c = args
        try:
            num_rendered, color, radii, geom, binning, img = be.forward(
                raster_settings, means3D_c, sh_c, colors_c, opac_c, scales_c, rots_c, cov_c, **_announce(ctx, be))
        except Exception:
            if raster_settings.debug:
                _dump("snapshot_fw.dump", *args, raster_settings._asdict())
                print("\nAn error occured in forward. Please forward snapshot_fw.dump for debugging.")
            raise
        ctx.raster_settings = raster_settings
        ctx.num_rendered = num_rendered
        _keep(ctx, (colors_c, means3D_c, scales_c, rots_c, cov_c, radii, sh_c, geom, binning, img), 7, 1, radii)
        return color, radii

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii):
        be = get_backend()
        rs = ctx.raster_settings
        colors_c, means3D_c, scales_c, rots_c, cov_c, radii, sh_c, geom, binning, img = ctx.saved_tensors
        if grad_out_color is None:
            grad_out_color = _zero_colour_grad(rs, means3D_c.device)
        try:
            g_means3D, g_means2D, g_sh, g_colors, g_opac, g_scales, g_rots, g_cov = be.backward(
                rs, ctx.num_rendered, grad_out_color, means3D_c, radii, sh_c, colors_c, scales_c, rots_c, cov_c,
                geom, binning, img)
        except Exception:
            if rs.debug:
                _dump("snapshot_bw.dump", grad_out_color, means3D_c, radii, sh_c, colors_c, scales_c, rots_c, cov_c,
                      ctx.num_rendered, rs._asdict())
                print("\nAn error occured in backward. Writing snapshot_bw.dump for debugging.\n")
            raise
        none_if_empty = lambda g, src: g if src.numel() > 0 else None
        return (g_means3D, g_means2D, none_if_empty(g_sh, sh_c), none_if_empty(g_colors, colors_c), g_opac,
                none_if_empty(g_scales, scales_c), none_if_empty(g_rots, rots_c), none_if_empty(g_cov, cov_c), None)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, raster_settings)


DEPTH_MODES = {"expected": _lib.DEPTH_EXPECTED, "inverse": _lib.DEPTH_INVERSE}


def _reverse_passes(ctx, be, grad_color, grad_depth, grad_alpha, camera_pass=None):
    """The reverse passes of a render with maps or camera gradients (at least one of the three gradients given, or no maps at
    all): the colour pass, the map pass, or the colour pass and then the map pass adding into its tensors.  Returns the gradients
    of the eight Gaussian inputs.  camera_pass: called as camera_pass(pose kind, workspace) right after each pass whose loss the
    caller differentiates, while that pass is the last one on the stream; the workspaces are asked for (return_ws) only then."""
    rs = ctx.raster_settings
    colors_c, means3D_c, scales_c, rots_c, cov_c, radii, sh_c, geom, binning, img = ctx.saved_tensors[:10]      # (a feature render keeps an eleventh)
    maps = grad_depth is not None or grad_alpha is not None
    keep_ws = {} if camera_pass is None else {"return_ws": True}
    g_sh = g_colors = None
    colour_used = grad_color is not None
    # A map gradient alone must not write into an arena the library may still be zero-filling (HipBackend.arena_fill_in_flight): the
    # colour pass joins that fill, so it runs first, on a zero gradient.  Without maps the colour pass is all there is to run.
    if not colour_used and (not maps or (hasattr(be, "arena_fill_in_flight") and be.arena_fill_in_flight(geom))):
        grad_color = _zero_colour_grad(rs, means3D_c.device)
    if grad_color is not None:
        g_means3D, g_means2D, g_sh, g_colors, g_opac, g_scales, g_rots, g_cov, *ws = be.backward(
            rs, ctx.num_rendered, grad_color, means3D_c, radii, sh_c, colors_c, scales_c, rots_c, cov_c, geom, binning, img, **keep_ws)
        if camera_pass is not None and (colour_used or not maps):
            camera_pass(_lib.POSE_COLOR, ws[0])
    if maps:
        into = None if grad_color is None else (g_means3D, g_means2D, g_opac, g_scales, g_rots, g_cov)
        g_means3D, g_means2D, g_opac, g_scales, g_rots, g_cov, *ws = be.depth_backward(
            rs, ctx.num_rendered, ctx.depth_mode, grad_depth, grad_alpha, means3D_c, radii, scales_c, rots_c, cov_c,
            geom, binning, img, into=into, sh_floats=3 * int(sh_c.shape[1]) if sh_c.numel() else 0, **keep_ws)
        if camera_pass is not None:
            camera_pass(_lib.POSE_DEPTH_INVERSE if ctx.depth_mode == _lib.DEPTH_INVERSE else _lib.POSE_DEPTH_EXPECTED, ws[0])
    none_if_empty = lambda g, src: g if (g is not None and src.numel() > 0) else None
    if not colour_used:
        g_sh = g_colors = None          # the maps give the colour inputs no gradient
    return (g_means3D, g_means2D, none_if_empty(g_sh, sh_c), none_if_empty(g_colors, colors_c), g_opac,
            none_if_empty(g_scales, scales_c), none_if_empty(g_rots, rots_c), none_if_empty(g_cov, cov_c))


class _RasterizeGaussiansDepth(torch.autograd.Function):
    """(color, radii, depth, alpha): _RasterizeGaussians' render followed by the depth and alpha maps of the same lists
    (include/gsr_depth.h).  The forward call is the plain one -- announcement, arena, binning hint as there -- then one walk over what
    it left.  Backward runs what the losses used: the colour pass, the map pass, or the colour pass and then the map pass adding into
    its tensors."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, mode):
        be = get_backend()
        if not hasattr(be, "depth_forward"):
            raise _lib.GsrError(f"the {getattr(be, 'name', type(be).__name__)} backend renders no depth or alpha map")
        args = _gaussian_inputs(means3D, (sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp), _INPUT_NAMES)
        means3D_c, sh_c, colors_c, opac_c, scales_c, rots_c, cov_c = args
        num_rendered, color, radii, geom, binning, img = be.forward(
            raster_settings, means3D_c, sh_c, colors_c, opac_c, scales_c, rots_c, cov_c, **_announce(ctx, be))
        depth, alpha = be.depth_forward(raster_settings, int(means3D_c.shape[0]), num_rendered, mode, geom, binning, img)
        ctx.raster_settings, ctx.num_rendered, ctx.depth_mode = raster_settings, num_rendered, mode
        _keep(ctx, (colors_c, means3D_c, scales_c, rots_c, cov_c, radii, sh_c, geom, binning, img), 7, 1, radii)
        return color, radii, depth.unsqueeze(0), alpha.unsqueeze(0)

    @staticmethod
    def backward(ctx, grad_color, _grad_radii, grad_depth, grad_alpha):
        if grad_color is None and grad_depth is None and grad_alpha is None:
            return (None,) * 10
        return _reverse_passes(ctx, get_backend(), grad_color, grad_depth, grad_alpha) + (None, None)


class _RasterizeGaussiansFeatures(torch.autograd.Function):
    """(color, radii, feature_map) for mode None, (color, radii, depth, alpha, feature_map) for a depth mode: _RasterizeGaussians' or
    _RasterizeGaussiansDepth's render followed by the [C,H,W] map of `features` [P,C] over the same lists (include/gsr_features.h).
    Backward runs what the losses used: the passes of _reverse_passes for colour, depth and alpha, then the feature pass adding into
    their tensors -- or the feature pass alone; a map whose gradient is None costs no reverse pass."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, features, raster_settings, mode):
        be = get_backend()
        if not hasattr(be, "features_forward") or (mode is not None and not hasattr(be, "depth_forward")):
            raise _lib.GsrError(f"the {getattr(be, 'name', type(be).__name__)} backend renders no feature map")
        args = _gaussian_inputs(means3D, (sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp), _INPUT_NAMES)
        means3D_c, sh_c, colors_c, opac_c, scales_c, rots_c, cov_c = args
        feat_c = _f32c(features, "features", means3D.device)
        P = int(means3D_c.shape[0])
        num_rendered, color, radii, geom, binning, img = be.forward(
            raster_settings, means3D_c, sh_c, colors_c, opac_c, scales_c, rots_c, cov_c, **_announce(ctx, be))
        fmap = be.features_forward(raster_settings, P, num_rendered, feat_c, geom, binning, img)
        ctx.raster_settings, ctx.num_rendered, ctx.depth_mode = raster_settings, num_rendered, mode
        _keep(ctx, (colors_c, means3D_c, scales_c, rots_c, cov_c, radii, sh_c, geom, binning, img, feat_c), 7, 1, radii)
        if mode is None:
            return color, radii, fmap
        depth, alpha = be.depth_forward(raster_settings, P, num_rendered, mode, geom, binning, img)
        return color, radii, depth.unsqueeze(0), alpha.unsqueeze(0), fmap

    @staticmethod
    def backward(ctx, grad_color, _grad_radii, *grad_maps):
        grad_depth, grad_alpha = (None, None) if ctx.depth_mode is None else grad_maps[:2]
        grad_feat = grad_maps[-1]
        others = grad_color is not None or grad_depth is not None or grad_alpha is not None
        if not others and grad_feat is None:
            return (None,) * 11
        be = get_backend()
        _colors_c, means3D_c, scales_c, rots_c, cov_c, radii, sh_c, geom, binning, img, feat_c = ctx.saved_tensors
        g = None
        # the feature pass alone must not write into an arena the library may still be zero-filling: the colour pass joins that fill
        # and runs first, on a zero gradient (_reverse_passes does that when it is given nothing)
        if others or (hasattr(be, "arena_fill_in_flight") and be.arena_fill_in_flight(geom)):
            g = _reverse_passes(ctx, be, grad_color, grad_depth, grad_alpha)
        g_feat = None
        if grad_feat is not None:
            into = None if g is None else (g[0], g[1], g[4], g[5], g[6], g[7])
            g_means3D, g_means2D, g_opac, g_scales, g_rots, g_cov, g_feat = be.features_backward(
                ctx.raster_settings, ctx.num_rendered, feat_c, grad_feat, means3D_c, radii, scales_c, rots_c, cov_c, geom, binning, img,
                into=into, sh_floats=3 * int(sh_c.shape[1]) if sh_c.numel() else 0, want_features_grad=ctx.needs_input_grad[8])
            if g is None:
                none_if_empty = lambda t, src: t if (t is not None and src.numel() > 0) else None
                g = (g_means3D, g_means2D, None, None, g_opac, none_if_empty(g_scales, scales_c), none_if_empty(g_rots, rots_c),
                     none_if_empty(g_cov, cov_c))
        return g + (g_feat, None, None)


class _RasterizeGaussiansPose(torch.autograd.Function):
    """_RasterizeGaussians (mode None: (color, radii)) or _RasterizeGaussiansDepth (mode 0 / 1: (color, radii, depth, alpha)) with
    the camera as tensor arguments: viewmatrix, projmatrix and campos receive gradients too (include/gsr_pose.h).  The forward call
    is theirs -- announcement, arena, binning hint.  Backward runs their reverse passes, then gsr_pose_backward once per pass that
    ran, on the workspace that pass just used; the colour and the map contributions are added in torch.  The Gaussians' gradients
    are computed whether or not anybody asked for them: the camera gradient is made from the same accumulator rows."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, viewmatrix, projmatrix, campos,
                raster_settings, mode):
        be = get_backend()
        if not hasattr(be, "pose_backward") or (mode is not None and not hasattr(be, "depth_forward")):
            raise _lib.GsrError(f"the {getattr(be, 'name', type(be).__name__)} backend has no camera gradients")
        if viewmatrix.numel() != 16 or projmatrix.numel() != 16 or campos.numel() != 3:
            raise _lib.GsrError("viewmatrix and projmatrix must have 16 elements and campos 3")
        args = _gaussian_inputs(means3D, (sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp), _INPUT_NAMES)
        means3D_c, sh_c, colors_c, opac_c, scales_c, rots_c, cov_c = args
        dev = means3D.device
        cam = [_f32c(t.detach(), n, dev) for t, n in ((viewmatrix, "viewmatrix"), (projmatrix, "projmatrix"), (campos, "campos"))]
        rs = raster_settings._replace(viewmatrix=cam[0], projmatrix=cam[1], campos=cam[2])
        num_rendered, color, radii, geom, binning, img = be.forward(
            rs, means3D_c, sh_c, colors_c, opac_c, scales_c, rots_c, cov_c, **_announce(ctx, be))
        ctx.raster_settings, ctx.num_rendered, ctx.depth_mode = rs, num_rendered, mode
        ctx.cam_like = [(tuple(t.shape), t.dtype, t.device) for t in (viewmatrix, projmatrix, campos)]
        _keep(ctx, (colors_c, means3D_c, scales_c, rots_c, cov_c, radii, sh_c, geom, binning, img), 7, 1, radii)
        if mode is None:
            return color, radii
        depth, alpha = be.depth_forward(rs, int(means3D_c.shape[0]), num_rendered, mode, geom, binning, img)
        return color, radii, depth.unsqueeze(0), alpha.unsqueeze(0)

    @staticmethod
    def backward(ctx, grad_color, _grad_radii, grad_depth=None, grad_alpha=None):
        if grad_color is None and grad_depth is None and grad_alpha is None and ctx.depth_mode is not None:
            return (None,) * 13
        be = get_backend()
        colors_c, means3D_c, scales_c, rots_c, cov_c, radii, sh_c, geom, _binning, _img = ctx.saved_tensors
        want = tuple(ctx.needs_input_grad[8:11])
        cams = []

        def camera_pass(kind, ws):
            cams.append(be.pose_backward(ctx.raster_settings, kind, ctx.num_rendered, means3D_c, radii, sh_c, colors_c, scales_c, rots_c,
                                         cov_c, geom, ws, want=want))
        gaussians = _reverse_passes(ctx, be, grad_color, grad_depth, grad_alpha, camera_pass)
        g_cam = []
        for k, (shape, dtype, device) in enumerate(ctx.cam_like):      # in the input tensors' shapes and dtypes
            parts = [c[k] for c in cams if c[k] is not None]
            if not want[k] or not parts:
                g_cam.append(None)
                continue
            g = parts[0] if len(parts) == 1 else parts[0] + parts[1]
            g_cam.append(g.reshape(shape).to(device=device, dtype=dtype))
        return gaussians + (g_cam[0], g_cam[1], g_cam[2], None, None)


class _RasterizeGaussiansFused(torch.autograd.Function):
    """Fused-step variant: takes the RAW parameters of scene/gaussian_model.py (xyz, features_dc,
    features_rest, opacity logits, log-scales, un-normalised quaternions); the activations (:33-41) and the
    torch.cat of get_features (:108-111) happen inside the per-Gaussian kernels, forward and backward."""

    @staticmethod
    def forward(ctx, means3D, means2D, features_dc, features_rest, opacity_raw, scaling_raw, rotation_raw, raster_settings):
        be = get_backend()
        m3, dc, rest, op, sc, rot = _gaussian_inputs(means3D, (features_dc, features_rest, opacity_raw, scaling_raw, rotation_raw),
                                                     ("features_dc", "features_rest", "opacity", "scaling", "rotation"))
        if dc.dim() != 3 or dc.shape[1] != 1 or rest.dim() != 3 or rest.shape[1] < 1:
            raise _lib.GsrError("features_dc must be [P,1,3] and features_rest [P,M-1,3] with M >= 2")
        empty = m3.new_empty((0,))
        # announce_backward: nothing is announced in the fused form (HipBackend.forward); it only lets a gradient arena set around
        # this call be claimed for this render, so that ONE arena around several renders in flight is refused here as well
        num_rendered, color, radii, geom, binning, img = be.forward(raster_settings, m3, dc, empty, op, sc, rot, empty,
                                                                    shs_rest=rest, raw_params=True, **_announce(ctx, be))
        ctx.raster_settings, ctx.num_rendered = raster_settings, num_rendered
        _keep(ctx, (m3, dc, rest, sc, rot, radii, geom, binning, img), 6, 0, radii)
        return color, radii

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii):
        be = get_backend()
        m3, dc, rest, sc, rot, radii, geom, binning, img = ctx.saved_tensors
        if grad_out_color is None:
            grad_out_color = _zero_colour_grad(ctx.raster_settings, m3.device)
        empty = m3.new_empty((0,))
        g_m3, g_m2, g_dc, _g_col, g_op, g_sc, g_rot, _g_cov, g_rest = be.backward(
            ctx.raster_settings, ctx.num_rendered, grad_out_color, m3, radii, dc, empty, sc, rot, empty, geom, binning, img,
            shs_rest=rest, raw_params=True)
        return g_m3, g_m2, g_dc, g_rest, g_op, g_sc, g_rot, None


def rasterize_gaussians_fused(means3D, means2D, features_dc, features_rest, opacity_raw, scaling_raw, rotation_raw, raster_settings):
    """(color, radii) from the raw Gaussian parameters; gradients flow to the raw parameters.  No camera gradient: the settings'
    viewmatrix, projmatrix and campos are constants here even when they require grad (include/gsr_pose.h has no raw_params form)."""
    return _RasterizeGaussiansFused.apply(means3D, means2D, features_dc, features_rest, opacity_raw, scaling_raw,
                                          rotation_raw, raster_settings)


class _GaussianNormals(torch.autograd.Function):
    """normals [P,3] of (means3D, scales, rotations) under a view matrix (include/gsr_normals.h).  Only `rotations` receives a gradient:
    the choice of the axis and the flip towards the camera are piecewise constant in the scales and the means."""

    @staticmethod
    def forward(ctx, means3D, scales, rotations, viewmatrix):
        be = get_backend()
        if not hasattr(be, "gaussian_normals_forward"):
            raise _lib.GsrError(f"the {getattr(be, 'name', type(be).__name__)} backend computes no Gaussian normals")
        dev = means3D.device
        m, s, r = _f32c(means3D, "means3D", dev), _f32c(scales, "scales", dev), _f32c(rotations, "rotations", dev)
        vm = _f32c(viewmatrix, "viewmatrix", dev)
        normals, axis = be.gaussian_normals_forward(vm, m, s, r)
        ctx.save_for_backward(r, vm, axis)
        return normals

    @staticmethod
    def backward(ctx, grad_normals):
        r, vm, axis = ctx.saved_tensors
        g = get_backend().gaussian_normals_backward(vm, r, axis, grad_normals) if ctx.needs_input_grad[2] else None
        return None, None, g, None


def gaussian_normals(means3D, scales, rotations, raster_settings) -> torch.Tensor:
    """[P,3] float32: per Gaussian, the axis of its smallest scale (ties: the lowest index) as column of the rotation the covariance is
    built from -- the quaternion as given, not normalised --, turned into the view space of raster_settings.viewmatrix and negated
    where it points away from the camera (include/gsr_normals.h).  Passed as `features=` to GaussianRasterizer.forward, or asked for
    with render(normals=True), it blends into the normal map.  Only `rotations` receives a gradient; the viewmatrix is read detached."""
    who = "gaussian_normals"
    for name, t, cols in (("means3D", means3D, 3), ("scales", scales, 3), ("rotations", rotations, 4)):
        _lib.require_tensor(who, name, t)
        if t.dim() != 2 or t.shape[1] != cols or t.shape[0] != means3D.shape[0]:
            raise _lib.GsrError(f"{who}: {name} must have dimensions (num_points, {cols}), got {tuple(t.shape)} "
                                f"for {int(means3D.shape[0]) if means3D.dim() else 0} points")
    vm = raster_settings.viewmatrix
    _lib.require_tensor(who, "viewmatrix", vm)
    if vm.numel() != 16:
        raise _lib.GsrError(f"{who}: viewmatrix must hold 16 values, got shape {tuple(vm.shape)}")
    return _GaussianNormals.apply(means3D, scales, rotations, vm.detach())


class GaussianRasterizer(nn.Module):
    """Constructed per render call by the reference (gaussian_renderer/__init__.py:51): O(us), no allocation."""

    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions: torch.Tensor) -> torch.Tensor:
        with torch.no_grad():
            rs = self.raster_settings
            return get_backend().mark_visible(positions, rs.viewmatrix, rs.projmatrix)

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, depth=None, features=None):
        """depth = None: (color, radii), the reference's call.  depth = "expected" or "inverse": (color, radii, depth, alpha) with
        depth [1,H,W] = sum z alpha T (or sum (1/z) alpha T), not normalised, no background term, and alpha [1,H,W] = 1 - T_final;
        gradients flow from all three images.  When grad mode is on and viewmatrix, projmatrix or campos of the settings requires
        grad, the camera receives gradients as well (_RasterizeGaussiansPose, include/gsr_pose.h); every other call goes where it
        went before.
        features = [P,C] float32 on the device, 1 <= C <= 64 (any strides, leaf or not): feature_map [C,H,W] = sum F[g, c] alpha T over
        the entries the colour pass blended, not normalised, no background term (include/gsr_features.h), is appended to what the
        call returns otherwise -- (color, radii, feature_map) or (color, radii, depth, alpha, feature_map) -- and gradients flow from
        every image to the Gaussians and from the map to `features`.  No camera gradient of the map is formed: camera tensors that
        require grad are refused together with `features`."""
        rs = self.raster_settings
        if depth is not None and depth not in DEPTH_MODES:
            raise _lib.GsrError(f"depth must be None, 'expected' or 'inverse', got {depth!r}")
        if features is not None:
            _lib.require_tensor("GaussianRasterizer", "features", features)
            if features.dim() != 2 or features.shape[0] != means3D.shape[0] or not 1 <= features.shape[1] <= _lib.FEATURES_MAX_C:
                raise _lib.GsrError(f"features must have dimensions (num_points, C) with 1 <= C <= {_lib.FEATURES_MAX_C}, "
                                    f"got {tuple(features.shape)} for {int(means3D.shape[0])} points")
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        empty = means3D.new_empty((0,), dtype=torch.float32)
        shs = empty if shs is None else shs
        colors_precomp = empty if colors_precomp is None else colors_precomp
        scales = empty if scales is None else scales
        rotations = empty if rotations is None else rotations
        cov3D_precomp = empty if cov3D_precomp is None else cov3D_precomp
        cam = (rs.viewmatrix, rs.projmatrix, rs.campos)
        if features is not None:
            if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in cam):
                raise _lib.GsrError("features together with camera tensors that require grad: no camera gradient of the feature map "
                                    "is formed (include/gsr_pose.h) -- detach viewmatrix, projmatrix and campos, or render the features "
                                    "in a call of their own")
            return _RasterizeGaussiansFeatures.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                                     features, rs, None if depth is None else DEPTH_MODES[depth])
        if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in cam):
            return _RasterizeGaussiansPose.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                                 *cam, rs, None if depth is None else DEPTH_MODES[depth])
        if depth is not None:
            return _RasterizeGaussiansDepth.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, rs,
                                                  DEPTH_MODES[depth])
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, rs)
