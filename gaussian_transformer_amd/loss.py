"""Image losses that produce dL/dimage for the rasterizer backward.

Restates utils/loss_utils.py:17-63 (l1_loss, ssim: 11x11 Gaussian window sigma 1.5,
C1=0.01^2, C2=0.03^2, zero padding 5, grouped conv) and utils/image_utils.py:17-19 (psnr),
and the training objective of train.py:91-92 with lambda_dssim = 0.2
(arguments/__init__.py:83).  Plain torch ops (MIOpen/rocBLAS on ROCm); SURVEY.md 8a-1 marks
them "reuse torch, do not rewrite".  Pinned by tests/golden/loss.npz.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from . import _lib

LAMBDA_DSSIM = 0.2

_window_cache = {}


def l1_loss(network_output: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    return torch.abs(network_output - gt).mean()


def l2_loss(network_output: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    return ((network_output - gt) ** 2).mean()


def _window(window_size: int, channel: int, like: torch.Tensor) -> torch.Tensor:
    key = (window_size, channel, like.device, like.dtype)
    w = _window_cache.get(key)
    if w is None:
        g = torch.tensor([math.exp(-(x - window_size // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(window_size)])
        g = (g / g.sum()).unsqueeze(1)
        w2 = g.mm(g.t()).float().unsqueeze(0).unsqueeze(0)
        w = w2.expand(channel, 1, window_size, window_size).contiguous().to(device=like.device, dtype=like.dtype)
        _window_cache[key] = w
    return w


def ssim(img1: torch.Tensor, img2: torch.Tensor, window_size: int = 11, size_average: bool = True) -> torch.Tensor:
    channel = img1.size(-3)
    w = _window(window_size, channel, img1)
    pad = window_size // 2
    mu1 = F.conv2d(img1, w, padding=pad, groups=channel)
    mu2 = F.conv2d(img2, w, padding=pad, groups=channel)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = F.conv2d(img1 * img1, w, padding=pad, groups=channel) - mu1_sq
    sigma2_sq = F.conv2d(img2 * img2, w, padding=pad, groups=channel) - mu2_sq
    sigma12 = F.conv2d(img1 * img2, w, padding=pad, groups=channel) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    return ssim_map.mean() if size_average else ssim_map.mean(1).mean(1).mean(1)


def psnr(img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
    mse = ((img1 - img2) ** 2).view(img1.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def training_loss(image: torch.Tensor, gt_image: torch.Tensor, lambda_dssim: float = LAMBDA_DSSIM) -> torch.Tensor:
    """(1-lambda) L1 + lambda (1 - SSIM): train.py:91-92."""
    return (1.0 - lambda_dssim) * l1_loss(image, gt_image) + lambda_dssim * (1.0 - ssim(image, gt_image))


class _FusedL1SSIM(torch.autograd.Function):
    """(1-lambda) L1 + lambda (1-SSIM) in one HIP kernel per direction (include/gsr_loss.h)."""

    @staticmethod
    def forward(ctx, image, gt_image, lambda_dssim):
        dev = image.device
        if dev.type != "cuda":
            raise _lib.GsrError(f"fused_l1_ssim_loss needs tensors on a HIP device, got {dev} (use training_loss for the torch path)")
        if image.dtype != torch.float32 or gt_image.dtype != torch.float32 or image.shape != gt_image.shape or image.dim() != 3:
            raise _lib.GsrError("fused_l1_ssim_loss: image and gt_image must be float32 [C,H,W] tensors of equal shape")
        img = image.contiguous(); gt = gt_image.to(dev).contiguous()
        Cn, H, W = (int(x) for x in img.shape)
        with torch.cuda.device(dev):
            ws = _lib.workspace("gsr_l1_ssim_workspace", dev, Cn, H, W)
            out = torch.empty((3,), dtype=torch.float32, device=dev)
            _lib.call("gsr_l1_ssim_forward", _lib.stream(dev), Cn, H, W, _lib.ptr(img), _lib.ptr(gt), float(lambda_dssim), _lib.ptr(out),
                      _lib.ptr(ws), ws.numel())
        ctx.save_for_backward(img, gt, ws)
        ctx.lambda_dssim = float(lambda_dssim)
        ctx.terms = out
        return out[0]

    @staticmethod
    def backward(ctx, grad_loss):
        img, gt, ws = ctx.saved_tensors
        dev = img.device
        Cn, H, W = (int(x) for x in img.shape)
        with torch.cuda.device(dev):
            g = grad_loss.to(device=dev, dtype=torch.float32).contiguous().reshape(1)
            grad = torch.empty_like(img)
            _lib.call("gsr_l1_ssim_backward", _lib.stream(dev), Cn, H, W, _lib.ptr(img), _lib.ptr(gt), ctx.lambda_dssim, _lib.ptr(g),
                      _lib.ptr(ws), ws.numel(), _lib.ptr(grad))
        return grad, None, None


def fused_l1_ssim_loss(image: torch.Tensor, gt_image: torch.Tensor, lambda_dssim: float = LAMBDA_DSSIM) -> torch.Tensor:
    """Drop-in for training_loss() on a HIP device: same value and gradient w.r.t. `image`
    (gt_image gets no gradient, as in the reference's use at train.py:90-93)."""
    return _FusedL1SSIM.apply(image, gt_image, lambda_dssim)


# ---------------------------------------------------------------- depth-normal consistency ----------------------------------------------------------------
# 2DGS's normal consistency term on the maps of one render (include/gsr_normals.h): the normals the depth map's finite differences
# imply against the rendered normal map, one HIP kernel per direction.

NORMAL_ALPHA_MIN = 0.05


def _normal_maps(who: str, depth, alpha, alpha_min, *normals):
    """depth and alpha as [H,W] (a leading 1 is dropped: the renderer's maps are [1,H,W]), checked together with the [3,H,W] normal
    map where one is given: types, dtypes and shapes first, devices last (a CPU test can check every message)."""
    named = (("depth", depth), ("alpha", alpha)) + tuple(("normals", n) for n in normals)
    for name, t in named:
        _lib.require_tensor(who, name, t)
    d = depth[0] if depth.dim() == 3 and depth.shape[0] == 1 else depth
    a = alpha[0] if alpha.dim() == 3 and alpha.shape[0] == 1 else alpha
    if d.dim() != 2 or d.shape[0] < 1 or d.shape[1] < 1:
        raise _lib.GsrError(f"{who}: depth must have shape [H,W] or [1,H,W], got {tuple(depth.shape)}")
    if a.shape != d.shape:
        raise _lib.GsrError(f"{who}: alpha must have depth's shape {tuple(d.shape)} (or a leading 1), got {tuple(alpha.shape)}")
    for n in normals:
        if tuple(n.shape) != (3,) + tuple(d.shape):
            raise _lib.GsrError(f"{who}: normals must have shape {(3,) + tuple(d.shape)}, got {tuple(n.shape)}")
    if not float(alpha_min) > 0.0:
        raise _lib.GsrError(f"{who}: alpha_min must be positive (D = depth / alpha is formed where alpha >= alpha_min), got {alpha_min}")
    for name, t in named:
        _lib.require_hip(who, name, t)
        if t.device != depth.device:
            raise _lib.GsrError(f"{who}: all maps must be on one device: {name} is on {t.device}, depth on {depth.device}")
    return d, a


class _NormalConsistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, alpha, normals, tanfovx, tanfovy, alpha_min):
        dev = depth.device
        d, a, n = depth.contiguous(), alpha.contiguous(), normals.contiguous()
        H, W = int(d.shape[0]), int(d.shape[1])
        with torch.cuda.device(dev):
            ws = _lib.workspace("gsr_normal_loss_workspace", dev, H, W)
            out = torch.empty((2,), dtype=torch.float32, device=dev)
            _lib.call("gsr_normal_loss_forward", _lib.stream(dev), H, W, tanfovx, tanfovy, alpha_min, _lib.ptr(d), _lib.ptr(a), _lib.ptr(n),
                      _lib.ptr(out), None, _lib.ptr(ws), ws.numel())
        ctx.save_for_backward(d, a, n)
        ctx.cfg = (tanfovx, tanfovy, alpha_min)
        frac = out[1]
        ctx.mark_non_differentiable(frac)
        return out[0], frac

    @staticmethod
    def backward(ctx, grad_loss, _grad_frac):
        d, a, n = ctx.saved_tensors
        dev = d.device
        H, W = int(d.shape[0]), int(d.shape[1])
        need = ctx.needs_input_grad
        with torch.cuda.device(dev):
            g = grad_loss.to(device=dev, dtype=torch.float32).contiguous().reshape(1)
            gd = torch.empty_like(d) if need[0] else None
            ga = torch.empty_like(a) if need[1] else None
            gn = torch.empty_like(n) if need[2] else None
            _lib.call("gsr_normal_loss_backward", _lib.stream(dev), H, W, *ctx.cfg, _lib.ptr(d), _lib.ptr(a), _lib.ptr(n), _lib.ptr(g),
                      _lib.ptr(gd), _lib.ptr(ga), _lib.ptr(gn))
        return gd, ga, gn, None, None, None


def normal_consistency_loss(depth: torch.Tensor, alpha: torch.Tensor, normals: torch.Tensor, tanfovx: float, tanfovy: float,
                            alpha_min: float = NORMAL_ALPHA_MIN) -> torch.Tensor:
    """mean over the image of A (1 - N . n~) at the valid pixels (include/gsr_normals.h): N = `normals` [3,H,W], the rendered normal map
    (render(normals=True)); n~ = the unit normal of the surface the depth map implies, from central differences of the back-projected
    points of D = depth / alpha; A = alpha taken as a constant.  depth, alpha: [H,W] or [1,H,W], the "expected" maps of
    render(depth="expected").  A pixel is valid when it is interior and it and its four neighbours have alpha >= alpha_min.
    Gradients flow to all three maps.  The result carries `.valid_fraction`, a detached scalar tensor.  No CPU fallback."""
    d, a = _normal_maps("normal_consistency_loss", depth, alpha, alpha_min, normals)
    loss, frac = _NormalConsistency.apply(d, a, normals, float(tanfovx), float(tanfovy), float(alpha_min))
    loss.valid_fraction = frac
    return loss


def surface_normals(depth: torch.Tensor, alpha: torch.Tensor, tanfovx: float, tanfovy: float, alpha_min: float = NORMAL_ALPHA_MIN) -> torch.Tensor:
    """[3,H,W]: the unit normals the depth map implies, n~ of normal_consistency_loss, exact zeros at invalid pixels.  No gradients:
    for viewing and for tests."""
    d, a = _normal_maps("surface_normals", depth, alpha, alpha_min)
    dev = d.device
    with torch.no_grad(), torch.cuda.device(dev):
        d, a = d.detach().contiguous(), a.detach().contiguous()
        H, W = int(d.shape[0]), int(d.shape[1])
        surf = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        ws = _lib.workspace("gsr_normal_loss_workspace", dev, H, W)
        out = torch.empty((2,), dtype=torch.float32, device=dev)
        zero_n = torch.zeros((3, H, W), dtype=torch.float32, device=dev)      # the loss against it lands in `out` and is dropped
        _lib.call("gsr_normal_loss_forward", _lib.stream(dev), H, W, float(tanfovx), float(tanfovy), float(alpha_min), _lib.ptr(d), _lib.ptr(a),
                  _lib.ptr(zero_n), _lib.ptr(out), _lib.ptr(surf), _lib.ptr(ws), ws.numel())
    return surf


# ---------------------------------------------------------------- B views in one call ----------------------------------------------------------------
# The image loss of the stacked trainer's step (train_stacked_transformer.py:203-222): B renders and B targets, each sanitised with
# clamp(nan_to_num(.), 0, 1), L1Loss and 1 - ssim over the whole batch, weighted 5.0/B * 0.1 and 0.2/B * 0.1.  One HIP kernel per
# direction over all views (include/gsr_loss.h: gsr_views_loss_*); every view is handed over by pointer, nothing is stacked.

MAX_VIEWS_PER_LAUNCH = 16          # GSR_VIEWS_LOSS_MAX_B: the native call splits a larger B into further launches
STACKED_W_L1 = 5.0 * 0.1           # train_stacked_transformer.py:219-220, each divided by the number of views
STACKED_W_SSIM = 0.2 * 0.1


def _as_view_inputs(who: str, name: str, x):
    """`x` as a list of tensors, each [3,H,W] (one view) or [k,3,H,W] (k views): a sequence of B images or one [B,3,H,W] tensor.
    Types, dtypes and shapes only; returns (tensors, number of views, (H, W))."""
    if isinstance(x, torch.Tensor):
        _lib.require_tensor(who, name, x)
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[0] < 1 or x.shape[2] < 1 or x.shape[3] < 1:
            raise _lib.GsrError(f"{who}: {name} must be a sequence of [3,H,W] tensors or one [B,3,H,W] tensor with B >= 1, got shape {tuple(x.shape)}")
        return [x], int(x.shape[0]), (int(x.shape[2]), int(x.shape[3]))
    if not isinstance(x, (list, tuple)):
        raise _lib.GsrError(f"{who}: {name} must be a sequence of tensors or one [B,3,H,W] tensor, got {type(x).__name__}")
    if len(x) == 0:
        raise _lib.GsrError(f"{who}: {name} is empty (at least one view is needed)")
    for i, t in enumerate(x):
        _lib.require_tensor(who, f"{name}[{i}]", t)
        if t.dim() != 3 or t.shape[0] != 3 or t.shape[1] < 1 or t.shape[2] < 1:
            raise _lib.GsrError(f"{who}: {name}[{i}] must have shape [3,H,W], got {tuple(t.shape)}")
        if tuple(t.shape) != tuple(x[0].shape):
            raise _lib.GsrError(f"{who}: all views must have one size: {name}[{i}] is {tuple(t.shape)}, {name}[0] is {tuple(x[0].shape)}")
    return list(x), len(x), (int(x[0].shape[1]), int(x[0].shape[2]))


def _validate_views(who: str, images, targets):
    """Types, dtypes, shapes, equal view sizes and matching counts first, devices last (a CPU test can check every message)."""
    imgs, B, hw = _as_view_inputs(who, "images", images)
    gts, Bt, hwt = _as_view_inputs(who, "targets", targets)
    if B != Bt:
        raise _lib.GsrError(f"{who}: {B} images but {Bt} targets")
    if hw != hwt:
        raise _lib.GsrError(f"{who}: images are {hw[0]} x {hw[1]} (H x W) but targets are {hwt[0]} x {hwt[1]}")
    for name, ts in (("images", imgs), ("targets", gts)):
        for i, t in enumerate(ts):
            label = f"{name}[{i}]" if t.dim() == 3 else name
            _lib.require_hip(who, label, t)
            if t.device != imgs[0].device:
                raise _lib.GsrError(f"{who}: all views must be on one device: {label} is on {t.device}, the first image on {imgs[0].device}")
    return imgs, gts, B, hw


def _view_pointers(tensors):
    """Device pointers of the views held by `tensors` (contiguous, [3,H,W] or [k,3,H,W] each), in order."""
    ptrs = []
    for t in tensors:
        if t.dim() == 3:
            ptrs.append(_lib.ptr(t))
        else:
            base, step = _lib.ptr(t), t.stride(0) * t.element_size()
            ptrs.extend(base + b * step for b in range(t.shape[0]))
    return ptrs


def _views_forward(imgs, gts, B, hw, w_l1, w_ssim, sanitize):
    """imgs, gts: contiguous tensors on one HIP device.  Returns (out3, terms [B,3], workspace), enqueued on the current stream."""
    dev = imgs[0].device
    with torch.cuda.device(dev):
        ws = _lib.workspace("gsr_views_loss_workspace", dev, B, hw[0], hw[1])
        out = torch.empty((3,), dtype=torch.float32, device=dev)
        terms = torch.empty((B, 3), dtype=torch.float32, device=dev)
        _lib.call("gsr_views_loss_forward", _lib.stream(dev), B, hw[0], hw[1],
                  _lib.ptr_array(_view_pointers(imgs)), _lib.ptr_array(_view_pointers(gts)),
                  float(w_l1), float(w_ssim), 1 if sanitize else 0, _lib.ptr(out), _lib.ptr(terms), _lib.ptr(ws), ws.numel())
    return out, terms, ws


class _MultiViewLoss(torch.autograd.Function):
    """w_l1 L1 + w_ssim (1 - SSIM) over B views in one HIP kernel per direction.  Inputs: n_img image tensors, then the target
    tensors, each [3,H,W] or [k,3,H,W]; one gradient per image tensor that requires grad, written in place by one launch."""

    @staticmethod
    def forward(ctx, w_l1, w_ssim, sanitize, n_img, B, hw, *tensors):
        imgs = [t.contiguous() for t in tensors[:n_img]]
        gts = [t.detach().contiguous() for t in tensors[n_img:]]
        out, terms, ws = _views_forward(imgs, gts, B, hw, w_l1, w_ssim, sanitize)
        ctx.save_for_backward(ws, *imgs, *gts)
        ctx.cfg = (float(w_l1), float(w_ssim), bool(sanitize), n_img, B, hw)
        ctx.terms = terms
        ctx.mark_non_differentiable(terms)
        return out[0], terms

    @staticmethod
    def backward(ctx, grad_loss, _grad_terms):
        w_l1, w_ssim, sanitize, n_img, B, hw = ctx.cfg
        ws, *rest = ctx.saved_tensors
        imgs, gts = rest[:n_img], rest[n_img:]
        dev = imgs[0].device
        with torch.cuda.device(dev):
            g = grad_loss.to(device=dev, dtype=torch.float32).contiguous().reshape(1)
            grads, gptrs = [], []
            for i, t in enumerate(imgs):
                k = 1 if t.dim() == 3 else int(t.shape[0])
                if ctx.needs_input_grad[6 + i]:
                    grads.append(torch.empty_like(t))
                    gptrs.extend(_view_pointers([grads[-1]]))
                else:
                    grads.append(None)
                    gptrs.extend([None] * k)                 # NULL: the kernel stores nothing for this view
            if any(p is not None for p in gptrs):
                _lib.call("gsr_views_loss_backward", _lib.stream(dev), B, hw[0], hw[1],
                          _lib.ptr_array(_view_pointers(imgs)), _lib.ptr_array(_view_pointers(gts)),
                          w_l1, w_ssim, 1 if sanitize else 0, _lib.ptr(g), _lib.ptr(ws), ws.numel(), _lib.ptr_array(gptrs))
        return (None,) * 6 + tuple(grads) + (None,) * len(gts)


def multi_view_loss(images, targets, w_l1: float, w_ssim: float, sanitize: bool = True) -> torch.Tensor:
    """w_l1 * L1 + w_ssim * (1 - SSIM) over B views, both means taken over all B*3*H*W entries (no SSIM window crosses a view).

    images, targets: a sequence of B float32 [3,H,W] tensors or one [B,3,H,W] tensor, all of one size on one HIP device.  With
    `sanitize`, every pixel x of both is read as clamp(nan_to_num(x), 0, 1) and the gradient is exactly 0 where the image's pixel
    is not finite or outside [0, 1], as autograd has it for those torch ops.  Each image that requires grad receives its gradient
    from one launch (targets get none); contiguous inputs are read in place.  The result carries `.terms`: [B,3], detached, per
    view (mean |x-y|, mean SSIM, mean (x-y)^2) of the sanitised images.  Raises GsrError for anything else: no CPU fallback."""
    imgs, gts, B, hw = _validate_views("multi_view_loss", images, targets)
    out, terms = _MultiViewLoss.apply(float(w_l1), float(w_ssim), bool(sanitize), len(imgs), B, hw, *imgs, *gts)
    out.terms = terms
    return out


def stacked_image_loss(images, targets) -> torch.Tensor:
    """The image loss of the reference's stacked trainer for B = len(images) views (train_stacked_transformer.py:203-222):
    0.5/B * L1 + 0.02/B * (1 - SSIM) of the sanitised renders and targets."""
    _, _, B, _ = _validate_views("stacked_image_loss", images, targets)
    return multi_view_loss(images, targets, STACKED_W_L1 / B, STACKED_W_SSIM / B, sanitize=True)


def view_metrics(images, targets, sanitize: bool = False) -> dict:
    """Per-view l1, ssim and psnr ([B] each, as train.py:163-186 reports them) from one forward launch; no graph is recorded."""
    imgs, gts, B, hw = _validate_views("view_metrics", images, targets)
    with torch.no_grad():
        _, terms, _ = _views_forward([t.detach().contiguous() for t in imgs], [t.detach().contiguous() for t in gts], B, hw, 0.0, 0.0, sanitize)
        return {"l1": terms[:, 0], "ssim": terms[:, 1], "psnr": 20 * torch.log10(1.0 / torch.sqrt(terms[:, 2]))}
