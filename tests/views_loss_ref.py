"""Seeded inputs and the references of the multi-view image loss (loss.multi_view_loss, include/gsr_loss.h: gsr_views_loss_*).
Helper, not collected.

The reference is this repository's own loss.l1_loss / loss.ssim (pinned by tests/golden/loss.npz) on the stacked [B,3,H,W] batch,
with torch.nan_to_num / torch.clamp in front, evaluated by torch on the CPU and differentiated by autograd: in float64 (the truth)
and in float32 (the yardstick).  With g the gradients of all views, err = max|g - g64|, the GPU tests assert
    err_hip         <= 2 err_torch32          + 1e-6 max|g64|
    |L_hip - L64|   <= 2 |L_torch32 - L64|    + 4 * 2^-24 |L64|
the bar of tests/test_gpu_loss_edges.py.  Inputs are uniform noise: the window of the kernel and torch's differ in the last place of
their normaliser (tests/test_aux_references.py), which moves SSIM of smooth images by ~1e-5 and of noise by ~1e-7.
"""
import functools

import numpy as np
import torch

from gaussian_transformer_amd import loss

UP = -1.75                      # upstream factor of backward()
U24 = 2.0 ** -24


def reference_weights(B):
    return (0.5 / B, 0.02 / B)


@functools.lru_cache(maxsize=None)
def noise_views(B, H, W, lo, hi, seed):
    """(images, targets): float32 [B,3,H,W], U[lo, hi) and U[0, 1)."""
    rng = np.random.default_rng(seed)
    img = rng.uniform(lo, hi, size=(B, 3, H, W)).astype(np.float32)
    gt = rng.uniform(0.0, 1.0, size=(B, 3, H, W)).astype(np.float32)
    img.setflags(write=False); gt.setflags(write=False)
    return img, gt


def plant(img, gt):
    """Copies with NaN, +inf, -inf, exact 0.0 and exact 1.0 planted in every view of img -- at the image corners, on both sides of the
    tile seams (x, y = 15 | 16) and inside -- and a few non-finite pixels in gt.  Returns (img, gt, {kind: boolean mask over img})."""
    img, gt = img.copy(), gt.copy()
    B, _, H, W = img.shape
    kinds = {"nan": np.nan, "pinf": np.inf, "ninf": -np.inf, "zero": 0.0, "one": 1.0}
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (15, 15), (15, 16), (16, 15), (16, 16), (7, 16), (16, 3), (H // 2, W // 2 + 1),
             (H - 2, 15), (15, W - 2), (3, 5), (20, 21)]
    masks = {k: np.zeros(img.shape, bool) for k in kinds}
    for b in range(B):
        for j, (y, x) in enumerate(spots):
            kind = list(kinds)[(j + b) % len(kinds)]          # every kind meets a corner and a seam in some view, all kinds in every view
            c = (j + 2 * b) % 3
            img[b, c, y, x] = kinds[kind]
            masks[kind][b, c, y, x] = True
        gt[b, b % 3, 15, 16] = np.nan
        gt[b, (b + 1) % 3, 0, W - 1] = np.inf
        gt[b, (b + 2) % 3, H - 1, 3] = -np.inf
    return img, gt, masks


def _sanitised(x, sanitize):
    return torch.clamp(torch.nan_to_num(x), 0.0, 1.0) if sanitize else x


def torch_loss(img, gt, w_l1, w_ssim, sanitize, dtype, up=UP):
    """The restated formula by torch on the CPU in `dtype`.  dict(loss, grad [B,3,H,W] float64 numpy, terms [B,3], psnr [B])."""
    x = torch.tensor(np.asarray(img)).to(dtype).requires_grad_(True)
    y = torch.tensor(np.asarray(gt)).to(dtype)
    sx, sy = _sanitised(x, sanitize), _sanitised(y, sanitize)
    L = w_l1 * loss.l1_loss(sx, sy) + w_ssim * (1.0 - loss.ssim(sx, sy))
    (L * up).backward()
    with torch.no_grad():
        B = x.shape[0]
        terms = torch.stack([(sx - sy).abs().reshape(B, -1).mean(1), loss.ssim(sx, sy, size_average=False),
                             ((sx - sy) ** 2).reshape(B, -1).mean(1)], dim=1)
        psnr = loss.psnr(sx, sy).reshape(B)
    return dict(loss=float(L.detach()), grad=x.grad.numpy().astype(np.float64), terms=terms.numpy().astype(np.float64),
                psnr=psnr.numpy().astype(np.float64))


@functools.lru_cache(maxsize=None)
def _noise_parts64(B, H, W, lo, hi, seed, sanitize):
    """float64 L1 and SSIM of a noise case with their gradients, once per case: every weighting is a linear combination of them."""
    img, gt = noise_views(B, H, W, lo, hi, seed)
    a = torch_loss(img, gt, 1.0, 0.0, sanitize, torch.float64, up=1.0)
    b = torch_loss(img, gt, 0.0, 1.0, sanitize, torch.float64, up=1.0)
    return a["loss"], a["grad"], 1.0 - b["loss"], -b["grad"], a["terms"], a["psnr"]


def noise_reference64(B, H, W, lo, hi, seed, sanitize, w_l1, w_ssim, up=UP):
    l1, g_l1, ssim, g_ssim, terms, psnr = _noise_parts64(B, H, W, lo, hi, seed, sanitize)
    return dict(loss=w_l1 * l1 + w_ssim * (1.0 - ssim), grad=up * (w_l1 * g_l1 - w_ssim * g_ssim), terms=terms, psnr=psnr)


def hip_loss(img, gt, w_l1, w_ssim, sanitize, up=UP, as_list=True, device="cuda"):
    """loss.multi_view_loss on the device.  dict(loss, grad float64 numpy, terms, L (tensor), grads (tensors))."""
    xs = [torch.tensor(np.ascontiguousarray(v), device=device, requires_grad=True) for v in np.asarray(img)]
    ys = [torch.tensor(np.ascontiguousarray(v), device=device) for v in np.asarray(gt)]
    L = loss.multi_view_loss(xs if as_list else torch.stack(xs), ys if as_list else torch.stack(ys), w_l1, w_ssim, sanitize=sanitize)
    (L * up).backward()
    return dict(loss=float(L.detach()), grad=np.stack([x.grad.cpu().numpy() for x in xs]).astype(np.float64),
                terms=L.terms.cpu().numpy().astype(np.float64), L=L.detach(), grads=[x.grad for x in xs], terms_t=L.terms)


def judge(name, hip, t32, r64, where=None):
    """Prints the figures, then asserts the bar on the loss and on the gradient (all views; `where`: only those elements)."""
    g, g32, g64 = hip["grad"], t32["grad"], r64["grad"]
    assert np.isfinite(hip["loss"]) and np.isfinite(g).all(), name
    if where is not None:
        g, g32, g64 = g[where], g32[where], g64[where]
    scale = np.abs(r64["grad"]).max()
    eh, et = np.abs(g - g64).max(), np.abs(g32 - g64).max()
    L64 = r64["loss"]
    dh, dt = abs(hip["loss"] - L64), abs(t32["loss"] - L64)
    print(f"VIEWS_LOSS {name:44s} err_hip={eh / scale:9.3e} err_torch32={et / scale:9.3e} max|g64|={scale:9.3e} abs_hip={eh:9.3e} "
          f"dL_hip={dh / abs(L64):9.3e} dL_torch32={dt / abs(L64):9.3e} L64={L64:.6e}")
    assert scale > 0
    assert dh <= 2 * dt + 4 * U24 * abs(L64), (name, hip["loss"], t32["loss"], L64)
    assert eh <= 2 * et + 1e-6 * scale, (name, eh, et, scale)
    return eh / scale, et / scale
