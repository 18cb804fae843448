"""Reference for include/gsr_normals.h in torch, parameterised by dtype: float64 is the truth, float32 -- the same statements in the
same order -- the yardstick the GPU tests' tolerances are taken from.  Gradients come from autograd.  Inputs are float32 numbers (the
C ABI's), widened; the two tangents are rounded to float32 first, as the C ABI's `float` arguments are.

Also the inputs the tests share (rows(), maps(), plane()), each a pure function of its arguments, and the two "borderline" measures the
GPU tests rely on being zero for their seeds: rows whose |n_v . p_v| lies below 1e-5 |p_v| (the flip could round either way), pixels whose
alpha lies strictly between alpha_min / 2 and 2 alpha_min or whose stencil has |c|^2 below 1e-24 (validity could round either way).
"""
import numpy as np
import torch

ALPHA_MIN = 0.05
C2_MIN = 1e-30


def _t(a, dtype):
    return a.detach().to(dtype) if isinstance(a, torch.Tensor) else torch.tensor(np.asarray(a), dtype=dtype)


# ---------------------------------------------------------------- per-Gaussian normals ----------------------------------------------------------------
def rot_columns(q):
    """quat_to_rot of csrc/gsr_device.h on (r, x, y, z) as given: [P,3,3] with [:, i, j] = R[i][j]."""
    r, x, y, z = q.unbind(1)
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
            2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
            2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, 1).reshape(-1, 3, 3)


def axis_of(scales):
    """The index of the smallest scale, scanning 0, 1, 2 with strict <, on the float32 numbers themselves."""
    s = np.asarray(scales, np.float32)
    k = np.zeros(len(s), np.int64)
    rows = np.arange(len(s))
    for j in (1, 2):
        k = np.where(s[:, j] < s[rows, k], j, k)
    return k


def gaussian_normals(means3D, scales, rotations, viewmatrix, dtype=torch.float64, rotations_grad=False):
    """dict(normals [P,3], axis [P] (k | flipped << 2), dot [P] = n_v . p_v before the flip, pv [P,3], q = the rotations tensor used
    (requires grad when asked, so that normals can be differentiated))."""
    q = _t(rotations, dtype).requires_grad_(rotations_grad)
    m = _t(viewmatrix, dtype).reshape(16)
    p = _t(means3D, dtype)
    k = torch.tensor(axis_of(scales))
    R = rot_columns(q)
    nw = R[torch.arange(len(k)), :, k] if len(k) else R.new_zeros((0, 3))
    nv = torch.stack([m[i] * nw[:, 0] + m[4 + i] * nw[:, 1] + m[8 + i] * nw[:, 2] for i in range(3)], 1)
    pv = torch.stack([m[i] * p[:, 0] + m[4 + i] * p[:, 1] + m[8 + i] * p[:, 2] + m[12 + i] for i in range(3)], 1)
    dot = nv[:, 0] * pv[:, 0] + nv[:, 1] * pv[:, 1] + nv[:, 2] * pv[:, 2]
    flip = (dot > 0).detach()
    normals = torch.where(flip[:, None], -nv, nv)
    return dict(normals=normals, axis=(k + 4 * flip.to(torch.int64)).numpy().astype(np.int32), dot=dot.detach(), pv=pv.detach(), q=q)


def gaussian_normals_grad(means3D, scales, rotations, viewmatrix, dL_dnormals, dtype=torch.float64):
    """dL/drotations [P,4] of <dL_dnormals, normals> by autograd."""
    g = gaussian_normals(means3D, scales, rotations, viewmatrix, dtype, rotations_grad=True)
    if g["normals"].numel() == 0:
        return torch.zeros((0, 4), dtype=dtype)
    (g["normals"] * _t(dL_dnormals, dtype)).sum().backward()
    return g["q"].grad


def borderline_rows(means3D, scales, rotations, viewmatrix):
    g = gaussian_normals(means3D, scales, rotations, viewmatrix)
    return int((g["dot"].abs() < 1e-5 * g["pv"].norm(dim=1)).sum())


def rows(P, seed=0):
    """P Gaussians in front of a camera that is rotated and shifted: (means3D, scales, rotations (unit), viewmatrix [4,4] in gsr.h's
    layout, i.e. x_view = x_world @ V[:3,:3] + V[3,:3])."""
    rng = np.random.default_rng(300 + seed)
    means = rng.uniform(-2.0, 2.0, size=(P, 3)).astype(np.float32)
    scales = np.exp(rng.uniform(-4.0, 0.0, size=(P, 3))).astype(np.float32)
    q = rng.normal(size=(P, 4))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    a, b = 0.4, -0.3
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    V = np.eye(4)
    V[:3, :3] = (Rx @ Ry).T
    V[3, :3] = (0.3, -0.2, 5.0)
    return means, scales, q, V.astype(np.float32)


# ---------------------------------------------------------------- depth to normals, and the loss ----------------------------------------------------------------
def _rays(H, W, tanfovx, tanfovy, dtype, device=None):
    tx, ty = float(np.float32(tanfovx)), float(np.float32(tanfovy))
    xs = ((2 * torch.arange(W, dtype=dtype, device=device) + 1) / W - 1) * tx
    ys = ((2 * torch.arange(H, dtype=dtype, device=device) + 1) / H - 1) * ty
    return xs, ys


def surface(depth, alpha, tanfovx, tanfovy, alpha_min=ALPHA_MIN, dtype=torch.float64):
    """(n~ [3,H,W], valid [H,W] bool, |c|^2 [H,W] (0 outside the interior)) from tensors of `dtype` (depth and alpha may require grad),
    on the device they are on (scripts/normals_bench.py times the float32 form on the card)."""
    H, W = depth.shape
    dev = depth.device
    ok = alpha.detach().to(torch.float32) >= torch.tensor(alpha_min, dtype=torch.float32, device=dev)
    D = torch.where(ok, depth / torch.where(ok, alpha, torch.ones_like(alpha)), torch.zeros_like(depth))
    n = torch.zeros((3, H, W), dtype=dtype, device=dev)
    valid = torch.zeros((H, W), dtype=torch.bool, device=dev)
    c2 = torch.zeros((H, W), dtype=dtype, device=dev)
    if H < 3 or W < 3:
        return n, valid, c2
    xs, ys = _rays(H, W, tanfovx, tanfovy, dtype, dev)
    Q = torch.stack([D * xs[None, :], D * ys[:, None], D])
    a = Q[:, 2:, 1:-1] - Q[:, :-2, 1:-1]
    b = Q[:, 1:-1, 2:] - Q[:, 1:-1, :-2]
    c = torch.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
    n2 = (c * c).sum(0)
    v = ok[1:-1, 1:-1] & ok[2:, 1:-1] & ok[:-2, 1:-1] & ok[1:-1, 2:] & ok[1:-1, :-2] & (n2.detach() > C2_MIN)
    unit = c / torch.sqrt(torch.where(v, n2, torch.ones_like(n2)))
    n = torch.nn.functional.pad(torch.where(v, unit, torch.zeros_like(unit)), (1, 1, 1, 1))
    valid[1:-1, 1:-1] = v
    c2[1:-1, 1:-1] = n2.detach()
    return n, valid, c2


def loss(depth, alpha, normals, tanfovx, tanfovy, alpha_min=ALPHA_MIN, dtype=torch.float64, grad=True):
    """dict(loss, fraction, surf, valid and, with grad, g_depth, g_alpha, g_normals) of the consistency term, all of `dtype`."""
    d, a, N = (_t(x, dtype).requires_grad_(grad) for x in (depth, alpha, normals))
    H, W = d.shape
    n, valid, c2 = surface(d, a, tanfovx, tanfovy, alpha_min, dtype)
    terms = torch.where(valid, a.detach() * (1 - (N * n).sum(0)), torch.zeros_like(d))
    L = terms.sum() / (H * W)
    out = dict(loss=L.detach(), fraction=float(valid.sum()) / (H * W), surf=n.detach(), valid=valid, c2=c2)
    if grad:
        if valid.any():
            L.backward()
        for name, t in (("g_depth", d), ("g_alpha", a), ("g_normals", N)):
            out[name] = torch.zeros_like(t) if t.grad is None else t.grad
    return out


def borderline_pixels(depth, alpha, tanfovx, tanfovy, alpha_min=ALPHA_MIN):
    a = _t(alpha, torch.float64)
    _n, valid, c2 = surface(_t(depth, torch.float64), a, tanfovx, tanfovy, alpha_min)
    between = (a > alpha_min / 2) & (a < 2 * alpha_min)
    return int(between.sum()) + int((valid & (c2 < 1e-24)).sum())


TANFOV = (0.7, 0.45)


def maps(H, W, seed=0, holes=True, alpha_min=ALPHA_MIN):
    """(depth, alpha, normals) float32: D = a tilted plane plus a low sinusoid, with noise of 1e-3 of the depth; alpha in [0.3, 1] with
    rectangular holes of alpha <= alpha_min / 2 (so no pixel's validity depends on rounding); depth = D alpha, as the renderer's
    "expected" map is; normals = alpha times a perturbed unit field."""
    rng = np.random.default_rng(7000 + 97 * H + W + 10007 * seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    u, v = (x + 0.5) / max(W, 1), (y + 0.5) / max(H, 1)
    D = 4.0 + 1.5 * u - 1.0 * v + 0.05 * np.sin(5.0 * u + 1.0) * np.cos(4.0 * v)
    D = D * (1.0 + 1e-3 * rng.uniform(-1.0, 1.0, size=(H, W)))
    alpha = rng.uniform(0.3, 1.0, size=(H, W))
    if holes and H >= 3 and W >= 3:
        for _ in range(1 + (H * W) // 600):
            hh, hw = int(rng.integers(1, max(2, H // 4 + 1))), int(rng.integers(1, max(2, W // 4 + 1)))
            y0, x0 = int(rng.integers(0, H - hh + 1)), int(rng.integers(0, W - hw + 1))
            alpha[y0:y0 + hh, x0:x0 + hw] = rng.uniform(0.0, alpha_min / 2, size=(hh, hw))
    alpha = alpha.astype(np.float32)
    depth = (D * alpha).astype(np.float32)
    n = rng.normal(size=(3, H, W)) * 0.3 + np.array([0.1, -0.2, -1.0])[:, None, None]
    n = n / np.linalg.norm(n, axis=0, keepdims=True)
    return depth, alpha, (n * alpha).astype(np.float32)


def plane(H, W, normal=(0.3, -0.2, -0.93), offset=-4.0, seed=0, dtype=np.float64):
    """The plane n . Q = offset seen through TANFOV: (depth, alpha, normals = A n, unit n [3]) with D = offset / (n . ray), alpha = A
    uniform in [0.3, 1]; `dtype` float64 keeps D exact to rounding, float32 gives the C ABI's inputs."""
    n = np.asarray(normal, np.float64)
    n = n / np.linalg.norm(n)
    xs, ys = _rays(H, W, *TANFOV, torch.float64)
    ray = np.stack(np.broadcast_arrays(xs.numpy()[None, :], ys.numpy()[:, None], np.ones((H, W))))
    D = offset / np.tensordot(n, ray, axes=1)
    assert (D > 0).all()
    A = np.random.default_rng(50 + seed).uniform(0.3, 1.0, size=(H, W))
    A = A.astype(np.float32).astype(np.float64)
    return (D * A).astype(dtype), A.astype(dtype), (A[None] * n[:, None, None]).astype(dtype), n
