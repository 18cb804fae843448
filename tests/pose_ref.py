"""Reference for the camera gradients (include/gsr_pose.h): dL/dviewmatrix, dL/dprojmatrix, dL/dcampos for any P, no pixel loop.

The C oracle (oracle/gsr_ref.c) differentiates a render with respect to what the camera reaches a Gaussian through: its NDC centre
(dL_dmeans2D), its conic (dL_dconic) and its colour (dL_dcolors).  With those per-Gaussian gradients g held constant, the surrogate

    S(V, Pm, c) = sum_i <g.ndc_i, ndc_i(Pm)> + f_i <g.conic_i, conic_i(V)> + <g.col_i, rgb_i(c)>  [+ <dL/dv_i, v_i(V)> for the maps]

has the loss's own gradient with respect to the three camera tensors, and autograd of S -- written in torch with oracle/dense_ref.py's
conventions: the coordinate clamped at 1.3 tanfov is a constant, a colour channel clamped at 0 passes nothing -- gives it in float64
or float32, according to the oracle library that made g.  f_i = det^2 / (det^2 + 1e-7), a constant per Gaussian, restates S11's
1 / (det^2 + 1e-7), which the oracle and the kernels use where the exact inverse has 1 / det^2 (dense_ref.py leaves it out: its
autograd differs by <= 1.3e-5 relative, which the comparison with it allows for, as tests/test_oracle_grad.py does).
Discrete decisions are constants: only Gaussians with radii > 0 enter, under the oracle's clamp masks.

Planted faults (`fault`), each a way an implementation of the camera gradient could be wrong:
    "no_W"        the path through T = J Wm is dropped (only t = Wm p + translation carries the view matrix)
    "no_masks"    the clamp masks are ignored: the clamped coordinate and the clamped colour channels pass their gradient
    "campos_sign" dL/dcampos with the sign of dL/dmeans3D's view-direction term
    "no_dvdz"     maps: the depth value's own dependence on the view matrix is dropped
"""
import numpy as np
import torch

from oracle import dense_ref, ref
from tests import depth_ref

def _dtype(precision):
    return torch.float32 if precision == "f32" else torch.float64


def surrogate_grads(*a, **kw):
    with torch.enable_grad():           # also from inside an autograd Function's backward (tests/pose_backend.py)
        return _surrogate_grads(*a, **kw)


def _surrogate_grads(S, radii, g_ndc, g_conic, g_col=None, clamped=None, dv=None, mode=None, precision="f64", fault=None, eps_form=True):
    """autograd.grad of S.  S: ref.Scene; radii [P]; g_ndc [P,>=2] (oracle dL_dmeans2D), g_conic [P,4] (oracle dL_dconic: xx, xy halved,
    -, yy), g_col [P,3] or None, clamped [P,3] (SH only), dv [P] = dL/dv for the maps (mode "expected" / "inverse").
    Returns dict(viewmatrix[16], projmatrix[16], campos[3]) as float64 numpy."""
    dt = _dtype(precision)
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=dt)
    keep = np.nonzero(np.asarray(radii) > 0)[0]
    V = t(np.asarray(S.viewmatrix).reshape(4, 4)).requires_grad_(True)
    Pm = t(np.asarray(S.projmatrix).reshape(4, 4)).requires_grad_(True)
    cp = t(np.asarray(S.campos).reshape(3)).requires_grad_(True)
    zero = dict(viewmatrix=np.zeros(16), projmatrix=np.zeros(16), campos=np.zeros(3))
    if keep.size == 0:
        return zero
    p = t(np.asarray(S.means3D).reshape(-1, 3)[keep])
    n = p.shape[0]
    hom = torch.cat([p, torch.ones(n, 1, dtype=dt)], 1)
    ph = hom @ Pm
    pv = (hom @ V)[:, :3]
    pw = 1.0 / (ph[:, 3] + 1e-7)
    ndc = ph[:, :2] * pw[:, None]
    total = (t(np.asarray(g_ndc)[keep, :2]) * ndc).sum()

    if S.cov3D_precomp is not None:
        c6 = t(np.asarray(S.cov3D_precomp).reshape(-1, 6)[keep])
        Sig = torch.stack([c6[:, 0], c6[:, 1], c6[:, 2], c6[:, 1], c6[:, 3], c6[:, 4], c6[:, 2], c6[:, 4], c6[:, 5]], 1).view(n, 3, 3)
    else:
        Rm = dense_ref._rot(t(np.asarray(S.rotations).reshape(-1, 4)[keep]))
        Mm = Rm * (float(S.scale_modifier) * t(np.asarray(S.scales).reshape(-1, 3)[keep]))[:, None, :]
        Sig = Mm @ Mm.transpose(1, 2)
    W, H = int(S.W), int(S.H)
    fx, fy = W / (2.0 * S.tanfovx), H / (2.0 * S.tanfovy)
    limx, limy = 1.3 * S.tanfovx, 1.3 * S.tanfovy
    tz = pv[:, 2]
    txtz, tytz = pv[:, 0] / tz, pv[:, 1] / tz
    clx = (txtz < -limx) | (txtz > limx); cly = (tytz < -limy) | (tytz > limy)
    cx, cy = txtz.clamp(-limx, limx) * tz, tytz.clamp(-limy, limy) * tz
    if fault != "no_masks":
        cx, cy = cx.detach(), cy.detach()
    tx = torch.where(clx, cx, pv[:, 0]); ty = torch.where(cly, cy, pv[:, 1])
    z0 = torch.zeros_like(tz)
    J = torch.stack([fx / tz, z0, -fx * tx / tz ** 2, z0, fy / tz, -fy * ty / tz ** 2], 1).view(n, 2, 3)
    Wm = V[:3, :3].t()
    Tm = J @ (Wm.detach() if fault == "no_W" else Wm)
    cov2 = Tm @ Sig @ Tm.transpose(1, 2)
    a = cov2[:, 0, 0] + 0.3; b = cov2[:, 0, 1]; c = cov2[:, 1, 1] + 0.3
    det = a * c - b * b
    gc = t(np.asarray(g_conic)[keep])
    conic_term = gc[:, 0] * (c / det) + 2.0 * gc[:, 1] * (-b / det) + gc[:, 3] * (a / det)
    f = (det * det / (det * det + 1e-7)).detach() if eps_form else 1.0
    total = total + (f * conic_term).sum()

    if g_col is not None and S.shs is not None:
        d = p - cp[None, :]
        d = d / d.norm(dim=1, keepdim=True)
        raw = dense_ref._sh_color(int(S.sh_degree), t(np.asarray(S.shs)[keep]), d) + 0.5
        if fault != "no_masks":
            raw = torch.where(torch.tensor(np.asarray(clamped)[keep].astype(bool)), raw.detach(), raw)
        total = total + (t(np.asarray(g_col)[keep]) * raw).sum()
    if dv is not None and fault != "no_dvdz":
        v = tz if mode == "expected" else 1.0 / tz
        total = total + (t(np.asarray(dv)[keep]) * v).sum()
    gV, gP, gC = torch.autograd.grad(total, (V, Pm, cp), allow_unused=True)
    out = dict(viewmatrix=np.zeros(16) if gV is None else gV.double().numpy().reshape(16),
               projmatrix=np.zeros(16) if gP is None else gP.double().numpy().reshape(16),
               campos=np.zeros(3) if gC is None else gC.double().numpy().reshape(3))
    if fault == "campos_sign":
        out["campos"] = -out["campos"]
    return out


def colour_grads(S, dL_dpix, precision="f64", fault=None, eps_form=True, nthreads=0):
    """Camera gradients of <dL_dpix, colour image of S> and the oracle's own gradient dict (dL_dmeans3D for the translation identity)."""
    r = ref.get(precision)
    nt = nthreads or r.max_threads()
    f = r.forward(S, nthreads=nt)
    g = r.backward(f, np.asarray(dL_dpix, np.float64), nthreads=nt)
    out = surrogate_grads(S, f["radii"], g["dL_dmeans2D"], g["dL_dconic"], g["dL_dcolors"], f["state"].geom()["clamped"],
                          precision=precision, fault=fault, eps_form=eps_form)
    out["oracle"] = g
    return out


def map_grads(S, mode, gD, gA, precision="f64", fault=None, eps_form=True):
    """Camera gradients of <gD, depth> + <gA, alpha> (gD / gA [H,W] or None) through tests/depth_ref.py's trick scene: its colour
    gradient's first channel is dL/dv."""
    t = depth_ref.trick_forward(S, mode, precision=precision)
    g = depth_ref.trick_backward(t, S, mode, gD, gA, precision=precision)
    out = surrogate_grads(S, t["radii"], g["dL_dmeans2D"], g["dL_dconic"], dv=g["dL_dv"], mode=mode, precision=precision, fault=fault,
                          eps_form=eps_form)
    out["oracle"] = g
    return out


def beyond_clamp(sc, every=4, factor=1.5):
    """(means3D, scales) of the synthetic scene `sc` with every `every`-th Gaussian moved beyond the 1.3 tanfov clamp (alternately in x
    and y, to `factor` tanfov) and made wide enough to still reach into the image: S11's clamped coordinate is then a constant."""
    m = np.asarray(sc.means3D, np.float64).copy(); s = np.asarray(sc.scales, np.float64).copy()
    cam = sc.camera
    for n, i in enumerate(range(0, len(m), every)):
        z = m[i, 2]
        ax, tan = (0, cam.tanfovx) if n % 2 == 0 else (1, cam.tanfovy)
        m[i, ax] = (1 if n % 4 < 2 else -1) * factor * tan * z
        s[i] = 0.3 * tan * z
    return m, s


def add(*gs):
    return {k: sum(np.asarray(g[k], np.float64) for g in gs) for k in ("viewmatrix", "projmatrix", "campos")}


def rel_err(a, b):
    """Error of a tensor judged relative to the largest absolute entry of the reference b (0 where b is all zero and a too)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    s = np.abs(b).max()
    return float(np.abs(a - b).max() / s) if s > 0 else float(np.abs(a).max())


def translation_identity(S, cam, dL_dmeans3D):
    """(lhs[3], rhs[3]) of  sum_i dL/dmeans3D_i[j] = sum_r V[4j+r] dV[12+r] + sum_c Pm[4j+c] dPm[12+c] - dcampos[j]:
    moving every Gaussian by delta is moving the camera by -delta."""
    V = np.asarray(S.viewmatrix, np.float64).reshape(16); Pm = np.asarray(S.projmatrix, np.float64).reshape(16)
    dV, dPm, dC = (np.asarray(cam[k], np.float64) for k in ("viewmatrix", "projmatrix", "campos"))
    lhs = np.asarray(dL_dmeans3D, np.float64).reshape(-1, 3).sum(0)
    rhs = np.array([sum(V[4 * j + r] * dV[12 + r] for r in range(4)) + sum(Pm[4 * j + c] * dPm[12 + c] for c in range(4)) - dC[j]
                    for j in range(3)])
    return lhs, rhs
