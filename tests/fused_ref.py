"""float64 restatement of the fused raw-parameter step (rasterize_gaussians_fused: opacity logits, log-scales, un-normalised
quaternions, features_dc / features_rest) on top of the CPU oracle: the activations and their Jacobians are applied here, in
float64 numpy, around oracle/gsr_ref.c, which only knows activated inputs.  No GPU code, no test functions."""
from dataclasses import dataclass

import numpy as np

from gaussian_transformer_amd import synth
from oracle import ref
from tests.helpers import build_report, oracle_scene

NORM_EPS = 1e-12          # F.normalize's clamp, act_normalize4's in gsr_device.h
RAW_KEYS = ("means3D", "means2D", "f_dc", "f_rest", "opacity", "scaling", "rotation")


def activate(logit, log_scale, quat_raw):
    """float64 (o, s, q_hat, |q|) of the raw parameters: sigmoid, exp, q / max(|q|, 1e-12)."""
    x = np.asarray(logit, np.float64).reshape(-1)
    o = 1.0 / (1.0 + np.exp(-x))
    s = np.exp(np.asarray(log_scale, np.float64))
    q = np.asarray(quat_raw, np.float64)
    n = np.sqrt((q * q).sum(axis=1))
    return o, s, q / np.maximum(n, NORM_EPS)[:, None], n


def chain_to_raw(g, x, o, s, q_hat, q_norm, opacity_jacobian=None):
    """Oracle gradients w.r.t. the activated inputs (g: the oracle's dict, dL_dopacity / dL_dscales / dL_drots / dL_dsh ...) ->
    gradients w.r.t. the raw ones, float64, keyed by RAW_KEYS.
      dlogit = dL_dopacity * o * sigma(-x), sigma(-x) evaluated as 1 / (1 + exp(x)) (never as 1 - o, which is gone above x ~ 37);
      dlog_s = dL_dscales * s;
      dq     = (dL_drots - q_hat (q_hat . dL_drots)) / max(|q|, 1e-12), without the projection where |q| < 1e-12 (the clamp is
               active there: q_hat = q * 1e12 is linear in q);
      dL_dsh [P,M,3] -> f_dc = [:, :1], f_rest = [:, 1:].
    opacity_jacobian: replaces o * sigma(-x) (the float32 model's o32 * (1 - o32))."""
    f64 = lambda a: np.asarray(a, np.float64)
    x = f64(x).reshape(-1)
    with np.errstate(over="ignore"):
        jac = f64(o) / (1.0 + np.exp(x)) if opacity_jacobian is None else f64(opacity_jacobian)
    dr = f64(g["dL_drots"])
    proj = np.where(f64(q_norm) < NORM_EPS, 0.0, (f64(q_hat) * dr).sum(axis=1))
    dsh = f64(g["dL_dsh"])
    return dict(means3D=f64(g["dL_dmeans3D"]), means2D=f64(g["dL_dmeans2D"]), f_dc=dsh[:, :1], f_rest=dsh[:, 1:],
                opacity=(f64(g["dL_dopacity"]).reshape(-1) * jac).reshape(-1, 1), scaling=f64(g["dL_dscales"]) * f64(s),
                rotation=(dr - f64(q_hat) * proj[:, None]) / np.maximum(f64(q_norm), NORM_EPS)[:, None])


@dataclass
class RawScene:
    """What the fused entry point is given (float32), around a synth scene that supplies camera, means and SH coefficients."""
    sc: synth.SyntheticScene
    logits: np.ndarray        # [P,1]
    log_scales: np.ndarray    # [P,3]
    quats: np.ndarray         # [P,4], any norm
    scale_modifier: float = 0.9

    @property
    def P(self):
        return self.sc.P


def make_raw_scene(P, width, height, deg, max_deg, s0, seed, logits=(-6.0, 8.0), qnorm=(0.3, 3.0), bg=(0.2, 0.1, 0.4), **kw):
    """synth.make_scene with its opacities / scales / rotations replaced: logits ~ seeded U[a, b], log-scales = log(scales),
    quaternions = the unit rotations rescaled to a seeded log-uniform norm.  Everything finite and moderate."""
    sc = synth.make_scene(P=P, width=width, height=height, sh_degree=deg, s0=s0, seed=seed, max_sh_degree=max_deg, bg=bg, **kw)
    rng = np.random.default_rng(1000 + seed)
    lg = rng.uniform(logits[0], logits[1], (P, 1)).astype(np.float32)
    ls = np.log(sc.scales.astype(np.float64)).astype(np.float32)
    assert float(ls.max(initial=-1e9)) <= 3.0
    n = np.exp(rng.uniform(np.log(qnorm[0]), np.log(qnorm[1]), (P, 1)))
    q = (sc.rotations.astype(np.float64) * n).astype(np.float32)
    return RawScene(sc, lg, ls, q)


def seeded_dL(raw, seed):
    cam = raw.sc.camera
    return np.random.default_rng(seed).normal(size=(3, cam.image_height, cam.image_width)).astype(np.float32)


class FusedOracles:
    """Both oracle precisions on the float64-activated scene, their gradients chained into raw space.  Computed once per scene and
    shared; nothing here is modified afterwards."""

    def __init__(self, raw: RawScene, dL, nthreads=0):
        self.raw = raw
        self.x = raw.logits.astype(np.float64).reshape(-1)
        self.o, self.s, self.q_hat, self.q_norm = activate(raw.logits, raw.log_scales, raw.quats)
        self.S = oracle_scene(raw.sc, opacities=self.o, scales=self.s, rotations=self.q_hat, scale_modifier=raw.scale_modifier)
        r32, r64 = ref.get("f32"), ref.get("f64")
        nt = nthreads or r32.max_threads()
        self.f32 = r32.forward(self.S, nthreads=nt); self.g32 = r32.backward(self.f32, dL, nthreads=nt)
        self.f64 = r64.forward(self.S, nthreads=nt); self.g64 = r64.backward(self.f64, dL, nthreads=nt)
        self.o32 = self.o.astype(np.float32)                 # a float32 evaluation holds o as this, and 1 - o as its complement
        self.raw64 = self.chain(self.g64)
        self.raw32 = self.chain(self.g32, float32_model=True)

    def chain(self, g, float32_model=False):
        jac = self.o32.astype(np.float64) * (1.0 - self.o32.astype(np.float64)) if float32_model else None
        return chain_to_raw(g, self.x, self.o, self.s, self.q_hat, self.q_norm, opacity_jacobian=jac)

    def as_hip(self, grads=None):
        """The float32 oracle's outputs in the shape of a HIP result (`grads`: raw-space gradients, default its own chain)."""
        return dict(color=self.f32["color"], radii=self.f32["radii"], grads=self.raw32 if grads is None else grads)


def radii_check(hip_radii, orc: FusedOracles):
    """In-kernel expf and the host's exp may differ in the last bit of a scale, which can move ceil(3 sigma) by one: no equality
    with the float32 oracle; instead at most 2 * (rows where the two oracle precisions differ) + 2 rows may differ from the float64
    oracle, by at most 1."""
    h = np.asarray(hip_radii).astype(np.int64); r64 = orc.f64["radii"].astype(np.int64); r32 = orc.f32["radii"].astype(np.int64)
    d = np.abs(h - r64)
    out = dict(hip_vs_f64_rows=int((d != 0).sum()), f32_vs_f64_rows=int((r32 != r64).sum()), max_abs=int(d.max(initial=0)))
    out["ok"] = bool(out["hip_vs_f64_rows"] <= 2 * out["f32_vs_f64_rows"] + 2 and out["max_abs"] <= 1)
    return out


def fused_parity_report(orc: FusedOracles, hip):
    """helpers.parity_report for the fused path.  hip: dict(color, radii, grads keyed by RAW_KEYS), all in raw-parameter space.
    Same structure, so helpers.assert_parity applies its bars unchanged; `radii_equal` holds radii_check's verdict (see there)."""
    o = orc
    H = {k: np.asarray(hip["grads"][k], np.float64).reshape(np.asarray(o.raw64[k]).shape) for k in RAW_KEYS}
    H = {k: v for k, v in H.items() if v.size}
    rad = radii_check(hip["radii"], o)
    return build_report(o.S, o.f32, o.f64, hip["color"], H, {k: o.raw32[k] for k in H}, {k: o.raw64[k] for k in H},
                        radii=rad, radii_equal=rad["ok"])
