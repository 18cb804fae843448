"""Several renders in flight before one backward pass: the step builder and the expectations shared by tests/test_gpu_inflight.py
(the HIP library) and tests/test_inflight_host.py (the oracle-backed stand-in).  No test functions.

The trainer's step renders, per camera of the batch, the prediction with gradients and the target without, writes
clamp(nan_to_num(image), 0, 1) into a batch tensor and calls backward once: between a render's forward call and its backward call
the rasterizer sees 2 B - 1 other forward calls and up to B - 1 other backward calls, of scenes with another P, in reverse order.
run_step() restates that order on whatever backend rasterizer.get_backend() returns; the expectations are
  1. expect_parity      -- every render of the step under helpers.assert_parity against the float32 / float64 oracle, unchanged;
  2. expect_bit_equal   -- with the deterministic reverse pass, every gradient equals that render done alone, bit for bit;
  3. expect_shared_sum  -- shared leaves: .grad within (B - 1) * 2^-24 * sum_i |g_i| of the float64 sum of the lone gradients
                           (the roundings of B - 1 float32 additions, in whatever order autograd takes them).
MixedStep is the same step on ONE GaussianParams through render() / render_fused(), judged in raw-parameter space
(expect_raw_parity, and 2 and 3 with keys=RAW)."""
import dataclasses

import numpy as np

from gaussian_transformer_amd import synth
from gaussian_transformer_amd.camera import look_at_camera
from oracle import ref
from tests import fused_ref as fr
from tests.helpers import (assert_image_certified, assert_image_constructive, assert_parity, oracle_runs, oracle_scene,
                           parity_report)

B = 4
W, H = 160, 96
BG = (0.35, 0.3, 0.45)
PRED = dict(P=4001, width=W, height=H, sh_degree=3, s0=0.03, seed=191, bg=BG)      # M = 16, P odd and above the bucketed depth order's minimum
TARGET = dict(P=2500, width=W, height=H, sh_degree=3, s0=0.03, seed=192, bg=BG)
LOGGED = dict(P=1777, width=W, height=H, sh_degree=3, s0=0.04, seed=193, bg=BG)    # the every-fifth-step image logging renders
EYES = ((1.5, 0.0, 0.0), (-2.0, 0.5, 1.0), (0.5, -1.5, -1.0))                      # besides the scene's own camera at the origin
PARAMS = ("means3D", "opacities", "shs", "scales", "rotations")
GRADS = PARAMS + ("means2D",)
RAW = ("means3D", "f_dc", "f_rest", "opacity", "scaling", "rotation")              # the leaves of a GaussianParams (fused_ref.RAW_KEYS without means2D)


def clamp_mask(color):
    """Where clamp(nan_to_num(x), 0, 1) passes a gradient on (torch: min <= x <= max, x finite)."""
    c = np.asarray(color)
    return np.isfinite(c) & (c >= 0.0) & (c <= 1.0)


def _scene(kw, dc_gain):
    sc = synth.make_scene(**kw)
    sc.shs[:, 0, :] *= dc_gain            # colours 0.5 +- 1.4, clamped below at 0: a real share of the pixels leaves [0, 1], a real share stays inside
    return sc


class Fixture:
    """Scenes, cameras, upstream gradients and -- computed once, shared by every case, never modified -- the oracle runs.
    `lone(scene name, i)` renders camera i alone on the backend under test and returns dict(color, radii[, grads]); the clamp
    mask of the prediction renders comes from those images (a forward pass is deterministic: every case asserts that its
    in-flight image has the same mask), and the oracle is fed the masked dL that results."""

    def __init__(self, device):
        self.device = device
        self.scenes = dict(pred=_scene(PRED, 10.0), target=_scene(TARGET, 10.0), logged=_scene(LOGGED, 10.0))
        cam0 = self.scenes["pred"].camera
        self.cams = [cam0] + [look_at_camera(np.array(e), np.array([0.0, 0.0, 6.0]), (0.0, -1.0, 0.0), cam0.FoVx, W, H) for e in EYES]
        assert len(self.cams) == B
        self.dL = np.random.default_rng(1191).normal(size=(B, 3, H, W)).astype(np.float32)
        self.S = {n: [oracle_scene(sc, viewmatrix=c.world_view_transform, projmatrix=c.full_proj_transform, campos=c.camera_center)
                      for c in self.cams] for n, sc in self.scenes.items()}
        self._rs = {}
        self._leaves = {}
        r32 = ref.get("f32")
        nt = r32.max_threads()
        self.fwd32 = {n: [r32.forward(S, nthreads=nt) for S in self.S[n]] for n in ("target", "logged")}
        first = [self.lone("pred", i, backward=False) for i in range(B)]
        self.mask = [clamp_mask(f["color"]) for f in first]
        self.dLm = [(self.dL[i] * self.mask[i]).astype(np.float32) for i in range(B)]
        self.orc = [oracle_runs(self.S["pred"][i], self.dLm[i]) for i in range(B)]
        inside = np.mean([m.mean() for m in self.mask])
        assert 0.05 < inside < 0.95, f"share of pixels inside [0, 1]: {inside}"       # both a clamped and an unclamped share
        # the cameras composite visibly different subsets (the oracle's own radii, before anything is rendered in flight)
        vis = [self.orc[i][0]["radii"] > 0 for i in range(B)]
        for i in range(B):
            for j in range(i + 1, B):
                assert (vis[i] != vis[j]).sum() > 50, (i, j)

    # ---- tensors ------------------------------------------------------------------------------------------------------------
    def t(self, a, grad=False):
        import torch
        return torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=self.device).requires_grad_(grad)

    def leaves(self, name, grad):
        """A fresh set of parameter tensors of scene `name` (same values every time)."""
        sc = self.scenes[name]
        return dict(means3D=self.t(sc.means3D, grad), opacities=self.t(sc.opacities.reshape(sc.P, 1), grad), shs=self.t(sc.shs, grad),
                    scales=self.t(sc.scales, grad), rotations=self.t(sc.rotations, grad))

    def fixed_leaves(self, name):
        """The one set of gradient-free tensors of a scene rendered under no_grad."""
        if name not in self._leaves:
            self._leaves[name] = self.leaves(name, False)
        return self._leaves[name]

    def settings(self, name, i):
        from gaussian_transformer_amd import GaussianRasterizationSettings
        if (name, i) not in self._rs:
            sc, c = self.scenes[name], self.cams[i]
            self._rs[(name, i)] = GaussianRasterizationSettings(H, W, c.tanfovx, c.tanfovy, self.t(sc.bg), 1.0, self.t(c.world_view_transform),
                                                                self.t(c.full_proj_transform), sc.sh_degree, self.t(c.camera_center), False, False)
        return self._rs[(name, i)]

    def render(self, name, i, lv):
        """(color, radii, means2D) of camera i on scene `name` with the parameter tensors lv."""
        import torch
        from gaussian_transformer_amd import GaussianRasterizer
        m2 = torch.zeros((self.scenes[name].P, 3), dtype=torch.float32, device=self.device, requires_grad=lv["means3D"].requires_grad)
        color, radii = GaussianRasterizer(raster_settings=self.settings(name, i))(means2D=m2, **lv)
        return color, radii, m2

    def lone(self, name, i, backward=True):
        """Camera i alone: forward, backward, nothing in between, from a synchronised device."""
        import torch
        if self.device != "cpu":
            torch.cuda.synchronize()
        lv = self.leaves(name, backward)
        color, radii, m2 = self.render(name, i, lv)
        out = dict(color=color.detach().cpu().numpy(), radii=radii.cpu().numpy())
        if backward:
            torch.clamp(torch.nan_to_num(color), 0.0, 1.0).backward(self.t(self.dL[i]))
            out["grads"] = _grads_of(lv, m2)
        return out


def _grads_of(lv, m2):
    g = {k: lv[k].grad.cpu().numpy() for k in PARAMS}
    g["means2D"] = m2.grad.cpu().numpy()
    return g


def _named(gs):
    return {k: g.cpu().numpy() for k, g in zip(GRADS, gs)}


def run_step(fx, shared=False, order="one", target_first=False, after_render=None, middle=None, before_backward=None):
    """One training step in the reference's order on the current backend.
      shared          False: every render gets leaf copies of its own (its gradient lands in its own .grad); True: one set of
                      leaves, accumulated by autograd as in training;
      order           "one": one backward() through the batch tensor (renders in reverse order); "forward": render by render in
                      forward order (torch.autograd.grad per render; shared leaves: backward() per render); "retain": "one" with
                      retain_graph, then render 0 once more through torch.autograd.grad;
      target_first    the target render of a camera before its prediction render (the step then ends with a prediction render)
      after_render(i), middle(), before_backward(live)    hooks: after camera i's two renders / between the forwards and the backward
                      (live: the prediction renders' tensors, dict(lv, m2, color, c, radii) each).
    Returns dict(renders=[dict(color, radii, grads | means2D)], targets=[dict(color, radii)], shared=grads of the shared leaves,
    again=render 0's second gradients, images, gts)."""
    import torch
    dev = fx.device
    images = torch.zeros((B, 3, H, W), dtype=torch.float32, device=dev)
    gts = torch.zeros_like(images)
    tgt = fx.fixed_leaves("target")
    base = fx.leaves("pred", True) if shared else None
    live, targets = [], []

    def target(i):
        with torch.no_grad():
            tc, tr, _ = fx.render("target", i, tgt)
            gts[i] = torch.clamp(torch.nan_to_num(tc), 0.0, 1.0)
        targets.append((tc, tr))

    for i in range(B):
        if target_first:
            target(i)
        lv = base if shared else fx.leaves("pred", True)
        color, radii, m2 = fx.render("pred", i, lv)
        c = torch.clamp(torch.nan_to_num(color), 0.0, 1.0)
        images[i] = c
        live.append(dict(lv=lv, m2=m2, color=color, c=c, radii=radii))
        if not target_first:
            target(i)
        if after_render is not None:
            after_render(i)
    if middle is not None:
        middle()
    dL = fx.t(fx.dL)
    if before_backward is not None:
        before_backward(live)
    per_render = [None] * B
    again = None
    if order in ("one", "retain"):
        (images * dL).sum().backward(retain_graph=(order == "retain"))
        if order == "retain":
            r = live[0]
            again = _named(torch.autograd.grad(r["c"], [r["lv"][k] for k in PARAMS] + [r["m2"]], grad_outputs=dL[0]))
    elif order == "forward":
        for i, r in enumerate(live):
            if shared:
                r["c"].backward(dL[i])
            else:
                per_render[i] = _named(torch.autograd.grad(r["c"], [r["lv"][k] for k in PARAMS] + [r["m2"]], grad_outputs=dL[i]))
    else:
        raise ValueError(order)
    out = dict(renders=[], targets=[dict(color=c.cpu().numpy(), radii=r.cpu().numpy()) for c, r in targets], again=again,
               images=images.detach().cpu().numpy(), gts=gts.cpu().numpy(), shared=None)
    for i, r in enumerate(live):
        d = dict(color=r["color"].detach().cpu().numpy(), radii=r["radii"].cpu().numpy())
        if shared:
            d["means2D"] = r["m2"].grad.cpu().numpy()
        else:
            d["grads"] = per_render[i] if per_render[i] is not None else _grads_of(r["lv"], r["m2"])
        out["renders"].append(d)
    if shared:
        out["shared"] = {k: base[k].grad.cpu().numpy() for k in PARAMS}
    return out


def forward_only(fx, name):
    """B renders of scene `name` under no_grad (the image logging block): [dict(color, radii)]."""
    import torch
    out = []
    with torch.no_grad():
        for i in range(B):
            c, r, _ = fx.render(name, i, fx.fixed_leaves(name))
            out.append((torch.clamp(torch.nan_to_num(c), 0.0, 1.0), c, r))
    return [dict(color=c.cpu().numpy(), radii=r.cpu().numpy()) for _, c, r in out]


class MixedStep:
    """Case F: the step on a GaussianParams (raw leaves: xyz, features_dc / features_rest, opacity logits, log-scales, un-normalised
    quaternions), camera i through render() -- torch's activations and their autograd around the rasterizer -- or through
    render_fused() -- raw-parameter gradients written by the kernels -- as `fns[i]` says ("render" / "fused").  Everything is
    judged in raw-parameter space against the float64 chain of tests/fused_ref.py; the oracle runs are computed once, on the dL
    masked by the clamp of each camera's lone image.
    Logits are U[-6, 4], not fused_ref's U[-6, 8]: render() hands the rasterizer sigmoid(x) rounded to float32 by torch, which may
    sit an ulp (2^-24) from the correctly rounded value the float32 model holds; in o (1 - o) that is 2^-24 / (1 - o) of the row --
    1.8e-4 at x = 8, over the 1e-4 float32-against-float32 bar of assert_parity whatever the rasterizer does (measured on the
    oracle stand-in: p99 1.3e-4), 3.3e-6 at x = 4.  Saturated logits have their own derived bar in tests/test_gpu_fused_parity.py."""

    def __init__(self, device, fns):
        import torch
        from gaussian_transformer_amd.render import TorchCamera
        assert len(fns) == B
        self.device, self.fns = device, tuple(fns)
        raw = fr.make_raw_scene(P=PRED["P"], width=W, height=H, deg=3, max_deg=3, s0=0.03, seed=291, bg=BG, logits=(-6.0, 4.0))
        raw.sc.shs[:, 0, :] *= 10.0                       # as _scene(): a real share of the pixels leaves [0, 1]
        self.raw = raw
        cam0 = raw.sc.camera
        self.cams = [cam0] + [look_at_camera(np.array(e), np.array([0.0, 0.0, 6.0]), (0.0, -1.0, 0.0), cam0.FoVx, W, H) for e in EYES]
        self.tcams = [TorchCamera(c, device) for c in self.cams]
        self.bg = torch.tensor(np.asarray(raw.sc.bg, np.float32), device=device)
        self.dL = np.random.default_rng(1291).normal(size=(B, 3, H, W)).astype(np.float32)
        first = [self.lone(i, backward=False) for i in range(B)]
        self.mask = [clamp_mask(f["color"]) for f in first]
        self.dLm = [(self.dL[i] * self.mask[i]).astype(np.float32) for i in range(B)]
        inside = np.mean([m.mean() for m in self.mask])
        assert 0.05 < inside < 0.95, f"share of pixels inside [0, 1]: {inside}"
        self.orc = [fr.FusedOracles(fr.RawScene(dataclasses.replace(raw.sc, camera=self.cams[i]), raw.logits, raw.log_scales, raw.quats,
                                                raw.scale_modifier), self.dLm[i]) for i in range(B)]

    def t(self, a):
        import torch
        return torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=self.device)

    def params(self):
        """A fresh GaussianParams (same values every time)."""
        from gaussian_transformer_amd.model import GaussianParams
        raw = self.raw
        pc = GaussianParams(3)
        pc._xyz, pc._features_dc, pc._features_rest = self.t(raw.sc.means3D), self.t(raw.sc.shs[:, :1]), self.t(raw.sc.shs[:, 1:])
        pc._opacity, pc._scaling, pc._rotation = self.t(raw.logits), self.t(raw.log_scales), self.t(raw.quats)
        for p in self.leaves(pc).values():
            p.requires_grad_(True)
        return pc

    @staticmethod
    def leaves(pc):
        return dict(means3D=pc._xyz, f_dc=pc._features_dc, f_rest=pc._features_rest, opacity=pc._opacity, scaling=pc._scaling,
                    rotation=pc._rotation)

    def call(self, i, pc):
        from gaussian_transformer_amd.render import PipelineParams, render, render_fused
        fn = dict(render=render, fused=render_fused)[self.fns[i]]
        return fn(self.tcams[i], pc, PipelineParams(), self.bg, self.raw.scale_modifier)

    def _result(self, pc, pkg, own_leaves=True):
        d = dict(color=pkg["render"].detach().cpu().numpy(), radii=pkg["radii"].cpu().numpy())
        if pkg["viewspace_points"].grad is not None:
            d["means2D"] = pkg["viewspace_points"].grad.cpu().numpy()
            if own_leaves:
                d["grads"] = dict({k: p.grad.cpu().numpy() for k, p in self.leaves(pc).items()}, means2D=d["means2D"])
        return d

    def lone(self, i, backward=True):
        """Camera i alone on parameters of its own: forward, backward, nothing in between, from a synchronised device."""
        import torch
        if self.device != "cpu":
            torch.cuda.synchronize()
        pc = self.params()
        if not backward:
            with torch.no_grad():
                return self._result(pc, self.call(i, pc))
        pkg = self.call(i, pc)
        torch.clamp(torch.nan_to_num(pkg["render"]), 0.0, 1.0).backward(self.t(self.dL[i]))
        return self._result(pc, pkg)

    def rotation_sum_bound(self, lones):
        """Per-element bound for the shared `rotation` leaf.  Through render() a render's gradient does not reach that leaf as one
        addend: F.normalize is q / max(|q|, eps), whose backward sends autograd two of them, a_i = g_i / |q| through the numerator
        and b_i = -q_hat (q_hat . g_i) / |q| through the norm (g_i: the rasterizer's dL/dq_hat).  They nearly cancel wherever g_i
        is along q_hat, so |a_i| + |b_i| can exceed |a_i + b_i| without limit and (B - 1) 2^-24 sum |a_i + b_i| does not bound the
        roundings of the additions that actually happen.  With x_j the addends as they arrive (a_i and b_i of every render()
        camera, the one written gradient of every render_fused() camera; n of them), summing them in any order is within
        (n - 1) 2^-24 sum |x_j| of their exact sum, and the lone gradients' own additions fl(a_i + b_i) add at most
        2^-24 sum (|a_i| + |b_i|): n 2^-24 sum_j |x_j| in all.  Were normalize's backward one fused expression (one addend), this
        bound would only be looser.  a_i and b_i are taken from the float64 oracle (within 1e-3 of what the device holds, against
        the bound's 1 / n of slack); every other leaf keeps expect_shared_sum's own bound."""
        tot, n = 0.0, 0
        for i in range(B):
            if self.fns[i] == "fused":
                tot = tot + np.abs(lones[i]["grads"]["rotation"].astype(np.float64)); n += 1
                continue
            o = self.orc[i]
            g = np.asarray(o.g64["dL_drots"], np.float64)
            qn = np.maximum(o.q_norm, fr.NORM_EPS)[:, None]
            tot = tot + np.abs(g / qn) + np.abs(o.q_hat * (o.q_hat * g).sum(axis=1)[:, None] / qn); n += 2
        return n * 2.0 ** -24 * tot

    def step(self, shared):
        """B renders in flight, clamp(nan_to_num(image)) into a batch tensor, one backward.  shared: ONE GaussianParams for all of
        them (as in training) instead of a copy per render.  dict(renders=[dict(color, radii, means2D[, grads])], shared=grads)."""
        import torch
        base = self.params() if shared else None
        images = torch.zeros((B, 3, H, W), dtype=torch.float32, device=self.device)
        live = []
        for i in range(B):
            pc = base if shared else self.params()
            pkg = self.call(i, pc)
            images[i] = torch.clamp(torch.nan_to_num(pkg["render"]), 0.0, 1.0)
            live.append((pc, pkg))
        (images * self.t(self.dL)).sum().backward()
        return dict(renders=[self._result(pc, pkg, own_leaves=not shared) for pc, pkg in live],
                    shared={k: p.grad.cpu().numpy() for k, p in self.leaves(base).items()} if shared else None)


# ---- expectations ----------------------------------------------------------------------------------------------------------------
def expect_parity(fx, i, got, tag=""):
    """Expectation 1: render i of an in-flight step passes the bar a lone render passes (helpers.assert_parity on
    parity_report(S_i, masked dL_i)), and holds exact zeros -- no NaN, nothing stale -- wherever no gradient exists."""
    assert np.array_equal(clamp_mask(got["color"]), fx.mask[i]), f"{tag} render {i}: another set of pixels is clamped than in the lone render"
    for k, v in got["grads"].items():
        assert np.isfinite(v).all(), f"{tag} render {i}: gradient {k} is not finite in {int((~np.isfinite(v)).sum())} elements"
        culled = got["radii"] == 0
        assert np.all(v[culled] == 0), f"{tag} render {i}: gradient {k} of a culled Gaussian is not zero"
    rep = parity_report(fx.S["pred"][i], fx.dLm[i], hip=got, oracles=fx.orc[i])
    for k, g in rep["grads"].items():
        print(f"[{tag} render {i}] {k:9s} vs f64: fail_frac {g['fail_frac']:.2e} p99 {g['p99']:.2e} | f32 oracle vs f64: "
              f"{rep['grads_f32_oracle'][k]['fail_frac']:.2e} {rep['grads_f32_oracle'][k]['p99']:.2e} | vs f32: "
              f"{rep['grads_vs_f32'][k]['fail_frac']:.2e} {rep['grads_vs_f32'][k]['p99']:.2e} maxnorm {rep['grads_maxnorm_vs_f32'][k]:.2e}")
    assert rep["grads"]["means3D"]["rows"] > 200, rep["grads"]["means3D"]
    assert_parity(rep)
    return rep


def expect_raw_parity(mx, i, got, tag=""):
    """Expectation 1 in raw-parameter space: render i of a MixedStep, whichever entry point it went through, under
    helpers.assert_parity against the float64 oracle with the activations and their Jacobians restated in float64
    (fused_ref.fused_parity_report on the masked dL_i; radii as fused_ref.radii_check, since exp is evaluated on the device)."""
    assert np.array_equal(clamp_mask(got["color"]), mx.mask[i]), f"{tag} render {i}: another set of pixels is clamped than in the lone render"
    for k, v in got["grads"].items():
        assert np.isfinite(v).all(), f"{tag} render {i}: gradient {k} is not finite in {int((~np.isfinite(v)).sum())} elements"
        assert np.all(v[got["radii"] == 0] == 0), f"{tag} render {i}: gradient {k} of a culled Gaussian is not zero"
    rep = fr.fused_parity_report(mx.orc[i], got)
    for k, g in rep["grads"].items():
        print(f"[{tag} render {i} {mx.fns[i]}] {k:9s} vs f64: fail_frac {g['fail_frac']:.2e} p99 {g['p99']:.2e} | f32 oracle vs f64: "
              f"{rep['grads_f32_oracle'][k]['fail_frac']:.2e} {rep['grads_f32_oracle'][k]['p99']:.2e} | vs f32: "
              f"{rep['grads_vs_f32'][k]['fail_frac']:.2e} {rep['grads_vs_f32'][k]['p99']:.2e} maxnorm {rep['grads_maxnorm_vs_f32'][k]:.2e}")
    assert rep["radii"]["ok"], (tag, i, rep["radii"])
    assert rep["grads"]["means3D"]["rows"] > 200, rep["grads"]["means3D"]
    assert_parity(rep)
    return rep


def expect_forward_only(fx, name, i, got, tag=""):
    """A gradient-free render interleaved with the others: radii equal to, image certified against, the float32 oracle."""
    f = fx.fwd32[name][i]
    assert np.array_equal(got["radii"], f["radii"]), f"{tag} {name} render {i}: radii differ from the float32 oracle"
    assert_image_certified(got["color"], f["color"], f["state"].decision_margin())
    assert_image_constructive(got["color"], f)


def expect_step_parity(fx, step, tag=""):
    for i in range(B):
        expect_parity(fx, i, step["renders"][i], tag)
        expect_forward_only(fx, "target", i, step["targets"][i], tag)
        assert np.array_equal(step["images"][i], np.clip(step["renders"][i]["color"], 0.0, 1.0)), (tag, i)
        assert np.array_equal(step["gts"][i], np.clip(step["targets"][i]["color"], 0.0, 1.0)), (tag, i)


def expect_bit_equal(lone, got, tag="", keys=PARAMS):
    """Expectation 2 (deterministic reverse pass): image, radii and every gradient tensor equal the lone render's bit for bit."""
    assert np.array_equal(lone["color"], got["color"]), (tag, "image")
    assert np.array_equal(lone["radii"], got["radii"]), (tag, "radii")
    for k in tuple(keys) + ("means2D",):
        a, b = lone["grads"][k], got["grads"][k]
        assert np.array_equal(a, b), (tag, k, int((a != b).sum()), float(np.abs(a.astype(np.float64) - b).max()))
    assert max(float(np.abs(lone["grads"][k]).max()) for k in keys) > 0


def expect_shared_sum(lones, step, tag="", weights=None, keys=PARAMS, bounds=None):
    """Expectation 3: the shared leaves' .grad against the float64 sum of the lone per-render gradients, element by element within
    (n - 1) * 2^-24 * sum_i |g_i| (n addends); each render's own means2D (never shared) bit for bit.
    bounds: {key: per-element bound} for a leaf that a render's gradient does not reach as ONE addend (MixedStep.rotation_sum_bound)."""
    w = [1.0] * len(lones) if weights is None else weights
    n = int(round(sum(w)))
    for k in keys:
        terms = [wi * l["grads"][k].astype(np.float64) for wi, l in zip(w, lones)]
        want = np.sum(terms, axis=0)
        bound = (n - 1) * 2.0 ** -24 * np.sum([np.abs(x) for x in terms], axis=0)
        if bounds is not None and k in bounds:
            bound = np.asarray(bounds[k], np.float64).reshape(want.shape)
        got = step["shared"][k].astype(np.float64)
        assert np.isfinite(got).all(), (tag, k)
        err = np.abs(got - want)
        bad = err > bound
        print(f"[{tag}] shared {k:9s} max err/bound {float((err / np.maximum(bound, 1e-300)).max()):.3f} over {int((bound > 0).sum())} elements")
        assert not bad.any(), (tag, k, int(bad.sum()), float(err[bad].max()), float(bound[bad].min()))
        assert float(np.abs(want).max()) > 0
    for i, l in enumerate(lones):
        assert np.array_equal(step["renders"][i]["means2D"], l["grads"]["means2D"]), (tag, "means2D", i)
