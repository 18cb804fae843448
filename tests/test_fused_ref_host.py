"""tests/fused_ref.py on the CPU: its chain rule against torch.autograd in float64, and a mutation check -- the float32 oracle's
gradients pushed through deliberately wrong chains must be rejected by helpers.assert_parity (no library is built or run)."""
import numpy as np
import pytest
import torch

from tests import fused_ref as fr
from tests.helpers import assert_parity

# scene A of tests/test_gpu_fused_parity.py (deg 3)
SCENE_A = dict(P=3001, width=128, height=80, s0=0.04, logits=(-6.0, 8.0), qnorm=(0.3, 3.0))


def _edge_inputs():
    rng = np.random.default_rng(7)
    P = 64
    x = rng.uniform(-6, 8, P); x[:4] = [30.0, -30.0, 16.5, 0.0]
    ls = rng.uniform(-5, 3, (P, 3))
    q = rng.normal(size=(P, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q *= np.exp(rng.uniform(np.log(0.3), np.log(3.0), (P, 1)))
    q[4] *= 1e-3 / np.linalg.norm(q[4]); q[5] *= 1e3 / np.linalg.norm(q[5])
    q[6] = 0.0                                                   # exactly zero: the clamp of F.normalize is active
    return x, ls, q, rng


def test_chain_to_raw_matches_autograd_in_float64():
    """sigmoid / exp / F.normalize feeding a random linear functional: d/d(raw) by autograd = chain_to_raw of the functional's weights."""
    x, ls, q, rng = _edge_inputs()
    P = len(x)
    w = dict(dL_dopacity=rng.normal(size=P), dL_dscales=rng.normal(size=(P, 3)), dL_drots=rng.normal(size=(P, 4)),
             dL_dsh=rng.normal(size=(P, 16, 3)), dL_dmeans3D=rng.normal(size=(P, 3)), dL_dmeans2D=rng.normal(size=(P, 3)))
    tx, tls, tq = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, ls, q))
    tw = {k: torch.tensor(v) for k, v in w.items()}
    L = (torch.sigmoid(tx) * tw["dL_dopacity"]).sum() + (torch.exp(tls) * tw["dL_dscales"]).sum() + \
        (torch.nn.functional.normalize(tq, dim=1) * tw["dL_drots"]).sum()
    L.backward()
    o, s, qh, qn = fr.activate(x, ls, q)
    np.testing.assert_allclose(o, torch.sigmoid(tx).detach().numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(qh, torch.nn.functional.normalize(tq, dim=1).detach().numpy(), rtol=1e-12, atol=0)
    assert qn[6] == 0.0 and np.all(qh[6] == 0.0)
    got = fr.chain_to_raw(w, x, o, s, qh, qn)
    # torch's sigmoid backward is y * (1 - y): once y is rounded to float64, 1 - y carries 2^-53 / (1 - o) of relative error
    # (2e-3 at x = +30), which is the reference's error, not the chain's; every other row is held to 1e-12 of its own magnitude
    bar = {"opacity": 1e-12 + 2.0 * 2.0 ** -53 / (1.0 - o), "scaling": np.full(P, 1e-12), "rotation": np.full(P, 1e-12)}
    assert (bar["opacity"] > 2e-12).sum() <= 2 and bar["opacity"][0] < 3e-3         # only the +30 and +16.5 rows need that allowance
    for name, a, b in (("opacity", got["opacity"].reshape(-1), tx.grad.numpy()), ("scaling", got["scaling"], tls.grad.numpy()),
                       ("rotation", got["rotation"], tq.grad.numpy())):
        a = a.reshape(P, -1); b = b.reshape(P, -1)
        rel = np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), 1e-300)
        assert np.all(rel <= bar[name]), (name, int((rel / bar[name]).argmax()), float((rel / bar[name]).max()))
    # sigma' is even, and autograd is exact to rounding at x = -30 (1 - y = 1): that pins the +30 row to 1e-12 as well
    assert abs(got["opacity"][0, 0] / w["dL_dopacity"][0] - tx.grad[1].item() / w["dL_dopacity"][1]) <= 1e-12 * abs(tx.grad[1].item() / w["dL_dopacity"][1])
    assert abs(got["opacity"][0, 0]) > 0 and abs(got["opacity"][1, 0]) > 0          # logits +-30: sigma(-x) did not collapse to 0
    np.testing.assert_array_equal(got["rotation"][6], w["dL_drots"][6] * 1e12)
    np.testing.assert_array_equal(got["f_dc"], w["dL_dsh"][:, :1]); np.testing.assert_array_equal(got["f_rest"], w["dL_dsh"][:, 1:])
    np.testing.assert_array_equal(got["means3D"], w["dL_dmeans3D"])


@pytest.fixture(scope="module")
def scene_a():
    raw = fr.make_raw_scene(deg=3, max_deg=3, seed=54, **SCENE_A)
    return fr.FusedOracles(raw, fr.seeded_dL(raw, 154))


def _mutations(o):
    """name -> raw-space gradients of the float32 oracle through a wrong chain, and the tensors the mutation touches."""
    g = o.g32
    f64 = lambda a: np.asarray(a, np.float64)
    good = o.raw32
    dr = f64(g["dL_drots"])
    inv = 1.0 / np.maximum(o.q_norm, fr.NORM_EPS)[:, None]
    proj = (o.q_hat * dr).sum(axis=1)[:, None]
    o32 = o.o32.astype(np.float64)
    rolled = np.roll(f64(g["dL_dsh"]), 1, axis=1)
    return {
        "projection_dropped": (dict(good, rotation=dr * inv), ("rotation",)),
        "inverse_norm_dropped": (dict(good, rotation=dr - o.q_hat * proj), ("rotation",)),
        "scale_factor_dropped": (dict(good, scaling=f64(g["dL_dscales"])), ("scaling",)),
        "sigmoid_jacobian_is_o": (dict(good, opacity=(f64(g["dL_dopacity"]).reshape(-1) * o32).reshape(-1, 1)), ("opacity",)),
        "dc_rest_off_by_one_coefficient": (dict(good, f_dc=rolled[:, :1], f_rest=rolled[:, 1:]), ("f_dc", "f_rest")),
    }


def test_bars_accept_the_float32_chain(scene_a):
    rep = fr.fused_parity_report(scene_a, scene_a.as_hip())
    for k in fr.RAW_KEYS:
        print(k, {n: f"{rep['grads_f32_oracle'][k][n]:.2e}" for n in ("fail_frac", "p99")})
    assert rep["radii"]["ok"], rep["radii"]
    assert_parity(rep)


@pytest.mark.parametrize("name", ["projection_dropped", "inverse_norm_dropped", "scale_factor_dropped", "sigmoid_jacobian_is_o",
                                  "dc_rest_off_by_one_coefficient"])
def test_bars_reject_a_wrong_chain(scene_a, name):
    grads, touched = _mutations(scene_a)[name]
    rep = fr.fused_parity_report(scene_a, scene_a.as_hip(grads))
    with pytest.raises(AssertionError):
        assert_parity(rep)
    # ... by the row bars against float64 themselves (not only by the net against the float32 oracle), and at the tensors the mutation touches only
    untouched = dict(rep, **{n: {k: v for k, v in rep[n].items() if k not in touched}
                             for n in ("grads", "grads_f32_oracle", "grads_vs_f32", "grads_maxnorm_vs_f32", "grads_maxnorm_where")})
    assert_parity(untouched)
    for k in touched:
        g, base = rep["grads"][k], rep["grads_f32_oracle"][k]
        assert g["fail_frac"] > 2.0 * base["fail_frac"] + 1e-3, (k, g, base)


def test_radii_check_counts_rows(scene_a):
    r = scene_a.f64["radii"].copy()
    base = fr.radii_check(scene_a.f32["radii"], scene_a)
    assert base["ok"] and base["hip_vs_f64_rows"] == base["f32_vs_f64_rows"]
    vis = np.nonzero(r > 0)[0]
    r2 = r.copy(); r2[vis[0]] += 2
    assert not fr.radii_check(r2, scene_a)["ok"]                                # off by 2 in one row
    r3 = r.copy(); r3[vis[:2 * base["f32_vs_f64_rows"] + 3]] += 1
    assert not fr.radii_check(r3, scene_a)["ok"]                                # off by 1 in too many rows
    r4 = r.copy(); r4[vis[:2]] += 1
    assert fr.radii_check(r4, scene_a)["ok"]
