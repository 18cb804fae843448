"""tests/contrib_ref.py (the reference of the blend-weight statistics, include/gsr_contrib.h) certifies itself on the CPU: the float32
walk against the float64 walk on the six scenes of tests/test_gpu_contrib.py, the sum against an independent route through the oracle's
backward pass, and two planted faults against the gates the device is held to.

Recorded here (float32 against float64 walk, margin helpers.MARGIN_CERT = 2e-4):

    scene      visible  flagged (slack_count > 0)  share    counts differ on
    SCENES[0]        1        0                    0        0
    SCENES[1]       63        0                    0        0
    SCENES[2]      498        2                    0.4 %    0
    SCENES[3]     2981       36                    1.2 %    1
    SCENES[4]     3951      539                   13.6 %    0
    REPLICA        201       16                    8.0 %    0

with no violation of |count32 - count64| <= slack_count or |sum32 - sum64| <= slack_weight + 1e-6 count on any scene.  At a margin of
1e-5 SCENES[3] has one violation (one count off by one), so the margin cannot be that tight.  The condition every later user of the
reference relies on: the share of flagged Gaussians stays <= 20 % on every scene -- the slack is the exception, not the rule.
"""
import dataclasses

import numpy as np
import pytest

from oracle import ref
from tests import contrib_ref as cr
from tests import depth_ref as dr
from tests.helpers import cpu_math_as_recorded
from tests.test_gpu_depth import REPLICA

CONFIGS = dr.SCENES + (REPLICA,)
IDS = [f"P{c[0]}" for c in dr.SCENES] + [REPLICA]
RECORDED = dict(zip(CONFIGS, ((1, 0), (63, 0), (498, 2), (2981, 36), (3951, 539), (201, 16))))      # visible, flagged
MAX_FLAGGED_SHARE = 0.20


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_float32_walk_against_float64_walk(cfg):
    S, a, b = cr.walks(cfg)
    vis = cr.visible(a, b)
    dc, ds = np.abs(a["count"] - b["count"]), np.abs(a["sum"] - b["sum"])
    sl, sw = a["slack_count"], a["slack_weight"]
    flagged = int((vis & (sl > 0)).sum())
    es, em = cr.own_error(a, b)
    print(cfg, "pairs", a["num_rendered"], "visible", int(vis.sum()), "flagged", flagged, "counts differ on", int((dc > 0).sum()),
          "largest count", int(a["count"].max()), "largest sum", float(a["sum"].max()), "clean rel err sum", es, "max", em)
    assert vis.any()
    assert not (dc > sl).any(), np.nonzero(dc > sl)[0][:8]
    assert not (ds > sw + 1e-6 * np.maximum(a["count"], 1)).any()
    assert flagged <= MAX_FLAGGED_SHARE * vis.sum()
    assert es < 5e-5 and em < 5e-5                       # float32 sums of at most a few thousand terms: recorded <= 1.1e-5 and 1.9e-5
    # rows no walk ever blends are empty in every field, and the fields agree with each other
    for w in (a, b):
        none = w["count"] == 0
        assert not w["sum"][none].any() and not w["max"][none].any()
        seen = ~none
        assert (w["max"][seen] > 0).all() and (w["max"][seen] <= w["sum"][seen] * (1 + 1e-12)).all()
        assert (w["sum"][seen] <= w["count"][seen] * w["max"][seen] * (1 + 1e-12)).all()
        assert not w["count"][w["radii"] == 0].any()
    if cpu_math_as_recorded():                           # numpy's float32 exp decides which decisions are borderline
        assert (int(vis.sum()), flagged) == RECORDED[cfg]
    # the float32 walk passes the device's gates against itself
    st = cr.gates(a["sum"], a["max"], a["count"], a, b, cr.rel_of(a, b), opacity=S.opacities)
    assert (st["bad_count"], st["bad_sum"], st["bad_max"]) == (0, 0, 0), st


def test_the_hot_gaussian_of_the_replica_scene():
    _S, a, _b = cr.walks(REPLICA)
    assert int(a["count"][0]) == int(a["count"].max()) > 60000          # recorded: 69 632 pixels, sum 33 215
    assert 3.0e4 < a["sum"][0] < 3.6e4


@pytest.mark.parametrize("cfg", (dr.SCENES[1], dr.SCENES[3], REPLICA), ids=["P64", "P3000", REPLICA])
def test_sum_against_the_oracles_backward_pass(cfg):
    """An independent route to the sum: with colors_precomp = (1, 0, 0), no background and dL = (1, 0, 0) everywhere, the float64
    oracle's dL_dcolors[:, 0] is the sum of alpha T over the pairs it blended."""
    S, _a, b = cr.walks(cfg)
    P = int(np.asarray(S.means3D).shape[0])
    col = np.zeros((P, 3)); col[:, 0] = 1.0
    Sp = dataclasses.replace(S, shs=None, colors_precomp=col, bg=np.zeros(3), sh_degree=0)
    r = ref.get("f64")
    f = r.forward(Sp, nthreads=r.max_threads())
    dL = np.zeros((3, S.H, S.W)); dL[0] = 1.0
    want = np.asarray(r.backward(f, dL, nthreads=r.max_threads())["dL_dcolors"], np.float64)[:, 0]
    assert want.max() > 0
    np.testing.assert_allclose(b["sum"], want, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("fault", ["count_stop", "alpha_only"])
def test_planted_faults_miss_the_gates(fault):
    """SCENES[4]: 2644 pixels stop before the end of their lists."""
    cfg = dr.SCENES[4]
    S, a, b = cr.walks(cfg)
    bad = cr.walk(S, "f32", fault=fault, fwd=a["fwd"])
    st = cr.gates(bad["sum"], bad["max"], bad["count"], a, b, cr.rel_of(a, b), opacity=S.opacities)
    print(fault, st)
    if fault == "count_stop":
        assert st["bad_count"] > 0 and st["bad_sum"] > 0
    else:
        assert st["bad_count"] == 0 and st["bad_sum"] > 0.5 * st["visible"] and st["bad_max"] > 0
