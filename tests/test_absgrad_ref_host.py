"""The absgrad reference (tests/absgrad_ref.py) held against the oracle and against itself, on the CPU.

  * its float64 signed sums are the float64 oracle's dL_dmeans2D[:, :2]: the definition of include/gsr_absgrad.h is the oracle's;
  * abs >= |signed| row by row;
  * its float32 evaluation keeps HALF of the gates the device is held to (helpers.F32_FAIL_FRAC_MAX, F32_P99_MAX) against its float64
    evaluation, so those gates are ones a plain float32 evaluation keeps with a margin;
  * every planted fault misses them on the four scenes with P >= 500.

Observed (fail fraction / p99 of the float32 walk's abs rows against the float64 walk's): P1 0 / 1.5e-7, P64 0 / 3.3e-6, P500 0 / 4.5e-6,
P3000 3.4e-4 / 1.1e-5 (one row of 2981, 4.6e-3 off: one borderline decision), P4000 0 / 5.1e-6, replica 0 / 6.4e-6, large 0 / 2.7e-6,
P500 under the L1 sign pattern 0 / 4.2e-6; float64 signed sums against the float64 oracle: <= 1.5e-15 of the tensor's maximum; medians
of ||abs|| / ||signed||: 1.70, 2.01, 2.94, 2.68, 3.08, 8.89.
"""
import numpy as np
import pytest

from oracle import ref
from tests import absgrad_ref as ar
from tests import depth_ref as dr
from tests.helpers import F32_FAIL_FRAC_MAX, F32_P99_MAX, grad_rows

REPLICA = "replica"
SIX = dr.SCENES + (REPLICA,)
SIX_IDS = [f"P{c[0]}" for c in dr.SCENES] + [REPLICA]
BIG = (dr.SCENES[2], dr.SCENES[3], dr.SCENES[4], ar.LARGE)      # the four scenes with P >= 500
BIG_IDS = ["P500", "P3000", "P4000", "large"]


def misses(st):
    return st["fail_frac"] > 0.5 * F32_FAIL_FRAC_MAX or st["p99"] > 0.5 * F32_P99_MAX


@pytest.mark.parametrize("cfg", SIX, ids=SIX_IDS)
def test_float64_signed_sums_are_the_oracles_means2D_gradient(cfg):
    S, dL, _w32, w64 = ar.walks(cfg)
    r64 = ref.get("f64")
    g = r64.backward(w64["fwd"], dL, nthreads=r64.max_threads())
    want = np.asarray(g["dL_dmeans2D"], np.float64)[:, :2]
    err = np.abs(w64["signed"] - want).max() / max(np.abs(want).max(), 1e-300)
    print(f"{cfg}: signed sums vs float64 oracle, max error / max = {err:.2e}; median ratio {ar.ratio_median(w64['abs'], w64['signed']):.2f}")
    assert err <= 1e-12


@pytest.mark.parametrize("cfg", SIX + (ar.LARGE,), ids=SIX_IDS + ["large"])
def test_abs_dominates_signed_and_float32_keeps_half_the_gates(cfg):
    S, dL, w32, w64 = ar.walks(cfg)
    for w in (w32, w64):
        assert (w["abs"] >= np.abs(w["signed"]) * (1 - 1e-12)).all()
        assert (w["abs"] >= 0).all()
        assert (w["abs"][w["radii"] <= 0] == 0).all()
    st = grad_rows(w32["abs"], w64["abs"])
    print(f"{cfg}: float32 walk vs float64 walk: {st}")
    assert not misses(st), st


def test_the_l1_sign_pattern_keeps_half_the_gates():
    S, dL, w32, w64 = ar.walks(dr.SCENES[2], "l1")
    st = grad_rows(w32["abs"], w64["abs"])
    print(f"l1: {st}")
    assert not misses(st), st
    assert ar.ratio_median(w64["abs"], w64["signed"]) > 1.3


@pytest.mark.parametrize("fault", ar.FAULTS)
@pytest.mark.parametrize("cfg", BIG, ids=BIG_IDS)
def test_planted_faults_miss_the_gates(cfg, fault):
    S, dL, w32, w64 = ar.walks(cfg)
    bad = ar.walk(S, dL, "f32", fault=fault, fwd=w32["fwd"])
    st = grad_rows(bad["abs"], w64["abs"])
    assert misses(st), (fault, st)


def test_absgrad_is_another_statistic_than_the_signed_gradient():
    for cfg in SIX[1:]:
        _S, _dL, _w32, w64 = ar.walks(cfg)
        assert ar.ratio_median(w64["abs"], w64["signed"]) > 1.3, cfg
