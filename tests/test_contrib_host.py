"""include/gsr_contrib.h without a device: the header against the ctypes table and the row struct, the refusals that are decided before
the HIP runtime is asked for anything, the collector's own refusals, and the two pruning rules of densify.DensityController
(prune_by_max_weight, prune_by_weight_sum) against hand-made vectors on every controller that inherits them."""
import ctypes as C
import os
import re

import pytest
import torch

from gaussian_transformer_amd import _lib, rasterizer
from gaussian_transformer_amd.densify import (GROUPS, DensityController, FusedDensityController, FusedMCMCController, MCMCController,
                                              MCMCParams)
from gaussian_transformer_amd.model import GaussianParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID = 0, 1
SENTINEL = "gsr_set_option: unknown option 'sentinel'"
BIG = 1 << 40
A = 1 << 20                        # made-up device addresses, only compared, never followed
ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling", "rotation": "_rotation"}


def test_header_declares_exactly_what_the_ctypes_stub_binds():
    header = open(os.path.join(ROOT, "include", "gsr_contrib.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decls = dict(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", code, flags=re.S))
    assert set(decls) == {"gsr_contrib_accumulate", "gsr_contrib_read"} == set(_lib.CONTRIB_SIGNATURES)
    for name, args in decls.items():
        assert len(_lib.CONTRIB_SIGNATURES[name][1]) == len(args.split(",")), name
    others = (_lib.SIGNATURES, _lib.CHAMFER_SIGNATURES, _lib.SEQUENCE_SIGNATURES, _lib.ROWS_SIGNATURES, _lib.DENSITY_SIGNATURES,
              _lib.MCMC_SIGNATURES, _lib.DEPTH_SIGNATURES, _lib.FEATURES_SIGNATURES, _lib.POSE_SIGNATURES)
    assert not any(set(_lib.CONTRIB_SIGNATURES) & set(t) for t in others)
    assert "#define GSR_ABI_VERSION 2" in open(os.path.join(ROOT, "include", "gsr.h")).read()   # purely additive
    assert re.search(r"typedef struct \{ uint64_t sum_q32; uint32_t max_bits; uint32_t count; \} gsr_contrib_row_t;", code)
    low = header.lower()
    assert "raw_params" in low and "deterministic_bwd" in low and "not refused" in low and "2^32 - 1" in low and "does not saturate" in low
    from gaussian_transformer_amd import build
    assert "contrib_stats.hip" in build.SOURCES and "-munsafe-fp-atomics" not in build.SOURCES["contrib_stats.hip"]
    lib = _lib.load()
    for name in decls:
        assert hasattr(lib, name)


def test_row_struct():
    assert C.sizeof(_lib.ContribRow) == _lib.CONTRIB_ROW_BYTES == 16
    assert (_lib.ContribRow.sum_q32.offset, _lib.ContribRow.max_bits.offset, _lib.ContribRow.count.offset) == (0, 8, 12)
    assert _lib.CONTRIB_MAX_PIXELS == 2 ** 32 - 1


def acc(**kw):
    a = dict(P=10, W=32, H=32, R=100, geom=A, geom_n=BIG, binning=2 * A, binning_n=BIG, img=3 * A, img_n=BIG, rows=4 * A)
    a.update(kw)
    return lambda L: L.gsr_contrib_accumulate(None, a["P"], a["W"], a["H"], a["R"], a["geom"], a["geom_n"], a["binning"], a["binning_n"],
                                              a["img"], a["img_n"], a["rows"])


def read(P=10, rows=A, s=2 * A, m=3 * A, n=4 * A):
    return lambda L: L.gsr_contrib_read(None, P, rows, s, m, n)


B, R_ = "gsr_contrib_accumulate: ", "gsr_contrib_read: "
CASES = [
    (acc(P=-1), INVALID, B + "bad sizes"),
    (acc(W=0), INVALID, B + "bad sizes"),
    (acc(H=-3), INVALID, B + "bad sizes"),
    (acc(R=-1), INVALID, B + "bad sizes"),
    (acc(W=65536 * 16), INVALID, B + "image too large"),
    (acc(P=0, rows=None, geom=None), OK, SENTINEL),                         # nothing to do: nothing is looked at
    (acc(R=0, rows=None, img=None, geom_n=0), OK, SENTINEL),
    # (the workspace refusals and the missing pointers come after view_geom, which asks the HIP runtime for two temporary sizes:
    # tests/test_gpu_contrib_cabi.py)
    (acc(W=0, geom_n=0, rows=None), INVALID, B + "bad sizes"),               # two checks broken at once: the earlier one answers
    (read(P=-1), INVALID, R_ + "bad sizes"),
    (read(s=None, m=None, n=None), INVALID, R_ + "weight_sum, weight_max and pixel_count are all NULL"),
    (read(P=0, s=None, m=None, n=None), INVALID, R_ + "weight_sum, weight_max and pixel_count are all NULL"),
    (read(P=0, rows=None), OK, SENTINEL),
    (read(rows=None), INVALID, R_ + "missing rows"),
]


@pytest.mark.parametrize("k", range(len(CASES)), ids=[f"{k:02d}" for k in range(len(CASES))])
def test_return_code_and_message(k):
    call, rc, text = CASES[k]
    lib = _lib.load()
    assert lib.gsr_set_option(b"sentinel", 0) == INVALID and lib.gsr_last_error().decode() == SENTINEL
    got, said = call(lib), lib.gsr_last_error().decode()
    assert got == rc
    assert said == text if isinstance(text, str) else text.fullmatch(said), said


# ---- the collector's own refusals: decided in Python, before the library is called ----
class _Stats(rasterizer.ContributionStats):
    def __init__(self, P):                     # no device here: the rows are never touched by these tests
        self.P, self.device, self.rows, self.views, self.pixels_added = P, torch.device("cpu"), None, 0, 0


def test_collector_refuses_another_P_another_device_and_a_full_count(monkeypatch):
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append(name))
    monkeypatch.setattr(rasterizer, "ptr", lambda t: None)
    st = _Stats(7)
    cpu = torch.device("cpu")
    none = torch.empty(0)
    with pytest.raises(_lib.GsrError, match="holds 7 Gaussians on cpu, the render has 8 on cpu"):
        st._add_view(cpu, None, 8, 4, 4, 1, none, none, none)
    with pytest.raises(_lib.GsrError, match="holds 7 Gaussians on cpu, the render has 7 on meta"):
        st._add_view(torch.device("meta"), None, 7, 4, 4, 1, none, none, none)
    st.pixels_added = 2 ** 32 - 1 - 16
    st._add_view(cpu, None, 7, 4, 4, 1, none, none, none)              # exactly 2^32 - 1: the last view that fits
    assert (st.views, st.pixels_added, calls) == (1, 2 ** 32 - 1, ["gsr_contrib_accumulate"])
    with pytest.raises(_lib.GsrError, match="1 more would pass the 4294967295"):
        st._add_view(cpu, None, 7, 1, 1, 1, none, none, none)
    assert (st.views, st.pixels_added, calls) == (1, 2 ** 32 - 1, ["gsr_contrib_accumulate"])


def test_collector_is_a_context_that_nests_and_restores():
    a, b = _Stats(1), _Stats(2)
    assert rasterizer._contrib_stats is None
    with rasterizer.collect_contribution(a) as got:
        assert got is a and rasterizer._contrib_stats is a
        with rasterizer.collect_contribution(b):
            assert rasterizer._contrib_stats is b
        assert rasterizer._contrib_stats is a
    assert rasterizer._contrib_stats is None


# ---- the pruning rules ----
P_ = 8


def _model(seed=0):
    g = torch.Generator().manual_seed(seed)
    m = GaussianParams(1)
    shapes = {"xyz": (P_, 3), "f_dc": (P_, 1, 3), "f_rest": (P_, 3, 3), "opacity": (P_, 1), "scaling": (P_, 3), "rotation": (P_, 4)}
    for k in GROUPS:
        setattr(m, ATTR[k], torch.randn(shapes[k], generator=g).requires_grad_(True))
    return m


def _controller(kind):
    m = _model()
    if kind in (MCMCController, FusedMCMCController):
        ctl = kind(m, MCMCParams(cap_max=100))
    else:
        ctl = kind(m)
    # one Adam step, so that every row has moments of its own to be pruned with it
    for g in ctl.optimizer.param_groups:
        p = g["params"][0]
        p.grad = torch.arange(p.numel(), dtype=torch.float32).reshape(p.shape) / p.numel() + 0.25
    ctl.optimizer.step()
    return ctl


class _Vectors:
    def __init__(self, w_sum, w_max, n_pix):
        self.v = (torch.tensor(w_sum, dtype=torch.float32), torch.tensor(w_max, dtype=torch.float32), torch.tensor(n_pix, dtype=torch.int32))

    def read(self):
        return self.v


def _snapshot(ctl):
    out = {}
    for g in ctl.optimizer.param_groups:
        p = g["params"][0]
        st = ctl.optimizer.state[p]
        out[g["name"]] = (p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone())
    return out


def _assert_rows_kept(ctl, before, keep):
    keep = torch.tensor(keep)
    for g in ctl.optimizer.param_groups:
        p = g["params"][0]
        assert p is getattr(ctl.model, ATTR[g["name"]]) and p.requires_grad
        st = ctl.optimizer.state[p]
        for got, was in zip((p.detach(), st["exp_avg"], st["exp_avg_sq"]), before[g["name"]]):
            assert torch.equal(got, was[keep]), g["name"]
    m = ctl.model
    assert m.xyz_gradient_accum.shape[0] == m.denom.shape[0] == m.max_radii2D.shape[0] == len(keep)


CONTROLLERS = [DensityController, FusedDensityController, MCMCController, FusedMCMCController]


@pytest.mark.parametrize("kind", CONTROLLERS, ids=[c.__name__ for c in CONTROLLERS])
def test_prune_by_max_weight(kind):
    ctl = _controller(kind)
    before = _snapshot(ctl)
    #            0 kept   1 below  2 never seen  3 at the threshold: kept  4 seen, tiny  5 kept  6 never seen  7 kept
    w_max = [0.5, 0.0099, 0.0, 0.01, 1e-6, 0.99, 0.0, 0.0100001]
    n_pix = [10, 3, 0, 1, 200, 1, 0, 2]
    n = ctl.prune_by_max_weight(_Vectors([1.0] * P_, w_max, n_pix), threshold=0.01)
    assert n == 4
    _assert_rows_kept(ctl, before, [0, 3, 5, 7])


@pytest.mark.parametrize("kind", CONTROLLERS, ids=[c.__name__ for c in CONTROLLERS])
def test_prune_by_max_weight_default_threshold_and_nothing_to_prune(kind):
    ctl = _controller(kind)
    before = _snapshot(ctl)
    assert ctl.prune_by_max_weight(_Vectors([1.0] * P_, [0.011] * P_, [1] * P_)) == 0
    _assert_rows_kept(ctl, before, list(range(P_)))
    assert ctl.prune_by_max_weight(_Vectors([1.0] * P_, [0.009] * P_, [1] * P_)) == P_
    assert ctl.model._xyz.shape[0] == 0


@pytest.mark.parametrize("kind", CONTROLLERS, ids=[c.__name__ for c in CONTROLLERS])
def test_prune_by_weight_sum_ties_go_by_index(kind):
    ctl = _controller(kind)
    before = _snapshot(ctl)
    w_sum = [3.0, 0.0, 2.0, 0.0, 2.0, 5.0, 0.0, 2.0]       # ascending, stable: 1 3 6 | 2 4 7 | 0 | 5
    n = ctl.prune_by_weight_sum(_Vectors(w_sum, [0.5] * P_, [1] * P_), fraction=0.5)
    assert n == 4                                           # the three zeros and, of the three 2.0s, the one with the lowest index
    _assert_rows_kept(ctl, before, [0, 4, 5, 7])


@pytest.mark.parametrize("kind", CONTROLLERS, ids=[c.__name__ for c in CONTROLLERS])
def test_prune_by_weight_sum_fraction_0_and_1_and_volume_power(kind):
    ctl = _controller(kind)
    before = _snapshot(ctl)
    st = _Vectors([float(k + 1) for k in range(P_)], [0.5] * P_, [1] * P_)
    assert ctl.prune_by_weight_sum(st, fraction=0.0) == 0
    _assert_rows_kept(ctl, before, list(range(P_)))
    # volume_power: the score is weight_sum * (product of the activated scales)^power; by hand in float64
    vol = torch.exp(before["scaling"][0].to(torch.float64)).prod(dim=1)
    score = torch.tensor([float(k + 1) for k in range(P_)], dtype=torch.float64) * vol.pow(0.5)
    lowest = set(torch.sort(score, stable=True).indices[:2].tolist())
    assert ctl.prune_by_weight_sum(st, fraction=0.25, volume_power=0.5) == 2
    keep = [k for k in range(P_) if k not in lowest]
    _assert_rows_kept(ctl, before, keep)
    with pytest.raises(ValueError, match="hold 8 Gaussians, the model 6"):
        ctl.prune_by_weight_sum(st, fraction=0.5)
    with pytest.raises(ValueError, match="fraction must lie in"):
        ctl.prune_by_weight_sum(st, fraction=1.5)
    st6 = _Vectors([1.0] * 6, [0.5] * 6, [1] * 6)
    assert ctl.prune_by_weight_sum(st6, fraction=1.0) == 6
    assert ctl.model._xyz.shape[0] == 0 and ctl.model._opacity.shape == (0, 1)
