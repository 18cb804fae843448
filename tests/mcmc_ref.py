"""The MCMC density-control rule of include/gsr_mcmc.h outside torch, and the inputs the MCMC tests share.

`reference` evaluates the rule with Python integers (weights, CDF, draws, histogram, ranks) and the standard library's decimal
at 50 digits (sigmoid, x, D, scaling_new, opacity_new; D in the literal double-sum form of the header).  `assert_state` holds a
controller's result against it: every copied value bit for bit, every moment, the corrected opacity and scaling of the sources
within ONE float32 ulp of the exact value (correct rounding alone gives 0.5 ulp; a float64 evaluation adds about 5e-13 relative).

`build_inputs` draws a cloud with opacity logits in [-12, 12] and CERTIFIES it on the CPU: every alive row's sigmoid * 2^20 keeps
its fractional part at least 1e-6 away from 0.5, so the integer weights cannot differ between two double `exp` implementations,
and no logit lies within 1e-6 of the dead threshold L.  Offenders are moved.  t_j = floor(u_j * total) is one IEEE double
multiply of exactly represented numbers and needs no certificate.
"""
from __future__ import annotations

import bisect
import functools
import math
from decimal import Decimal, getcontext

import numpy as np
import torch

from gaussian_transformer_amd.densify import GROUPS

MIN_OPACITY, N_MAX = 0.005, 51
L = float(np.float32(math.log(MIN_OPACITY / (1.0 - MIN_OPACITY))))
MODES = ("none", "all", "one_alive", "mixed")
PREC = 50


def _sigmoid_dec(v: float) -> Decimal:
    return 1 / (1 + (-Decimal(v)).exp())


def weight(v: float) -> int:
    """floor(sigmoid(v) * 2^20 + 0.5) with the sigmoid at 50 digits."""
    getcontext().prec = PREC
    return int((_sigmoid_dec(v) * (1 << 20) + Decimal("0.5")).to_integral_value(rounding="ROUND_FLOOR"))


def D_exact(x: Decimal, N: int) -> Decimal:
    """sum_{m=1..N} sum_{k=0..m-1} C(m-1, k) (-1)^k x^(k+1) / sqrt(k+1), the header's literal form."""
    getcontext().prec = PREC
    total = Decimal(0)
    pw = [x ** (k + 1) / Decimal(k + 1).sqrt() for k in range(N)]
    for m in range(1, N + 1):
        for k in range(m):
            total += math.comb(m - 1, k) * (-1) ** k * pw[k]
    return total


def correction(logit: float, scaling_row, N: int, m: float = MIN_OPACITY):
    """(opacity_new, [scaling_new] * 3, o, clamped) of one source as float64 roundings of the 50-digit values."""
    getcontext().prec = PREC
    o = _sigmoid_dec(logit)
    x = 1 - ((1 - o).ln() / N).exp()
    D = D_exact(x, N)
    assert D > 0
    shift = (o / D).ln()
    lo, hi = Decimal(m), 1 - Decimal(2) ** -23
    oc = min(max(x, lo), hi)
    return float((oc / (1 - oc)).ln()), [float(Decimal(float(s)) + shift) for s in scaling_row], float(o), oc != x


def reference(d, u, n_grow=None, m: float = MIN_OPACITY, n_max: int = N_MAX):
    """The plan for the inputs d (build_inputs) and the uniforms u (float32 tensor): relocation (n_grow None) or growth by n_grow.
    Returns a dict: dead [P] bool, src (list, one per draw), dests (list), hist [P], counts, source_of [P_new] (the row every row
    of the new state is a copy of), sources (rows with c > 0), exact_opacity / exact_scaling (float64, per source), N, o, clamped."""
    getcontext().prec = PREC
    op = d["par"]["opacity"].reshape(-1).numpy()
    sc = d["par"]["scaling"].numpy()
    P = op.shape[0]
    thr = np.float32(math.log(m / (1.0 - m)))
    dead = op <= thr
    w = [0 if dead[i] else weight(float(op[i])) for i in range(P)]
    cdf, run = [], 0
    for v in w:
        run += v
        cdf.append(run)
    total = run
    dead_rows = [int(i) for i in np.nonzero(dead)[0]]
    n = len(dead_rows) if n_grow is None else n_grow
    dests = dead_rows if n_grow is None else [P + j for j in range(n)]
    un = u.numpy()
    src, hist = [], [0] * P
    if total > 0:
        for j in range(n):
            t = min(int(math.floor(float(np.float64(un[j]) * np.float64(total)))), total - 1)
            i = bisect.bisect_right(cdf, t)                      # the smallest i with C_i > t
            src.append(i)
            hist[i] += 1
    P_new = P if n_grow is None else P + n
    source_of = np.arange(P_new)
    if total > 0:
        source_of[dests] = src
    elif n_grow is not None:
        source_of[P:] = np.arange(n) % P                          # growth with nothing to draw from: plain copies
    sources = [i for i in range(P) if hist[i] > 0]
    ex_op, ex_sc, Ns, os_, clamped = [], [], [], [], []
    for i in sources:
        N = min(hist[i] + 1, n_max)
        a, b, o, c = correction(float(op[i]), sc[i], N, m)
        ex_op.append(a); ex_sc.append(b); Ns.append(N); os_.append(o); clamped.append(c)
    return {"dead": dead, "src": src, "dests": dests, "hist": np.asarray(hist), "source_of": source_of, "sources": np.asarray(sources, dtype=np.int64),
            "exact_opacity": np.asarray(ex_op, dtype=np.float64), "exact_scaling": np.asarray(ex_sc, dtype=np.float64).reshape(-1, 3),
            "N": np.asarray(Ns, dtype=np.int64), "o": np.asarray(os_, dtype=np.float64), "clamped": np.asarray(clamped, dtype=bool),
            "counts": {"n_dead": len(dead_rows), "n_draws": len(src), "n_sources": len(sources), "P_new": P_new}, "total": total}


def ulp32(v):
    """One float32 ulp at the magnitude of the float64 values v."""
    a = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    return 2.0 ** (e - 23)


def assert_state(par, mom, d, ref, label=""):
    """par {group: tensor}, mom {group: (exp_avg, exp_avg_sq)} or None: the state after the change, against the inputs d and the plan
    ref.  Returns the largest error of a corrected opacity / scaling in float32 ulps of the exact value."""
    so = ref["source_of"]
    P_new = so.shape[0]
    rows = np.arange(P_new)
    corrected = ref["hist"][so] > 0
    fresh = (so != rows) | corrected
    worst = 0.0
    for n in GROUPS:
        got = par[n].detach().cpu().numpy().reshape(P_new, -1)
        before = d["par"][n].numpy().reshape(d["par"][n].shape[0], -1)
        if n in ("opacity", "scaling"):
            plain = ~corrected
            assert np.array_equal(got[plain], before[so[plain]]), (label, n, "rows that were not corrected")
            assert np.array_equal(got[corrected], got[so[corrected]]), (label, n, "a copy differs from its source's new value")
            if len(ref["sources"]):
                exact = ref["exact_opacity"].reshape(-1, 1) if n == "opacity" else ref["exact_scaling"]
                err = np.abs(got[ref["sources"]].astype(np.float64) - exact) / ulp32(exact)
                worst = max(worst, float(err.max()))
                assert (err <= 1.0).all(), (label, n, float(err.max()))
        else:
            assert np.array_equal(got, before[so]), (label, n)
        if mom is not None:
            for k in (0, 1):
                gm = mom[n][k].detach().cpu().numpy().reshape(P_new, -1)
                bm = d["mom"][n][k].numpy().reshape(before.shape[0], -1)
                assert not gm[fresh].any(), (label, n, "moments of a source, a destination or an appended row are not zero")
                assert np.array_equal(gm[~fresh], bm[rows[~fresh]]), (label, n, "moments of an untouched row changed")
    return worst


def _uncertified(op64, thr):
    s = 1.0 / (1.0 + np.exp(-op64))
    frac = np.mod(s * float(1 << 20), 1.0)
    return ((np.abs(frac - 0.5) < 1e-6) & (op64 > thr)) | (np.abs(op64 - thr) < 1e-6)


@functools.lru_cache(maxsize=None)
def build_inputs(P: int, rest_width: int, seed: int = 0, mode: str = "mixed"):
    """Float32 CPU inputs, shared and never modified by the tests (they clone).  mode: "none" (no dead row), "all" (every row dead:
    total = 0), "one_alive" (row P // 2 alone is alive), "mixed" (logits uniform in [-12, 12]: about 28 % dead)."""
    assert mode in MODES
    gen = torch.Generator().manual_seed(7000 * P + 10 * rest_width + seed)
    r = lambda *s: torch.rand(*s, generator=gen)
    n = lambda *s: torch.randn(*s, generator=gen)
    lo, hi = np.log(0.004), np.log(1.2)
    par = {"xyz": n(P, 3), "f_dc": n(P, 1, 3), "f_rest": n(P, rest_width, 3), "opacity": -12.0 + 24.0 * r(P, 1),
           "scaling": lo + (hi - lo) * r(P, 3), "rotation": n(P, 4) + 0.1}
    if mode == "none":
        par["opacity"] = (L + 0.5) + (12.0 - L - 0.5) * r(P, 1)
    elif mode in ("all", "one_alive"):
        par["opacity"] = -12.0 + (L - 0.5 + 12.0) * r(P, 1)
        if mode == "one_alive":
            par["opacity"][P // 2] = 3.0
    for _ in range(8):                                           # the certificate: move offenders
        bad = torch.from_numpy(_uncertified(par["opacity"].double().numpy().reshape(-1), L))
        if not bad.any():
            break
        par["opacity"][bad] += 1e-3
    op64 = par["opacity"].double().numpy().reshape(-1)
    assert not _uncertified(op64, L).any(), "a row is still within the margin of a rounding boundary or of L"
    assert op64.min() >= -12.0 and op64.max() <= 12.01
    mom = {k: (0.01 * n(*v.shape), 1e-4 * r(*v.shape)) for k, v in par.items()}
    return {"par": par, "mom": mom}


def clone_inputs(d, device="cpu"):
    t = lambda x: x.detach().clone().to(device=device)
    return {"par": {k: t(v) for k, v in d["par"].items()}, "mom": {k: (t(a), t(b)) for k, (a, b) in d["mom"].items()}}


STEP = 3.0
ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling", "rotation": "_rotation"}


def make_controller(d, cls, cap_max=10 ** 9, moments=True, **kw):
    """A controller of class cls over the (cloned) inputs d, its optimiser state set from them; kw: MCMCParams fields and adam=."""
    from gaussian_transformer_amd.densify import MCMCParams, OptimizationParams
    from gaussian_transformer_amd.model import GaussianParams
    adam = kw.pop("adam", "torch")
    m = GaussianParams(3)
    for k in GROUPS:
        setattr(m, ATTR[k], d["par"][k].requires_grad_(True))
    ctl = cls(m, MCMCParams(cap_max=cap_max, **kw), OptimizationParams(), adam=adam)
    if moments:
        for g in ctl.optimizer.param_groups:
            a, b = d["mom"][g["name"]]
            ctl.optimizer.state[g["params"][0]] = {"step": torch.tensor(STEP), "exp_avg": a, "exp_avg_sq": b}
    return ctl


def state_of(ctl):
    """({group: parameter}, {group: (exp_avg, exp_avg_sq)} or None, {group: step}) of a controller."""
    par, mom, step = {}, {}, {}
    for g in ctl.optimizer.param_groups:
        p = g["params"][0]
        st = ctl.optimizer.state.get(p)
        par[g["name"]] = p
        if st:
            mom[g["name"]] = (st["exp_avg"], st["exp_avg_sq"])
            step[g["name"]] = float(st["step"])
    return par, (mom if mom else None), step


@functools.lru_cache(maxsize=None)
def uniforms(n: int, seed: int = 11) -> torch.Tensor:
    return torch.rand(n, generator=torch.Generator().manual_seed(100 * n + seed), dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def cached_reference(P, rest, mode, grow_n=None, seed=11):
    """reference() for build_inputs(P, rest, mode=mode) and uniforms(P or grow_n, seed), computed once per session."""
    d = build_inputs(P, rest, mode=mode)
    return reference(d, uniforms(P if grow_n is None else grow_n, seed), grow_n)
