"""The visibility-masked Adam step (include/gsr_optim.h: gsr_adam_step_masked) restated twice, for the tests to measure against.

SparseAdam64: float64, numpy.  oracle.aux_ref.adam_step applied to the visible rows only; the step count is one per tensor and
advances on every call, whatever the mask holds.

TorchMaskedAdam: torch's own arithmetic in the dtype and on the device asked for.  One dense torch.optim.Adam step, then the invisible
rows of param, exp_avg and exp_avg_sq put back.  In float32 on the GPU this is the yardstick one float32 evaluation is held against;
in float64 on the CPU it must agree with SparseAdam64 (tests/test_sparse_adam_host.py).
"""
import numpy as np
import torch

from oracle import aux_ref


class SparseAdam64:
    """State of one [P, w] tensor in float64."""

    def __init__(self, param, exp_avg=None, exp_avg_sq=None, step=0):
        self.p = np.array(param, dtype=np.float64)
        assert self.p.ndim >= 1
        self.m = np.zeros_like(self.p) if exp_avg is None else np.array(exp_avg, dtype=np.float64).reshape(self.p.shape)
        self.v = np.zeros_like(self.p) if exp_avg_sq is None else np.array(exp_avg_sq, dtype=np.float64).reshape(self.p.shape)
        self.step = int(step)

    def update(self, grad, mask, lr, betas=(0.9, 0.999), eps=1e-8):
        """mask: P booleans; grad None: the tensor is skipped and its step does not advance, as in torch."""
        if grad is None:
            return
        self.step += 1
        P = self.p.shape[0]
        rows = np.flatnonzero(np.asarray(mask).reshape(P))
        if rows.size == 0:
            return
        g = np.asarray(grad, dtype=np.float64).reshape(P, -1)[rows]
        p, m, v = (x.reshape(P, -1)[rows] for x in (self.p, self.m, self.v))           # copies (fancy indexing)
        aux_ref.adam_step(p, g, m, v, self.step, lr, betas[0], betas[1], eps)
        for x, y in ((self.p, p), (self.m, m), (self.v, v)):
            x.reshape(P, -1)[rows] = y                                                   # reshape of a contiguous array: a view


class TorchMaskedAdam:
    """torch.optim.Adam over one-tensor groups, every step followed by the restoration of the invisible rows."""

    def __init__(self, params, groups, dtype=torch.float32, device="cpu", preset=None):
        """params: list of arrays [P, ...]; groups: one dict(lr, betas, eps) per tensor; preset: (step, exp_avg list, exp_avg_sq list)."""
        self.params = [torch.tensor(np.asarray(p), dtype=dtype, device=device).requires_grad_(True) for p in params]
        self.opt = torch.optim.Adam([dict(params=[p], **g) for p, g in zip(self.params, groups)])
        if preset is not None:
            step0, m0, v0 = preset
            for p, m, v in zip(self.params, m0, v0):
                self.opt.state[p] = dict(step=torch.tensor(float(step0)), exp_avg=torch.tensor(np.asarray(m), dtype=dtype, device=device).view(p.shape),
                                         exp_avg_sq=torch.tensor(np.asarray(v), dtype=dtype, device=device).view(p.shape))

    def state(self, i):
        st = self.opt.state.get(self.params[i], {})
        if not st:
            z = torch.zeros_like(self.params[i])
            return dict(step=0, exp_avg=z, exp_avg_sq=z.clone())
        return st

    @torch.no_grad()
    def step(self, grads, mask):
        """grads: list of arrays (None: no gradient for that tensor); mask: P booleans."""
        keep = ~torch.tensor(np.asarray(mask, dtype=bool), device=self.params[0].device)
        saved = []
        for p, g in zip(self.params, grads):
            p.grad = None if g is None else torch.tensor(np.asarray(g), dtype=p.dtype, device=p.device).view(p.shape)
            st = self.opt.state.get(p, {})
            saved.append((p.detach().clone(), st["exp_avg"].clone() if st else torch.zeros_like(p), st["exp_avg_sq"].clone() if st else torch.zeros_like(p)))
        self.opt.step()
        for p, g, (p0, m0, v0) in zip(self.params, grads, saved):
            if g is None:
                continue
            st = self.opt.state[p]
            p[keep] = p0[keep]
            st["exp_avg"][keep] = m0[keep]
            st["exp_avg_sq"][keep] = v0[keep]


def fresh_masks(P, steps, seed=0, never=5, late=(1, 8)):
    """One mask per step: about a third of the rows at random, rows r % never == 0 never, rows r % never == late[0] not before step late[1]
    (0-based) -- so some rows are never seen and some are seen for the first time late."""
    rng = np.random.default_rng([seed, P])
    r = np.arange(P)
    out = []
    for t in range(steps):
        m = rng.random(P) < 0.35
        m[r % never == 0] = False
        m[(r % never == late[0]) & (t < late[1])] = False
        if t == late[1]:
            m[r % never == late[0]] = True                                               # all of them first seen at this very step
        out.append(m)
    return out
