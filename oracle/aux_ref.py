"""Float64 CPU references for the two other hand-written kernels of a training step besides the loss (oracle/ssim_ref.py):
the Adam step (csrc/adam.hip) and the 3-nearest-neighbour mean squared distance (csrc/knn.hip).

TEST INFRASTRUCTURE ONLY.  Plain numpy; float32 inputs are converted exactly (every float32 is a float64).  Checked against
independent second routes (torch.optim.Adam on float64 CPU tensors; brute force against scipy's k-d tree) by
tests/test_aux_references.py, without a GPU.
"""
import numpy as np


# ---------------------------------------------------------------------------------------------
# Adam, as the reference's optimiser steps it (torch.optim.Adam: no weight decay, no amsgrad)
# ---------------------------------------------------------------------------------------------
def adam_step(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """One step, in place on the float64 arrays p, m, v; `step` is the 1-based count of this step."""
    g = np.asarray(g, dtype=np.float64)
    m += (g - m) * (1.0 - beta1)
    v *= beta2
    v += (1.0 - beta2) * g * g
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    p -= (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps))


class Adam64:
    """State of one tensor: float64 copies of param / exp_avg / exp_avg_sq and the step count."""

    def __init__(self, param, exp_avg=None, exp_avg_sq=None, step=0):
        self.p = np.array(param, dtype=np.float64)
        self.m = np.zeros_like(self.p) if exp_avg is None else np.array(exp_avg, dtype=np.float64)
        self.v = np.zeros_like(self.p) if exp_avg_sq is None else np.array(exp_avg_sq, dtype=np.float64)
        self.step = int(step)

    def update(self, grad, lr, betas=(0.9, 0.999), eps=1e-8):
        if grad is None:                 # torch skips the tensor: state untouched, step not advanced
            return
        self.step += 1
        adam_step(self.p, np.asarray(grad, dtype=np.float64).reshape(self.p.shape), self.m, self.v, self.step, lr, betas[0], betas[1], eps)


# ---------------------------------------------------------------------------------------------
# mean squared distance to the (up to) three nearest OTHER points
# ---------------------------------------------------------------------------------------------
def knn_mean_dist2_brute(points, chunk=2048):
    """Brute force in float64 on the coordinates as given (chunked N x N; fine up to ~20 k points).  Fewer than four points: the mean
    over the neighbours that exist, 0 for a single point (the rule of include/gsr_knn.h)."""
    p = np.asarray(points, dtype=np.float64)
    n = p.shape[0]
    k = min(3, n - 1)
    if k <= 0:
        return np.zeros((n,), dtype=np.float64)
    out = np.empty((n,), dtype=np.float64)
    for a in range(0, n, chunk):
        q = p[a:a + chunk]
        d = q[:, None, :] - p[None, :, :]                     # differences first, never |a|^2 + |b|^2 - 2ab
        d2 = (d * d).sum(axis=2)
        d2[np.arange(q.shape[0]), a + np.arange(q.shape[0])] = np.inf       # the point itself (coincident OTHER points stay, at 0)
        out[a:a + chunk] = np.sort(np.partition(d2, k - 1, axis=1)[:, :k], axis=1).mean(axis=1)
    return out


def knn_mean_dist2_kdtree(points):
    """The same with scipy's exact k-d tree in float64 (N >= 4), for clouds too large for the brute force."""
    from scipy.spatial import cKDTree
    p = np.asarray(points, dtype=np.float64)
    d, _ = cKDTree(p).query(p, k=4)
    return (d[:, 1:] ** 2).mean(axis=1)
