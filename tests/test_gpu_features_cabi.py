"""-m gpu: include/gsr_features.h called through ctypes on the workspaces of a real gsr_forward: what the entry points write and what they
leave alone.  Every output and gradient buffer is pre-filled with NaN, so a cell the call was to write and did not, or one it was to
leave and touched, shows.  Two runs of the reverse pass differ by the order of their float atomics: up to a few thousand float32 addends
per sum, so 1e-4 of the tensor's largest magnitude bounds the difference (TOL)."""
import numpy as np
import pytest
import torch

from gaussian_transformer_amd import _lib, rasterizer
from gaussian_transformer_amd._lib import ptr
from tests import depth_ref as dr
from tests import features_ref as fr
from tests.test_gpu_features import DEV, tensors

pytestmark = pytest.mark.gpu
WORKSPACE = 4
NAN = float("nan")
TOL = 1e-4


class Render:
    """gsr_forward on a scene through the backend; the pieces the feature calls take."""

    def __init__(self, S, Cn):
        self.S, self.Cn = S, Cn
        self.rs, inp = tensors(S, grad=False)
        self.inp = inp
        empty = torch.empty((0,), device=DEV)
        self.P = int(inp["means3D"].shape[0])
        be = rasterizer.get_backend()
        self.n, self.color, self.radii, self.geom, self.binning, self.img = be.forward(
            self.rs, inp["means3D"], inp["shs"], empty, inp["opacities"], inp["scales"], inp["rotations"], empty)
        self.mask = be.composited_mask(self.geom, self.P) if self.P else torch.zeros((0,), dtype=torch.bool, device=DEV)
        self.F = torch.tensor(fr.features(self.radii.cpu().numpy(), Cn), device=DEV) if self.P else torch.zeros((0, Cn), device=DEV)
        self.G = torch.tensor(fr.map_grad(S, Cn), device=DEV)
        self.ws = _lib.workspace("gsr_features_workspace_bytes", DEV, self.P, Cn)

    def forward(self, out):
        return _lib.load().gsr_features_forward(
            _lib.stream(torch.device(DEV)), self.P, self.Cn, self.S.W, self.S.H, self.n, ptr(self.F), ptr(self.geom), self.geom.numel(),
            ptr(self.binning), self.binning.numel(), ptr(self.img), self.img.numel(), ptr(out))

    def backward(self, g, accumulate, dF="own", ws_bytes=None):
        """g: dict of the six gradient buffers; dF: a tensor, None (NULL) or "own" (g["features"])."""
        rs, inp = self.rs, self.inp
        dF = g["features"] if isinstance(dF, str) else dF
        return _lib.load().gsr_features_backward(
            _lib.stream(torch.device(DEV)), self.P, self.Cn, self.S.W, self.S.H, self.n, ptr(inp["means3D"]), ptr(self.radii), ptr(inp["scales"]),
            float(rs.scale_modifier), ptr(inp["rotations"]), None, ptr(rs.viewmatrix), ptr(rs.projmatrix), ptr(rs.campos),
            float(rs.tanfovx), float(rs.tanfovy), ptr(self.F), ptr(self.G), ptr(self.geom), self.geom.numel(), ptr(self.binning),
            self.binning.numel(), ptr(self.img), self.img.numel(), ptr(self.ws), self.ws.numel() if ws_bytes is None else ws_bytes,
            accumulate, ptr(g["means2D"]), ptr(g["opacity"]), ptr(g["means3D"]), None, ptr(g["scales"]), ptr(g["rots"]), ptr(dF))

    def buffers(self, fill=NAN):
        P = self.P
        return {k: torch.full((P, w), fill, device=DEV) for k, w in (("means2D", 3), ("opacity", 1), ("means3D", 3), ("scales", 3), ("rots", 4),
                                                                     ("features", self.Cn))}


def ok(rc, what):
    _lib.check(rc, what)


@pytest.mark.parametrize("Cn", [3, 17])
def test_nan_prefilled_buffers(Cn):
    r = Render(fr.scene(dr.SCENES[3]), Cn)
    assert bool(r.mask.any()) and not bool(r.mask.all())               # some Gaussians are composited, some are not
    out = torch.full((Cn, r.S.H, r.S.W), NAN, device=DEV)
    ok(r.forward(out), "forward")
    assert not bool(torch.isnan(out).any())
    # accumulate = 0: everything is written; dL/dF is an exact zero outside the composited mask
    g = r.buffers()
    r.ws.fill_(255)                                                    # contents irrelevant before: NaN bit patterns
    ok(r.backward(g, 0), "backward")
    for k, t in g.items():
        assert not bool(torch.isnan(t).any()), k
        assert not bool(t[~r.mask].any()), k
    assert bool(g["features"][r.mask].any()) and bool(g["opacity"][r.mask].any())
    # accumulate = 1: rows outside the mask are bit for bit as they were, rows inside get the same gradient added
    base = {k: torch.randn_like(t) for k, t in g.items()}
    acc = {k: t.clone() for k, t in base.items()}
    acc["features"].fill_(NAN)
    ok(r.backward(acc, 1), "backward accumulate")
    for k in ("means2D", "opacity", "means3D", "scales", "rots"):
        assert torch.equal(acc[k][~r.mask], base[k][~r.mask]), k
        d = (acc[k] - base[k] - g[k])[r.mask].abs().max()
        assert float(d) <= TOL * float(g[k].abs().max()) + 1e-6 * float(base[k].abs().max()), (k, float(d))
    assert not bool(torch.isnan(acc["features"]).any()) and not bool(acc["features"][~r.mask].any())      # takes no part in accumulate
    assert float((acc["features"] - g["features"]).abs().max()) <= TOL * float(g["features"].abs().max())
    # dL_dfeatures = NULL: the Gaussians' gradients are the same, to the order of the atomics
    h = r.buffers()
    ok(r.backward(h, 0, dF=None), "backward without dL/dF")
    assert bool(torch.isnan(h["features"]).all())                      # ours, not passed: untouched
    for k in ("means2D", "opacity", "means3D", "scales", "rots"):
        assert not bool(torch.isnan(h[k]).any())
        assert float((h[k] - g[k]).abs().max()) <= TOL * float(g[k].abs().max()), k
    # a workspace one byte short
    assert r.backward(r.buffers(), 0, ws_bytes=r.ws.numel() - 1) == WORKSPACE
    assert _lib.load().gsr_last_error().decode() == f"features workspace {r.ws.numel() - 1} < {r.ws.numel()}"
    assert r.ws.numel() == _lib.workspace_bytes("gsr_features_workspace_bytes", r.P, Cn)


def test_no_gaussians_and_a_camera_that_sees_nothing():
    import dataclasses
    S = fr.scene(dr.SCENES[1])
    empty = dataclasses.replace(S, means3D=np.zeros((0, 3), np.float32), opacities=np.zeros((0, 1), np.float32), shs=np.zeros((0, 4, 3), np.float32),
                                scales=np.zeros((0, 3), np.float32), rotations=np.zeros((0, 4), np.float32))
    m = np.asarray(S.viewmatrix, np.float64).reshape(16)
    behind = dataclasses.replace(S, means3D=(np.asarray(S.means3D, np.float64) - 1000.0 * np.array([m[2], m[6], m[10]])).astype(np.float32))
    for name, Sx in (("P = 0", empty), ("R = 0", behind)):
        r = Render(Sx, 5)
        assert r.n == 0, name
        out = torch.full((5, S.H, S.W), NAN, device=DEV)
        ok(r.forward(out), name)
        assert not bool(out.any()) and not bool(torch.isnan(out).any()), name
        g = r.buffers()
        ok(r.backward(g, 0), name)
        for k, t in g.items():
            assert not bool(t.any()) and not bool(torch.isnan(t).any()), (name, k)      # P = 0: nothing to write
        if r.P:
            acc = r.buffers(fill=1.5)
            acc["features"].fill_(NAN)
            ok(r.backward(acc, 1), name)
            assert all(bool((acc[k] == 1.5).all()) for k in acc if k != "features") and not bool(acc["features"].any()), name
