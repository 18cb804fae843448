"""tests/oracle_backend.py's stand-in with camera gradients through tests/pose_ref.py, for CPU tests of the autograd plumbing of
_RasterizeGaussiansPose.  Test infrastructure, colour only (the stand-in renders no maps)."""
import numpy as np
import torch

from tests import pose_ref
from tests.oracle_backend import OracleBackend


class PoseOracleBackend(OracleBackend):
    def __init__(self, precision="f32"):
        super().__init__(precision)
        self.precision = precision
        self.calls = []              # names of the backend calls, in order
        self._dL = {}

    def forward(self, *a, **kw):
        self.calls.append("forward")
        return super().forward(*a, **kw)

    def backward(self, rs, num_rendered, dL_dpix, means3D, radii, shs, colors_precomp, scales, rotations, cov3D_precomp,
                 geom, binning, img, return_ws=False):
        self.calls.append("backward")
        out = super().backward(rs, num_rendered, dL_dpix, means3D, radii, shs, colors_precomp, scales, rotations, cov3D_precomp,
                               geom, binning, img)
        if not return_ws:
            return out
        key = int(geom[0])
        self._dL[key] = dL_dpix.detach().cpu().numpy().astype(np.float64)
        return out + (torch.tensor([key], dtype=torch.int64),)          # the "workspace": names the reverse pass it belongs to

    def pose_backward(self, rs, kind, num_rendered, means3D, radii, shs, colors_precomp, scales, rotations, cov3D_precomp, geom, acc_ws,
                      want=(True, True, True)):
        self.calls.append("pose_backward")
        assert kind == 0 and int(acc_ws[0]) == int(geom[0])
        f = self._states[int(geom[0])]
        g = self.r.backward(f, self._dL[int(geom[0])])
        st = f["state"]
        cam = pose_ref.surrogate_grads(st.sc, f["radii"], g["dL_dmeans2D"], g["dL_dconic"], g["dL_dcolors"], st.geom()["clamped"],
                                       precision=self.precision)
        t = lambda a, shape: torch.from_numpy(np.asarray(a, np.float32).reshape(shape).copy())
        return (t(cam["viewmatrix"], (4, 4)) if want[0] else None, t(cam["projmatrix"], (4, 4)) if want[1] else None,
                t(cam["campos"], (3,)) if want[2] else None)
