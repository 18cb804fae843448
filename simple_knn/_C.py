"""`distCUDA2` on HIP: mean squared distance to the three nearest neighbours (include/gsr_knn.h).

The reference imports `from simple_knn._C import distCUDA2` (scene/gaussian_model.py:20) and calls it once,
at scene/gaussian_model.py:134, on the SfM points to initialise the Gaussian scales.  No CPU fallback."""
import torch

from gaussian_transformer_amd import _lib


def distCUDA2(points: torch.Tensor) -> torch.Tensor:
    if points.device.type != "cuda":
        raise _lib.GsrError(f"distCUDA2 needs a tensor on a HIP device, got {points.device} (no CPU fallback)")
    if points.dim() != 2 or points.shape[1] != 3:
        raise _lib.GsrError("distCUDA2: points must have shape [N, 3]")
    pts = points.detach().to(torch.float32).contiguous()
    N = int(pts.shape[0])
    out = torch.empty((N,), dtype=torch.float32, device=pts.device)
    with torch.cuda.device(pts.device):
        ws = _lib.workspace("gsr_knn_workspace", pts.device, N)
        _lib.call("gsr_knn_mean_dist2", _lib.stream(pts.device), N, _lib.ptr(pts), _lib.ptr(out), _lib.ptr(ws), ws.numel())
    return out
