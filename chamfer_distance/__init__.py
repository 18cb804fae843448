"""Drop-in module name: the reference does
    from chamfer_distance import ChamferDistance
(train_stacked_transformer.py:24).  With this repo root on sys.path that import resolves here; the native
library is loaded on the first call, so the import itself needs neither a GPU nor the built library."""
from gaussian_transformer_amd.chamfer import ChamferDistance, ChamferDistanceFunction  # noqa: F401

__all__ = ["ChamferDistance", "ChamferDistanceFunction"]
