"""ctypes binding of libgsr_hip.so (C ABI: include/gsr.h).

This is the Python-side stub a maintainer of the reference would add in place of the pybind11
module `diff_gaussian_rasterization._C`.  There is NO CPU fallback: if the
library is missing, cannot be loaded, or a tensor is not on a HIP device, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GSR_LIB_PATH") or os.path.join(_HERE, "libgsr_hip.so")   # GSR_LIB_PATH: ablation builds (scripts/)

ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)
GSR_NUM_STAGES = 13

_p = C.c_void_p
_i32 = C.c_int32
_f = C.c_float
_sz = C.c_size_t

ADAM_MAX_GROUPS = 16
ADAM_MASK_BYTES, ADAM_MASK_RADII = 0, 1


class AdamGroup(C.Structure):          # gsr_adam_group_t of include/gsr_optim.h
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("n", C.c_int64), ("lr", C.c_float), ("step", C.c_int32)]


SIGNATURES = {
    "gsr_abi_version": (_i32, []),
    "gsr_last_error": (C.c_char_p, []),
    "gsr_workspace_sizes": (_i32, [_i32, _i32, _i32, C.POINTER(_sz), C.POINTER(_sz), C.POINTER(_sz)]),
    "gsr_binning_bytes": (_i32, [C.c_int64, _i32, _i32, C.POINTER(_sz)]),
    "gsr_backward_workspace_bytes": (_i32, [_i32, C.c_int64, C.POINTER(_sz)]),
    "gsr_forward": (_i32, [_p, _i32, _i32, _i32, _i32, _i32,          # stream P D M W H
                           _p, _p, _p, _p, _p,                        # bg means3D shs colors opacities
                           _p, _f, _p, _p,                            # scales mod rotations cov3D
                           _p, _p, _p, _f, _f,                        # view proj campos tanfovx tanfovy
                           _i32, _i32, _p, _p,                        # prefiltered debug out_color radii
                           _p, _sz, ALLOC_FN, _p, _p, _sz,            # geom, bytes, alloc, user, img, bytes
                           C.POINTER(C.c_int64),
                           _p, _i32]),                                # shs_rest raw_params (fused-step extension)
    "gsr_backward": (_i32, [_p, _i32, _i32, _i32, C.c_int64, _i32, _i32,   # stream P D M R W H
                            _p, _p, _p, _p, _p,                       # bg means3D radii shs colors
                            _p, _f, _p, _p,                           # scales mod rotations cov3D
                            _p, _p, _p, _f, _f,                       # view proj campos tanfovx tanfovy
                            _p, _p, _sz, _p, _sz, _p, _sz, _p, _sz,   # dL_dpix geom binning img bwd (+bytes)
                            _p, _p, _p, _p, _p, _p, _p, _p,           # 8 gradient outputs
                            _i32,                                     # debug
                            _p, _i32, _p]),                           # shs_rest raw_params dL_dsh_rest
    "gsr_mark_visible": (_i32, [_p, _i32, _p, _p, _p, _p]),
    "gsr_backward_prefill": (_i32, [_i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p]),   # P M + gsr_backward's 8 gradient outputs, dL_dsh_rest
    "gsr_composited_mask": (_i32, [_p, _i32, _p, C.c_size_t, _p]),
    "gsr_debug_read_geom": (_i32, [_p, _i32, _p, _p, _p, _p, _p, _p, _p]),
    "gsr_debug_read_binning": (_i32, [_p, C.c_int64, _i32, _i32, _p, _p, _p, _p, _p]),
    "gsr_debug_read_image_state": (_i32, [_p, _i32, _i32, _p, _p, _p]),
    "gsr_debug_read_lane_counters": (_i32, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "gsr_debug_read_wave_trace": (_i32, [_i32, _p, C.c_int64]),
    "gsr_debug_read_segments": (_i32, [_p, _i32, _i32, _p, _p]),
    "gsr_debug_read_bound_errors": (_i32, [_p, _i32, _p, _i32, _i32, _p, _p]),
    "gsr_l1_ssim_workspace": (_i32, [_i32, _i32, _i32, C.POINTER(_sz)]),
    "gsr_l1_ssim_forward": (_i32, [_p, _i32, _i32, _i32, _p, _p, _f, _p, _p, _sz]),
    "gsr_l1_ssim_backward": (_i32, [_p, _i32, _i32, _i32, _p, _p, _f, _p, _p, _sz, _p]),
    "gsr_views_loss_workspace": (_i32, [_i32, _i32, _i32, C.POINTER(_sz)]),                        # B H W bytes
    "gsr_views_loss_forward": (_i32, [_p, _i32, _i32, _i32, C.POINTER(_p), C.POINTER(_p),          # stream B H W imgs gts (host arrays of device pointers)
                                      _f, _f, _i32, _p, _p, _p, _sz]),                             # w_l1 w_ssim sanitize out3 terms ws ws_bytes
    "gsr_views_loss_backward": (_i32, [_p, _i32, _i32, _i32, C.POINTER(_p), C.POINTER(_p),
                                       _f, _f, _i32, _p, _p, _sz, C.POINTER(_p)]),                 # ... grad_loss ws ws_bytes grad_imgs
    "gsr_knn_workspace": (_i32, [_i32, C.POINTER(_sz)]),
    "gsr_knn_mean_dist2": (_i32, [_p, _i32, _p, _p, _p, _sz]),
    "gsr_adam_step": (_i32, [_p, _i32, C.POINTER(AdamGroup), C.c_double, C.c_double, C.c_double]),
    "gsr_adam_step_masked": (_i32, [_p, _i32, C.POINTER(AdamGroup), C.c_double, C.c_double, C.c_double, _i32, _p, _i32]),   # ... P mask mask_kind
    "gsr_set_option": (_i32, [C.c_char_p, _i32]),
    "gsr_get_option": (_i32, [C.c_char_p, C.POINTER(_i32)]),
    "gsr_set_profiling": (_i32, [_i32]),
    "gsr_get_stage_times": (_i32, [C.POINTER(C.c_char_p), C.POINTER(_f)]),
}

# include/gsr_chamfer.h (a table of its own: SIGNATURES is exactly gsr.h + gsr_loss.h + gsr_knn.h + gsr_optim.h)
CHAMFER_SIGNATURES = {
    "gsr_chamfer_workspace": (_i32, [_i32, _i32, _i32, C.POINTER(_sz)]),                 # B N M bytes
    "gsr_chamfer_forward": (_i32, [_p, _i32, _i32, _i32, _i32, _p, _p,                   # stream B N M D x1 x2
                                   _p, _p, _p, _p, _p, _sz]),                            # dist1 dist2 idx1 idx2 ws ws_bytes
    "gsr_chamfer_backward": (_i32, [_p, _i32, _i32, _i32, _i32, _p, _p, _p, _p,          # stream B N M D x1 x2 idx1 idx2
                                    _p, _p, _p, _p]),                                    # g1 g2 dx1 dx2
}

# include/gsr_sequence.h (likewise a table of its own)
SEQUENCE_SIGNATURES = {
    "gsr_box_sort_workspace": (_i32, [_i32, _i32, C.POINTER(_sz)]),                      # P n bytes
    "gsr_box_sort": (_i32, [_p, _i32, _i32, _p, _i32, _i32,                              # stream P D rows xyz_col n
                            _p, _p, _p, _p, _sz]),                                       # out_rows out_perm out_count ws ws_bytes
    "gsr_visible_union": (_i32, [_p, _i32, _i32, _p, _p, _f, _p, _p, _i32,               # stream P B means3D scales mod rotations cov3D raw_params
                                 _p, _p,                                                 # viewmatrices projmatrices (device)
                                 C.POINTER(_f), C.POINTER(_f), C.POINTER(_i32), C.POINTER(_i32),   # tanfovx tanfovy widths heights (host)
                                 _p, _p, _p]),                                           # radii_out visible_out counts_out
}

# include/gsr_rows.h (likewise a table of its own)
ROWS_SIGNATURES = {
    "gsr_rows_unpack": (_i32, [_p, _i32, _i32, _p, _p, _p, _p, _p, _p, _p]),             # stream P D rows xyz f_dc f_rest opacity scaling rotation
    "gsr_rows_grad_pack": (_i32, [_p, _i32, _i32, _i32, C.POINTER(_p), _p]),             # stream P D B arenas (host array of device pointers) grad_rows
}

# include/gsr_density.h (likewise a table of its own)
DENSITY_MAX_GROUPS = 16
DENSITY_COPY, DENSITY_XYZ, DENSITY_SCALING = 0, 1, 2


_GROUP_FIELDS = [("src", C.c_void_p), ("src_exp_avg", C.c_void_p), ("src_exp_avg_sq", C.c_void_p),      # one layout, two public types
                 ("dst", C.c_void_p), ("dst_exp_avg", C.c_void_p), ("dst_exp_avg_sq", C.c_void_p),
                 ("width_floats", C.c_int32), ("role", C.c_int32)]


class DensityGroup(C.Structure):       # gsr_density_group_t of include/gsr_density.h
    _fields_ = _GROUP_FIELDS


DENSITY_SIGNATURES = {
    "gsr_density_record": (_i32, [_p, _i32, _p, _i32, _p, _p, _p, _p, _p]),             # stream P grad2d stride radii visible accum denom max_radii
    "gsr_densify_plan_workspace": (_i32, [_i32, _i32, C.POINTER(_sz)]),                  # P N bytes
    "gsr_densify_plan": (_i32, [_p, _i32, _p, _p, _p, _p, _f, _f, _f, _f, _i32,          # stream P opacity scaling accum denom thr min_opacity cut prune_world N
                                _p, _p, _sz]),                                           # counts_host ws ws_bytes
    "gsr_densify_apply": (_i32, [_p, _i32, _i32, _i32, _i32, _i32, C.POINTER(DensityGroup),   # stream P N n_split P_new n_groups groups
                                 _p, _p, _p, _p, _sz]),                                  # scaling rotation noise ws ws_bytes
}

# include/gsr_mcmc.h (likewise a table of its own)
MCMC_MAX_GROUPS, MCMC_N_MAX = 16, 51
MCMC_RELOCATE, MCMC_GROW = 0, 1
MCMC_COPY, MCMC_OPACITY, MCMC_SCALING = 0, 1, 2


class McmcGroup(C.Structure):          # gsr_mcmc_group_t of include/gsr_mcmc.h
    _fields_ = _GROUP_FIELDS


MCMC_SIGNATURES = {
    "gsr_mcmc_plan_workspace": (_i32, [_i32, _i32, C.POINTER(_sz)]),                     # P n_draws bytes
    "gsr_mcmc_plan": (_i32, [_p, _i32, _i32, _p, _p, _f, C.c_double, _i32, _i32,         # stream mode P opacity scaling L min_opacity n_max n_draws
                             _p, _p, _p, _sz]),                                          # u counts_host ws ws_bytes
    "gsr_mcmc_apply": (_i32, [_p, _i32, _i32, _i32, _i32, C.POINTER(McmcGroup), _p, _sz]),   # stream mode P n_draws n_groups groups ws ws_bytes
    "gsr_mcmc_noise": (_i32, [_p, _i32, _p, _p, _p, _p, _p, _f, _f, _f]),                # stream P opacity scaling rotation noise xyz gate_k gate_t scale
    "gsr_mcmc_regularize_workspace": (_i32, [_i32, C.POINTER(_sz)]),                     # P bytes
    "gsr_mcmc_regularize": (_i32, [_p, _i32, _p, _p, _p, _i32, _p, _i32,                 # stream P opacity scaling grad_opacity stride_o grad_scaling stride_s
                                   C.c_double, C.c_double, _p, _p, _sz]),                # lambda_o lambda_s means_out ws ws_bytes
}

# include/gsr_depth.h (likewise a table of its own)
DEPTH_EXPECTED, DEPTH_INVERSE = 0, 1
DEPTH_SIGNATURES = {
    "gsr_depth_workspace_bytes": (_i32, [_i32, C.POINTER(_sz)]),                         # P bytes
    "gsr_depth_forward": (_i32, [_p, _i32, _i32, _i32, C.c_int64, _i32,                  # stream P W H R mode
                                 _p, _sz, _p, _sz, _p, _sz,                              # geom binning img (+bytes)
                                 _p, _p]),                                               # out_depth out_alpha
    "gsr_depth_backward": (_i32, [_p, _i32, _i32, _i32, C.c_int64, _i32,                 # stream P W H R mode
                                  _p, _p, _p, _f, _p, _p,                                # means3D radii scales mod rotations cov3D
                                  _p, _p, _p, _f, _f,                                    # view proj campos tanfovx tanfovy
                                  _p, _p,                                                # dL_ddepth dL_dalpha
                                  _p, _sz, _p, _sz, _p, _sz, _p, _sz,                    # geom binning img ws (+bytes)
                                  _i32,                                                  # accumulate
                                  _p, _p, _p, _p, _p, _p]),                              # dL_d{means2D opacity means3D cov3D scales rots}
}

# include/gsr_features.h (likewise a table of its own)
FEATURES_MAX_C = 64
FEATURES_SIGNATURES = {
    "gsr_features_workspace_bytes": (_i32, [_i32, _i32, C.POINTER(_sz)]),                # P C bytes
    "gsr_features_forward": (_i32, [_p, _i32, _i32, _i32, _i32, C.c_int64, _p,           # stream P C W H R features
                                    _p, _sz, _p, _sz, _p, _sz,                           # geom binning img (+bytes)
                                    _p]),                                                # out
    "gsr_features_backward": (_i32, [_p, _i32, _i32, _i32, _i32, C.c_int64,              # stream P C W H R
                                     _p, _p, _p, _f, _p, _p,                             # means3D radii scales mod rotations cov3D
                                     _p, _p, _p, _f, _f,                                 # view proj campos tanfovx tanfovy
                                     _p, _p,                                             # features dL_dout
                                     _p, _sz, _p, _sz, _p, _sz, _p, _sz,                 # geom binning img ws (+bytes)
                                     _i32,                                               # accumulate
                                     _p, _p, _p, _p, _p, _p,                             # dL_d{means2D opacity means3D cov3D scales rots}
                                     _p]),                                               # dL_dfeatures
}

# include/gsr_pose.h (likewise a table of its own)
POSE_COLOR, POSE_DEPTH_EXPECTED, POSE_DEPTH_INVERSE = 0, 1, 2
POSE_SIGNATURES = {
    "gsr_pose_workspace_bytes": (_i32, [_i32, C.POINTER(_sz)]),                          # P bytes
    "gsr_pose_backward": (_i32, [_p, _i32, _i32, _i32, _i32, _i32, _i32, C.c_int64,      # stream kind P D M W H R
                                 _p, _p, _p, _p, _p, _f, _p, _p,                         # means3D radii shs colors scales mod rotations cov3D
                                 _p, _p, _p, _f, _f,                                     # view proj campos tanfovx tanfovy
                                 _p, _sz, _p, _sz, _p, _sz,                              # geom acc ws (+bytes)
                                 _p, _p, _p]),                                           # dL_d{viewmatrix projmatrix campos}
}

# include/gsr_contrib.h (likewise a table of its own)
CONTRIB_ROW_BYTES = 16
CONTRIB_MAX_PIXELS = 2 ** 32 - 1       # pixels a row's count can hold (the header's capacity)


class ContribRow(C.Structure):         # gsr_contrib_row_t of include/gsr_contrib.h
    _fields_ = [("sum_q32", C.c_uint64), ("max_bits", C.c_uint32), ("count", C.c_uint32)]


CONTRIB_SIGNATURES = {
    "gsr_contrib_accumulate": (_i32, [_p, _i32, _i32, _i32, C.c_int64,                   # stream P W H R
                                      _p, _sz, _p, _sz, _p, _sz,                         # geom binning img (+bytes)
                                      _p]),                                              # rows
    "gsr_contrib_read": (_i32, [_p, _i32, _p, _p, _p, _p]),                              # stream P rows weight_sum weight_max pixel_count
}

# include/gsr_absgrad.h (likewise a table of its own)
ABSGRAD_SIGNATURES = {
    "gsr_absgrad_workspace_bytes": (_i32, [_i32, C.POINTER(_sz)]),                       # P bytes
    "gsr_absgrad_backward": (_i32, [_p, _i32, _i32, _i32, C.c_int64,                     # stream P W H R
                                    _p, _p,                                              # bg dL_dcolor
                                    _p, _sz, _p, _sz, _p, _sz, _p, _sz,                  # geom binning img ws (+bytes)
                                    _i32,                                                # accumulate
                                    _p, _p]),                                            # absgrad signed_sum
}

# include/gsr_normals.h (likewise a table of its own)
NORMAL_TILE_X, NORMAL_TILE_Y = 32, 8   # GSR_NORMAL_TILE_X, GSR_NORMAL_TILE_Y: the loss kernels' tile
NORMALS_SIGNATURES = {
    "gsr_gaussian_normals_forward": (_i32, [_p, _i32, _p, _p, _p, _p, _p, _p]),          # stream P means3D scales rotations view out_normals out_axis
    "gsr_gaussian_normals_backward": (_i32, [_p, _i32, _p, _p, _p, _p, _p]),             # stream P rotations view axis dL_dnormals dL_drots
    "gsr_normal_loss_workspace": (_i32, [_i32, _i32, C.POINTER(_sz)]),                   # H W bytes
    "gsr_normal_loss_forward": (_i32, [_p, _i32, _i32, _f, _f, _f, _p, _p, _p,           # stream H W tanfovx tanfovy alpha_min depth alpha normals
                                       _p, _p, _p, _sz]),                                # out2 out_surf ws ws_bytes
    "gsr_normal_loss_backward": (_i32, [_p, _i32, _i32, _f, _f, _f, _p, _p, _p,          # stream H W tanfovx tanfovy alpha_min depth alpha normals
                                        _p, _p, _p, _p]),                                # grad_loss dL_ddepth dL_dalpha dL_dnormals
}

_lock = threading.Lock()
_lib = None


class GsrError(RuntimeError):
    """A native failure of the HIP rasterizer (callers of the reference catch RuntimeError)."""


def load() -> C.CDLL:
    """Loads libgsr_hip.so once.  torch is imported first so that the library binds to the HIP
    runtime already living in the process (torch ships its own libamdhip64 with the same soname)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        import torch  # noqa: F401  (loads libamdhip64 before ours resolves it)
        if not os.path.exists(LIB_PATH):
            raise GsrError(
                f"HIP extension not built: {LIB_PATH} is missing. Run `python -m gaussian_transformer_amd.build` "
                "(there is no CPU fallback).")
        try:
            lib = C.CDLL(LIB_PATH)
        except OSError as e:
            raise GsrError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in {**SIGNATURES, **CHAMFER_SIGNATURES, **SEQUENCE_SIGNATURES, **ROWS_SIGNATURES, **DENSITY_SIGNATURES,
                                   **MCMC_SIGNATURES, **DEPTH_SIGNATURES, **FEATURES_SIGNATURES, **POSE_SIGNATURES, **CONTRIB_SIGNATURES,
                                   **ABSGRAD_SIGNATURES, **NORMALS_SIGNATURES}.items():
            fn = getattr(lib, name)       # AttributeError if the symbol is missing: loud by design
            fn.restype = res
            fn.argtypes = args
        if lib.gsr_abi_version() != 2:
            raise GsrError(f"libgsr_hip.so ABI version {lib.gsr_abi_version()} != 2")
        _lib = lib
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().gsr_last_error()
        raise GsrError(f"{what} failed (code {rc}): {msg.decode(errors='replace') if msg else ''}")


# ---- the one way to call the library.  torch is imported inside: this module loads without it. ----

def call(name: str, *args) -> None:
    """The native function `name` on `args`, checked.  `load` is looked up per call (the host tests replace it)."""
    check(getattr(load(), name)(*args), name)


def stream(dev):
    """The raw handle of the current stream on `dev`."""
    import torch
    return torch.cuda.current_stream(dev).cuda_stream


def ptr(t):
    """The device pointer of a dense tensor; NULL for None and for an empty tensor."""
    if t is None or t.numel() == 0:
        return None
    if not t.is_contiguous():      # the C ABI takes dense row-major buffers; the public entry points make them so
        raise GsrError(f"non-contiguous tensor of shape {tuple(t.shape)} passed to the native rasterizer")
    return t.data_ptr()


def ptr_array(ptrs):
    """A host array of device pointers (None: NULL)."""
    return (C.c_void_p * len(ptrs))(*ptrs)


def workspace_bytes(sizer: str, *sizes) -> int:
    """What the library's `sizer` (a gsr_*_workspace or gsr_*_workspace_bytes) asks for at these sizes."""
    n = C.c_size_t()
    check(getattr(load(), sizer)(*sizes, C.byref(n)), sizer)
    return n.value


def workspace(sizer: str, dev, *sizes):
    """A uint8 tensor on `dev` of as many bytes as `sizer` asks for, and of one byte where it asks for none: a workspace always has
    an address, so every call site passes ptr(ws), ws.numel().  (Only gsr_chamfer_workspace can say 0, for an empty batch, and
    gsr_chamfer_forward returns before it looks at the workspace then.)"""
    import torch
    return torch.empty((max(workspace_bytes(sizer, *sizes), 1),), dtype=torch.uint8, device=dev)


def require_tensor(who: str, name: str, t, dtype=None) -> None:
    """`t` is a torch.Tensor of `dtype` (None: float32), or GsrError naming the argument."""
    import torch
    dtype = torch.float32 if dtype is None else dtype
    if not isinstance(t, torch.Tensor):
        raise GsrError(f"{who}: {name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise GsrError(f"{who}: {name} must be {str(dtype).replace('torch.', '')}, got {str(t.dtype).replace('torch.', '')}")


def require_hip(who: str, name: str, t) -> None:
    if t.device.type != "cuda":
        raise GsrError(f"{who}: {name} must be on a HIP device, got {t.device} (no CPU fallback)")


def set_option(name: str, value: int) -> None:
    """Process-wide tuning knob of the native library (include/gsr.h: gsr_set_option)."""
    check(load().gsr_set_option(name.encode(), int(value)), f"gsr_set_option({name})")


def get_option(name: str) -> int:
    """Current value of a tuning knob (include/gsr.h: gsr_get_option)."""
    v = C.c_int32(0)
    check(load().gsr_get_option(name.encode(), C.byref(v)), f"gsr_get_option({name})")
    return int(v.value)


LANE_COUNTER_NAMES = ("staged", "visits", "block_visits", "lanes_ok", "lanes_past_last", "lanes_below_alpha",
                      "reductions", "dead_block_visits", "waves")


def read_lane_counters() -> dict:
    """Lane-slot accounting of the instrumented compositing kernels (set_option("count_lanes", 1) first); reads and
    resets the current device's counters.  Returns {"fwd": {...}, "bwd": {...}} with a derived "lane_efficiency"
    = lanes that blended / lane slots issued (64 per 8x8 block visit)."""
    f = (C.c_uint64 * 16)()
    b = (C.c_uint64 * 16)()
    check(load().gsr_debug_read_lane_counters(f, b), "gsr_debug_read_lane_counters")
    out = {}
    for tag, arr in (("fwd", f), ("bwd", b)):
        d = {n: int(arr[i]) for i, n in enumerate(LANE_COUNTER_NAMES)}
        slots = 64 * d["block_visits"]
        d["lane_slots"] = slots
        d["lane_efficiency"] = (d["lanes_ok"] / slots) if slots else 0.0
        out[tag] = d
    return out
