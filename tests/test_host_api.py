"""CPU tests of the host side: C-ABI library loads and exports every symbol of include/gsr.h,
the product path fails loudly without a GPU, and the Python API's validation / autograd plumbing
(exercised through an oracle-backed stand-in backend -- tests/oracle_backend.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from gaussian_transformer_amd import GaussianRasterizationSettings, GaussianRasterizer, _lib, rasterizer, synth
from gaussian_transformer_amd.model import GaussianParams
from gaussian_transformer_amd.render import PipelineParams, TorchCamera, render
from tests.oracle_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cabi_library_loads_and_exports_every_declared_symbol():
    from gaussian_transformer_amd.build import build_hip
    path = build_hip()                      # hipcc cross-compiles for gfx950 without a GPU
    lib = ctypes.CDLL(path)
    header = open(os.path.join(ROOT, "include", "gsr.h")).read() + open(os.path.join(ROOT, "include", "gsr_loss.h")).read() + open(os.path.join(ROOT, "include", "gsr_knn.h")).read() + open(os.path.join(ROOT, "include", "gsr_optim.h")).read()
    declared = set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", header)) - {"gsr_alloc_fn"}
    assert {"gsr_forward", "gsr_backward", "gsr_mark_visible", "gsr_workspace_sizes", "gsr_binning_bytes",
            "gsr_last_error", "gsr_abi_version"} <= declared
    for name in sorted(declared):
        assert hasattr(lib, name), name
    assert set(_lib.SIGNATURES) == declared            # the ctypes stub binds exactly the header
    assert _lib.load().gsr_abi_version() == 2


def test_drop_in_module_name_and_settings_fields():
    import diff_gaussian_rasterization as d
    assert d.GaussianRasterizer is GaussianRasterizer and d.GaussianRasterizationSettings is GaussianRasterizationSettings
    # field order / names of gaussian_renderer/__init__.py:36-49
    assert GaussianRasterizationSettings._fields == (
        "image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix",
        "sh_degree", "campos", "prefiltered", "debug")


def _settings(cam, bg, deg):
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float32))
    return GaussianRasterizationSettings(cam.image_height, cam.image_width, cam.tanfovx, cam.tanfovy, t(bg), 1.0,
                                         t(cam.world_view_transform), t(cam.full_proj_transform), deg, t(cam.camera_center),
                                         False, False)


def test_product_path_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    sc = synth.make_scene(P=10, width=32, height=32, sh_degree=0, s0=0.1)
    prev = rasterizer._set_backend_for_tests(None)
    try:
        rast = GaussianRasterizer(raster_settings=_settings(sc.camera, sc.bg, 0))
        t = lambda a: torch.tensor(a)
        with pytest.raises(RuntimeError, match="HIP device|no CPU fallback"):
            rast(means3D=t(sc.means3D), means2D=torch.zeros(10, 3), opacities=t(sc.opacities), shs=t(sc.shs),
                 scales=t(sc.scales), rotations=t(sc.rotations))
    finally:
        rasterizer._set_backend_for_tests(prev)


@pytest.fixture
def oracle_backend():
    prev = rasterizer._set_backend_for_tests(OracleBackend())
    yield
    rasterizer._set_backend_for_tests(prev)


def test_validation_messages(oracle_backend):
    sc = synth.make_scene(P=10, width=32, height=32, sh_degree=0, s0=0.1)
    rast = GaussianRasterizer(raster_settings=_settings(sc.camera, sc.bg, 0))
    t = lambda a: torch.tensor(a)
    with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
        rast(means3D=t(sc.means3D), means2D=torch.zeros(10, 3), opacities=t(sc.opacities), scales=t(sc.scales), rotations=t(sc.rotations))
    with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
        rast(means3D=t(sc.means3D), means2D=torch.zeros(10, 3), opacities=t(sc.opacities), shs=t(sc.shs),
             colors_precomp=torch.zeros(10, 3), scales=t(sc.scales), rotations=t(sc.rotations))
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair or precomputed 3D covariance"):
        rast(means3D=t(sc.means3D), means2D=torch.zeros(10, 3), opacities=t(sc.opacities), shs=t(sc.shs))
    with pytest.raises(RuntimeError, match="means3D must have dimensions"):
        rast(means3D=torch.zeros(10, 4), means2D=torch.zeros(10, 3), opacities=t(sc.opacities), shs=t(sc.shs),
             scales=t(sc.scales), rotations=t(sc.rotations))
    with pytest.raises(RuntimeError, match="float32"):
        rast(means3D=t(sc.means3D).double(), means2D=torch.zeros(10, 3), opacities=t(sc.opacities), shs=t(sc.shs),
             scales=t(sc.scales), rotations=t(sc.rotations))


def test_render_wrapper_dict_and_means2d_gradient(oracle_backend):
    """render() restates gaussian_renderer/__init__.py:18-100: dict keys, retain_grad on the dummy
    screenspace tensor, densification statistic of scene/gaussian_model.py:405-407."""
    sc = synth.make_scene(P=300, width=48, height=40, sh_degree=2, s0=0.08, seed=3)
    pc = GaussianParams.from_synthetic(sc, "cpu")
    cam = TorchCamera(sc.camera, "cpu")
    pkg = render(cam, pc, PipelineParams(), torch.tensor(sc.bg))
    assert set(pkg) == {"render", "viewspace_points", "visibility_filter", "radii"}
    assert pkg["render"].shape == (3, 40, 48) and pkg["radii"].dtype == torch.int32 and pkg["visibility_filter"].dtype == torch.bool
    (pkg["render"] * torch.tensor(sc.dL_dimage)).sum().backward()
    vsp = pkg["viewspace_points"]
    assert vsp.grad is not None and vsp.grad.shape == (300, 3) and float(vsp.grad[:, 2].abs().max()) == 0.0
    for p in pc.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all()
    pc.add_densification_stats(vsp, pkg["visibility_filter"])
    assert float(pc.denom.sum()) == float(pkg["visibility_filter"].sum())
    # the two optional Python paths of the wrapper give the same image
    img0 = pkg["render"].detach()
    img1 = render(cam, pc, PipelineParams(convert_SHs_python=True), torch.tensor(sc.bg))["render"].detach()
    img2 = render(cam, pc, PipelineParams(compute_cov3D_python=True), torch.tensor(sc.bg))["render"].detach()
    assert float((img0 - img1).abs().max()) < 1e-5 and float((img0 - img2).abs().max()) < 1e-5
    with torch.no_grad():
        img3 = render(cam, pc, PipelineParams(), torch.tensor(sc.bg), scaling_modifier=0.5)["render"]
    assert not img3.requires_grad and float((img3 - img0).abs().max()) > 1e-3


def test_gradient_arena_views(oracle_backend):
    """Backward can write the parameter gradients straight into one flat bucket (no packing copy)."""
    from gaussian_transformer_amd.rasterizer import arena_floats, gradient_arena
    sc = synth.make_scene(P=50, width=32, height=32, sh_degree=1, s0=0.1, max_sh_degree=1)
    t = lambda a: torch.tensor(a).requires_grad_(True)
    inp = dict(means3D=t(sc.means3D), shs=t(sc.shs), opacities=t(sc.opacities), scales=t(sc.scales), rotations=t(sc.rotations))
    rast = GaussianRasterizer(raster_settings=_settings(sc.camera, sc.bg, 1))
    dL = torch.tensor(sc.dL_dimage)
    c, _ = rast(means2D=torch.zeros(50, 3, requires_grad=True), **inp)
    ref_g = torch.autograd.grad(c, list(inp.values()), grad_outputs=dL)
    # the stand-in backend does not use the arena itself; check the carving helper and size rule
    assert arena_floats(50, 4) == 50 * (3 + 12 + 1 + 3 + 4)
    flat = torch.zeros(arena_floats(50, 4))
    with gradient_arena(flat) as f:
        assert f is flat and rasterizer._grad_arena is flat
    assert rasterizer._grad_arena is None
    assert all(torch.isfinite(g).all() for g in ref_g)


def test_every_option_the_library_accepts_is_documented_in_the_header():
    """include/gsr.h is the contract: a knob gsr_set_option / gsr_get_option knows must be described there."""
    import os, re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    api = open(os.path.join(root, "gaussian_transformer_amd", "csrc", "gsr_api.hip")).read()
    hdr = open(os.path.join(root, "include", "gsr.h")).read()
    rows = re.findall(r'^\s*\{"([a-z_0-9]+)", &g_[a-z_]+, OPT_[A-Z_0-9]+,', api, flags=re.M)      # the option table
    explicit = re.findall(r'strcmp\(name, "([a-z_0-9]+)"\)', api)                                # the irregular ones beside it
    assert len(rows) == len(set(rows)) and len(rows) > 10 and len(set(explicit)) >= 6
    names = sorted(set(rows) | set(explicit))
    assert len(names) > 15
    missing = [n for n in names if f'"{n}"' not in hdr]
    assert not missing, missing


BOOLEAN_OPTIONS = ("exact_tile_cull", "two_level_sort", "deterministic_bwd", "fill_in_tail", "asm_walk", "bwd_lpt")
# name -> (values accepted and read back unchanged, values refused, the refusal's text)
CHECKED_OPTIONS = {
    **{n: ((0, 1, 2), (-1, 3), f"{n} must be 0, 1 or 2")
       for n in ("tile_lists", "persistent_bwd", "prefill_at", "dense_fork", "dense_pergauss", "depth_buckets")},
    **{n: ((1, 2, 4), (0, 3, 8, -2), f"{n} must be 1, 2 or 4")
       for n in ("composite_waves_per_block", "fwd_blocks_per_wave", "bwd_blocks_per_wave")},
    "segment_entries": ((0, 64, 256, 65536), (-64, 63, 100, 65600), "segment_entries must be 0 or a multiple of 64 up to 65536"),
}
# name -> (value set, value read back): the options that map what they are given instead of refusing it
MAPPED_OPTIONS = {
    **{n: ((0, 0), (1, 1), (7, 1), (-3, 1)) for n in BOOLEAN_OPTIONS + ("depth_log_map",)},
    "count_lanes": ((0, 0), (1, 1), (2, 2), (5, 1), (-1, 1)),
    "fwd_pair_long": ((-1, -1), (0, 0), (64, 64), (100000, 100000), (-7, -1)),
}


def test_option_table_round_trip():
    """Every option by name: what gsr_set_option accepts is what gsr_get_option reads back, a refusal has its exact text and changes
    nothing, the read-only and the set-only names are unknown to the other function, and every value is put back."""
    lib = _lib.load()
    err = lambda: lib.gsr_last_error().decode()

    def get(name):
        v = ctypes.c_int32(-12345)
        assert lib.gsr_get_option(name.encode(), ctypes.byref(v)) == 0, name
        return v.value
    for name, (legal, illegal, text) in CHECKED_OPTIONS.items():
        prev = get(name)
        try:
            for v in legal:
                assert lib.gsr_set_option(name.encode(), v) == 0 and get(name) == v, (name, v)
                for bad in illegal:
                    assert lib.gsr_set_option(name.encode(), bad) == 1 and err() == text and get(name) == v, (name, bad)
        finally:
            assert lib.gsr_set_option(name.encode(), prev) == 0
    for name, pairs in MAPPED_OPTIONS.items():
        prev = get(name)
        try:
            for v, back in pairs:
                assert lib.gsr_set_option(name.encode(), v) == 0 and get(name) == back, (name, v)
        finally:
            assert lib.gsr_set_option(name.encode(), prev) == 0
    # set-only: accepted (negative values mean 0), unknown to gsr_get_option
    v = ctypes.c_int32(-12345)
    try:
        for pad in (128, -5, 0):
            assert lib.gsr_set_option(b"composite_lds_pad", pad) == 0
        assert lib.gsr_get_option(b"composite_lds_pad", ctypes.byref(v)) == 1 and v.value == -12345
        assert err() == "gsr_get_option: unknown option 'composite_lds_pad'"
    finally:
        assert lib.gsr_set_option(b"composite_lds_pad", 0) == 0
    # read-only: unknown to gsr_set_option
    for name in ("pergauss_path", "poll_timeouts"):
        before = get(name)
        assert lib.gsr_set_option(name.encode(), 1) == 1 and err() == f"gsr_set_option: unknown option '{name}'"
        assert get(name) == before
    # unknown and missing names, a missing destination
    assert lib.gsr_set_option(b"no_such_option", 1) == 1 and err() == "gsr_set_option: unknown option 'no_such_option'"
    assert lib.gsr_get_option(b"no_such_option", ctypes.byref(v)) == 1 and err() == "gsr_get_option: unknown option 'no_such_option'"
    assert lib.gsr_set_option(b"", 1) == 1 and err() == "gsr_set_option: unknown option ''"
    assert lib.gsr_set_option(None, 1) == 1 and err() == "gsr_set_option: unknown option '(null)'"
    assert lib.gsr_get_option(None, ctypes.byref(v)) == 1 and err() == "gsr_get_option: unknown option '(null)'"
    assert lib.gsr_get_option(b"tile_lists", None) == 1 and err() == "gsr_get_option: unknown option 'tile_lists'"
    assert lib.gsr_get_option(b"pergauss_path", None) == 1 and err() == "gsr_get_option: unknown option 'pergauss_path'"
    assert v.value == -12345
    # the three lists above are the library's whole option surface (the header test reads the same names out of the source)
    api = open(os.path.join(ROOT, "gaussian_transformer_amd", "csrc", "gsr_api.hip")).read()
    known = set(re.findall(r'^\s*\{"([a-z_0-9]+)", &g_', api, flags=re.M)) | set(re.findall(r'strcmp\(name, "([a-z_0-9]+)"\)', api))
    assert known == set(CHECKED_OPTIONS) | set(MAPPED_OPTIONS) | {"composite_lds_pad", "pergauss_path", "poll_timeouts"}
