"""-m gpu: a plain C program (tests/cabi/c_client.c) drives libgsr_hip.so directly -- no Python, no
torch, no C++ types across the boundary -- including the error paths (codes, not aborts)."""
import pytest

from tests import cabi_client as cc

pytestmark = pytest.mark.gpu


def test_plain_c_client_renders_and_differentiates(tmp_path):
    cc.run(cc.build(tmp_path, "c_client"))


def test_workspace_sizes_are_what_they_were():
    """gsr_workspace_sizes and gsr_binning_bytes ask rocPRIM for its temporary sizes, which wants a device (tests/test_cabi_refusals_host.py
    pins what needs none).  The numbers were recorded on an MI355X from the library before gsr_api.hip's carve functions came to share
    one bump allocator and its entry points one geometry-view helper: offsets and alignments must not have moved."""
    import ctypes as C

    from gaussian_transformer_amd import _lib
    lib = _lib.load()
    geom = {0: 16951808, 1: 16951808, 1023: 17152768, 1024: 17152768, 500000: 122013952}
    bwd = {0: 65792, 1: 65792, 1023: 133120, 1024: 133120, 500000: 33065728}
    img = {(16, 16): 1153792, (17, 1): 1152256, (800, 800): 27577600, (1920, 1080): 87323904}
    binning = {0: 1536, 1: 1536, 1023: 28928, 1024: 28928, 500000: 20004352}       # the same for every image size below
    for P in geom:
        for (W, H) in img:
            g, i, b, n = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
            assert lib.gsr_workspace_sizes(P, W, H, C.byref(g), C.byref(i), C.byref(b)) == 0
            assert (g.value, i.value, b.value) == (geom[P], img[W, H], bwd[P]), (P, W, H)
            assert lib.gsr_binning_bytes(P, W, H, C.byref(n)) == 0 and n.value == binning[P], (P, W, H)
    # likewise the three other queries that ask rocPRIM, recorded on an MI355X from the library before kNN's, the box sort's and the
    # densify plan's carve functions took that allocator over from their own (the queries without rocPRIM: tests/test_workspace_sizes_host.py)
    for name, want in (("gsr_knn_workspace", {(1,): 1792, (1024,): 13312, (1025,): 22272, (100000,): 2003200}),                 # N
                       ("gsr_densify_plan_workspace", {(1, 1): 4352, (1024, 2): 37376, (100000, 2): 3309056}),                # (P, N)
                       ("gsr_box_sort_workspace", {(1, 1): 1024, (1024, 8): 12544, (100000, 128): 2000384})):                # (P, n)
        for args, bytes_ in want.items():
            n = C.c_size_t()
            assert getattr(lib, name)(*args, C.byref(n)) == 0 and n.value == bytes_, (name, args, n.value)
