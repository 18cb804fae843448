"""The workspace size queries that never call into the HIP runtime, pinned to literal values.  No device is needed and none is used.

Every number below was recorded from the library of the commit BEFORE the workspace layouts came to be written with one carver
(gsr_internal.h: Bump) and one layout function each (carve_backward, l1_carve, views_carve, depth's and pose's views) -- built from
that commit and asked through this same ctypes binding -- not from the code under test: a layout function that moves an offset, drops
a rounding or adds one shows here.  Two roundings are easy to lose: the backward workspace's last piece (the dense stage's records) ends
unrounded, and gsr_backward_workspace_bytes sizes deterministic mode's slots from the options as they are when it is called (off by
default: R does not enter).  The three queries that ask rocPRIM for a temporary size want a device: tests/test_gpu_cabi.py pins those.
"""
import ctypes as C

import pytest

from gaussian_transformer_amd import _lib

PS = (0, 1, 63, 64, 1023, 1024, 500000)
BACKWARD = {0: 66048, 1: 81664, 63: 85504, 64: 85760, 1023: 383232, 1024: 383232, 500000: 66523392}      # the same for R in 0, 1, 12345
L1_SSIM = {(1, 1, 1): 512, (3, 16, 16): 9472, (3, 17, 1): 1024, (3, 37, 29): 38912}                      # (C, H, W)
VIEWS_LOSS = {(1, 1, 1): 1024, (1, 16, 16): 9984, (1, 37, 29): 39424, (3, 1, 1): 1024, (3, 16, 16): 28416, (3, 37, 29): 117248,
              (16, 1, 1): 2304, (16, 16, 16): 148992, (16, 37, 29): 622592, (17, 1, 1): 2304, (17, 16, 16): 158208,
              (17, 37, 29): 661504}                                                                      # (B, H, W)
CHAMFER = {(1, 1, 1): 16, (2, 5, 7): 192}                                                                # (B, N, M)
DEPTH = {0: 65792, 1: 66048, 63: 74752, 64: 75008, 1023: 215040, 1024: 215040, 500000: 73065728}
POSE = {0: 256, 1: 256, 63: 256, 64: 256, 1023: 1024, 1024: 1024, 500000: 500224}


def ask(name, *args):
    lib, n = _lib.load(), C.c_size_t()
    assert getattr(lib, name)(*args, C.byref(n)) == 0, (name, args, lib.gsr_last_error())
    return n.value


@pytest.mark.parametrize("R", (0, 1, 12345))
def test_backward_workspace_bytes(R):
    assert {P: ask("gsr_backward_workspace_bytes", P, R) for P in PS} == BACKWARD


@pytest.mark.parametrize("name, want", [("gsr_l1_ssim_workspace", L1_SSIM), ("gsr_views_loss_workspace", VIEWS_LOSS),
                                        ("gsr_chamfer_workspace", CHAMFER)])
def test_loss_and_chamfer_workspaces(name, want):
    assert {k: ask(name, *k) for k in want} == want


@pytest.mark.parametrize("name, want", [("gsr_depth_workspace_bytes", DEPTH), ("gsr_pose_workspace_bytes", POSE)])
def test_depth_and_pose_workspaces(name, want):
    assert tuple(want) == PS
    assert {P: ask(name, P) for P in PS} == want
