"""The multi-view image loss without a GPU: what multi_view_loss / stacked_image_loss / view_metrics refuse, with their messages, in
the order of gaussian_transformer_amd/sequence.py -- types, dtypes, shapes, equal view sizes and matching counts first, devices last
(there is no CPU fallback) -- and that header, ctypes table and build table name the new entry points."""
import os
import re

import pytest
import torch

from gaussian_transformer_amd import _lib, build, loss
from gaussian_transformer_amd._lib import GsrError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def v(h=8, w=9, dtype=torch.float32):
    return torch.zeros((3, h, w), dtype=dtype)


CALLS = {
    "multi_view_loss": lambda i, t: loss.multi_view_loss(i, t, 0.8, 0.2),
    "stacked_image_loss": lambda i, t: loss.stacked_image_loss(i, t),
    "view_metrics": lambda i, t: loss.view_metrics(i, t),
}


@pytest.mark.parametrize("who", list(CALLS))
def test_validation_messages(who):
    call = CALLS[who]
    bad = [
        (5, [v()], "images must be a sequence of tensors or one \\[B,3,H,W\\] tensor, got int"),
        ([v()], None, "targets must be a sequence of tensors or one \\[B,3,H,W\\] tensor, got NoneType"),
        ([], [], "images is empty"),
        ([v(), "x"], [v(), v()], "images\\[1\\] must be a torch.Tensor, got str"),
        ([v(), v(dtype=torch.float64)], [v(), v()], "images\\[1\\] must be float32, got float64"),
        ([v()], [v(dtype=torch.float16)], "targets\\[0\\] must be float32, got float16"),
        (torch.zeros((2, 3, 8, 9), dtype=torch.float64), [v(), v()], "images must be float32, got float64"),
        ([torch.zeros((4, 8, 9))], [v()], "images\\[0\\] must have shape \\[3,H,W\\], got \\(4, 8, 9\\)"),
        ([torch.zeros((3, 8))], [v()], "images\\[0\\] must have shape \\[3,H,W\\], got \\(3, 8\\)"),
        ([torch.zeros((3, 0, 9))], [torch.zeros((3, 0, 9))], "images\\[0\\] must have shape \\[3,H,W\\], got \\(3, 0, 9\\)"),
        (torch.zeros((3, 8, 9)), [v()], "images must be a sequence of \\[3,H,W\\] tensors or one \\[B,3,H,W\\] tensor with B >= 1, got shape \\(3, 8, 9\\)"),
        (torch.zeros((0, 3, 8, 9)), [v()], "with B >= 1, got shape \\(0, 3, 8, 9\\)"),
        (torch.zeros((2, 4, 8, 9)), [v(), v()], "images must be a sequence of \\[3,H,W\\] tensors or one \\[B,3,H,W\\] tensor"),
        ([v(), v(8, 10)], [v(), v()], "all views must have one size: images\\[1\\] is \\(3, 8, 10\\), images\\[0\\] is \\(3, 8, 9\\)"),
        ([v(), v()], [v(), v(7, 9)], "all views must have one size: targets\\[1\\] is \\(3, 7, 9\\)"),
        ([v(), v()], [v()], "2 images but 1 targets"),
        (torch.zeros((3, 3, 8, 9)), [v(), v()], "3 images but 2 targets"),
        ([v()], [v(9, 8)], "images are 8 x 9 \\(H x W\\) but targets are 9 x 8"),
    ]
    for images, targets, msg in bad:
        with pytest.raises(GsrError, match=who + ": " + ".*" + msg):
            call(images, targets)


@pytest.mark.parametrize("who", list(CALLS))
def test_devices_are_checked_last_and_there_is_no_cpu_fallback(who):
    call = CALLS[who]
    with pytest.raises(GsrError, match=who + ": images\\[0\\] must be on a HIP device, got cpu \\(no CPU fallback\\)"):
        call([v(), v()], [v(), v()])
    with pytest.raises(GsrError, match=who + ": images must be on a HIP device, got cpu"):
        call(torch.zeros((2, 3, 8, 9)), torch.zeros((2, 3, 8, 9)))
    # mismatched counts or sizes are refused before any device is looked at (every tensor here is on the CPU)
    with pytest.raises(GsrError, match="2 images but 3 targets"):
        call([v(), v()], [v(), v(), v()])
    with pytest.raises(GsrError, match="all views must have one size"):
        call([v(), v(5, 5)], [v(), v()])


def test_reference_weights():
    assert loss.STACKED_W_L1 == 5.0 * 0.1 and loss.STACKED_W_SSIM == 0.2 * 0.1


def test_header_ctypes_table_and_build_table_agree():
    header = open(os.path.join(ROOT, "include", "gsr_loss.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decls = dict(re.findall(r"int32_t\s+(gsr_views_loss_[a-z_]+)\s*\(([^;]*)\)\s*;", code))
    assert set(decls) == {"gsr_views_loss_workspace", "gsr_views_loss_forward", "gsr_views_loss_backward"}
    for name, args in decls.items():
        assert len(_lib.SIGNATURES[name][1]) == len(args.split(",")), name
    m = re.search(r"#define\s+GSR_VIEWS_LOSS_MAX_B\s+(\d+)", header)
    assert m and int(m.group(1)) == loss.MAX_VIEWS_PER_LAUNCH
    internal = open(os.path.join(ROOT, "gaussian_transformer_amd", "csrc", "gsr_internal.h")).read()
    assert int(re.search(r"#define\s+GSR_VIEWS_MAX_B\s+(\d+)", internal).group(1)) == loss.MAX_VIEWS_PER_LAUNCH
    assert "ssim_loss.hip" in build.SOURCES


def test_library_exports_the_entry_points():
    import ctypes
    lib = ctypes.CDLL(build.build_hip())
    for name in ("gsr_views_loss_workspace", "gsr_views_loss_forward", "gsr_views_loss_backward"):
        assert hasattr(lib, name), name


def test_invalid_arguments_are_refused_before_anything_is_launched():
    """The argument checks of gsr_views_loss_* need no device: every refused call returns GSR_ERR_INVALID_ARGUMENT (1) with a message."""
    import ctypes as C
    lib = _lib.load()
    nb = C.c_size_t()
    assert lib.gsr_views_loss_workspace(3, 37, 29, C.byref(nb)) == 0
    tiles = 3 * 2
    assert nb.value >= 36 * 3 * 37 * 29 + 36 * 3 * tiles and nb.value % 256 == 0
    fake = (C.c_void_p * 3)(256, 512, 768)            # never dereferenced: every call below is refused first
    hole = (C.c_void_p * 3)(256, None, 768)
    out = C.c_void_p(1024)
    fwd = lambda B, H, W, imgs, gts, ws, n: lib.gsr_views_loss_forward(None, B, H, W, imgs, gts, 0.5, 0.5, 1, out, out, ws, n)
    bwd = lambda B, H, W, imgs, gts, ws, n, g: lib.gsr_views_loss_backward(None, B, H, W, imgs, gts, 0.5, 0.5, 1, None, ws, n, g)
    ws = C.c_void_p(4096)
    refused = [
        lib.gsr_views_loss_workspace(0, 37, 29, C.byref(nb)), lib.gsr_views_loss_workspace(3, 0, 29, C.byref(nb)),
        lib.gsr_views_loss_workspace(3, 37, -1, C.byref(nb)), lib.gsr_views_loss_workspace(3, 37, 29, None),
        fwd(0, 37, 29, fake, fake, ws, 1 << 40), fwd(-2, 37, 29, fake, fake, ws, 1 << 40), fwd(3, 0, 29, fake, fake, ws, 1 << 40),
        fwd(3, 37, 0, fake, fake, ws, 1 << 40), fwd(3, 37, 29, None, fake, ws, 1 << 40), fwd(3, 37, 29, fake, None, ws, 1 << 40),
        fwd(3, 37, 29, hole, fake, ws, 1 << 40), fwd(3, 37, 29, fake, hole, ws, 1 << 40), fwd(3, 37, 29, fake, fake, None, 1 << 40),
        fwd(3, 37, 29, fake, fake, ws, nb.value - 1),
        bwd(0, 37, 29, fake, fake, ws, 1 << 40, fake), bwd(3, 37, 29, hole, fake, ws, 1 << 40, fake),
        bwd(3, 37, 29, fake, fake, None, 1 << 40, fake), bwd(3, 37, 29, fake, fake, ws, nb.value - 1, fake),
        bwd(3, 37, 29, fake, fake, ws, 1 << 40, None),
    ]
    assert refused == [1] * len(refused), refused
    assert b"gsr_views_loss_backward" in lib.gsr_last_error()
