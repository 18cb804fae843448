"""-m gpu: a plain C program (tests/cabi/views_loss_client.c) drives gsr_views_loss_* of libgsr_hip.so directly -- the error paths, then
forward and backward on B = 3 views of 37 x 29 -- and prints the three numbers the Python call returns, bit for bit."""
import numpy as np
import pytest
import torch

from gaussian_transformer_amd import loss
from tests import cabi_client as cc
from tests import views_loss_ref as vr

pytestmark = pytest.mark.gpu


def test_plain_c_client_views_loss(tmp_path):
    B, H, W = 3, 37, 29
    img, gt, _ = vr.plant(*vr.noise_views(B, H, W, -0.5, 1.5, 7))
    w_l1, w_ssim = (np.float32(x) for x in vr.reference_weights(B))
    prob, out = tmp_path / "problem.bin", tmp_path / "grads.bin"
    with open(prob, "wb") as f:
        f.write(np.array([B, H, W, 1], dtype=np.int32).tobytes())
        f.write(np.array([w_l1, w_ssim], dtype=np.float32).tobytes())
        f.write(img.tobytes()); f.write(gt.tobytes())
    said = cc.run(cc.build(tmp_path, "views_loss_client"), prob, out).splitlines()
    line = [l for l in said if l.startswith("out3")][0].split()
    got = np.array([int(x, 16) for x in line[1:4]], dtype=np.uint32).view(np.float32)
    # the Python call on the same bytes: the same three numbers (loss, L1, SSIM over all views) and the same gradients, bit for bit
    xs = [torch.tensor(v, device="cuda", requires_grad=True) for v in img]
    L = loss.multi_view_loss(xs, torch.tensor(gt, device="cuda"), float(w_l1), float(w_ssim), sanitize=True)
    L.backward()
    assert got[0] == np.float32(L.detach().cpu().numpy())
    r64 = vr.torch_loss(img, gt, float(w_l1), float(w_ssim), True, torch.float64)
    assert abs(got[1] - r64["terms"][:, 0].mean()) <= 1e-6 and abs(got[2] - r64["terms"][:, 1].mean()) <= 1e-5
    terms = np.array([int(x, 16) for x in [l for l in said if l.startswith("terms")][0].split()[1:]], dtype=np.uint32).view(np.float32)
    assert np.array_equal(terms.reshape(B, 3), L.terms.cpu().numpy())
    grads = np.fromfile(out, dtype=np.float32).reshape(B, 3, H, W)
    assert np.array_equal(grads.view(np.uint32), np.stack([x.grad.cpu().numpy() for x in xs]).view(np.uint32))
