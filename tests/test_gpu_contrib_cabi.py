"""-m gpu: a plain C program (tests/cabi/contrib_client.c) drives gsr_forward, gsr_contrib_accumulate and gsr_contrib_read of
libgsr_hip.so directly on depth_ref.SCENES[2] (P = 500, 64 x 48): every refusal of the two calls with its code and its text, in the
header's order, on rows that hold a pattern and must keep it; P == 0 and R == 0; the all-NULL read; then one view and the same view
again, whose rows the Python side compares byte for byte with the public collector's and with integer arithmetic."""
import numpy as np
import pytest
import torch

from gaussian_transformer_amd.rasterizer import ContributionStats, GaussianRasterizer, collect_contribution
from tests import cabi_client as cc
from tests import depth_ref as dr
from tests.test_gpu_depth import scene, tensors

pytestmark = pytest.mark.gpu
ROW = np.dtype([("sum_q32", "<u8"), ("max_bits", "<u4"), ("count", "<u4")])


def test_plain_c_client_contrib(tmp_path):
    S = scene(dr.SCENES[2])
    P = int(np.asarray(S.means3D).shape[0])
    assert S.scale_modifier == 1.0                                      # depth_ref's scenes are unscaled
    prob, res = tmp_path / "problem.bin", tmp_path / "result.bin"
    with open(prob, "wb") as f:
        cc.write_scene(f, S)
    cc.run(cc.build(tmp_path, "contrib_client"), prob, res)
    got = cc.read_result(res, [("R", np.int64, ()), ("one", ROW, (P,)), ("two", ROW, (P,)), ("w_sum", np.float32, (P,)), ("w_max", np.float32, (P,)),
                               ("n_pix", np.int32, (P,))])
    one, two, w_sum, w_max, n_pix = (got[k] for k in ("one", "two", "w_sum", "w_max", "n_pix"))
    assert int(got["R"]) > 0

    # the public collector on the same scene: the same bytes
    rs, inp = tensors(S, grad=False)
    st = ContributionStats(P, "cuda")
    with collect_contribution(st), torch.no_grad():
        GaussianRasterizer(rs)(**inp)
    want = st.rows.cpu().numpy().view(ROW).reshape(P)
    assert want["count"].any()
    np.testing.assert_array_equal(one, want)
    # the same view again, in integers
    np.testing.assert_array_equal(two["sum_q32"], 2 * one["sum_q32"])
    np.testing.assert_array_equal(two["count"], 2 * one["count"])
    np.testing.assert_array_equal(two["max_bits"], one["max_bits"])
    # the three outputs, read by two calls with NULLs among them
    np.testing.assert_array_equal(w_sum, (two["sum_q32"].astype(np.float64) * 2.0 ** -32).astype(np.float32))
    np.testing.assert_array_equal(w_max.view(np.uint32), two["max_bits"])
    np.testing.assert_array_equal(n_pix, two["count"].astype(np.int32))
