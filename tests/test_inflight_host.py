"""tests/inflight.py on the CPU: the step builder and the expectations of tests/test_gpu_inflight.py run on the oracle-backed
stand-in (orders A, C and D; expectations 1 and 3), and the expectations must reject three planted faults -- a stand-in that hands
render i the gradients of render i - 1, one that drops a render's contribution, one that leaves a NaN row where no gradient
exists.  The proof that the GPU test can fail; no library is built or run.  Also on the CPU: case F's step (one GaussianParams,
judged in raw-parameter space) with every camera through render(), the bookkeeping of gradient-arena claims, and the check that
decides whether a gradient arena can hold a render's gradients."""
import numpy as np
import pytest
import torch

from gaussian_transformer_amd import rasterizer
from tests import inflight as fl
from tests.oracle_backend import OracleBackend


@pytest.fixture(scope="module")
def backend():
    be = OracleBackend("f32")
    prev = rasterizer._set_backend_for_tests(be)
    yield be
    rasterizer._set_backend_for_tests(prev)


@pytest.fixture(scope="module")
def fx(backend):
    f = fl.Fixture("cpu")
    f.lones = [f.lone("pred", i) for i in range(fl.B)]
    return f


@pytest.mark.parametrize("order", ["one", "forward", "retain"])
def test_step_orders_per_render_leaves(fx, order):
    """A and C on per-render leaf copies: every render of the step under assert_parity; the stand-in's reverse pass is a fixed
    single-threaded sum, so each render also equals the lone render bit for bit."""
    step = fl.run_step(fx, shared=False, order=order)
    fl.expect_step_parity(fx, step, order)
    for i in range(fl.B):
        fl.expect_bit_equal(fx.lones[i], step["renders"][i], f"{order} {i}")
    if order == "retain":
        fl.expect_bit_equal(fx.lones[0], dict(step["renders"][0], grads=step["again"]), "second backward of render 0")


@pytest.mark.parametrize("order", ["one", "forward"])
def test_step_orders_shared_leaves(fx, order):
    step = fl.run_step(fx, shared=True, order=order)
    fl.expect_shared_sum(fx.lones, step, order)


def test_no_grad_block_in_the_middle(fx):
    """D: B forward-only renders of a third scene between the forwards and the backward."""
    logged = []
    step = fl.run_step(fx, shared=False, middle=lambda: logged.extend(fl.forward_only(fx, "logged")))
    fl.expect_step_parity(fx, step, "D")
    for i in range(fl.B):
        fl.expect_forward_only(fx, "logged", i, logged[i], "D")
    shared = fl.run_step(fx, shared=True, middle=lambda: fl.forward_only(fx, "logged"))
    fl.expect_shared_sum(fx.lones, shared, "D")


def test_raw_leaves_through_render(backend):
    """Case F's builder and expectations with all B cameras through render() (the stand-in has no fused entry point): torch's
    activations and their autograd around the rasterizer meet the float64 chain of tests/fused_ref.py under assert_parity, each
    in-flight render equals the lone one, and ONE GaussianParams accumulates the float64 sum within its bound -- and the bound
    rejects a sum that lacks one render."""
    mx = fl.MixedStep("cpu", ("render",) * fl.B)
    lones = [mx.lone(i) for i in range(fl.B)]
    step = mx.step(shared=False)
    for i in range(fl.B):
        fl.expect_raw_parity(mx, i, step["renders"][i], "F host")
        fl.expect_bit_equal(lones[i], step["renders"][i], f"F host {i}", keys=fl.RAW)
    shared = mx.step(shared=True)
    fl.expect_shared_sum(lones, shared, "F host", keys=fl.RAW, bounds=dict(rotation=mx.rotation_sum_bound(lones)))
    short = dict(shared, shared={k: v - lones[2]["grads"][k] for k, v in shared["shared"].items()})
    with pytest.raises(AssertionError, match="F host short"):
        fl.expect_shared_sum(lones, short, "F host short", keys=fl.RAW, bounds=dict(rotation=mx.rotation_sum_bound(lones)))
    with pytest.raises(AssertionError):
        fl.expect_raw_parity(mx, 1, dict(step["renders"][1], grads=step["renders"][0]["grads"]), "F host swapped")


def test_arena_claims_overlap_release_and_expiry():
    """HipBackend._claim_arena / _release_arena (host bookkeeping only: no library is loaded): overlapping memory is refused while
    the owner's workspace is alive, whether or not it was released; disjoint memory is not; a claim ends with release or with
    the owner's workspace (a render whose graph died without a backward call)."""
    from gaussian_transformer_amd import _lib
    be = object.__new__(rasterizer.HipBackend)
    be._arena_claims = {}
    flat = torch.zeros(64)
    g1, g2 = torch.zeros(8, dtype=torch.uint8), torch.zeros(8, dtype=torch.uint8)
    be._claim_arena(flat[:32], g1)
    with pytest.raises(_lib.GsrError, match="still owned by another render in flight"):
        be._claim_arena(flat[16:48], g2)
    with pytest.raises(_lib.GsrError, match="still owned by another render in flight"):
        be._claim_arena(flat[:32], g2)
    be._claim_arena(flat[32:], g2)                       # adjacent, not overlapping
    be._release_arena(g1)
    g3 = torch.zeros(8, dtype=torch.uint8)
    be._claim_arena(flat[:32], g3)                       # released by its owner's backward call
    with pytest.raises(_lib.GsrError):
        be._claim_arena(flat[:8], g1)
    del g3                                               # the owner's graph is gone: it never ran backward, and never will
    be._claim_arena(flat[:8], g1)
    assert len(be._arena_claims) == 2


@pytest.mark.parametrize("has_sr", (True, False))
@pytest.mark.parametrize("M", (0, 1, 16))
def test_arena_is_accepted_from_exactly_arena_floats_elements_float32_and_dense(M, has_sr):
    """The one check behind HipBackend.forward (which only stops announcing), backward and depth_backward (which raise): the
    boundary is arena_floats(P, M, has_sr) = P (3 + 3 M + 1 + 7 with scales and rotations) elements, one short is refused."""
    from gaussian_transformer_amd import _lib
    P = 5
    n = P * (4 + 3 * M + (7 if has_sr else 0))
    assert rasterizer.arena_floats(P, M, has_sr) == n
    cpu = torch.device("cpu")
    fits = lambda t: rasterizer._arena_fits(t, cpu, P, M, has_sr)
    assert fits(torch.zeros(n)) and fits(torch.zeros(n + 3)) and not fits(torch.zeros(n - 1))
    assert not fits(torch.zeros(n, dtype=torch.float64)) and not fits(torch.zeros(n, dtype=torch.float16))
    assert not fits(torch.zeros(2 * n)[::2]) and fits(torch.zeros(2 * n)[n:])          # a strided view; a dense slice
    assert not fits(torch.zeros(n, device="meta"))                                     # another device than the render's
    for bad in (torch.zeros(n - 1), torch.zeros(n, dtype=torch.float64), torch.zeros(2 * n)[::2]):
        with rasterizer.gradient_arena(bad):
            with pytest.raises(_lib.GsrError, match=f"gradient arena must be a contiguous float32 tensor on the render device with at least {n} elements"):
                rasterizer._usable_arena(cpu, P, M, has_sr)
    good = torch.zeros(n)
    with rasterizer.gradient_arena(good):
        assert rasterizer._usable_arena(cpu, P, M, has_sr) is good
    assert rasterizer._usable_arena(cpu, P, M, has_sr) is None                         # none set: nothing to refuse


# ---- planted faults -----------------------------------------------------------------------------------------------------------
class _Faulty(OracleBackend):
    """The stand-in with a fault in the gradients of the prediction renders (recognised by their P), counted in forward order."""

    def __init__(self, fault, P):
        super().__init__("f32")
        self.fault, self.P, self.order = fault, P, []

    def forward(self, rs, means3D, *a, **kw):
        out = super().forward(rs, means3D, *a, **kw)
        if means3D.shape[0] == self.P:
            self.order.append(int(out[3][0]))
        return out

    def backward(self, rs, num_rendered, dL_dpix, means3D, radii, *a):
        geom = a[-3]
        i = self.order.index(int(geom[0]))
        if self.fault == "previous" and i > 0:        # render i is handed what belongs to render i - 1 (its state, this call's dL)
            a = a[:-3] + (torch.tensor([self.order[i - 1]], dtype=torch.int64),) + a[-2:]
        g = list(super().backward(rs, num_rendered, dL_dpix, means3D, radii, *a))
        if self.fault == "dropped" and i == 2:
            g = [torch.zeros_like(x) for x in g]
        if self.fault == "nan_row" and i == 1:
            row = int(np.nonzero(radii.numpy() == 0)[0][0])
            g[5] = g[5].clone(); g[5][row] = float("nan")          # dL/dscales of a culled Gaussian
        return tuple(g)


def _faulty_step(fx, fault, shared):
    be = _Faulty(fault, fx.scenes["pred"].P)
    prev = rasterizer._set_backend_for_tests(be)
    try:
        return fl.run_step(fx, shared=shared)
    finally:
        rasterizer._set_backend_for_tests(prev)


def test_expectations_reject_the_previous_renders_gradients(fx):
    step = _faulty_step(fx, "previous", shared=False)
    fl.expect_parity(fx, 0, step["renders"][0], "planted")                 # render 0 has no predecessor: untouched, and accepted
    for i in range(1, fl.B):
        with pytest.raises(AssertionError):
            fl.expect_parity(fx, i, step["renders"][i], "planted")
        with pytest.raises(AssertionError):
            fl.expect_bit_equal(fx.lones[i], step["renders"][i], "planted")
    with pytest.raises(AssertionError, match="shared"):
        fl.expect_shared_sum(fx.lones, _faulty_step(fx, "previous", shared=True), "planted shared")


def test_expectations_reject_a_dropped_contribution(fx):
    shared = _faulty_step(fx, "dropped", shared=True)
    with pytest.raises(AssertionError, match="planted shared"):
        fl.expect_shared_sum(fx.lones, shared, "planted shared")
    step = _faulty_step(fx, "dropped", shared=False)
    for i in range(fl.B):
        if i == 2:
            with pytest.raises(AssertionError):
                fl.expect_parity(fx, i, step["renders"][i], "planted")
        else:
            fl.expect_parity(fx, i, step["renders"][i], "planted")


def test_expectations_reject_a_nan_row_where_no_gradient_exists(fx):
    step = _faulty_step(fx, "nan_row", shared=False)
    with pytest.raises(AssertionError, match="gradient scales is not finite in 3 elements"):
        fl.expect_parity(fx, 1, step["renders"][1], "planted")
    with pytest.raises(AssertionError):
        fl.expect_bit_equal(fx.lones[1], step["renders"][1], "planted")
    fl.expect_parity(fx, 0, step["renders"][0], "planted")
    shared = _faulty_step(fx, "nan_row", shared=True)
    with pytest.raises(AssertionError, match="scales"):
        fl.expect_shared_sum(fx.lones, shared, "planted shared")
