"""-m gpu: dist.GradientExchange on the device, fed by the HIP backward pass.

Two gloo ranks in fresh child processes, both on cuda:0 (RCCL refuses two ranks on one device), each render their two cameras per
iteration the way bench.py's step() does -- arena(), forward + backward inside gradient_arena(...), the second camera through a scratch
arena added to the first, the union of the composited masks, launch(visible=union) -- under deterministic_bwd = 1 and
dense_pergauss = 1, so that the announced zero-fill runs on the library's second stream and gradients repeat bit for bit.  This
exercises what only a device runs: the pinned count word and its event, comm_stream (direct + overlap), gloo's asynchronous
all-reduce of device tensors, and an arena zero-filled beside a forward pass while another arena's exchange is in flight.

The parent renders the same cameras itself, with no exchange, on the default stream, and checks
  (a) every rank's pre-exchange arena against its own, bit for bit;
  (b) its per-camera gradients against the float64 oracle (helpers.assert_parity);
  (c) every post-exchange arena against the float32 sum of the two ranks' inputs, bit for bit (two ranks: one rounding, whatever
      the algorithm), identical on both ranks, zero outside the union;
  (d) every non-zero gradient row inside the union of that rank's composited masks."""
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = dict(P=20000, width=320, height=240, sh_degree=3, s0=0.02, seed=93)     # M = 16, no shs_rest: the forward pass zero-fills
ITERS = 3
WORLD = 2
BUCKET_BYTES = (1 << 20) + 20                   # not a multiple of a row (59 floats) nor of any parameter's width
COMBOS = [                                      # side: the compute work runs inside torch.cuda.stream(s) on a non-default stream
    dict(name="sync_allreduce_dense", mode="sync", algo="allreduce", sparse=False, sh_active=None, delayed=False, side=False),
    dict(name="sync_direct_sparse", mode="sync", algo="direct", sparse=True, sh_active=None, delayed=False, side=True),
    dict(name="overlap_allreduce_sparse_delayed", mode="overlap", algo="allreduce", sparse=True, sh_active=None, delayed=True, side=False),
    dict(name="overlap_direct_sparse", mode="overlap", algo="direct", sparse=True, sh_active=None, delayed=False, side=True),
    dict(name="overlap_allreduce_dense_sh4", mode="overlap", algo="allreduce", sparse=False, sh_active=4, delayed=False, side=True),
]

def _degree(combo):
    return 1 if combo["sh_active"] == 4 else 3     # active SH degree 1: only the first 4 coefficient columns get a gradient


def _camera(sc, k):
    """Camera k of 2 * WORLD, yawed about the cloud's centre by an angle of its own (bench.py rank_camera) with half the scene
    camera's field of view: the cameras composite about a third of the Gaussians, so the sparse exchange compacts for real."""
    import math
    from gaussian_transformer_amd.camera import look_at_camera
    ang = (k - (2 * WORLD - 1) / 2.0) * math.radians(12.0)
    centre = np.array([0.0, 0.0, 6.0])
    eye = centre + 6.0 * np.array([math.sin(ang), 0.0, -math.cos(ang)])
    return look_at_camera(eye, centre, (0.0, -1.0, 0.0), 0.5 * sc.camera.FoVx, sc.camera.image_width, sc.camera.image_height)


def _upstream(sc, it):
    H, W = sc.camera.image_height, sc.camera.image_width
    return (np.random.default_rng(500 + it).normal(size=(3, H, W)) / (3.0 * H * W)).astype(np.float32)


class _Renderer:
    def __init__(self, dev):
        from gaussian_transformer_amd import GaussianRasterizationSettings, synth
        from gaussian_transformer_amd.render import TorchCamera
        self.dev = dev
        self.sc = sc = synth.make_scene(**SCENE)
        self.P, self.M = sc.P, sc.shs.shape[1]
        t = lambda a, g=False: torch.tensor(a, dtype=torch.float32, device=dev).requires_grad_(g)
        self.params = dict(means3D=t(sc.means3D, True), opacities=t(sc.opacities, True), shs=t(sc.shs, True),
                           scales=t(sc.scales, True), rotations=t(sc.rotations, True))
        self.cams = [_camera(sc, k) for k in range(2 * WORLD)]
        self.settings = {}
        for deg in (3, 1):
            for k, c in enumerate(self.cams):
                tc = TorchCamera(c, dev)
                self.settings[deg, k] = GaussianRasterizationSettings(
                    image_height=c.image_height, image_width=c.image_width, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=t(sc.bg),
                    scale_modifier=1.0, viewmatrix=tc.world_view_transform, projmatrix=tc.full_proj_transform, sh_degree=deg,
                    campos=tc.camera_center, prefiltered=False, debug=False)
        self.dL = [t(_upstream(sc, it)) for it in range(ITERS)]

    def render(self, deg, k, it, arena):
        """bench.py render_backward(): forward and backward inside gradient_arena(arena), the composited mask in between."""
        from gaussian_transformer_amd import GaussianRasterizer
        from gaussian_transformer_amd.rasterizer import composited_mask, gradient_arena
        m2 = torch.zeros((self.P, 3), dtype=torch.float32, device=self.dev, requires_grad=True)
        with gradient_arena(arena):
            color, radii = GaussianRasterizer(raster_settings=self.settings[deg, k])(means2D=m2, **self.params)
            mask = composited_mask(color)
            grads = torch.autograd.grad(color, list(self.params.values()) + [m2], grad_outputs=self.dL[it])
        assert mask is not None
        return color, radii, mask, grads[-1]

    def rank_step(self, deg, rank, it, arena, scratch):
        """One rank's iteration: its two cameras, the second one's gradients added from a scratch arena (bench.py step())."""
        _, _, m0, _ = self.render(deg, 2 * rank, it, arena)
        _, _, m1, _ = self.render(deg, 2 * rank + 1, it, scratch)
        arena.add_(scratch)
        return m0 | m1


def _rows(flat, P, M):
    """Arena [means3D 3P | shs 3MP | opacities P | scales 3P | rotations 4P] -> [P, 59] rows."""
    out, off = [], 0
    for w in (3, 3 * M, 1, 3, 4):
        out.append(flat[off:off + w * P].reshape(P, w)); off += w * P
    return np.concatenate(out, axis=1)


def _child_main(rank, port, outdir):
    import torch.distributed as dist
    from gaussian_transformer_amd import _lib
    from gaussian_transformer_amd.dist import GradientExchange
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    try:
        _lib.set_option("deterministic_bwd", 1)
        _lib.set_option("dense_pergauss", 1)
        R = _Renderer(dev)
        scratch = None
        for combo in COMBOS:
            deg = _degree(combo)
            n_buffers = 2 if combo["delayed"] else ITERS   # not delayed: every iteration's exchange stays in flight until finish()
            ex = GradientExchange(R.P, R.M, dev, mode=combo["mode"], algo=combo["algo"], bucket_bytes=BUCKET_BYTES, n_buffers=n_buffers)
            if scratch is None:
                scratch = torch.zeros_like(ex.arenas[0])
            s = torch.cuda.Stream(device=dev) if combo["side"] else torch.cuda.current_stream(dev)
            torch.cuda.synchronize()                         # the arenas' and inputs' fills on the default stream are done
            pre, post, unions, launched = [None] * ITERS, [None] * ITERS, [None] * ITERS, []
            with torch.cuda.stream(s):
                for it in range(ITERS):
                    arena = ex.arena()
                    union = R.rank_step(deg, rank, it, arena, scratch)
                    pre[it] = arena.cpu().numpy()
                    unions[it] = union.cpu().numpy()
                    ex.sh_active = combo["sh_active"]
                    ex.launch(visible=union if combo["sparse"] else None)
                    launched.append(arena)
                    if combo["mode"] == "sync":
                        post[it] = arena.cpu().numpy()
                    elif combo["delayed"]:                   # bench.py: wait for the arena launched one step earlier, read it
                        prev = ex.arenas[ex.cur]
                        ex.wait(ex.cur)
                        if it > 0:
                            assert prev is launched[it - 1]
                            post[it - 1] = prev.cpu().numpy()
                ex.finish()
                for it in range(ITERS):
                    if post[it] is None:
                        post[it] = launched[it].cpu().numpy()
            torch.cuda.synchronize()
            np.savez(os.path.join(outdir, f"{combo['name']}_rank{rank}.npz"), pre=np.stack(pre), post=np.stack(post),
                     union=np.stack(unions), overflows=ex.sparse_overflows, union_rows=ex.union_rows)
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


@pytest.mark.timeout(300)
def test_exchange_on_the_device_equals_the_sum_of_the_ranks_renders(tmp_path):
    from gaussian_transformer_amd import _lib
    from tests.helpers import assert_parity, oracle_scene, parity_report
    port = _free_port()
    code = f"import sys; sys.path.insert(0, {ROOT!r}); from tests.test_gpu_dist_exchange import _child_main; " \
           f"_child_main(int(sys.argv[1]), {port}, {str(tmp_path)!r})"
    py = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    errs = [open(tmp_path / f"rank{r}.err", "w+") for r in range(WORLD)]
    procs = [subprocess.Popen(py + ["-c", code, str(r)], cwd=ROOT, stdout=errs[r], stderr=subprocess.STDOUT) for r in range(WORLD)]
    opts = {k: _lib.get_option(k) for k in ("deterministic_bwd", "dense_pergauss")}
    try:
        # the parent's own renders of the same cameras: default stream, no exchange
        _lib.set_option("deterministic_bwd", 1)
        _lib.set_option("dense_pergauss", 1)
        R = _Renderer(torch.device("cuda", 0))
        P, M = R.P, R.M
        expect, hip = {}, None
        for deg in (3, 1):
            for it in range(ITERS):
                for r in range(WORLD):
                    arena = torch.zeros((P * (3 + 3 * M + 8),), dtype=torch.float32, device="cuda")
                    scratch = torch.zeros_like(arena)
                    if (deg, it, r) == (3, 0, 0):            # the first camera's own gradients, for the oracle
                        color, radii, _, g2 = R.render(deg, 0, it, arena)
                        g = _rows(arena.cpu().numpy(), P, M)
                        hip = dict(color=color.detach().cpu().numpy(), radii=radii.cpu().numpy(),
                                   grads=dict(means3D=g[:, :3], shs=g[:, 3:3 + 3 * M].reshape(P, M, 3), opacities=g[:, 3 + 3 * M:4 + 3 * M],
                                              scales=g[:, 4 + 3 * M:7 + 3 * M], rotations=g[:, 7 + 3 * M:], means2D=g2.cpu().numpy()))
                    R.rank_step(deg, r, it, arena, scratch)
                    expect[deg, it, r] = arena.cpu().numpy()
        # (b) the parent's gradients against the float64 oracle
        c = R.cams[0]
        S = oracle_scene(R.sc, W=c.image_width, H=c.image_height, tanfovx=c.tanfovx, tanfovy=c.tanfovy, viewmatrix=c.world_view_transform,
                         projmatrix=c.full_proj_transform, campos=c.camera_center)
        assert_parity(parity_report(S, _upstream(R.sc, 0), hip=hip))
        # the children, each with a time limit; one failing ends the other
        deadline = time.monotonic() + 180
        while time.monotonic() < deadline and any(p.poll() is None for p in procs) and all(p.poll() in (None, 0) for p in procs):
            time.sleep(0.5)
        for r, p in enumerate(procs):
            if p.poll() != 0:
                errs[r].seek(0)
                tail = errs[r].read()[-6000:]
                raise AssertionError(f"rank {r} " + ("timed out" if p.returncode is None else f"exited with {p.returncode}") + f":\n{tail}")
    finally:
        for p in procs:
            if p.poll() is None:
                p.terminate()
                try:
                    p.wait(timeout=20)
                except subprocess.TimeoutExpired:
                    p.kill()
        for f in errs:
            f.close()
        for k, v in opts.items():
            _lib.set_option(k, v)

    for combo in COMBOS:
        name, deg = combo["name"], _degree(combo)
        got = [np.load(tmp_path / f"{name}_rank{r}.npz") for r in range(WORLD)]
        for it in range(ITERS):
            what = f"{name} iteration {it}"
            pres = [got[r]["pre"][it] for r in range(WORLD)]
            for r in range(WORLD):
                # (a) double buffering, announcement, side streams and a concurrent exchange change no bit of the gradients
                assert np.array_equal(pres[r].view(np.uint32), expect[deg, it, r].view(np.uint32)), f"{what}: rank {r}'s arena differs from the parent's render"
                # (d) gradients only where a camera of this rank composited (the masks themselves are not compared with the parent's:
                # stale workspace bytes may mark a few more Gaussians, include/gsr.h gsr_composited_mask)
                nz = (_rows(pres[r], P, M) != 0).any(axis=1)
                assert not (nz & ~got[r]["union"][it].astype(bool)).any(), f"{what}: rank {r} has gradient rows outside its masks"
                assert nz.any()
            # (c) the exact sum: two ranks add with one rounding in either algorithm, so every rank holds the float32 sum x0 + x1
            exact = (pres[0] + pres[1]).astype(np.float32)
            union = np.logical_or.reduce([got[r]["union"][it].astype(bool) for r in range(WORLD)])
            for r in range(WORLD):
                post = got[r]["post"][it]
                assert np.array_equal(post.view(np.uint32), exact.view(np.uint32)), \
                    f"{what}: rank {r}'s exchanged arena is not x0 + x1 (max |diff| {np.abs(post.astype(np.float64) - exact).max():.3e})"
                assert (_rows(post, P, M)[~union] == 0).all(), f"{what}: rank {r} has non-zero rows outside the union"
            if combo["sh_active"] is not None:
                assert (_rows(pres[0], P, M)[:, 3 + 3 * combo["sh_active"]:3 + 3 * M] == 0).all()
            print(f"{what}: union {int(union.sum())} of {P} rows")
            assert union.sum() < 0.8 * P                      # the compacted buffer's capacity drops below P after the first launch
        for r in range(WORLD):
            assert int(got[r]["overflows"]) == 0, name
            if combo["sparse"]:
                assert int(got[r]["union_rows"]) == int(np.logical_or.reduce([got[q]["union"][-1].astype(bool) for q in range(WORLD)]).sum())
