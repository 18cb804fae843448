"""Every GradientExchange combination (dist.py) against exact sums, over gloo with world sizes 2 and 3.

mode (sync, overlap) x algo (allreduce, direct) x payload (dense, active SH columns, sparse that fits, sparse that overflows),
each driven through two call patterns: B = 1, 2, 3 launches followed by one finish(), and bench.py's delayed update (arena(),
fill, launch, then wait for the arena launched one step earlier).  Every rank's arena holds distinct random values per launch,
zero outside that rank's mask; the parent checks every launch's result against the rank-order float32 sum ((x0 + x1) + x2)
and the float64 sum of the ranks' inputs -- never against another run of the exchange."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

P, M = 61, 4
WIDTHS = (("means3D", 3), ("shs", 3 * M), ("opacities", 1), ("scales", 3), ("rotations", 4))
ROW = sum(w for _, w in WIDTHS)                 # 23 floats per Gaussian
BUCKET_BYTES = 4 * 37                           # 37 floats: pieces cut rows (and parameters' columns) at odd places
ITERS = 3                                       # arenas and compacted buffers are reused
MODES, ALGOS = ("sync", "overlap"), ("allreduce", "direct")
PAYLOADS = ("dense", "sh_active", "sparse", "overflow")
PATTERNS = ("B1", "B2", "B3", "delayed")


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _n_launches(pattern):
    return ITERS * int(pattern[1]) if pattern[0] == "B" else ITERS + 1


def _inputs(rank, payload, pattern, t):
    """Rank `rank`'s arena rows [P, ROW] and mask for launch t of a case: the same in every mode and algorithm."""
    rng = np.random.default_rng([rank, PAYLOADS.index(payload), PATTERNS.index(pattern), t])
    if payload == "overflow":                   # nested masks: the union grows from launch to launch and outgrows the capacity
        u = np.random.default_rng([rank, 99]).uniform(size=P)
        vis = u < 0.1 + 0.8 * t / (_n_launches(pattern) - 1)
    else:
        vis = rng.uniform(size=P) < rng.uniform(0.2, 0.7)
    vis[:3] = False                             # rows no rank sees
    x = np.where(vis[:, None], rng.normal(size=(P, ROW)), 0.0).astype(np.float32)
    K = None
    if payload == "sh_active":                  # 1, 2, 3, 1, ... active columns: changes while earlier launches are in flight
        K = 1 + t % (M - 1)
        x[:, 3 + 3 * K:3 + 3 * M] = 0.0
    return x, vis, K


def _fill(ex, arena, x):
    v = ex.views(arena)
    off = 0
    for n, w in WIDTHS:
        v[n].reshape(P, w).copy_(torch.from_numpy(x[:, off:off + w])); off += w


def _read(ex, arena):
    v = ex.views(arena)
    return np.concatenate([v[n].reshape(P, -1).numpy() for n, _ in WIDTHS], axis=1).copy()


def _run_case(rank, mode, algo, payload, pattern):
    from gaussian_transformer_amd.dist import GradientExchange
    B = int(pattern[1]) if pattern[0] == "B" else 1
    slack = {"sparse": (1.0, P), "overflow": (1.0, 0)}.get(payload, (1.25, 1024))
    ex = GradientExchange(P, M, "cpu", mode=mode, algo=algo, bucket_bytes=BUCKET_BYTES, n_buffers=max(2, B), sparse_slack=slack)
    recs = []

    def start(t):
        x, vis, K = _inputs(rank, payload, pattern, t)
        arena = ex.arena()
        _fill(ex, arena, x)
        ex.sh_active = K
        mask = torch.from_numpy(vis.copy()) if payload in ("sparse", "overflow") else None
        ex.launch(visible=mask)
        rec = dict(x=x, vis=vis, mask=mask, arena=arena)
        if mode == "sync":                      # one arena: complete on return, and handed out again by the next arena()
            rec["out"] = _read(ex, arena)
        recs.append(rec)
        return rec

    if pattern[0] == "B":
        for it in range(ITERS):
            batch = [start(it * B + b) for b in range(B)]
            ex.finish()
            for rec in batch:
                rec.setdefault("out", _read(ex, rec["arena"]))
    else:
        prev = None
        for t in range(_n_launches(pattern)):
            rec = start(t)
            if mode == "overlap":               # bench.py step(): the arena launched one step earlier is waited for and read
                assert (prev is None) or (prev["arena"] is ex.arenas[ex.cur])
                ex.wait(ex.cur)
                if prev is not None:
                    prev["out"] = _read(ex, prev["arena"])
            prev = rec
        ex.finish()
        prev.setdefault("out", _read(ex, prev["arena"]))
    launches = [dict(x=r["x"], vis=r["vis"], out=r["out"],
                     mask_after=None if r["mask"] is None else r["mask"].numpy().copy()) for r in recs]
    return dict(launches=launches, overflows=ex.sparse_overflows, union_rows=ex.union_rows)


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.set_num_threads(1)
        out = {}
        for mode in MODES:
            for algo in ALGOS:
                for payload in PAYLOADS:
                    for pattern in PATTERNS:
                        out[mode, algo, payload, pattern] = _run_case(rank, mode, algo, payload, pattern)
        q.put((rank, out, None))
    except Exception:
        import traceback
        q.put((rank, None, traceback.format_exc()))
        raise
    finally:
        dist.destroy_process_group()


def _bits_equal(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
        d = np.abs(a.astype(np.float64) - b.astype(np.float64))
        raise AssertionError(f"{what}: {int((a.view(np.uint32) != b.view(np.uint32)).sum())} elements differ in their bits, "
                             f"max |diff| {d.max():.3e}")


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 3])
def test_every_exchange_mode_equals_the_exact_sum(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs: p.start()
    res = {}
    try:
        for _ in range(world):
            r, out, err = q.get(timeout=180)
            assert err is None, f"rank {r}:\n{err}"
            res[r] = out
    finally:
        for p in procs:
            p.join(30)
            if p.is_alive():
                p.terminate()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    eps = 2.0 ** -24
    for payload in PAYLOADS:
        for pattern in PATTERNS:
            n = _n_launches(pattern)
            # the reference sums, from the inputs every rank handed in
            xs = [[res[r]["sync", "allreduce", payload, pattern]["launches"][t]["x"] for r in range(world)] for t in range(n)]
            rank_order, s64, abs64, unions = [], [], [], []
            for t in range(n):
                acc = xs[t][0].copy()
                for r in range(1, world):
                    acc = (acc + xs[t][r]).astype(np.float32)
                rank_order.append(acc)
                s64.append(np.sum([x.astype(np.float64) for x in xs[t]], axis=0))
                abs64.append(np.sum([np.abs(x.astype(np.float64)) for x in xs[t]], axis=0))
                unions.append(np.logical_or.reduce([res[r]["sync", "allreduce", payload, pattern]["launches"][t]["vis"]
                                                    for r in range(world)]))
            for algo in ALGOS:
                for mode in MODES:
                    case = (mode, algo, payload, pattern)
                    for t in range(n):                                  # every rank holds the same bits
                        for r in range(1, world):
                            _bits_equal(res[r][case]["launches"][t]["out"], res[0][case]["launches"][t]["out"],
                                        f"{case} launch {t}: rank {r} vs rank 0")
                    for r in range(world):
                        o = res[r][case]
                        assert len(o["launches"]) == n, case
                        for t, L in enumerate(o["launches"]):
                            what = f"{case} rank {r} launch {t}"
                            _bits_equal(L["x"], xs[t][r], what + " input")
                            if algo == "direct" or world == 2:
                                _bits_equal(L["out"], rank_order[t], what + " vs the rank-order float32 sum")
                            else:                 # a ring adds in an order set by the element's place in the buffer: two roundings
                                err = np.abs(L["out"].astype(np.float64) - s64[t])
                                bad = err > 2 * eps * abs64[t]
                                assert not bad.any(), f"{what}: {int(bad.sum())} elements beyond two roundings, worst " \
                                                      f"{float((err / np.maximum(abs64[t], 1e-30)).max()):.3e} of sum |x_r|"
                            assert (L["out"][~unions[t]] == 0).all(), what + ": rows outside the union are not zero"
                            if L["mask_after"] is not None:
                                assert np.array_equal(L["mask_after"], L["vis"]), what + ": the caller's mask was overwritten"
                        if payload == "overflow":
                            assert o["overflows"] > 0, case
                        if payload == "sparse":
                            assert o["overflows"] == 0, case
                        if payload in ("sparse", "overflow"):           # the launch waited for last is the last one in every pattern here
                            assert o["union_rows"] == int(unions[-1].sum()), (case, o["union_rows"], int(unions[-1].sum()))
                # overlap changes no bit of what sync computes.  Not asserted for a ring of three in the overflow case: there the
                # capacity depends on which unions were known at launch, i.e. on when earlier exchanges were waited for, so the same
                # launch may go compacted in one mode and dense in the other -- another buffer position, another summation order
                # (both results are held to the two-rounding bound above)
                if algo == "allreduce" and world > 2 and payload == "overflow":
                    continue
                for t in range(n):
                    _bits_equal(res[0]["overlap", algo, payload, pattern]["launches"][t]["out"],
                                res[0]["sync", algo, payload, pattern]["launches"][t]["out"],
                                f"{(algo, payload, pattern)} launch {t}: overlap vs sync")
