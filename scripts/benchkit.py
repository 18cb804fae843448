"""What the feature benchmarks under scripts/ share: the timed windows, the alternation of competing routes, the two summaries of a list
of samples, a synth scene as tensors and rasterizer settings, one backend forward pass as a record, and the command line with its
write-out.  One copy of the measurement method, so that the numbers under profiles/*/bench.json stay comparable with each other; a
feature's script is its bench_*() functions on top of this.  `import benchkit` from a script run as python scripts/x_bench.py,
`from scripts import benchkit` elsewhere.  Importing it starts nothing on the device and does not load the native library.

The timed windows differ on purpose and are not to be unified: a script keeps the form its committed numbers were taken with."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np
import torch
from gaussian_transformer_amd import _lib, rasterizer


# ---- timed windows ----

def timed(fn):
    """(device ms, result): two events around fn(), the device not drained before, the host waiting on the second event only."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); r = fn(); e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def timed_dev_wall(fn):
    """(device ms, wall ms, result): the device drained before and after; two events around fn(), and the host clock from just before
    the first is recorded to the end of the closing synchronise."""
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    w0 = time.perf_counter()
    t0.record()
    out = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), (time.perf_counter() - w0) * 1e3, out


def timed_drained(fn):
    """(device ms, result) of the drained window."""
    ms, _wall, out = timed_dev_wall(fn)
    return ms, out


def timed_peak(fn, before):
    """(device ms, peak bytes allocated above the starting allocation, result) of the drained window; before() (clearing .grad) runs
    ahead of it."""
    before()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms, out = timed_drained(fn)
    return ms, torch.cuda.max_memory_allocated() - base, out


def alternate(fns, reps, warmup, timed=timed, rotate=True):
    """{name: [ms, ...]}: every function once per repetition, the order rotated by one from each repetition to the next (two names:
    a flip) or, rotate off, kept; the first `warmup` repetitions dropped.  timed(fn) -> (ms, ...) is one of the windows above."""
    names = list(fns)
    ts = {k: [] for k in names}
    for i in range(warmup + reps):
        s = i % len(names) if rotate else 0
        for k in names[s:] + names[:s]:
            ms = timed(fns[k])[0]
            if i >= warmup:
                ts[k].append(ms)
    return ts


# ---- summaries of a list of samples ----

def stats_quantiles(xs):
    a = np.sort(np.asarray(xs, np.float64))
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), p10_ms=float(np.quantile(a, 0.1)), p90_ms=float(np.quantile(a, 0.9)), n=int(a.size))


def stats_minmax(ms, count="reps", digits=None):
    """min / median / max; count: the key the number of samples goes under (None: not reported); digits: rounded to so many."""
    r = (lambda v: v) if digits is None else (lambda v: round(v, digits))
    out = {"min_ms": r(min(ms)), "median_ms": r(statistics.median(ms)), "max_ms": r(max(ms))}
    if count:
        out[count] = len(ms)
    return out


# ---- a synth scene on the device ----

def _t(a, dev, grad=False):
    return torch.tensor(np.asarray(a, np.float32), device=dev).requires_grad_(grad)


def scene_tensors(sc, dev, requires_grad=False, shs=True):
    """The Gaussians of a synth scene as the rasterizer's keyword arguments (the results that report per parameter list them in this
    order).  shs off: without the SH coefficients, for a render with colours of its own."""
    P = int(sc.means3D.shape[0])
    keys = ("means3D", "opacities", "shs", "scales", "rotations") if shs else ("means3D", "opacities", "scales", "rotations")
    return {k: _t(np.asarray(getattr(sc, k)).reshape(P, 1) if k == "opacities" else getattr(sc, k), dev, requires_grad) for k in keys}


def scene_settings(sc, dev, bg=None, sh_degree=None, camera_grad=False):
    """The settings of the scene's own camera.  bg, sh_degree: instead of the scene's; camera_grad: the three camera tensors require grad."""
    cam = sc.camera
    return rasterizer.GaussianRasterizationSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
        bg=_t(sc.bg, dev) if bg is None else bg, scale_modifier=1.0,
        viewmatrix=_t(np.asarray(cam.world_view_transform).reshape(4, 4), dev, camera_grad),
        projmatrix=_t(np.asarray(cam.full_proj_transform).reshape(4, 4), dev, camera_grad),
        sh_degree=sc.sh_degree if sh_degree is None else sh_degree, campos=_t(cam.camera_center, dev, camera_grad), prefiltered=False, debug=False)


class Forward:
    """One forward pass of the backend over scene_tensors() `x` (SH colours, or `colors` [P,3] in their place): what it returned, and
    the calls that re-read its workspaces with the placeholders of the unused arguments filled in."""

    def __init__(self, rs, x, colors=None, empty=None):
        """empty: the placeholder tensor of an earlier record, for a pass inside a timed window (none is allocated then)."""
        self.rs, self.x, self.be = rs, x, rasterizer.get_backend()
        self.empty = torch.empty(0, device=x["means3D"].device) if empty is None else empty
        self.shs, self.colors = (x["shs"], self.empty) if colors is None else (self.empty, colors)
        self.n, self.color, self.radii, self.geom, self.binning, self.img = self.be.forward(
            rs, x["means3D"], self.shs, self.colors, x["opacities"], x["scales"], x["rotations"], self.empty)

    def workspace_args(self):
        """The three workspaces as the library takes them: pointer, size, three times."""
        return tuple(v for w in (self.geom, self.binning, self.img) for v in (_lib.ptr(w), w.numel()))

    @property
    def geo(self):
        """The tail of the arguments of depth_backward and features_backward."""
        return (self.x["means3D"], self.radii, self.x["scales"], self.x["rotations"], self.empty, self.geom, self.binning, self.img)

    def backward(self, dL, **kw):
        x = self.x
        return self.be.backward(self.rs, self.n, dL, x["means3D"], self.radii, self.shs, self.colors, x["scales"], x["rotations"], self.empty,
                                self.geom, self.binning, self.img, **kw)


# ---- the command line and the result file ----

CONFIGS = ("cfg2_table_300k_800", "cfg3_synth_1M_1080p")


def parser(reps, warmup, out, configs=False, trace_friendly=False, reps_flag="--reps"):
    """--reps (or reps_flag), --warmup and --out profiles/<out>/bench.json with this script's defaults; on request --configs and
    --trace-friendly.  A script adds its own flags to what this returns and hands it to parse()."""
    ap = argparse.ArgumentParser()
    ap.add_argument(reps_flag, type=int, default=reps)
    ap.add_argument("--warmup", type=int, default=warmup)
    if configs:
        ap.add_argument("--configs", nargs="+", default=list(CONFIGS))
    if trace_friendly:
        ap.add_argument("--trace-friendly", action="store_true", help="3 repetitions, 1 warm-up, nothing written: for a run under a profiler")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", out, "bench.json"))
    return ap


def parse(ap):
    """The arguments, after the check that there is a device to measure on; --trace-friendly already applied to reps and warmup."""
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit(f"{os.path.basename(sys.argv[0])} measures on a HIP device; none found (no CPU fallback, no number)")
    if getattr(args, "trace_friendly", False):
        args.reps, args.warmup = 3, 1
    return args


def write_json(obj, path, indent=1):
    """The result file, its directory made if missing.  indent None: one JSON line, which is printed as well."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        if indent is None:
            f.write(json.dumps(obj) + "\n")
        else:
            json.dump(obj, f, indent=indent)
    print(json.dumps(obj) if indent is None else f"wrote {path}")
