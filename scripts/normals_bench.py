#!/usr/bin/env python3
"""What the surface-normal feature costs (informational; bench.py is the headline metric).  Device events, the variants of a group
alternating inside every repetition, medians with p10-p90:

  loss     the fused consistency loss (include/gsr_normals.h), forward + backward, against the float32 torch formulation of
           tests/normals_ref.py with autograd on the same card and the same maps, at 800 x 800 and 1920 x 1080; each of the two kernels
           alone with the bytes it has to move per pixel (forward: 20 read; backward: 20 read, 20 written) and the share of the HBM rate
           a float4 copy reaches on this card (6.29 TB/s) that this comes to;
  normals  gsr_gaussian_normals_forward / _backward at P = 300 k and 1 M (40 and 16 bytes read, 16 written per Gaussian each way);
  step     render + loss + backward at configs 2 and 3: colour + expected depth (L1 + SSIM and a linear depth term) against the same
           with normals=True and the consistency term added.

    python scripts/normals_bench.py [--reps 50] [--warmup 5] [--out profiles/normals/bench.json]
"""
import json
import numpy as np
import torch
import benchkit
from benchkit import alternate, stats_quantiles as stats
from gaussian_transformer_amd import _lib, synth
from gaussian_transformer_amd.loss import fused_l1_ssim_loss, normal_consistency_loss
from gaussian_transformer_amd.model import GaussianParams
from gaussian_transformer_amd.rasterizer import GaussianRasterizationSettings, gaussian_normals
from gaussian_transformer_amd.render import PipelineParams, TorchCamera, render
from tests import normals_ref as nr

HBM_COPY_TBS = 6.29        # float4 copy on an MI355X (the rate a streaming kernel can be held against; the specification says 8.0)


def bench_loss(H, W, reps, warmup, dev):
    tx, ty = nr.TANFOV
    d, a, n = (torch.tensor(x, device=dev) for x in nr.maps(H, W, holes=False))       # every interior stencil valid: the most arithmetic
    p, st = _lib.ptr, _lib.stream(dev)
    ws = _lib.workspace("gsr_normal_loss_workspace", dev, H, W)
    out2 = torch.empty(2, device=dev)
    gd, ga, gn = torch.empty_like(d), torch.empty_like(a), torch.empty_like(n)

    def fwd():
        _lib.call("gsr_normal_loss_forward", st, H, W, tx, ty, nr.ALPHA_MIN, p(d), p(a), p(n), p(out2), None, p(ws), ws.numel())

    def bwd():
        _lib.call("gsr_normal_loss_backward", st, H, W, tx, ty, nr.ALPHA_MIN, p(d), p(a), p(n), None, p(gd), p(ga), p(gn))

    dg, ag, ng = (t.clone().requires_grad_(True) for t in (d, a, n))

    def fused():                                       # through the public function: allocations and autograd included
        dg.grad = ag.grad = ng.grad = None
        normal_consistency_loss(dg, ag, ng, tx, ty).backward()

    def torch32():
        dg.grad = ag.grad = ng.grad = None
        s, valid, _c2 = nr.surface(dg, ag, tx, ty, dtype=torch.float32)
        (torch.where(valid, ag.detach() * (1 - (ng * s).sum(0)), torch.zeros_like(dg)).sum() / (H * W)).backward()

    ts = alternate(dict(fused=fused, torch32=torch32, fwd=fwd, bwd=bwd), reps, warmup)
    fused(); g_f = dg.grad.clone(); torch32()
    agree = float((g_f - dg.grad).abs().max() / dg.grad.abs().max())
    px = H * W
    f, b = float(np.median(ts["fwd"])), float(np.median(ts["bwd"]))
    rate = lambda bytes_px, ms: bytes_px * px / (ms * 1e-3) / 1e12
    return dict(H=H, W=W, fused_fwd_bwd=stats(ts["fused"]), torch_f32_fwd_bwd=stats(ts["torch32"]),
                torch_over_fused=float(np.median(ts["torch32"]) / np.median(ts["fused"])), dL_ddepth_fused_vs_torch_max_rel=agree,
                forward_call=dict(stats(ts["fwd"]), bytes_per_pixel=20, tb_per_s=rate(20, f), share_of_copy_rate=rate(20, f) / HBM_COPY_TBS),
                backward_call=dict(stats(ts["bwd"]), bytes_per_pixel=40, tb_per_s=rate(40, b), share_of_copy_rate=rate(40, b) / HBM_COPY_TBS))


def bench_gaussians(P, reps, warmup, dev):
    gen = torch.Generator(device=dev).manual_seed(P)
    means = torch.rand((P, 3), device=dev, generator=gen) * 4 - 2
    scales = torch.exp(-4 * torch.rand((P, 3), device=dev, generator=gen))
    q = torch.nn.functional.normalize(torch.randn((P, 4), device=dev, generator=gen), dim=1).requires_grad_(True)
    V = torch.tensor(nr.rows(1)[3], device=dev)
    rs = GaussianRasterizationSettings(4, 4, 0.5, 0.5, torch.zeros(3, device=dev), 1.0, V, torch.eye(4, device=dev), 0, torch.zeros(3, device=dev), False, False)
    G = torch.randn((P, 3), device=dev, generator=gen)
    p, st = _lib.ptr, _lib.stream(dev)
    out, axis, g = torch.empty((P, 3), device=dev), torch.empty((P,), dtype=torch.int32, device=dev), torch.empty((P, 4), device=dev)
    qd = q.detach()

    def fwd():
        _lib.call("gsr_gaussian_normals_forward", st, P, p(means), p(scales), p(qd), p(V), p(out), p(axis))

    def bwd():
        _lib.call("gsr_gaussian_normals_backward", st, P, p(qd), p(V), p(axis), p(G), p(g))

    def both():                                        # through the autograd function
        q.grad = None
        (gaussian_normals(means, scales, q, rs) * G).sum().backward()
    fwd()
    ts = alternate(dict(fwd=fwd, bwd=bwd, both=both), reps, warmup)
    return dict(P=P, forward_call=stats(ts["fwd"]), backward_call=stats(ts["bwd"]), autograd_fwd_bwd=stats(ts["both"]))


def bench_step(name, reps, warmup, dev):
    sc = synth.make_config(name)
    pc = GaussianParams.from_synthetic(sc, dev)
    cam = TorchCamera(sc.camera, dev)
    H, W = int(sc.camera.image_height), int(sc.camera.image_width)
    pipe, bg = PipelineParams(), torch.zeros(3, device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    target = torch.rand((3, H, W), device=dev, generator=gen)
    wD = torch.rand((1, H, W), device=dev, generator=gen) / (H * W)
    params = (pc._xyz, pc._features_dc, pc._features_rest, pc._opacity, pc._scaling, pc._rotation)
    last = {}

    def clear():
        for t in params:
            t.grad = None

    def base():
        clear()
        o = render(cam, pc, pipe, bg, depth="expected")
        (fused_l1_ssim_loss(o["render"], target) + (o["depth"] * wD).sum()).backward()

    def full():
        clear()
        o = render(cam, pc, pipe, bg, depth="expected", normals=True)
        term = normal_consistency_loss(o["depth"], o["alpha"], o["normals"], sc.camera.tanfovx, sc.camera.tanfovy)
        (fused_l1_ssim_loss(o["render"], target) + (o["depth"] * wD).sum() + 0.05 * term).backward()
        last["term"], last["fraction"] = term.detach(), term.valid_fraction

    ts = alternate(dict(base=base, full=full), reps, warmup)
    b, f = float(np.median(ts["base"])), float(np.median(ts["full"]))
    return dict(config=name, P=int(pc._xyz.shape[0]), H=H, W=W, colour_depth=stats(ts["base"]), colour_depth_normals_loss=stats(ts["full"]),
                added_ms=f - b, added_frac=(f - b) / b, normal_term=float(last["term"]), valid_fraction=float(last["fraction"]))


def main():
    args = benchkit.parse(benchkit.parser(50, 5, "normals", configs=True))
    dev = torch.device("cuda:0")
    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, hbm_copy_tb_per_s=HBM_COPY_TBS, loss=[], gaussian_normals=[], step=[])
    for H, W in ((800, 800), (1080, 1920)):
        out["loss"].append(bench_loss(H, W, args.reps, args.warmup, dev))
        print(json.dumps(out["loss"][-1]), flush=True)
    for P in (300_000, 1_000_000):
        out["gaussian_normals"].append(bench_gaussians(P, args.reps, args.warmup, dev))
        print(json.dumps(out["gaussian_normals"][-1]), flush=True)
    for name in args.configs:
        out["step"].append(bench_step(name, args.reps, args.warmup, dev))
        print(json.dumps(out["step"][-1]), flush=True)
    benchkit.write_json(out, args.out)


if __name__ == "__main__":
    main()
