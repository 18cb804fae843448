#!/usr/bin/env python3
"""A whole 3DGS optimisation loop on the HIP path, shaped like the reference's train.py:66-128: camera of the iteration
-> render -> 0.8 L1 + 0.2 (1 - SSIM) -> backward -> densification statistics / clone / split / prune / opacity reset
-> Adam step.  Target images come from a hidden "ground truth" set of Gaussians seen from a ring of cameras; the trained
set starts from a perturbed, thinned copy.  Informational (bench.py is the headline metric).

    python scripts/train_synthetic.py [--iters 600] [--P 20000] [--size 256] [--density torch|hip|mcmc|mcmc_hip] [--cap N] [--adam hip|hip_sparse]
                                      [--prune-contribution ITER:THRESHOLD] [--absgrad] [--densify-grad-threshold X]
                                      [--lambda-normal X [--normal-from ITER]]

--density mcmc / mcmc_hip: MCMC density control (densify.MCMCController / FusedMCMCController, include/gsr_mcmc.h) with a budget of
--cap Gaussians: regularisers before the step, position noise after it, relocation and growth every `densify_every` iterations.
--prune-contribution ITER:THRESHOLD: after iteration ITER the blend weights of every training camera are collected under no_grad
(rasterizer.collect_contribution, include/gsr_contrib.h) and the Gaussians whose largest weight stays below THRESHOLD are pruned
(DensityController.prune_by_max_weight); the record holds the Gaussians and the PSNR before and after.
--absgrad: the densification statistics are fed with the per-pixel absolute sums of dL/dmeans2D (rasterizer.collect_absgrad around
loss.backward(), include/gsr_absgrad.h) in place of viewspace_points.grad; --densify-grad-threshold X sets the threshold they are held
to (default: OptimizationParams' 0.0002; AbsGS and gsplat use about 0.0008 with absgrad).  Not for mcmc / mcmc_hip, whose rule reads no
statistics.
--lambda-normal X: from iteration --normal-from on (default: a third of the run) X times 2DGS's depth-normal consistency term
(loss.normal_consistency_loss, include/gsr_normals.h) is added to the image loss; those iterations render through render(depth="expected",
normals=True) instead of the raw-parameter path, which has no maps.  The record holds the term's final value over the training
cameras ("normal_term", also for a run without the flag, where nothing optimises it).
"""
import argparse, json, math, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from gaussian_transformer_amd import synth
from gaussian_transformer_amd.camera import look_at_camera
from gaussian_transformer_amd.densify import (DensityController, FusedDensityController, FusedMCMCController, MCMCController, MCMCParams,
                                              OptimizationParams)
from gaussian_transformer_amd.loss import fused_l1_ssim_loss, normal_consistency_loss, psnr
from gaussian_transformer_amd.model import GaussianParams
from gaussian_transformer_amd.rasterizer import AbsGrad, ContributionStats, collect_absgrad, collect_contribution
from gaussian_transformer_amd.render import PipelineParams, TorchCamera, render, render_fused


DEFAULT_CAP = 26619      # the count a --density hip run at the defaults ends at (profiles/density/bench.json): the same final set size


def run(iters=600, P=20000, size=256, ncam=8, seed=0, densify_from=100, densify_every=100, log=None, density="torch", adam="hip", cap=None,
        prune_contribution=None, absgrad=False, densify_grad_threshold=None, lambda_normal=0.0, normal_from=None):
    dev = torch.device("cuda", 0)
    sc = synth.make_scene(P=P, width=size, height=size, sh_degree=1, s0=0.03, seed=seed, zmin=3.0, zmax=6.0)
    truth = GaussianParams.from_synthetic(sc, dev, requires_grad=False)
    centre = np.array([0.0, 0.0, 4.5])
    cams = []
    for k in range(ncam):
        a = (k - (ncam - 1) / 2.0) * math.radians(8.0)
        eye = centre + 4.5 * np.array([math.sin(a), 0.0, -math.cos(a)])
        cams.append(TorchCamera(look_at_camera(eye, centre, (0.0, -1.0, 0.0), sc.camera.FoVx, size, size), dev))
    pipe, bg = PipelineParams(), torch.zeros(3, device=dev)
    with torch.no_grad():
        targets = [render_fused(c, truth, pipe, bg)["render"].clone() for c in cams]
    # the trained model: every third Gaussian of the truth, displaced, grey, fat and faint
    rng = np.random.default_rng(seed + 1)
    keep = np.arange(0, P, 3)
    sc0 = synth.SyntheticScene(sc.camera, (sc.means3D[keep] + rng.normal(0, 0.02, (len(keep), 3))).astype(np.float32),
                               (sc.scales[keep] * 1.5).astype(np.float32), sc.rotations[keep], np.full((len(keep), 1), 0.3, np.float32),
                               (sc.shs[keep] * 0.0).astype(np.float32), sc.sh_degree, sc.bg, sc.dL_dimage)
    model = GaussianParams.from_synthetic(sc0, dev)
    opt = OptimizationParams(densify_from_iter=densify_from, densification_interval=densify_every, opacity_reset_interval=10 ** 9,
                             densify_until_iter=iters)
    if densify_grad_threshold is not None:
        opt.densify_grad_threshold = float(densify_grad_threshold)
    mcmc = density in ("mcmc", "mcmc_hip")
    if mcmc:
        params = MCMCParams(cap_max=cap if cap is not None else DEFAULT_CAP, refine_start=densify_from, refine_every=densify_every, refine_stop=iters)
        ctl = (FusedMCMCController if density == "mcmc_hip" else MCMCController)(model, params, opt, spatial_lr_scale=1.0, adam=adam)
    else:
        ctl = (FusedDensityController if density == "hip" else DensityController)(model, opt, spatial_lr_scale=1.0, adam=adam)
    gen = torch.Generator(device=dev).manual_seed(seed)

    def evaluate():
        with torch.no_grad():
            imgs = [render_fused(c, model, pipe, bg)["render"] for c in cams]
            return (float(np.mean([float(fused_l1_ssim_loss(i, t)) for i, t in zip(imgs, targets)])),
                    float(np.mean([float(psnr(i[None], t[None]).mean()) for i, t in zip(imgs, targets)])))
    def normal_term(c):
        """The consistency term of the model seen from camera c, on the maps of one render."""
        m = render(c, model, pipe, bg, depth="expected", normals=True)
        return m, normal_consistency_loss(m["depth"], m["alpha"], m["normals"], math.tan(c.FoVx * 0.5), math.tan(c.FoVy * 0.5))
    normal_from = iters // 3 if normal_from is None else int(normal_from)
    loss0, psnr0 = evaluate()
    hist = []
    pruned = None
    t0 = time.perf_counter()
    for it in range(1, iters + 1):
        ctl.update_learning_rate(it)
        k = int(rng.integers(ncam))
        if lambda_normal > 0.0 and it >= normal_from:
            pkg, term = normal_term(cams[k])
            loss = fused_l1_ssim_loss(pkg["render"], targets[k]) + lambda_normal * term
        else:
            pkg = render_fused(cams[k], model, pipe, bg)
            loss = fused_l1_ssim_loss(pkg["render"], targets[k])
        if absgrad and not mcmc:
            buf = AbsGrad(int(model._xyz.shape[0]), dev)           # this view's sums (the set's size changes at a densification)
            with collect_absgrad(buf):
                loss.backward()
            stats_kw = {"absgrad": buf}
        else:
            loss.backward()
            stats_kw = {}
        with torch.no_grad():
            ev = ctl.after_backward(it, pkg["viewspace_points"], pkg["visibility_filter"], pkg["radii"], extent=3.0, generator=gen, **stats_kw)
            if mcmc:
                ev = None                  # the two regularisation terms (device tensors): not an event, and reading them would wait
            if adam == "hip_sparse":       # rows of Gaussians outside this view stand still (include/gsr_optim.h); a no-op right after a densification
                ctl.optimizer.step(visibility=pkg["radii"])
            else:
                ctl.optimizer.step()
            ctl.optimizer.zero_grad(set_to_none=True)
            if mcmc:
                ctl.after_step(it, generator=gen)
                ev = {"P": int(model._xyz.shape[0])} if densify_from <= it < iters and it % densify_every == 0 else None      # relocated and grown
        if prune_contribution is not None and it == prune_contribution[0]:
            _, psnr_before = evaluate()
            stats = ContributionStats(int(model._xyz.shape[0]), dev)
            with torch.no_grad(), collect_contribution(stats):
                for c in cams:
                    render_fused(c, model, pipe, bg)
                n = ctl.prune_by_max_weight(stats, threshold=prune_contribution[1])
            pruned = {"it": it, "threshold": prune_contribution[1], "views": stats.views, "P_before": stats.P, "P_after": int(model._xyz.shape[0]),
                      "pruned": n, "psnr_before": round(psnr_before, 2), "psnr_after": round(evaluate()[1], 2)}
            if log:
                log(pruned)
        if it % 50 == 0 or ev:
            rec = {"it": it, "loss": round(float(loss.detach()), 5), "P": int(model._xyz.shape[0]), "event": ev}
            hist.append(rec)
            if log:
                log(rec)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    loss1, psnr1 = evaluate()
    with torch.no_grad():
        term1 = float(np.mean([float(normal_term(c)[1]) for c in cams]))
    return {"lambda_normal": lambda_normal, "normal_from": normal_from, "normal_term": round(term1, 6), "density": density, "adam": adam, "absgrad": bool(absgrad and not mcmc), "densify_grad_threshold": opt.densify_grad_threshold, "iters": iters, "seconds": round(dt, 2), "it_per_s": round(iters / dt, 1), "P_start": len(keep), "P_end": int(model._xyz.shape[0]),
            "loss_first": round(loss0, 5), "loss_last": round(loss1, 5), "psnr_first": round(psnr0, 2), "psnr": round(psnr1, 2),
            "prune_contribution": pruned, "history": hist}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=600)
    ap.add_argument("--P", type=int, default=20000)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--density", choices=("torch", "hip", "mcmc", "mcmc_hip"), default="torch",
                    help="density control: torch index arithmetic (DensityController), the HIP path (FusedDensityController), or MCMC "
                         "density control in torch (MCMCController) / on the HIP path (FusedMCMCController)")
    ap.add_argument("--cap", type=int, default=None, help="mcmc / mcmc_hip: the budget of Gaussians (default: what --density hip ends at)")
    ap.add_argument("--adam", choices=("hip", "hip_sparse"), default="hip",
                    help="hip = HipAdam over all rows; hip_sparse = HipSparseAdam with the view's radii as visibility")
    ap.add_argument("--prune-contribution", default=None, metavar="ITER:THRESHOLD",
                    help="after iteration ITER, prune the Gaussians whose largest blend weight over all training cameras is below THRESHOLD")
    ap.add_argument("--absgrad", action="store_true", help="densification statistics from the per-pixel absolute sums of dL/dmeans2D")
    ap.add_argument("--densify-grad-threshold", type=float, default=None, help="OptimizationParams.densify_grad_threshold (default 0.0002; about 0.0008 with --absgrad)")
    ap.add_argument("--lambda-normal", type=float, default=0.0, help="weight of the depth-normal consistency term (0: off; 2DGS uses 0.05)")
    ap.add_argument("--normal-from", type=int, default=None, help="first iteration the term is added at (default: iters / 3)")
    a = ap.parse_args()
    prune = None
    if a.prune_contribution:
        at, thr = a.prune_contribution.split(":")
        prune = (int(at), float(thr))
    out = run(a.iters, a.P, a.size, density=a.density, adam=a.adam, cap=a.cap, prune_contribution=prune, absgrad=a.absgrad, densify_grad_threshold=a.densify_grad_threshold,
              lambda_normal=a.lambda_normal, normal_from=a.normal_from, log=lambda r: print(json.dumps(r), flush=True))
    out.pop("history")
    print(json.dumps(out))
