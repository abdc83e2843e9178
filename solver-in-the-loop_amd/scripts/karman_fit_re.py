#!/usr/bin/env python
"""Identify the Reynolds number of a karman-2d flow from its frames: the differentiable solver fits its own viscosity, as PhiFlow's does
(diffuse(..., 1 / re * dt * res * res) is an ordinary differentiable op in /root/reference/karman-2d/karman_train.py:175-178).

One log Re per simulation is fitted with Adam to K consecutive frames: the solver steps K - 1 times from the first frame
(KarmanFlow(re_grad=True): the gradient with respect to re comes from sol_karman_step_bwd_large_re) and the loss is the squared
velocity error against the later frames.  Input: a scene directory of scripts/karman.py (`velo_*` / `dens_*` frames, params.pickle), or
--synthetic (frames generated here by the same step at known Reynolds numbers, so that the result can be judged).  Prints the trajectory
and writes re_fit.json."""
import argparse
import json
import math
import os
import pickle

import numpy as np
import torch


def frame_loss(out, frame):
    """squared velocity error of a state (d, vy, vx) against a frame (d, vy, vx), summed over faces and simulations"""
    return ((out[1] - frame[1]) ** 2).sum() + ((out[2] - frame[2]) ** 2).sum()


def fit_re(step, frames, re0, iters=40, lr=0.2, print_fn=print):
    """Fits log Re [B] to `frames` = K consecutive states (d, vy, vx): from frames[0], `step(d, vy, vx, re) -> (d, vy, vx)` is applied
    K - 1 times and the loss sums frame_loss over frames[1:].  Adam(lr) on log Re, started at re0 [B], `iters` iterations.
    -> (Re [B] after the last update, history: a list of (loss, [Re...]) BEFORE each update plus the final evaluation)."""
    log_re = torch.log(torch.as_tensor(re0, dtype=frames[0][1].dtype, device=frames[0][1].device)).clone().requires_grad_(True)
    opt = torch.optim.Adam([log_re], lr=lr)
    history = []

    def evaluate():
        cur = frames[0]
        loss = 0.0
        for f in frames[1:]:
            cur = step(*cur, torch.exp(log_re))
            loss = loss + frame_loss(cur, f)
        return loss

    for it in range(iters + 1):
        opt.zero_grad()
        loss = evaluate()
        history.append((float(loss.detach()), torch.exp(log_re).detach().cpu().tolist()))
        print_fn("iteration %3d  loss %.6e  Re %s" % (it, history[-1][0], " ".join("%.4e" % r for r in history[-1][1])))
        if it == iters:
            break
        loss.backward()
        opt.step()
    return torch.exp(log_re).detach(), history


def flow_stepper(sim, dom, B, Y, X, res):
    """step(d, vy, vx, re) through KarmanFlow.step on [B,Y,X] / [B,Y+1,X] / [B,Y,X+1] tensors"""
    import sol_amd
    bcv, bcm = sol_amd.velocity_bc_masks(Y, X, batch_size=B)

    def step(d, vy, vx, re):
        vel = sol_amd.StaggeredGrid([vy.reshape(B, Y + 1, X, 1), vx.reshape(B, Y, X + 1, 1)], dom.box)
        s = sim.step(sol_amd.Fluid(dom, density=d.reshape(B, Y, X, 1), velocity=vel, batch_size=B), re=re, res=res, velBCy=bcv, velBCyMask=bcm)
        return (s.density.data.reshape(B, Y, X), s.velocity.data[0].data.reshape(B, Y + 1, X), s.velocity.data[1].data.reshape(B, Y, X + 1))

    return step


def main(argv=None):
    from _common import add_advection_arg, add_multi_launch_arg, advection_from_args, agreed_advection, agreed_multi_launch, add_scene_args, add_substeps_arg, agreed_substeps, flow_kwargs, logger, scene_from_args, select_gpu, substeps_from_args
    import sol_amd
    from sol_amd import scene, synthetic
    p = argparse.ArgumentParser(description="Parameter Parser", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--gpu", default="0", help="visible GPUs")
    p.add_argument("--input", default=None, help="scene directory (sim_NNNNNN) with velo_*/dens_* frames and params.pickle")
    p.add_argument("--synthetic", action="store_true", help="fit frames generated here at known Reynolds numbers instead of --input")
    p.add_argument("--start", default=None, type=int, help="first frame (default: the first one in the directory)")
    p.add_argument("-k", "--frames", default=4, type=int, help="consecutive frames to fit (K - 1 solver steps)")
    p.add_argument("--re0", default=None, type=float, help="starting Reynolds number (default: 4 x the recorded / true one)")
    p.add_argument("--iters", default=40, type=int, help="Adam iterations")
    p.add_argument("--lr", default=0.2, type=float, help="Adam learning rate on log Re")
    p.add_argument("-r", "--res", default=32, type=int, help="--synthetic: resolution of the reference axis")
    p.add_argument("-b", "--batch", default=3, type=int, help="--synthetic: simulations")
    p.add_argument("--seed", default=11, type=int, help="--synthetic: seed of the initial state")
    p.add_argument("-o", "--output", default=None, help="directory for re_fit.json (default: --input, or the current directory)")
    add_scene_args(p)
    add_substeps_arg(p, auto=False)
    add_advection_arg(p, generates=False)
    add_multi_launch_arg(p, generates=False)
    params = vars(p.parse_args(argv))
    if (params["input"] is None) == (not params["synthetic"]):
        raise SystemExit("give --input DIR or --synthetic")
    select_gpu(params["gpu"])
    log = logger()
    K = params["frames"]
    if K < 2:
        raise SystemExit("--frames must be at least 2")
    f = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda").contiguous()
    rec = scene_from_args(params)
    if params["synthetic"]:
        res, length, B = params["res"], 100, params["batch"]
        Y, X = 2 * res, res
        re_true = synthetic.reynolds(B).tolist()
        first = tuple(f(t) for t in synthetic.state(B, Y, X, params["seed"]))
        nsub = substeps_from_args(params) or 1
        fa = advection_from_args(params)
        advection = agreed_advection({"advection": fa[0], "correction_strength": fa[1]}, (None, None), "the flags")
        multi_launch = agreed_multi_launch(False, params["multi_launch"])
    else:
        with open(os.path.join(params["input"], "params.pickle"), "rb") as fh:
            meta = pickle.load(fh)
        res, length, B = meta["res"], meta.get("len", 100), 1
        rec = rec if rec is not None else meta.get("scene")      # (periodic boundaries travel in the record: KarmanFlow refuses re_grad on them, by name)
        nsub = agreed_substeps(meta.get("diffusion_substeps"), substeps_from_args(params), "params.pickle")      # the count the frames were generated with
        advection = agreed_advection(meta, advection_from_args(params), "params.pickle")      # the scheme the frames were generated with
        multi_launch = agreed_multi_launch(meta.get("multi_launch"), params["multi_launch"])      # the path the frames were generated on
        names = sorted(n for n in os.listdir(params["input"]) if n.startswith("velo_") and n.endswith(".npz"))
        start = int(names[0][5:11]) if params["start"] is None else params["start"]
        re_true = [float(meta["re"])]
        loaded = []
        for i in range(start, start + K):
            v = scene.read_zipped_array(os.path.join(params["input"], "velo_%06d.npz" % i)).astype(np.float32)
            dpath = os.path.join(params["input"], "dens_%06d.npz" % i)
            Y, X = v.shape[1] - 1, v.shape[2] - 1
            d = scene.read_zipped_array(dpath)[..., 0] if os.path.exists(dpath) else np.zeros((1, Y, X))
            vy, vx = scene.split_staggered(v)
            loaded.append((f(d), f(vy), f(vx)))
    dom = sol_amd.Domain([Y, X], box=sol_amd.box[0:length * 2, 0:length])
    sim = sol_amd.KarmanFlow(pressure_solver=params["pressure_solver"], re_grad=True, diffusion_substeps=nsub, multi_launch=multi_launch, **advection, **flow_kwargs(rec))
    step = flow_stepper(sim, dom, B, Y, X, res)
    if params["synthetic"]:
        loaded = [first]
        with torch.no_grad():
            for _ in range(K - 1):
                loaded.append(step(*loaded[-1], f(re_true)))
    re0 = [params["re0"]] * B if params["re0"] else [4.0 * r for r in re_true]
    log.info("%dx%d, B = %d, %d frames, pressure solver %s, diffusion substeps %d, start Re %s" % (Y, X, B, K, params["pressure_solver"], nsub, re0))
    re_fit, history = fit_re(step, loaded, re0, params["iters"], params["lr"], log.info)
    result = {"grid": [Y, X], "frames": K, "iters": params["iters"], "lr": params["lr"], "re_start": re0, "re_fit": re_fit.cpu().tolist(),
              "re_recorded": re_true, "log_ratio": [math.log(a / b) for a, b in zip(re_fit.cpu().tolist(), re_true)],
              "loss_first": history[0][0], "loss_last": history[-1][0]}
    out = params["output"] or params["input"] or "."
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "re_fit.json"), "w") as fh:
        fh.write(json.dumps(result) + "\n")
    log.info(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
