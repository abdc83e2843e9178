#!/usr/bin/env python
"""Inference roll-out with the trained corrector -- flags of /root/reference/karman-2d/karman_apply.py:
20-31, loop :138-158 (simulator.step -> model.predict correction -> write denTf/velTf/corTf frames).
Solver step + CNN run on the GPU (make_rollout: SolRollout, or LargeGridRollout beyond the one-workgroup grids such as -r 128; one frame
per call so that every frame can be written)."""
import argparse
import pickle

import numpy as np
import torch

from _common import (inherit_boundaries, add_advection_arg, add_multi_launch_arg, advection_from_args, agreed_advection, agreed_multi_launch, add_buoyancy_arg, add_scene_args, add_substeps_arg, agreed_buoyancy, agreed_substeps, buoyancy_from_args, flow_kwargs, logger,
                     scene_from_args, select_gpu, substeps_from_args)
import sol_amd
from sol_amd import ops, scene


def main(argv=None):
    p = argparse.ArgumentParser(description="Parameter Parser", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--gpu", default="0", help="visible GPUs")
    p.add_argument("-s", "--scale", default=4, type=int, help="simulation scale for high-res")
    p.add_argument("-r", "--res", default=32, type=int, help="resolution of the reference axis")
    p.add_argument("-l", "--len", default=100, type=int, help="length of the reference axis")
    p.add_argument("--re", default=1e6, type=float, help="Reynolds number")
    p.add_argument("--initdH", default=None, help="load hires (will be downsampled) density")
    p.add_argument("--initvH", default=None, help="load hires (will be downsampled) velocity")
    p.add_argument("-t", "--simsteps", default=500, type=int, help="simulation steps")
    p.add_argument("-o", "--output", default="/tmp/phiflow/run", help="path to an output directory")
    p.add_argument("--stats", default="/tmp/phiflow/data/dataStats.pickle", help="path to datastats")
    p.add_argument("--model", default="/tmp/phiflow/tf/model.pt", help="path to a trained model")
    p.add_argument("--any-width", action="store_true", help="run the correction network on rows of any width (pitched rows with column-masked convolutions) instead of refusing a width the convolutions do not take")
    p.add_argument("--conv-padding", default=None, choices=["zeros", "circular"],
                   help="padding of the correction network's convolutions (default: what the model was trained with, recorded in the stats "
                        "and with the model; an explicit value overrides the record)")
    add_scene_args(p, warm_start=True)
    add_buoyancy_arg(p)
    add_substeps_arg(p, auto=False)
    add_advection_arg(p, generates=False)
    add_multi_launch_arg(p, generates=False)
    params = vars(p.parse_args(argv))
    select_gpu(params["gpu"])
    log = logger()
    res = params["res"]
    Y, X = 2 * res, res
    dom = sol_amd.Domain([Y, X], box=sol_amd.box[0:params["len"] * 2, 0:params["len"]])
    d0 = scene.downsample(scene.read_zipped_array(params["initdH"]), params["scale"]) if params["initdH"] else np.zeros((1, Y, X, 1))
    if params["initvH"]:
        vn = scene.downsample_staggered(scene.read_zipped_array(params["initvH"]), params["scale"])
    else:
        vn = np.zeros((1, Y + 1, X + 1, 2))
        vn[..., 0] = 1.0
        vn[..., vn.shape[1] // 2 + 10:vn.shape[1] // 2 + 20, vn.shape[2] // 2 - 2:vn.shape[2] // 2 + 2, 1] = 1.0
    path = scene.scene_create(params["output"])
    logger(path + "/run.log")
    log.info(params)
    with open(path + "/params.pickle", "wb") as f:
        pickle.dump(params, f)
    with open(params["stats"], "rb") as f:
        data_stats = pickle.load(f)
    log.info({k: v for k, v in data_stats.items() if k != "scene"})
    model = sol_amd.ConvNet.load(params["model"])
    model.summary(print_fn=log.info)
    # the scene: the one the model was trained on (dataStats "scene"), else the flags, else the reference's sphere
    rec = data_stats.get("scene")
    flags = scene_from_args(params)
    flags = inherit_boundaries(flags, rec)
    if rec is not None and flags is not None and not sol_amd.karman.scenes_equal(rec, flags):
        log.info("--obstacle / --obstacle-mask ignored: the model was trained on the scene of %s" % params["stats"])
    rec = rec if rec is not None else flags
    sim = sol_amd.KarmanFlow(**flow_kwargs(rec))
    log.info("scene: %s" % sol_amd.karman.describe_scene(sim.scene()))
    # the buoyancy force the model was trained with (dataStats "buoyancy"; absent: off); stats without the record take the flag
    buoyancy = agreed_buoyancy(data_stats["buoyancy"], buoyancy_from_args(params), params["stats"]) if "buoyancy" in data_stats \
        else buoyancy_from_args(params)
    log.info("buoyancy: %s" % (buoyancy,))
    # the diffusion substeps likewise (dataStats "diffusion_substeps"; stats without the record take the flag, else 1)
    nsub = agreed_substeps(data_stats["diffusion_substeps"], substeps_from_args(params), params["stats"]) if "diffusion_substeps" in data_stats \
        else (substeps_from_args(params) or 1)
    log.info("diffusion substeps: %d" % nsub)
    # and the advection scheme (dataStats "advection" / "correction_strength"; absent: semi_lagrangian, or the flags)
    flags_adv = advection_from_args(params)
    advection = agreed_advection(data_stats, flags_adv, params["stats"]) if "advection" in data_stats \
        else agreed_advection({"advection": flags_adv[0], "correction_strength": flags_adv[1]}, (None, None), "the flags")
    log.info("advection: %s" % (advection,))
    # and the multi-launch path (dataStats "multi_launch"; absent: off, or the flag)
    multi_launch = agreed_multi_launch(data_stats.get("multi_launch"), params["multi_launch"])
    log.info("multi-launch path: %s" % multi_launch)
    active, inflow = sim.scene_arrays(dom)
    velBCy, velBCyMask = sol_amd.velocity_bc_masks(Y, X)
    masks = ops.SceneMasks(active, inflow, velBCy.reshape(Y + 1, X), velBCyMask.reshape(Y + 1, X),
                           pressure_solver=params["pressure_solver"], multi_launch=multi_launch,
                           boundaries=sol_amd.karman.record_boundaries(rec or {}))
    log.info("pressure solver: %s" % masks.pressure_solver)
    # the padding of the network's convolutions: the one the model was trained with (dataStats "conv_padding", else the model file's
    # record; absent: zeros); an explicit flag overrides it
    conv_padding = data_stats.get("conv_padding") or model.conv_padding
    if params["conv_padding"] is not None and params["conv_padding"] != conv_padding:
        log.info("--conv-padding %s overrides the record: the model was trained with %s padding" % (params["conv_padding"], conv_padding))
        conv_padding = params["conv_padding"]
    log.info("convolution padding: %s" % conv_padding)
    large = masks.large
    warm = bool(params["cg_warm_start"]) and large and masks.pressure_solver == "cg"
    if params["cg_warm_start"] and not warm:
        log.info("--cg-warm-start ignored: %s" % ("the direct pressure solve has no iteration to start" if large and ops.is_direct(masks.pressure_solver)
                                                  else "it belongs to the CG solve of the large grids"))
    # (a CG scene runs eagerly, every solve stops at convergence; a direct-solve scene replays one captured step)
    ro = sol_amd.make_rollout(model, masks, 1, Y, X, dom.dx[1], data_stats["std"][1], data_stats["ext.std"][0],
                              use_graph=ops.is_direct(masks.pressure_solver), cg_warm_start=warm, any_width=params["any_width"],
                              buoyancy=buoyancy, diffusion_substeps=nsub, multi_launch=multi_launch, conv_padding=conv_padding, **advection)
    f = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda").contiguous()
    vy0, vx0 = scene.split_staggered(np.asarray(vn, dtype=np.float32))
    d, vy, vx = f(np.asarray(d0)[..., 0]), f(vy0), f(vx0)
    re = f([params["re"]])

    def stag(a, b):
        return sol_amd.StaggeredGrid([a.reshape(1, Y + 1, X, 1), b.reshape(1, Y, X + 1, 1)]).staggered_tensor().cpu().numpy()

    zero = np.zeros((1, Y + 1, X + 1, 2), dtype=np.float32)
    scene.scene_write(path, [d.reshape(1, Y, X, 1).cpu().numpy(), stag(vy, vx), zero], ["denTf", "velTf", "corTf"], 0)
    cor = (torch.zeros_like(vy), torch.zeros_like(vx))
    for i in range(1, params["simsteps"]):
        if large:
            # the roll-out hands out the correction it applied: no second, uncorrected solver step per frame
            ro.run(d, vy, vx, re, 1, corr=cor)
            cy, cx = cor
        else:
            py, px = vy.clone(), vx.clone()
            # uncorrected step (for the written correction field) and corrected step
            cfg = ops.karman_cfg(1, Y, X, dom.dx[1], res=res, masks=masks)
            with torch.no_grad():
                _, sy, sx = ops.karman_step(d, py, px, re, cfg, masks)
            ro.run(d, vy, vx, re, 1)
            cy, cx = vy - sy, vx - sx
        scene.scene_write(path, [d.reshape(1, Y, X, 1).cpu().numpy(), stag(vy, vx), stag(cy, cx)], ["denTf", "velTf", "corTf"], i)
        if i % 100 == 0:
            log.info("step {:06d}".format(i))
    return path


if __name__ == "__main__":
    main()
