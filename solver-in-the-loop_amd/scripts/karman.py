#!/usr/bin/env python
"""karman-2d data generation -- same flags as /root/reference/karman-2d/karman.py:33-47, the loop of
:138-159 on the fused HIP solver step (one kernel launch per frame, state stays on the GPU).
-r <= 64 runs the fused one-workgroup-per-simulation kernel; larger grids (the reference's 256x128 `-r 128`
reference solutions, Makefile:19-28) run the multi-launch path (nothing is kept for a backward pass here): the direct pressure solver where the scene's blob builds,
else the preconditioned CG.  --obstacle / --obstacle-mask choose the scene (recorded in params.pickle as "scene").  --buoyancy FY[,FX]
(large grids only): the density pushes the velocity; recorded in params.pickle as "buoyancy" (a pair, or None: off), so that training and
roll-out pick it up from the data.  --diffusion-substeps N|auto: explicit diffusion substeps per step (auto: the smallest count for which
dt res^2 / (n Re) <= 1/4, ops.min_diffusion_substeps); recorded in params.pickle as "diffusion_substeps" (an integer, 1: the single stencil).
--advection semi_lagrangian|mac_cormack, --mc-strength S (mac_cormack: large grids only): the advection scheme of the step; recorded in
params.pickle as "advection" and "correction_strength", picked up from there by training, roll-out and the Re fit.
--multi-launch: the multi-launch path on a grid the one-workgroup kernels would serve (-r 16 ... 64, or a width such as -r 48), where
--buoyancy, mac_cormack and the substeps then work; recorded in params.pickle as "multi_launch" and picked up like them."""
import argparse
import pickle

import numpy as np
import torch

from _common import (add_boundaries_arg, with_boundaries, add_advection_arg, add_buoyancy_arg, add_multi_launch_arg, add_scene_args, add_substeps_arg, advection_from_args, buoyancy_from_args, flow_kwargs,
                     logger, scene_from_args, select_gpu, substeps_from_args)
import sol_amd
from sol_amd import ops, scene


def main(argv=None):
    p = argparse.ArgumentParser(description="Parameter Parser", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--gpu", default="0", help="visible GPUs")
    p.add_argument("--cuda", action="store_true", help="(accepted for compatibility; the solver is always the HIP kernel)")
    p.add_argument("-o", "--output", default=None, help="path to an output directory")
    p.add_argument("--thumb", action="store_true", help="(ignored: no PNG thumbnails)")
    p.add_argument("-t", "--simsteps", default=1500, type=int, help="simulation steps: an epoch")
    p.add_argument("-s", "--skipsteps", default=999, type=int, help="skip first steps; (vortices may not form)")
    p.add_argument("-r", "--res", default=32, type=int, help="resolution of the reference axis")
    p.add_argument("--re", default=1e6, type=float, help="Effective Reynolds number")
    p.add_argument("--initdH", default=None, help="load hires (will be downsampled) density")
    p.add_argument("--initvH", default=None, help="load hires (will be downsampled) velocity")
    p.add_argument("-d", "--scale", default=4, type=int, help="down-sampling scale of hires")
    p.add_argument("-l", "--len", default=100, type=int, help="length of the reference axis")
    p.add_argument("--seed", default=0, type=int, help="seed for random number generator")
    add_scene_args(p)
    add_buoyancy_arg(p)
    add_substeps_arg(p)
    add_advection_arg(p)
    add_multi_launch_arg(p)
    add_boundaries_arg(p)
    params = vars(p.parse_args(argv))
    select_gpu(params["gpu"])
    log = logger()
    res = params["res"]
    Y, X = 2 * res, res
    dom = sol_amd.Domain([Y, X], box=sol_amd.box[0:params["len"] * 2, 0:params["len"]])
    rec = with_boundaries(scene_from_args(params), params)
    params["boundaries"] = params["boundaries"] or "open"
    params["buoyancy"] = buoyancy_from_args(params)
    params["diffusion_substeps"] = substeps_from_args(params, [params["re"]], res) or 1
    name, strength = advection_from_args(params)
    params["advection"], params["correction_strength"] = name or "semi_lagrangian", 1.0 if strength is None else float(strength)
    sim = sol_amd.KarmanFlow(pressure_solver=params["pressure_solver"], buoyancy=params["buoyancy"],
                             diffusion_substeps=params["diffusion_substeps"], advection=params["advection"],
                             correction_strength=params["correction_strength"], multi_launch=params["multi_launch"], **flow_kwargs(rec))
    params["scene"] = sim.scene()
    d0 = scene.downsample(scene.read_zipped_array(params["initdH"]), params["scale"]) if params["initdH"] else np.zeros((1, Y, X, 1))
    if params["initvH"]:
        vn = scene.downsample_staggered(scene.read_zipped_array(params["initvH"]), params["scale"])
    else:                                   # karman.py:106-110: warm start + sideways poke
        vn = np.zeros((1, Y + 1, X + 1, 2))
        vn[..., 0] = 1.0
        vn[..., vn.shape[1] // 2 + 10:vn.shape[1] // 2 + 20, vn.shape[2] // 2 - 2:vn.shape[2] // 2 + 2, 1] = 1.0
    st = sol_amd.Fluid(dom, density=d0, velocity=vn, batch_size=1)
    velBCy, velBCyMask = sol_amd.velocity_bc_masks(Y, X, batch_size=1)
    path = None
    if params["output"]:
        path = scene.scene_create(params["output"])
        logger(path + "/run.log")
        with open(path + "/params.pickle", "wb") as f:
            pickle.dump(params, f)
    log.info({k: v for k, v in params.items() if k != "scene"})
    log.info("scene: %s" % sol_amd.karman.describe_scene(params["scene"]))

    def write(state, i):
        scene.scene_write(path, [state.density.data.cpu().numpy(), state.velocity.staggered_tensor().cpu().numpy()], ["dens", "velo"], i)

    if params["skipsteps"] == 0 and path:
        write(st, 0)
    with torch.no_grad():
        for i in range(1, params["simsteps"]):
            st = sim.step(st, re=[params["re"]], res=res, velBCy=velBCy, velBCyMask=velBCyMask)
            if i == 1:
                log.info("pressure solver: %s" % sim.pressure_solver_used)
            info = sim.solve_info
            if "converged" in info and not bool(info["converged"].all()):
                raise RuntimeError("step {}: the CG pressure solve did not converge within {} iterations (iterations {}); "
                                   "the scene may be unsolvable (an enclosed fluid region?)".format(
                                       i, sim._solver["cg_max_iter"], info["iterations"].tolist()))
            if i % 100 == 0:
                log.info("Step {:06d}".format(i) + (", CG iterations {}".format(info["iterations"].tolist()) if "converged" in info else ""))
            if params["skipsteps"] < i and path:
                write(st, i)
    return path


if __name__ == "__main__":
    main()
