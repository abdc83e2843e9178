#!/usr/bin/env python
"""karman-3d (BASELINE.json configs[4]) from the command line: data generation / roll-out of the 3-D wake flow, optionally
with a trained 3-D corrector, and a SOL-n training demo on frames generated on the fly.

The reference has no 3-D script (/root/reference/README.md:37-38); the flags follow karman-2d/karman.py:33-47 and
karman_apply.py:20-31 (-r res of the reference axis -> grid 2r x r x r, --re, -t steps, -s skip, -o output, --model) so that
the 2-D workflow carries over.  Frames are written like the 2-D scenes: dens_%06d.npz [1,Y,X,Z,1], velo_%06d.npz
[1,Y+1,X+1,Z+1,3] (staggered tensor, zero padded at the high ends, components reversed on disk as PhiFlow does).
--buoyancy FY[,FX[,FZ]]: the density pushes the velocity (generation, --model roll-out and --train-sol alike); recorded in params.pickle
and in the model file as "buoyancy" (a triple, or None: off), so that a roll-out of the trained corrector picks it up.
--diffusion-substeps N|auto: the velocity is diffused by N explicit substeps per solver step (the single stencil is stable only while
dt res^2 / Re <= 1/6; auto: karman3d.min_diffusion_substeps3d of --re), for generation, --model roll-out and --train-sol alike; recorded
in params.pickle and in the model file as "diffusion_substeps" and picked up from there like the force.
--advection semi_lagrangian|mac_cormack, --mc-strength S: the advection scheme of the solver step (mac_cormack keeps what the
semi-Lagrangian step smears; S in [0, 1] is its correction strength), for generation, --model roll-out and --train-sol alike; recorded in
params.pickle and in the model file as "advection" and "correction_strength" and picked up from there like the force.
--obstacle sphere|cylinder: the sphere of the scene, or the disc of the 2-D scene extruded along z (karman3d.cylinder_arrays3d: the wake);
recorded in params.pickle and in the model file as "obstacle" and picked up from there like the force.  --pressure-solver direct_extruded
solves the cylinder's pressure without iteration (any mask that does not depend on z).
--boundaries open|periodic-z: the spanwise axis periodic (Scene3D(boundaries=): the wake in a box periodic along the span), for generation,
--model roll-out and --train-sol alike; recorded in params.pickle and in the model file as "boundaries" and picked up from there like the
force.  With --obstacle cylinder it selects --pressure-solver direct_extruded unless another solver is named (auto names none).
--conv-padding zeros|circular: the correction network's padding along z (--train-sol and the --model roll-out); circular needs
--boundaries periodic-z; recorded in params.pickle and in the model file as "conv_padding" and picked up from there like the force."""
import argparse
import pickle

import numpy as np
import torch

from _common import (add_advection_arg, add_buoyancy_arg, add_substeps_arg, advection_from_args, agreed_advection, agreed_buoyancy, agreed_substeps,
                     buoyancy_from_args, logger, select_gpu, substeps_from_args)
import sol_amd
from sol_amd import karman3d as k3, scene, synthetic
from sol_amd.precond3d import extruded_solver_refusal3d

OBSTACLES = ("sphere", "cylinder")
BOUNDARIES = ("open", "periodic-z")


def staggered3d(vy, vx, vz):
    B, Y1, X, Z = vy.shape
    t = np.zeros((B, Y1, X + 1, Z + 1, 3), dtype=np.float32)
    t[:, :, :X, :Z, 0] = vy
    t[:, :Y1 - 1, :, :Z, 1] = vx
    t[:, :Y1 - 1, :X, :, 2] = vz
    return t


def parse_params(argv=None):
    """The flags, with "buoyancy" as a triple (or None), "diffusion_substeps" as N, `auto` resolved from --re, or None when absent, and
    "advection" / "mc_strength" validated (None when absent).  Touches no device."""
    p = argparse.ArgumentParser(description="Parameter Parser", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--gpu", default="0", help="visible GPUs")
    p.add_argument("-o", "--output", default=None, help="path to an output directory")
    p.add_argument("-t", "--simsteps", default=100, type=int, help="simulation steps")
    p.add_argument("-s", "--skipsteps", default=0, type=int, help="skip first steps when writing")
    p.add_argument("-r", "--res", default=32, type=int, help="resolution of the reference axis (grid 2r x r x r)")
    p.add_argument("--re", default=1e6, type=float, help="Effective Reynolds number")
    p.add_argument("-l", "--len", default=100, type=int, help="length of the reference axis")
    p.add_argument("--model", default=None, help="trained 3-D corrector (.pt written by --train-sol): applied after every solver step")
    p.add_argument("--train-sol", default=0, type=int, help="SOL-n training demo: n unrolled steps per training step on frames generated first")
    p.add_argument("--train-steps", default=4, type=int, help="training steps of the demo")
    p.add_argument("--lr", default=1e-5, type=float)
    p.add_argument("--seed", default=0, type=int)
    p.add_argument("--obstacle-mask", default=None, help="[Y,X,Z] .npy mask of the scene (1 = fluid, 0 = solid) instead of the sphere")
    p.add_argument("--obstacle", default=None, choices=OBSTACLES, help="the scene's obstacle: sphere, or cylinder (the disc extruded along z); "
                   "default: sphere, or what the --model file recorded")
    p.add_argument("--pressure-solver", default="auto", choices=k3.PRESSURE_SOLVERS3D,
                   help="direct (capacitance blob), cg (preconditioned CG, any mask), auto (direct where it builds, else cg) or direct_extruded "
                        "(opt-in: the direct solve for a mask that does not depend on z, such as --obstacle cylinder)")
    p.add_argument("--boundaries", default=None, choices=BOUNDARIES, help="open, or periodic-z: the spanwise axis periodic; default: open, or what "
                   "the --model file recorded")
    p.add_argument("--conv-padding", default=None, choices=("zeros", "circular"), help="padding of the correction network along z (--train-sol and "
                   "the --model roll-out): zeros (Conv3D's 'same'), or circular on --boundaries periodic-z; default: zeros, or what the --model "
                   "file recorded")
    add_buoyancy_arg(p, ncomp=3)
    add_substeps_arg(p, bound="1/6")
    add_advection_arg(p, where="")
    params = vars(p.parse_args(argv))
    if params["obstacle"] is not None and params["obstacle_mask"]:
        p.error("--obstacle and --obstacle-mask both name the scene's obstacle: give one")
    params["advection"], params["mc_strength"] = advection_from_args(params)
    params["buoyancy"] = buoyancy_from_args(params, ncomp=3)
    params["diffusion_substeps"] = substeps_from_args(params, [params["re"]], params["res"], minimum=k3.min_diffusion_substeps3d)
    return params


def apply_model_record(params, record=None):
    """The run's parameters as recorded in params.pickle: parse_params' with the force and the substep count the run uses.  record: the
    dict of the --model file (None: no model) -- the force and the count the corrector was trained with win, a flag that contradicts them
    is an error, and a model without a record takes the flag.  No flag and no record: no force, one substep.  The advection likewise:
    "advection" and "correction_strength" are the scheme the run uses (the model's record, else the flags, else semi_lagrangian / 1).
    "obstacle" likewise: the model's record, else the flag, else the sphere (a model without a record was trained on it)."""
    params = dict(params)
    if record is not None and "obstacle" in record and not params.get("obstacle_mask"):
        if params.get("obstacle") is not None and params["obstacle"] != record["obstacle"]:
            raise SystemExit("--obstacle %s contradicts the obstacle recorded in %s (%s)" % (params["obstacle"], params["model"], record["obstacle"]))
        params["obstacle"] = record["obstacle"]
    params["obstacle"] = params.get("obstacle") or "sphere"
    if record is not None and "boundaries" in record:
        if params.get("boundaries") is not None and params["boundaries"] != record["boundaries"]:
            raise SystemExit("--boundaries %s contradicts the boundaries recorded in %s (%s)" % (params["boundaries"], params["model"], record["boundaries"]))
        params["boundaries"] = record["boundaries"]
    params["boundaries"] = params.get("boundaries") or "open"
    if record is not None and "conv_padding" in record:
        if params.get("conv_padding") is not None and params["conv_padding"] != record["conv_padding"]:
            raise SystemExit("--conv-padding %s contradicts the padding recorded in %s (%s)" % (params["conv_padding"], params["model"], record["conv_padding"]))
        params["conv_padding"] = record["conv_padding"]
    params["conv_padding"] = params.get("conv_padding") or "zeros"
    if params["conv_padding"] == "circular" and params["boundaries"] != "periodic-z":
        raise SystemExit("--conv-padding circular pads the correction network circularly along z and needs --boundaries periodic-z "
                         "(the boundaries are %s)" % params["boundaries"])
    if params["boundaries"] == "periodic-z" and params["obstacle"] == "cylinder" and not params.get("obstacle_mask") and params.get("pressure_solver", "auto") == "auto":
        params["pressure_solver"] = "direct_extruded"       # (the dense periodic blob refuses an obstacle that spans the axis on all but small grids)
    if record is not None and "buoyancy" in record:
        params["buoyancy"] = agreed_buoyancy(record["buoyancy"], params["buoyancy"], params["model"])
    if record is not None and "diffusion_substeps" in record:
        params["diffusion_substeps"] = agreed_substeps(record["diffusion_substeps"], params["diffusion_substeps"], params["model"])
    params["diffusion_substeps"] = params["diffusion_substeps"] or 1
    flags = (params.get("advection"), params.get("mc_strength"))
    if record is not None and "advection" in record:
        params.update(agreed_advection(record, flags, params["model"]))
    else:
        params.update({"advection": flags[0] or "semi_lagrangian", "correction_strength": 1.0 if flags[1] is None else float(flags[1])})
    return params


def main(argv=None):
    params = parse_params(argv)
    blob = torch.load(params["model"], map_location="cpu") if params["model"] else None
    params = apply_model_record(params, blob)
    res = params["res"]
    Y, X, Z = 2 * res, res, res
    if blob is not None or params["train_sol"]:       # a grid the corrector does not take: say so before a device is asked for or a frame generated
        reason = k3.net3d_circular_shape_reason if params["conv_padding"] == "circular" else k3.net3d_shape_reason
        why = reason(Y, X, Z, train=bool(params["train_sol"]))
        if why is not None:
            raise SystemExit("karman3d.py: the correction network does not run at %d x %d x %d -- %s" % (Y, X, Z, why))
    select_gpu(params["gpu"])
    log = logger()
    dev = "cuda"
    active = np.load(params["obstacle_mask"]) if params["obstacle_mask"] else None
    if active is None and params["obstacle"] == "cylinder":
        active = k3.cylinder_arrays3d(Y, X, Z, length=float(params["len"]))[0]
    sc = k3.Scene3D(Y, X, Z, length=float(params["len"]), device=dev, active=active, pressure_solver=params["pressure_solver"],
                    **({} if params["boundaries"] == "open" else {"boundaries": params["boundaries"]}))
    buoyancy, nsub = params["buoyancy"], params["diffusion_substeps"]
    adv = {"advection": params["advection"], "correction_strength": params["correction_strength"]}
    sim = k3.Karman3DFlow(sc, 1, buoyancy=buoyancy, diffusion_substeps=nsub, **adv)
    f = lambda a: torch.as_tensor(a, dtype=torch.float32, device=dev).contiguous()
    # karman.py:106-110 in 3-D: uniform flow along y + a sideways poke behind the obstacle
    vy = np.ones((1, Y + 1, X, Z), dtype=np.float32)
    vx = np.zeros((1, Y, X + 1, Z), dtype=np.float32)
    vz = np.zeros((1, Y, X, Z + 1), dtype=np.float32)
    vx[:, Y // 2 + Y // 12:Y // 2 + Y // 6, X // 2 - 2:X // 2 + 2, Z // 2 - 2:Z // 2 + 2] = 1.0
    st = (f(np.zeros((1, Y, X, Z))), f(vy), f(vx), f(vz))
    re = f([params["re"]])
    path = None
    if params["output"]:
        path = scene.scene_create(params["output"])
        logger(path + "/run.log")
        with open(path + "/params.pickle", "wb") as fh:
            pickle.dump(params, fh)
    log.info(params)
    hint = ""
    if params["pressure_solver"] == "auto" and sc.pressure_solver == "cg" and extruded_solver_refusal3d(sc.active_np) is None:
        hint = " (the mask does not depend on z: --pressure-solver direct_extruded solves it without iteration)"
    log.info("pressure solver: %s%s" % (sc.pressure_solver, hint))
    log.info("obstacle: %s" % (params["obstacle_mask"] or params["obstacle"]))
    log.info("boundaries: %s" % params["boundaries"])
    log.info("conv padding: %s" % params["conv_padding"])
    log.info("buoyancy: %s" % (buoyancy,))
    log.info("diffusion substeps: %d" % nsub)
    log.info("advection: %s (correction strength %g)" % (adv["advection"], adv["correction_strength"]))
    net = ro = None
    if blob is not None:
        net = k3.MarsMoon3D(device=dev)
        net.set_weights([w.numpy() for w in blob["weights"]])
        ro = k3.Karman3DRollout(net, sc, 1, blob["std_v"], blob["std_re"], buoyancy=buoyancy, diffusion_substeps=nsub,
                                conv_padding=params["conv_padding"], **adv)
    frames = []
    with torch.no_grad():
        for i in range(1, params["simsteps"]):
            st = ro.step(*st, re) if ro is not None else sim.step(*st, re)
            if params["train_sol"]:
                frames.append(tuple(t.clone() for t in st))
            if i % 50 == 0:
                log.info("Step {:06d}".format(i))
            if path and i > params["skipsteps"]:
                scene.scene_write(path, [st[0].reshape(1, Y, X, Z, 1).cpu().numpy(),
                                         staggered3d(st[1].cpu().numpy(), st[2].cpu().numpy(), st[3].cpu().numpy())], ["dens", "velo"], i)
    loss = None
    if params["train_sol"]:
        ms = params["train_sol"]
        if len(frames) < ms + 1:
            raise SystemExit("karman3d.py: --train-sol %d needs at least %d simulation steps" % (ms, ms + 2))
        std_v = tuple(float(torch.stack([fr[c] for fr in frames]).abs().std()) + 1e-6 for c in (1, 2, 3))
        net = k3.MarsMoon3D(seed=params["seed"], device=dev)
        w = net.get_weights()
        w[22] = w[22] * 0.01
        net.set_weights(w)
        tr = k3.Karman3DTrainer(net, sc, 1, ms, std_v, max(params["re"], 1.0), use_graph=True, buoyancy=buoyancy, diffusion_substeps=nsub,
                                conv_padding=params["conv_padding"], **adv)
        rng = np.random.default_rng(params["seed"])
        for it in range(params["train_steps"]):
            k = int(rng.integers(0, len(frames) - ms))
            gts = [frames[k + 1 + j][1:] for j in range(ms)]
            loss = float(tr.train_step(*frames[k], re, gts, lr=params["lr"]))
            log.info("train step {:04d}: loss={}".format(it + 1, loss))
        if path:
            torch.save({"name": net.name, "weights": [torch.as_tensor(a) for a in net.get_weights()], "std_v": std_v,
                        "std_re": max(params["re"], 1.0), "buoyancy": buoyancy, "diffusion_substeps": nsub, "obstacle": params["obstacle"], "boundaries": params["boundaries"],
                        "conv_padding": params["conv_padding"], **adv}, path + "/model3d.pt")
    return path if path else loss


if __name__ == "__main__":
    main()
