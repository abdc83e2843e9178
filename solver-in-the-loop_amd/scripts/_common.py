import logging
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def logger(path=None):
    log = logging.getLogger("sol")
    if not log.handlers:
        log.addHandler(logging.StreamHandler())
    log.setLevel(logging.INFO)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        log.addHandler(logging.FileHandler(path))
    return log


def add_scene_args(p, warm_start=False):
    """--obstacle / --obstacle-mask / --pressure-solver of the 2-D scripts (defaults: the reference's sphere, automatic solver);
    warm_start: also --cg-warm-start (the roll-out script, which performs consecutive solves of one scene)."""
    p.add_argument("--obstacle", action="append", default=None, metavar="SPEC",
                   help="obstacle in domain coordinates, repeatable: sphere:CY,CX,R | box:Y0:Y1,X0:X1 | none (default: sphere:50,50,10)")
    p.add_argument("--obstacle-mask", default=None, metavar="FILE.npy", help="[Y, X] fluid mask (1 = fluid) for exactly this grid")
    p.add_argument("--pressure-solver", default="auto", choices=("auto", "direct", "cg", "direct_scattered"),
                   help="pressure solve of the solver step (direct_scattered: the direct solve for obstacles beyond one window, large grids only)")
    if warm_start:
        p.add_argument("--cg-warm-start", action="store_true",
                       help="start every CG pressure solve from the previous frame's pressure (large grids; ignored with the direct solve)")


def scene_from_args(params):
    """scene_record of the scene flags, or None when neither flag is given."""
    import numpy as np
    from sol_amd import karman
    if params["obstacle"] is not None and params["obstacle_mask"] is not None:
        raise SystemExit("give --obstacle or --obstacle-mask, not both")
    if params["obstacle_mask"] is not None:
        return karman.scene_record(active=np.load(params["obstacle_mask"]))
    if params["obstacle"] is not None:
        try:
            return karman.scene_record(obstacles=karman.parse_obstacles(params["obstacle"]))
        except ValueError as e:
            raise SystemExit(str(e))
    return None


_BUOYANCY_SPELLING = {2: "FY[,FX]", 3: "FY[,FX[,FZ]]"}


def add_buoyancy_arg(p, ncomp=2):
    """--buoyancy FY[,FX] of karman.py, karman_train.py and karman_apply.py; ncomp=3: --buoyancy FY[,FX[,FZ]] of karman3d.py"""
    p.add_argument("--buoyancy", default=None, metavar=_BUOYANCY_SPELLING[ncomp],
                   help="buoyancy force per unit density: the density pushes the velocity (%sPhiFlow's buoyancy_factor b "
                        "is FY = 9.81 b).  Stored with the data like the scene; absent: off" % ("large grids only; " if ncomp == 2 else ""))


def buoyancy_from_args(params, ncomp=2):
    """(fy, fx) of --buoyancy FY[,FX] -- ncomp=3: (fy, fx, fz) of --buoyancy FY[,FX[,FZ]] --, or None when the flag is absent."""
    if params.get("buoyancy") is None:
        return None
    try:
        vals = [float(v) for v in str(params["buoyancy"]).split(",")]
        if not 1 <= len(vals) <= ncomp:
            raise ValueError
        if ncomp == 3:
            from sol_amd import karman3d
            return karman3d.buoyancy_force3d(tuple(vals))
        from sol_amd import ops
        return ops.buoyancy_force(tuple(vals + [0.0])[:2])
    except ValueError:
        raise SystemExit("bad --buoyancy %r: expected %s (finite numbers)" % (params["buoyancy"], "FY or FY,FX" if ncomp == 2 else "FY, FY,FX or FY,FX,FZ"))


def agreed_buoyancy(recorded, flag, where):
    """The force of a run that reads data: what the data recorded (None: off), unless --buoyancy says otherwise -- a contradiction."""
    norm = lambda f: None if f is None or all(v == 0.0 for v in f) else tuple(float(v) for v in f)
    if flag is not None and norm(flag) != norm(recorded):
        raise SystemExit("--buoyancy %s contradicts the force recorded in %s (%s)" % (flag, where, recorded))
    return norm(recorded)


def add_advection_arg(p, generates=True, where="large grids only; "):
    """--advection semi_lagrangian|mac_cormack and --mc-strength S of karman.py; the scripts that read data default to what the data recorded.
    where: on which grids mac_cormack runs, for the help text (karman3d.py: every grid, "")"""
    p.add_argument("--advection", default=None, choices=["semi_lagrangian", "mac_cormack"],
                   help="advection scheme of the solver step (mac_cormack: %skeeps what the semi-Lagrangian step smears).  "
                        "Stored with the data like the scene; absent: %s" % (where, "semi_lagrangian" if generates else "what the data recorded"))
    p.add_argument("--mc-strength", default=None, type=float, metavar="S",
                   help="correction strength of mac_cormack, 0 <= S <= 1; absent: %s" % ("1" if generates else "what the data recorded"))


def advection_from_args(params):
    """(name, strength) of --advection / --mc-strength with None for an absent flag; a strength outside [0, 1] ends the run"""
    from sol_amd import ops
    name, s = params.get("advection"), params.get("mc_strength")
    try:
        ops.advection_arg(name or "semi_lagrangian", 1.0 if s is None else s, "--advection")
    except ValueError as e:
        raise SystemExit("bad --advection / --mc-strength: %s" % e)
    return name, s


def agreed_advection(recorded, flags, where):
    """The advection of a run that reads data, as KarmanFlow / trainer keywords: what the data recorded ("advection", "correction_strength";
    absent: semi_lagrangian), unless the flags say otherwise -- a contradiction.  recorded: a dict with those keys, or None."""
    rec = recorded or {}
    name, s = rec.get("advection") or "semi_lagrangian", float(1.0 if rec.get("correction_strength") is None else rec["correction_strength"])
    if flags[0] is not None and flags[0] != name:
        raise SystemExit("--advection %s contradicts the scheme recorded in %s (%s)" % (flags[0], where, name))
    if flags[1] is not None and name == "mac_cormack" and float(flags[1]) != s:
        raise SystemExit("--mc-strength %s contradicts the strength recorded in %s (%s)" % (flags[1], where, s))
    return {"advection": name, "correction_strength": s}


def add_multi_launch_arg(p, generates=True):
    """--multi-launch of the karman-2d scripts: the multi-launch solver path (KarmanFlow / SceneMasks / trainers with multi_launch=True)
    on a grid the fused one-workgroup kernels would serve -- what --buoyancy, --advection mac_cormack and --diffusion-substeps need there.
    Recorded with the data; the scripts that read data take it from there as well."""
    p.add_argument("--multi-launch", action="store_true",
                   help="run the multi-launch solver path on a grid the one-workgroup kernels would serve (Y, X >= 16): buoyancy, mac_cormack and "
                        "diffusion substeps are built on it.  Stored with the data; %s" % ("absent: off" if generates else "also taken from what the data recorded"))


def agreed_multi_launch(recorded, flag):
    """The path of a run that reads data: multi-launch when the data recorded it or the flag asks for it (a choice of kernels, not of
    physics: nothing to contradict)"""
    return bool(recorded) or bool(flag)


def add_substeps_arg(p, auto=True, bound="1/4"):
    """--diffusion-substeps N|auto of karman.py (auto: the smallest stable count for the run's Reynolds numbers); the scripts that read
    data take N only and default to what the data recorded.  bound: the single stencil's stability bound in the help text (karman3d.py: 1/6)"""
    p.add_argument("--diffusion-substeps", default=None, metavar="N|auto" if auto else "N",
                   help="explicit diffusion substeps per solver step (the single stencil is stable only while dt res^2 / Re <= %s)%s.  "
                        "Stored with the data like the scene; absent: %s"
                        % (bound, "; auto: the smallest stable count (min_diffusion_substeps) for the run's Reynolds numbers" if auto else "",
                           "1" if auto else "what the data recorded"))


def substeps_from_args(params, re_numbers=None, res=None, dt=1.0, minimum=None):
    """n of --diffusion-substeps: an integer >= 1, `auto` (re_numbers given: ops.min_diffusion_substeps over them -- or `minimum`, a function
    of the same arguments: karman3d.min_diffusion_substeps3d), or None when absent"""
    from sol_amd import ops
    v = params.get("diffusion_substeps")
    if v is None:
        return None
    if str(v).strip().lower() == "auto":
        if re_numbers is None:
            raise SystemExit("--diffusion-substeps auto belongs to data generation; this script takes the count from the data (or N)")
        return (minimum or ops.min_diffusion_substeps)(min(float(r) for r in re_numbers), res, dt)
    try:
        return ops.diffusion_substeps_arg(int(str(v)), "--diffusion-substeps")
    except ValueError:
        raise SystemExit("bad --diffusion-substeps %r: expected an integer >= 1%s" % (v, " or 'auto'" if re_numbers is not None else ""))


def agreed_substeps(recorded, flag, where):
    """The substep count of a run that reads data: what the data recorded (None / absent: 1), unless the flag says otherwise -- a contradiction."""
    rec = 1 if recorded is None else int(recorded)
    if flag is not None and int(flag) != rec:
        raise SystemExit("--diffusion-substeps %s contradicts the count recorded in %s (%s)" % (flag, where, rec))
    return rec


def flow_kwargs(rec):
    """KarmanFlow / GraphTrainer keywords of a scene_record (None: the default scene); a record with periodic boundaries adds them."""
    from sol_amd import karman
    if rec is None:
        return {}
    kw = {"boundaries": tuple(rec["boundaries"])} if "boundaries" in rec else {}
    if rec["active"] is not None:
        return dict(kw, active=rec["active"])
    return dict(kw, obstacles=karman.parse_obstacles(rec["obstacles"]) if rec["obstacles"] else [])


BOUNDARIES = {"open": ("open", "open"), "periodic-x": ("open", "periodic")}


def add_boundaries_arg(p):
    """--boundaries open|periodic-x of karman.py: periodic lateral sides (the x axis wraps; the multi-launch path with a direct solve).
    Recorded in params.pickle ("boundaries", and inside "scene"); the scripts that read data take it from the scene record."""
    p.add_argument("--boundaries", default=None, choices=sorted(BOUNDARIES),
                   help="domain boundaries: open on all sides, or periodic along x (needs the multi-launch path: -r 128, or --multi-launch).  "
                        "Stored with the data like the scene; absent: open")


def with_boundaries(rec, params):
    """The scene record with the --boundaries flag applied (None stays None while the flag is absent or open)"""
    from sol_amd import karman
    b = BOUNDARIES[params.get("boundaries") or "open"]
    if b == ("open", "open"):
        return rec
    rec = dict(rec) if rec is not None else karman.scene_record()
    rec["boundaries"] = b
    return rec


def inherit_boundaries(rec, recorded):
    """A scene given by flags (which carry no boundaries) takes those of the recorded scene before the two are compared"""
    if rec is not None and recorded is not None and "boundaries" in recorded and "boundaries" not in rec:
        rec = dict(rec, boundaries=recorded["boundaries"])
    return rec


def boundaries_name(rec):
    """"open" or "periodic-x" of a scene record (None: open), as the scripts record it beside the scene"""
    from sol_amd import karman
    b = karman.record_boundaries(rec or {})
    for name, pair in BOUNDARIES.items():
        if tuple(b) == pair:
            return name
    return "%s,%s" % tuple(b)


def select_gpu(gpu):
    """`--gpu` of the reference scripts sets CUDA_VISIBLE_DEVICES (karman_train.py:49).  Same here (HIP honours
    HIP_VISIBLE_DEVICES / CUDA_VISIBLE_DEVICES) when the process is not a rank of a launcher, which owns the device choice,
    and as long as no device has been initialised yet."""
    import os
    import torch
    if "LOCAL_RANK" in os.environ or gpu in (None, "", "-1") or torch.cuda.is_initialized():
        return
    os.environ.setdefault("HIP_VISIBLE_DEVICES", str(gpu))
