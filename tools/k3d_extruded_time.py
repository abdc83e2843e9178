#!/usr/bin/env python
"""karman-3d direct pressure solve for obstacles extruded along z: the cylinder on "direct_extruded" against the cylinder
on CG, with the sphere on the dense direct solve as the yardstick; one JSON line, also written to profiles/k3d_extruded_time.json.

At 128 x 64 x 64, B = 1 and B = 6, in ONE process, the three scenes ALTERNATED (a, b, c, a, b, c: a drift of the clock hits all), HIP
events around eager calls, the minimum over the blocks of each:
  * the pressure solve alone (sol_karman3d_pressure_solve; right-hand side -div of a seeded unprojected velocity field), with the CG
    iterations;
  * the forward step and the forward + adjoint step on a spun-up state;
  * the kernel split of the extruded solve (sol_prof_begin / sol_prof_end: device time per kernel, us per solve): the three correction
    launches next to the launches of the two applications of G;
  * the SOL-16 training step (Karman3DTrainer, B = 1, replayed graph) on the cylinder, both solvers, alternated.
The acceptance line of the option: "solve_speedup_cg_over_extruded" >= 10 at B = 1.  The file records what was measured, on whatever
clock the box held ("clocks": rocm-smi's lines, read only, before and after); compare the numbers of one file with each other only.
Usage: python tools/k3d_extruded_time.py [reps]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch          # noqa: E402
import sol_amd        # noqa: E402,F401
from sol_amd import _lib                          # noqa: E402
from sol_amd import karman3d as k3, synthetic     # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
DEV = "cuda"
Y, X, Z = 128, 64, 64
SCENES = (("cylinder_cg", "cylinder", "cg"), ("cylinder_extruded", "cylinder", "direct_extruded"), ("sphere_direct", "sphere", "direct"))


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def alternated(fns, reps, rounds=4):
    """us per call of every function, `rounds` blocks of each in turn; the minimum over the blocks of each"""
    for f in fns:
        f()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(rounds):
        for k, f in enumerate(fns):
            t[k].append(timed(f, reps))
    return [min(v) for v in t]


def clocks():
    """rocm-smi's clock lines (read only), as tools/k3d_maccormack_time.py records them"""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
        return [l.strip() for l in r.stdout.splitlines() if "sclk" in l or "mclk" in l]
    except Exception as e:
        return ["unavailable: %s" % e]


def kernels(fn, reps):
    torch.cuda.synchronize()
    with _lib.profile() as p:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    return {k.strip("()").replace(" ", ""): round(tot / reps, 3) for k, (calls, tot) in sorted(p.kernels.items())}


def state(B, seed=1):
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    return (torch.rand(B, Y, X, Z, generator=gen).to(DEV), (1.0 + 0.1 * rn(B, Y + 1, X, Z)).to(DEV), (0.1 * rn(B, Y, X + 1, Z)).to(DEV),
            (0.1 * rn(B, Y, X, Z + 1)).to(DEV))


def scene_of(obstacle, solver):
    active = k3.cylinder_arrays3d(Y, X, Z)[0] if obstacle == "cylinder" else None
    return k3.Scene3D(Y, X, Z, device=DEV, active=active, pressure_solver=solver)


def batch_run(scenes, B, reps):
    re = synthetic.reynolds(B).float().to(DEV)
    _, vy, vx, vz = state(B, 3)              # the solve's right-hand side: -div of an unprojected field
    rhs = (-((vy[:, 1:] - vy[:, :-1]) + (vx[:, :, 1:] - vx[:, :, :-1]) + (vz[..., 1:] - vz[..., :-1]))).contiguous()
    sims, sts, r = [], [], {}
    for name, _, _ in SCENES:
        sim = k3.Karman3DFlow(scenes[name], B)
        with torch.no_grad():
            st = sim.step(*state(B), re)       # spun-up state for the step timings
            st = sim.step(*st, re)
        sims.append(sim)
        sts.append(st)
        r[name] = {"solver": scenes[name].pressure_solver}
    w = [torch.randn(t.shape, generator=torch.Generator().manual_seed(7)).to(DEV) for t in sts[0][1:]]

    def fb(sim, st):
        v = [t.clone().requires_grad_(True) for t in st[1:]]
        out = sim.step(st[0], v[0], v[1], v[2], re)
        sum((a * b).sum() for a, b in zip(out[1:], w)).backward()

    us = alternated([lambda s=s: s.pressure_solve(rhs) for s in sims], reps)
    for (name, _, _), sim, t in zip(SCENES, sims, us):
        r[name]["solve_us"] = t
        if sim.cg:
            r[name]["solve_iterations"] = sim.solve_info["iterations"].tolist()
            r[name]["solve_converged"] = sim.solve_info["converged"].tolist()
    with torch.no_grad():
        us = alternated([lambda s=s, st=st: s.step(*st, re) for s, st in zip(sims, sts)], reps)
    for (name, _, _), t in zip(SCENES, us):
        r[name]["step_fwd_us"] = t
    us = alternated([lambda s=s, st=st: fb(s, st) for s, st in zip(sims, sts)], reps)
    for (name, _, _), sim, t in zip(SCENES, sims, us):
        r[name]["step_fwd_bwd_us"] = t
        if sim.cg:
            r[name]["iterations_fwd"] = sim.solve_info["iterations"].tolist()
            r[name]["iterations_bwd"] = sim.solve_info["iterations_bwd"].tolist()
    ext = sims[1]
    ks = kernels(lambda: ext.pressure_solve(rhs), min(reps, 20))
    corr = {k: v for k, v in ks.items() if k.startswith("k3e_")}
    r["extruded_solve_kernels_us"] = ks
    r["correction_launches_us"] = sum(corr.values())
    r["one_G_us"] = sum(v for k, v in ks.items() if k.startswith("k3_t")) / 2.0          # (k3_fill: the entry point's copy of the right-hand side)
    r["correction_over_one_G"] = r["correction_launches_us"] / r["one_G_us"]
    r["sphere_solve_kernels_us"] = kernels(lambda: sims[2].pressure_solve(rhs), min(reps, 20))
    r["sphere_correction_launches_us"] = sum(v for k, v in r["sphere_solve_kernels_us"].items() if k.startswith("k3_cap"))
    for what in ("solve_us", "step_fwd_us", "step_fwd_bwd_us"):
        r[what.replace("_us", "") + "_speedup_cg_over_extruded"] = r["cylinder_cg"][what] / r["cylinder_extruded"][what]
        r[what.replace("_us", "") + "_extruded_over_sphere"] = r["cylinder_extruded"][what] / r["sphere_direct"][what]
    return r


def trainers(scenes, steps):
    ms = 16
    re = synthetic.reynolds(1).float().to(DEV)
    fns, trs = [], []
    for name in ("cylinder_cg", "cylinder_extruded"):
        net = k3.MarsMoon3D(seed=3, device=DEV)
        w = net.get_weights()
        w[22] = w[22] * 0.01
        net.set_weights(w)
        tr = k3.Karman3DTrainer(net, scenes[name], 1, ms, (0.2, 0.2, 0.2), synthetic.STD_RE, use_graph=True)
        with torch.no_grad():
            st = tr.sim.step(*state(1, 11), re)
            gs, gts = st, []
            for _ in range(ms):
                gs = tr.sim.step(*gs, re)
                gts.append(tuple(t.clone() for t in gs[1:]))
        tr.fwd_bwd(*st, re, gts)                        # warm-up + capture
        torch.cuda.synchronize()
        trs.append(tr)
        fns.append(lambda tr=tr, st=st, gts=gts: tr.fwd_bwd(*st, re, gts))
    us = alternated(fns, steps, rounds=2)
    r = {"msteps": ms, "B": 1, "use_graph": True}
    for name, tr, t in zip(("cylinder_cg", "cylinder_extruded"), trs, us):
        r[name] = {"sol16_step_ms": t / 1e3, "loss": float(tr._loss)}
    r["cylinder_cg"]["iterations_fwd_last"] = int(trs[0].sim.solve_info["iterations"][0])
    r["cylinder_cg"]["iterations_bwd_last"] = int(trs[0].sim.solve_info["iterations_bwd"][0])
    r["speedup_cg_over_extruded"] = us[0] / us[1]
    return r


def main():
    out = {"tool": "k3d_extruded_time", "reps": REPS, "device": torch.cuda.get_device_name(0), "grid": [Y, X, Z],
           "cg_max_iter": k3.CG_MAX_ITER3D, "cg_rtol": 1e-6, "cg_atol": 1e-9, "clocks_before": clocks()}
    scenes = {name: scene_of(ob, solver) for name, ob, solver in SCENES}
    out["extruded_blob"] = {"nS2": int(scenes["cylinder_extruded"].direct_header[4]), "SP2": int(scenes["cylinder_extruded"].direct_header[5]),
                            "words": int(scenes["cylinder_extruded"].direct.numel())}
    for B in (1, 6):
        out["B%d" % B] = batch_run(scenes, B, REPS)
    out["train_sol16"] = trainers(scenes, 3)
    out["accepted"] = bool(out["B1"]["solve_speedup_cg_over_extruded"] >= 10.0)
    out["clocks"] = clocks()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "k3d_extruded_time.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
