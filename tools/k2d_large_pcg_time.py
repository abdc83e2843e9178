#!/usr/bin/env python
"""karman-2d large-grid pressure solves, direct vs preconditioned CG: one JSON line, also written to
profiles/k2d_large_pcg_time.json.

At 256 x 128, B = 1, per scene: the pressure solve alone in us (sol_karman_pressure_solve_large; right-hand side -div of a seeded
unprojected velocity field) with its CG iterations, the forward step in us (HIP events around eager calls; the CG step's eager call
stops issuing iterations once converged) with its iterations, and the price of ONE empty tail iteration: the captured CG step
(full launch budget, every launch of a finished simulation returns at once) replayed with two budgets beyond convergence,
(t(K2) - t(K1)) / (K2 - K1).  Scenes: default sphere (direct and CG), two cylinders in tandem and a plate (CG: the direct blob is
refused).
Usage: python tools/k2d_large_pcg_time.py [reps]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np    # noqa: E402
import torch          # noqa: E402
from sol_amd import fluid, karman, ops   # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
DEV = "cuda"
Y, X, B = 256, 128, 1
SCENES = {"sphere_direct": (None, "direct"), "sphere_cg": (None, "cg"),
          "two_cylinders_cg": (["sphere:50,50,10", "sphere:120,50,10"], "auto"), "plate_cg": (["box:70:73,20:80"], "auto")}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def state(seed):
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    return (torch.rand(B, Y, X, generator=gen).to(DEV), (1.0 + 0.1 * rn(B, Y + 1, X)).to(DEV), (0.1 * rn(B, Y, X + 1)).to(DEV))


def scene_run(specs, solver, reps):
    dom = fluid.Domain([Y, X], box=fluid.box[0:200, 0:100])
    flow = karman.KarmanFlow(obstacles=None if specs is None else karman.parse_obstacles(specs))
    active, inflow = flow.scene_arrays(dom)
    bc, _ = karman.velocity_bc_masks(Y, X)
    mk = ops.SceneMasks(active, inflow, bc.reshape(Y + 1, X), bc.reshape(Y + 1, X), DEV, pressure_solver=solver)
    cfg = ops.karman_cfg(B, Y, X, dom.dx[1], masks=mk)
    re = torch.full((B,), 1.6e5, device=DEV)
    ws = torch.empty((ops.large_workspace_bytes(cfg, mk) + 3) // 4, dtype=torch.float32, device=DEV)
    with torch.no_grad():
        st = ops.karman_step_large(*state(1), re, cfg, mk, ws)         # spun-up state for the step timings
        st = ops.karman_step_large(*st, re, cfg, mk, ws)
    r = {"scene": flow.scene()["obstacles"], "solver": mk.pressure_solver, "grid": [Y, X], "B": B}
    info = {}
    with torch.no_grad():
        r["step_fwd_us"] = timed(lambda: ops.karman_step_large(*st, re, cfg, mk, ws, info), reps)
    if mk.pressure_solver != "cg":
        return r
    r["step_iterations"], r["step_converged"] = int(info["iterations"][0]), int(info["converged"][0])
    _, vy, vx = state(3)
    rhs = (-((vy[:, 1:] - vy[:, :-1]) + (vx[:, :, 1:] - vx[:, :, :-1]))).contiguous()
    sinfo = {}
    r["solve_us"] = timed(lambda: ops.pressure_solve_large(rhs, cfg, mk, ws, sinfo), reps)
    r["solve_iterations"], r["solve_converged"] = int(sinfo["iterations"][0]), int(sinfo["converged"][0])
    # one empty tail iteration: captured steps (the full budget) with two budgets beyond convergence
    k1 = r["step_iterations"] + 16
    k2 = k1 + 200
    t = {}
    for k in (k1, k2):
        c = ops.karman_cfg(B, Y, X, dom.dx[1], masks=mk, cg_max_iter=k)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s), torch.no_grad():
            with torch.cuda.graph(g, stream=s):
                ops.karman_step_large(*st, re, c, mk, ws)
        torch.cuda.current_stream().wait_stream(s)
        t[k] = timed(g.replay, reps)
        del g
    r["captured_step_us"] = {str(k): v for k, v in t.items()}
    r["empty_tail_iteration_us"] = (t[k2] - t[k1]) / (k2 - k1)
    return r


def main():
    out = {"tool": "k2d_large_pcg_time", "reps": REPS, "cg_max_iter": 2000, "cg_rtol": 1e-6, "cg_atol": 1e-9,
           "device": torch.cuda.get_device_name(0)}
    for name, (specs, solver) in SCENES.items():
        out[name] = scene_run(specs, solver, REPS)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "k2d_large_pcg_time.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
