#!/usr/bin/env python
"""karman-2d buoyancy on large grids: what the force adds to a forward step, to its adjoint and to a training step, one JSON
line, also written to profiles/k2d_buoyancy_time.json.

At 256 x 128, B = 2, the default sphere (direct solve), in ONE process and on a spun-up state, each pair ALTERNATED (a, b, a, b: a drift
of the clock hits both), HIP events around eager calls:
  * forward: ops.karman_step_saved with F = (0.981, 0) (sol_karman_step_fwd_large_saved_buoy: one streaming launch more) against the
    plain call;
  * adjoint: ops.karman_step_large_bwd_buoy with fixed random cotangents (the velocity adjoint, k_lb_buoyancy_adj, then the density
    adjoint's launches) against the plain velocity adjoint ops.karman_step_large_bwd -- and, as the like-for-like yardstick, against
    the plain velocity adjoint FOLLOWED by the density adjoint (what density_grad=True runs without a force);
  * a LargeGridTrainer step (mars_moon, msteps = 2, captured graph, fwd_bwd only) with and without the force;
and the kernel split of the buoyant forward step and adjoint (sol_prof_begin / sol_prof_end: device time per kernel, us per call).
Reported as ratios to the plain calls.  No threshold: the file records what was measured, on whatever clock the box held ("clocks":
rocm-smi's lines after the runs); compare the numbers of one file with each other and with nothing else.
Usage: python tools/k2d_buoyancy_time.py [reps]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch          # noqa: E402
import sol_amd        # noqa: E402
from sol_amd import _lib, fluid, karman, ops   # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
DEV = "cuda"
Y, X, B = 256, 128, 2
FORCE = (0.981, 0.0)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def alternated(a, b, reps, rounds=4):
    """us per call of a and of b, `rounds` blocks of each in turn; the minimum over the blocks of each"""
    a(), b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(a, reps))
        tb.append(timed(b, reps))
    return min(ta), min(tb)


def clocks():
    """rocm-smi's clock lines (read only), as tools/k2d_large_rollout_time.py records them"""
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
    return {k: round(tot / reps, 3) for k, (calls, tot) in sorted(p.kernels.items())}


def main():
    dom = fluid.Domain([Y, X], box=fluid.box[0:200, 0:100])
    flow = karman.KarmanFlow()
    active, inflow = flow.scene_arrays(dom)
    bc, _ = karman.velocity_bc_masks(Y, X)
    mk = ops.SceneMasks(active, inflow, bc.reshape(Y + 1, X), bc.reshape(Y + 1, X), DEV)
    cfg = ops.karman_cfg(B, Y, X, dom.dx[1], masks=mk)
    re = torch.full((B,), 1.6e5, device=DEV)
    gen = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)
    st = (torch.rand(B, Y, X, generator=gen, dtype=torch.float32).to(DEV), (1.0 + 0.1 * rn(B, Y + 1, X)).to(DEV), (0.1 * rn(B, Y, X + 1)).to(DEV))
    ws = torch.empty((ops.large_workspace_bytes(cfg, mk) + 3) // 4, dtype=torch.float32, device=DEV)
    with torch.no_grad():
        for _ in range(2):                                                     # spun-up state
            st = ops.karman_step_large(*st, re, cfg, mk, ws, buoyancy=FORCE)
        _, svy, svx = ops.karman_step_saved(*st, re, cfg, mk, ws, buoyancy=FORCE)
    wd, wy, wx = rn(B, Y, X).to(DEV), rn(B, Y + 1, X).to(DEV), rn(B, Y, X + 1).to(DEV)
    wsb = torch.empty((ops.large_bwd_workspace_bytes(cfg, mk) + 3) // 4, dtype=torch.float32, device=DEV)
    wsd = torch.empty((ops.density_bwd_workspace_bytes(cfg) + 3) // 4, dtype=torch.float32, device=DEV)
    fwd_b = lambda: ops.karman_step_saved(*st, re, cfg, mk, ws, buoyancy=FORCE)
    fwd_p = lambda: ops.karman_step_saved(*st, re, cfg, mk, ws)
    bwd_b = lambda: ops.karman_step_large_bwd_buoy(st[0], svy, svx, re, wy, wx, wd, cfg, mk, FORCE, workspace=wsb, density_workspace=wsd)
    bwd_p = lambda: ops.karman_step_large_bwd(svy, svx, re, wy, wx, cfg, mk, wsb)

    def bwd_pd():
        gy, gx = ops.karman_step_large_bwd(svy, svx, re, wy, wx, cfg, mk, wsb)
        return ops.karman_density_bwd(st[0], svy, svx, re, wd, cfg, mk, gy, gx, wsd)

    r = {"tool": "k2d_buoyancy_time", "reps": REPS, "device": torch.cuda.get_device_name(0), "scene": flow.scene()["obstacles"],
         "solver": mk.pressure_solver, "grid": [Y, X], "B": B, "force": list(FORCE)}
    with torch.no_grad():
        r["forward_buoyant_us"], r["forward_plain_us"] = alternated(fwd_b, fwd_p, REPS)
        r["adjoint_buoyant_us"], r["adjoint_velocity_only_us"] = alternated(bwd_b, bwd_p, REPS)
        r["adjoint_buoyant_again_us"], r["adjoint_velocity_and_density_us"] = alternated(bwd_b, bwd_pd, REPS)
        r["forward_ratio"] = r["forward_buoyant_us"] / r["forward_plain_us"]
        r["adjoint_ratio_to_velocity_only"] = r["adjoint_buoyant_us"] / r["adjoint_velocity_only_us"]
        r["adjoint_ratio_to_velocity_and_density"] = r["adjoint_buoyant_again_us"] / r["adjoint_velocity_and_density_us"]
        preps = min(REPS, 50)                                                  # (every launch carries two events)
        r["forward_buoyant_kernels_us"] = kernels(fwd_b, preps)
        r["adjoint_buoyant_kernels_us"] = kernels(bwd_b, preps)
    # a training step: LargeGridTrainer, mars_moon, msteps = 2, B = 2, captured graph
    ms = 2
    gt = (torch.stack([svy] * ms).contiguous(), torch.stack([svx] * ms).contiguous())
    trainers = []
    for f in (FORCE, None):
        net = sol_amd.model_mars_moon(cin=3, cout=2, seed=0)
        tr = sol_amd.LargeGridTrainer(net, B, Y, X, ms, (0.2, 0.2), 1.0e6, buoyancy=f)
        trainers.append(lambda tr=tr: tr.fwd_bwd(*st, re, *gt))
    r["trainer_buoyant_us"], r["trainer_plain_us"] = alternated(trainers[0], trainers[1], max(4, REPS // 5))
    r["trainer_ratio"] = r["trainer_buoyant_us"] / r["trainer_plain_us"]
    r["trainer"] = {"net": "mars_moon", "msteps": ms, "use_graph": True}
    r["clocks"] = clocks()
    line = json.dumps(r)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "k2d_buoyancy_time.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
