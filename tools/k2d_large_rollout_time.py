#!/usr/bin/env python
"""karman-2d roll-out with the corrector on large grids: LargeGridRollout at 256 x 128, B = 1 and 6, mars_moon -- one
JSON line, also written to profiles/k2d_large_rollout_time.json.  HIP events, 5 warm-up runs and `reps` (20) timed runs of a 20-step
roll-out per configuration, all in one process; us per step = run time / 20, median over the runs (min and max kept).

1. Default sphere (direct solve): the captured roll-out, the eager roll-out, and as the yardstick the composition the library offered
   before this class, timed the same way: ops.karman_step_large + ConvNet.predict on torch-assembled features + the torch to_staggered
   add (what LargeGridTrainer._solver_fwd and the correction of the training schedule compose).
2. Two cylinders (CG solve, eager): us per step and the iterations of every solve of one 20-step roll-out, cold and warm started, with
   the same yardstick composition (cold).
The clock the device held is read before and after (rocm-smi --showclocks, read only) and kept as text.
Usage: python tools/k2d_large_rollout_time.py [reps]"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "k2d_large_rollout_time.json")
Y, X, NSTEPS, WARMUP = 256, 128, 20, 5
TWO = ["sphere:50,50,10", "sphere:120,50,10"]
STD_V, STD_RE = (0.2, 0.2), 1.7e6


def clocks():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
        return [l.strip() for l in r.stdout.splitlines() if "sclk" in l or "mclk" in l]
    except Exception as e:
        return ["unavailable: %s" % e]


def setup(specs, B):
    import torch
    import sol_amd
    from sol_amd import fluid, karman, ops
    dom = fluid.Domain([Y, X], box=fluid.box[0:200, 0:100])
    active, inflow = karman.KarmanFlow(obstacles=None if specs is None else karman.parse_obstacles(specs)).scene_arrays(dom)
    bc = karman.velocity_bc_masks(Y, X)[0].reshape(Y + 1, X)
    mk = ops.SceneMasks(active, inflow, bc, bc, "cuda")
    net = sol_amd.model_mars_moon(cin=3, cout=2, seed=0)
    w = net.get_weights()                            # small last layer: an untrained corrector fed back through the solver (bench.py)
    w[22] = w[22] * 0.01
    net.set_weights(w)
    cfg = ops.karman_cfg(B, Y, X, dom.dx[1], masks=mk)
    gen = torch.Generator().manual_seed(1)
    d, vy, vx = (t.to("cuda") for t in (torch.rand(B, Y, X, generator=gen), 1.0 + 0.1 * torch.randn(B, Y + 1, X, generator=gen),
                                        0.1 * torch.randn(B, Y, X + 1, generator=gen)))
    re = torch.full((B,), 1.6e5, device="cuda")
    with torch.no_grad():
        d, vy, vx = ops.karman_step_large(d, vy, vx, re, cfg, mk)       # spun up in the scene
    return dom, mk, net, cfg, (d, vy, vx, re)


def timed(run, reps):
    """run(): one 20-step roll-out from the same start; us per step over `reps` runs after WARMUP runs"""
    import torch
    ts = []
    for it in range(WARMUP + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        if it >= WARMUP:
            ts.append(e0.elapsed_time(e1) * 1e3 / NSTEPS)
    return {"median_us_per_step": statistics.median(ts), "min_us_per_step": min(ts), "max_us_per_step": max(ts)}


def rollout_run(ro, st):
    import torch
    bufs = [torch.empty_like(t) for t in st[:3]]

    def run():
        for b, s in zip(bufs, st[:3]):
            b.copy_(s)
        ro.reset_guess()                             # every timed run starts cold, like the first frame of a roll-out
        return ro.run(*bufs, st[3], NSTEPS)
    return run


def composed_run(mk, net, cfg, st, B):
    """the parent's means: the solver step, the features and the correction in torch, the network through ConvNet.predict"""
    import torch
    from sol_amd import ops
    ws = torch.empty((ops.large_workspace_bytes(cfg, mk) + 3) // 4, dtype=torch.float32, device="cuda")
    fs = [1.0 / STD_V[0], 1.0 / STD_V[1], 1.0 / STD_RE]
    zplane = torch.zeros(B, Y, X, device="cuda")

    def run():
        d, vy, vx, re = st
        re_plane = (re * fs[2]).reshape(B, 1, 1).expand(B, Y, X)
        with torch.no_grad():
            for _ in range(NSTEPS):
                d, vy, vx = ops.karman_step_large(d, vy, vx, re, cfg, mk, ws)
                feat = torch.stack([vy[:, :Y] * fs[0], vx[:, :, :X] * fs[1], re_plane, zplane], dim=-1)
                out = net.predict(feat[..., :3])
                vy[:, :Y].add_(out[..., 0], alpha=STD_V[0])
                vx[:, :, :X].add_(out[..., 1], alpha=STD_V[1])
    return run


def main():
    sys.path.insert(0, ROOT)
    import torch
    import sol_amd
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    out = {"tool": "k2d_large_rollout_time", "reps": reps, "warmup": WARMUP, "steps_per_run": NSTEPS, "grid": [Y, X], "network": "mars_moon",
           "device": torch.cuda.get_device_name(0), "clocks_before": clocks(), "sphere_direct": {}, "two_cylinders_cg": {}}
    for B in (1, 6):
        dom, mk, net, cfg, st = setup(None, B)
        r = {}
        for name, graph in (("captured", True), ("eager", False)):
            ro = sol_amd.LargeGridRollout(net, mk, B, Y, X, dom.dx[1], STD_V, STD_RE, use_graph=graph)
            r[name] = timed(rollout_run(ro, st), reps)
        r["parent_composition_eager"] = timed(composed_run(mk, net, cfg, st, B), reps)
        out["sphere_direct"]["B%d" % B] = r
        dom, mk, net, cfg, st = setup(TWO, B)
        r = {}
        for name, warm in (("cold", False), ("warm", True)):
            ro = sol_amd.LargeGridRollout(net, mk, B, Y, X, dom.dx[1], STD_V, STD_RE, use_graph=False, cg_warm_start=warm)
            run = rollout_run(ro, st)
            r[name] = timed(run, reps)
            its = run()
            r[name]["iterations"] = its.tolist()
            r[name]["iterations_total"] = int(its.sum())
            r[name]["converged"] = bool(ro.solve_info["converged"].all())
        r["parent_composition_eager_cold"] = timed(composed_run(mk, net, cfg, st, B), reps)
        out["two_cylinders_cg"]["B%d" % B] = r
    out["clocks_after"] = clocks()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
