#!/usr/bin/env python
"""karman-2d large-grid step: forward and adjoint, direct and CG: one JSON line, also written to
profiles/k2d_large_bwd_time.json.

At 256 x 128, B = 1 and 6, for the default sphere (direct solve) and two cylinders in tandem (CG solve), all in ONE process and on a
spun-up state: the plain forward step in us (ops.karman_step_large under no_grad: the launch sequence of the data-generation path,
the yardstick), the forward step that keeps the post-diffusion velocity (KarmanStepFn.forward, ops.karman_step_saved), the adjoint alone
(ops.karman_step_large_bwd on the saved state with a fixed random cotangent), with both scatter forms (LDS tile window, option
k2d_adj_tile = 1, and global atomics only), HIP events around eager calls; the CG iterations of both solves; and the adjoint's
kernel split (sol_prof_begin / sol_prof_end: per-kernel device time summed over the repetitions, us per call of the adjoint).
Usage: python tools/k2d_large_bwd_time.py [reps]"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch          # noqa: E402
from sol_amd import _lib, fluid, karman, ops   # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
DEV = "cuda"
Y, X = 256, 128
SCENES = {"sphere_direct": None, "two_cylinders_cg": ["sphere:50,50,10", "sphere:120,50,10"]}


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


def state(B, seed):
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    return (torch.rand(B, Y, X, generator=gen).to(DEV), (1.0 + 0.1 * rn(B, Y + 1, X)).to(DEV), (0.1 * rn(B, Y, X + 1)).to(DEV))


def scene_run(specs, B, reps):
    dom = fluid.Domain([Y, X], box=fluid.box[0:200, 0:100])
    flow = karman.KarmanFlow(obstacles=None if specs is None else karman.parse_obstacles(specs))
    active, inflow = flow.scene_arrays(dom)
    bc, _ = karman.velocity_bc_masks(Y, X)
    mk = ops.SceneMasks(active, inflow, bc.reshape(Y + 1, X), bc.reshape(Y + 1, X), DEV)
    cfg = ops.karman_cfg(B, Y, X, dom.dx[1], masks=mk)
    re = torch.full((B,), 1.6e5, device=DEV)
    ws = torch.empty((ops.large_workspace_bytes(cfg, mk) + 3) // 4, dtype=torch.float32, device=DEV)
    with torch.no_grad():
        st = ops.karman_step_large(*state(B, 1), re, cfg, mk, ws)         # spun-up state
        st = ops.karman_step_large(*st, re, cfg, mk, ws)
    r = {"scene": flow.scene()["obstacles"], "solver": mk.pressure_solver, "grid": [Y, X], "B": B}
    info = {}
    with torch.no_grad():
        r["step_fwd_us"] = timed(lambda: ops.karman_step_large(*st, re, cfg, mk, ws, info), reps)
    vy, vx = st[1].clone().requires_grad_(True), st[2].clone().requires_grad_(True)
    r["step_fwd_saved_us"] = timed(lambda: ops.karman_step_large(st[0], vy, vx, re, cfg, mk, ws, info), reps)
    out = ops.karman_step_large(st[0], vy, vx, re, cfg, mk, ws, info)
    svy, svx, _ = out[1].grad_fn.saved_tensors
    gen = torch.Generator().manual_seed(3)
    wy, wx = torch.randn(B, Y + 1, X, generator=gen).to(DEV), torch.randn(B, Y, X + 1, generator=gen).to(DEV)
    nb = _lib.load().sol_karman_step_bwd_large_workspace_bytes(ctypes.byref(cfg))
    wsb = torch.empty((nb + 3) // 4, dtype=torch.float32, device=DEV)
    binfo = {}
    bwd = lambda: ops.karman_step_large_bwd(svy, svx, re, wy, wx, cfg, mk, wsb, binfo)
    r["step_bwd_us"] = timed(bwd, reps)
    _lib.set_option("k2d_adj_tile", 0)
    try:
        r["step_bwd_global_atomics_us"] = timed(bwd, reps)
    finally:
        _lib.set_option("k2d_adj_tile", 1)
    r["bwd_over_fwd"] = r["step_bwd_us"] / r["step_fwd_us"]
    if mk.pressure_solver == "cg":
        r["fwd_iterations"], r["fwd_converged"] = info["iterations"].tolist(), info["converged"].tolist()
        r["bwd_iterations"], r["bwd_converged"] = binfo["iterations_bwd"].tolist(), binfo["converged_bwd"].tolist()
    # kernel split of the adjoint (device time per kernel, us per adjoint call) and of the plain forward step
    for key, fn in (("bwd_kernels_us", bwd), ("fwd_kernels_us", lambda: ops.karman_step_large(*st, re, cfg, mk, ws))):
        torch.cuda.synchronize()
        preps = reps if mk.pressure_solver == "direct" else min(reps, 3)      # (every launch carries two events: ~1 500 launches per CG solve)
        with torch.no_grad(), _lib.profile() as p:
            for _ in range(preps):
                fn()
        r[key] = {k: round(v[1] / preps, 3) for k, v in sorted(p.kernels.items(), key=lambda kv: -kv[1][1])}
        r[key.replace("_us", "_launches")] = int(sum(v[0] for v in p.kernels.values()) // preps)
    return r


def main():
    out = {"tool": "k2d_large_bwd_time", "reps": REPS, "cg_max_iter": 2000, "cg_rtol": 1e-6, "cg_atol": 1e-9,
           "device": torch.cuda.get_device_name(0)}
    for name, specs in SCENES.items():
        for B in (1, 6):
            out["%s_B%d" % (name, B)] = scene_run(specs, B, REPS)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "k2d_large_bwd_time.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
