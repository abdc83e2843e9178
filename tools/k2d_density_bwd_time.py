#!/usr/bin/env python
"""karman-2d density adjoint: what it adds to a backward pass, one JSON line, also written to
profiles/k2d_density_bwd_time.json.

At 256 x 128, B = 2, the default sphere (direct solve), in ONE process and on a spun-up state: the density adjoint alone
(ops.karman_density_bwd on the saved state with a fixed random cotangent, written and added onto a velocity gradient) with both scatter
forms (LDS tile window, option k2d_dens_adj_tile = 1, and global atomics only), and the velocity adjoint alone
(ops.karman_step_large_bwd, the code path that exists without the density gradient) -- HIP events around eager calls; and the density
adjoint's kernel split (sol_prof_begin / sol_prof_end: device time per kernel, us per call).  No threshold: the file records what was
measured, on whatever clock the box held; compare the density adjoint to the velocity adjoint of the same file and to nothing else.
Usage: python tools/k2d_density_bwd_time.py [reps]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch          # noqa: E402
from sol_amd import _lib, fluid, karman, ops   # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
DEV = "cuda"
Y, X, B = 256, 128, 2


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


def main():
    dom = fluid.Domain([Y, X], box=fluid.box[0:200, 0:100])
    flow = karman.KarmanFlow()
    active, inflow = flow.scene_arrays(dom)
    bc, _ = karman.velocity_bc_masks(Y, X)
    mk = ops.SceneMasks(active, inflow, bc.reshape(Y + 1, X), bc.reshape(Y + 1, X), DEV)
    cfg = ops.karman_cfg(B, Y, X, dom.dx[1], masks=mk)
    re = torch.full((B,), 1.6e5, device=DEV)
    gen = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=gen)
    st = (torch.rand(B, Y, X, generator=gen).to(DEV), (1.0 + 0.1 * rn(B, Y + 1, X)).to(DEV), (0.1 * rn(B, Y, X + 1)).to(DEV))
    ws = torch.empty((ops.large_workspace_bytes(cfg, mk) + 3) // 4, dtype=torch.float32, device=DEV)
    with torch.no_grad():
        st = ops.karman_step_large(*st, re, cfg, mk, ws)                  # spun-up state
        st = ops.karman_step_large(*st, re, cfg, mk, ws)
        _, svy, svx = ops.karman_step_large_saved(*st, re, cfg, mk, ws)
    gen = torch.Generator().manual_seed(3)
    wd = torch.randn(B, Y, X, generator=gen).to(DEV)
    wy, wx = torch.randn(B, Y + 1, X, generator=gen).to(DEV), torch.randn(B, Y, X + 1, generator=gen).to(DEV)
    wsd = torch.empty((ops.density_bwd_workspace_bytes(cfg) + 3) // 4, dtype=torch.float32, device=DEV)
    wsb = torch.empty((ops.large_bwd_workspace_bytes(cfg, mk) + 3) // 4, dtype=torch.float32, device=DEV)
    gy, gx = torch.zeros_like(svy), torch.zeros_like(svx)
    dens = lambda: ops.karman_density_bwd(st[0], svy, svx, re, wd, cfg, mk, workspace=wsd)
    dens_acc = lambda: ops.karman_density_bwd(st[0], svy, svx, re, wd, cfg, mk, gy, gx, workspace=wsd)
    vel = lambda: ops.karman_step_large_bwd(svy, svx, re, wy, wx, cfg, mk, wsb)
    r = {"tool": "k2d_density_bwd_time", "reps": REPS, "device": torch.cuda.get_device_name(0), "scene": flow.scene()["obstacles"],
         "solver": mk.pressure_solver, "grid": [Y, X], "B": B}
    r["velocity_bwd_us"] = timed(vel, REPS)
    r["density_bwd_us"] = timed(dens, REPS)
    r["density_bwd_accumulate_us"] = timed(dens_acc, REPS)
    _lib.set_option("k2d_dens_adj_tile", 0)
    try:
        r["density_bwd_global_atomics_us"] = timed(dens, REPS)
    finally:
        _lib.set_option("k2d_dens_adj_tile", 1)
    r["velocity_bwd_again_us"] = timed(vel, REPS)                          # the yardstick once more: did the box move meanwhile?
    r["density_over_velocity"] = r["density_bwd_us"] / r["velocity_bwd_us"]
    for key, fn in (("density_kernels_us", dens), ("velocity_kernels_us", vel)):
        torch.cuda.synchronize()
        preps = min(REPS, 50)                                              # (every launch carries two events)
        with _lib.profile() as p:
            for _ in range(preps):
                fn()
        r[key] = {k: round(v[1] / preps, 3) for k, v in sorted(p.kernels.items(), key=lambda kv: -kv[1][1])}
        r[key.replace("_us", "_launches")] = int(sum(v[0] for v in p.kernels.values()) // preps)
    line = json.dumps(r)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "k2d_density_bwd_time.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
