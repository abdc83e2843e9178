#!/usr/bin/env python
"""karman-2d large-grid pressure solves on obstacles beyond one window: the scattered direct solve against the preconditioned CG
(DESIGN 4.5-4.7): one JSON line, also written to profiles/k2d_large_scattered_time.json.

At 256 x 128, scenes two cylinders in tandem and a plate across the channel, B = 1 and B = 6, in ONE process and with HIP events
around eager calls (one warm-up call, then `reps` calls in one event pair), alternating the two solvers per quantity:
  solve_us      the pressure solve alone (ops.pressure_solve_large; right-hand side -div of a seeded unprojected velocity field)
  step_fwd_us   the forward step (ops.karman_step_large on a spun-up state)
  adjoint_us    the adjoint (ops.karman_step_large_bwd on the saved state of that step, a seeded cotangent)
each with "cg" (the yardstick: what these scenes ran before; iterations reported) and with "direct_scattered"; the default sphere
with "direct" (the one-window solve) for the step and the adjoint; and the device time of each kernel of one scattered forward step
(sol_prof_begin / sol_prof_end: the dispatch packets' own timestamps), the capacitance kernel k_l_capacitance_sc among them.
Usage: python tools/k2d_large_scattered_time.py [reps]"""
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
SCENES = {"two_cylinders": ["sphere:50,50,10", "sphere:120,50,10"], "plate": ["box:70:73,20:80"]}


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


class Case:
    """one scene, one solver, one batch size: masks, cfg, workspaces, a spun-up state and its saved adjoint state"""

    def __init__(self, specs, solver, B):
        dom = fluid.Domain([Y, X], box=fluid.box[0:200, 0:100])
        flow = karman.KarmanFlow(obstacles=None if specs is None else karman.parse_obstacles(specs))
        active, inflow = flow.scene_arrays(dom)
        bc, _ = karman.velocity_bc_masks(Y, X)
        self.mk = mk = ops.SceneMasks(active, inflow, bc.reshape(Y + 1, X), bc.reshape(Y + 1, X), DEV, pressure_solver=solver)
        self.cfg = cfg = ops.karman_cfg(B, Y, X, dom.dx[1], masks=mk)
        self.B, self.re = B, torch.full((B,), 1.6e5, device=DEV)
        words = lambda n: torch.empty((n + 3) // 4, dtype=torch.float32, device=DEV)
        self.ws, self.wb = words(ops.large_workspace_bytes(cfg, mk)), words(ops.large_bwd_workspace_bytes(cfg, mk))
        with torch.no_grad():
            st = ops.karman_step_large(*state(B, 1), self.re, cfg, mk, self.ws)
            self.st = ops.karman_step_large(*st, self.re, cfg, mk, self.ws)
            _, self.svy, self.svx = ops.karman_step_large_saved(*self.st, self.re, cfg, mk, self.ws)
        gen = torch.Generator().manual_seed(3)
        self.w = [torch.randn(t.shape, generator=gen).to(DEV) for t in self.st[1:]]
        _, vy, vx = state(B, 3)
        self.rhs = (-((vy[:, 1:] - vy[:, :-1]) + (vx[:, :, 1:] - vx[:, :, :-1]))).contiguous()
        self.info = {"solve": {}, "step": {}, "adjoint": {}}

    def solve(self):
        return ops.pressure_solve_large(self.rhs, self.cfg, self.mk, self.ws, self.info["solve"])

    def step(self):
        with torch.no_grad():
            return ops.karman_step_large(*self.st, self.re, self.cfg, self.mk, self.ws, self.info["step"])

    def adjoint(self):
        return ops.karman_step_large_bwd(self.svy, self.svx, self.re, self.w[0], self.w[1], self.cfg, self.mk, self.wb, self.info["adjoint"])

    def iterations(self, what):
        i = self.info[what]
        k = "iterations_bwd" if what == "adjoint" else "iterations"
        return i[k].tolist() if k in i else None


def main():
    out = {"tool": "k2d_large_scattered_time", "reps": REPS, "grid": [Y, X], "cg_max_iter": 2000, "cg_rtol": 1e-6, "cg_atol": 1e-9,
           "device": torch.cuda.get_device_name(0), "unit": "us per call, HIP events around eager calls"}
    for B in (1, 6):
        for name, specs in SCENES.items():
            cases = {"cg": Case(specs, "cg", B), "direct_scattered": Case(specs, "direct_scattered", B)}
            hdr = cases["direct_scattered"].mk.direct_header
            r = {"B": B, "nS": int(hdr[5]), "SP": int(hdr[6]), "rows_x_cols": [int(hdr[3]), int(hdr[4])]}
            for what in ("solve", "step_fwd", "adjoint"):
                for solver, c in cases.items():
                    fn = {"solve": c.solve, "step_fwd": c.step, "adjoint": c.adjoint}[what]
                    r["%s_us_%s" % (what, solver)] = timed(fn, REPS)
                    its = c.iterations("step" if what == "step_fwd" else what)
                    if its is not None:
                        r["%s_iterations_cg" % what] = its
                r["%s_speedup" % what] = r["%s_us_cg" % what] / r["%s_us_direct_scattered" % what]
            # agreement of the two paths on the timed step (relative L2 of the velocity)
            a, b = cases["direct_scattered"].step(), cases["cg"].step()
            r["step_rel_l2_vs_cg"] = [float((x.double() - y.double()).norm() / y.double().norm()) for x, y in zip(a[1:], b[1:])]
            # per-kernel device time of ONE scattered forward step
            c = cases["direct_scattered"]
            torch.cuda.synchronize()
            with _lib.profile() as p:
                c.step()
                torch.cuda.synchronize()
            r["step_kernels_us"] = {k: {"calls": v[0], "total_us": v[1]} for k, v in sorted(p.kernels.items())}
            r["capacitance_kernel_us"] = p.kernels.get("k_l_capacitance_sc", (0, None))[1]
            out["%s_B%d" % (name, B)] = r
            del cases, c
        c = Case(None, "direct", B)
        out["sphere_direct_B%d" % B] = {"B": B, "step_fwd_us": timed(c.step, REPS), "adjoint_us": timed(c.adjoint, REPS)}
        del c
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "k2d_large_scattered_time.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
