#!/usr/bin/env python
"""karman-3d pressure solves, direct vs preconditioned CG: one JSON line.

Per scene: the pressure solve alone (sol_karman3d_pressure_solve; right-hand side -div of a seeded unprojected velocity field) in
us with its CG iterations -- for CG also with the launch budget cut to the iterations it used (the price of the empty tail) --, the
forward step and the forward + adjoint step in us (HIP events around eager calls) with the iterations of both solves; and the SOL-16 training step (B = 1, replayed graph) on the cylinder with CG next
to the sphere with the direct solve.  Scenes: sphere 128 x 64 x 64 (direct and CG), cylinder 128 x 64 x 64 (CG; the direct blob is
refused), sphere 256 x 128 x 128 (CG, forward only).
Usage: python tools/k3d_pcg_time.py [reps]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import torch          # noqa: E402
import sol_oracle3d as o                        # noqa: E402  (the obstacle masks)
from sol_amd import karman3d as k3, synthetic   # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
DEV = "cuda"


def mask(Y, X, Z, obstacle):
    return o.geometry(Y, X, Z, obstacle=obstacle).active


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


def state(Y, X, Z, seed=1):
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    return (torch.rand(1, Y, X, Z, generator=gen).to(DEV), (1.0 + 0.1 * rn(1, Y + 1, X, Z)).to(DEV), (0.1 * rn(1, Y, X + 1, Z)).to(DEV),
            (0.1 * rn(1, Y, X, Z + 1)).to(DEV))


def scene_run(Y, X, Z, obstacle, solver, adjoint, reps):
    sc = k3.Scene3D(Y, X, Z, device=DEV, active=mask(Y, X, Z, obstacle), pressure_solver=solver)
    sim = k3.Karman3DFlow(sc, 1)
    re = synthetic.reynolds(1).float().to(DEV)
    with torch.no_grad():
        st = sim.step(*state(Y, X, Z), re)         # spun-up state for the step timings
        st = sim.step(*st, re)
    _, vy, vx, vz = state(Y, X, Z, 3)              # the solve's right-hand side: -div of an unprojected field
    rhs = (-((vy[:, 1:] - vy[:, :-1]) + (vx[:, :, 1:] - vx[:, :, :-1]) + (vz[..., 1:] - vz[..., :-1]))).contiguous()
    r = {"solver": sc.pressure_solver, "obstacle": obstacle, "grid": [Y, X, Z]}
    r["solve_us"] = timed(lambda: sim.pressure_solve(rhs), reps)
    if sc.pressure_solver == "cg":
        r["solve_iterations"] = int(sim.solve_info["iterations"][0])
        r["solve_converged"] = int(sim.solve_info["converged"][0])
        exact = k3.Karman3DFlow(sc, 1, cg_max_iter=max(1, r["solve_iterations"]))
        r["solve_us_budget_exact"] = timed(lambda: exact.pressure_solve(rhs), reps)
        del exact
    with torch.no_grad():
        r["step_fwd_us"] = timed(lambda: sim.step(*st, re), reps)
    if sc.pressure_solver == "cg":
        r["iterations_fwd"] = int(sim.solve_info["iterations"][0])
    if adjoint:
        w = [torch.randn(t.shape, generator=torch.Generator().manual_seed(7)).to(DEV) for t in st[1:]]

        def fb():
            v = [t.clone().requires_grad_(True) for t in st[1:]]
            out = sim.step(st[0], v[0], v[1], v[2], re)
            sum((a * b).sum() for a, b in zip(out[1:], w)).backward()
        r["step_fwd_bwd_us"] = timed(fb, reps)
        if sc.pressure_solver == "cg":
            r["iterations_bwd"] = int(sim.solve_info["iterations_bwd"][0])
            r["converged_bwd"] = int(sim.solve_info["converged_bwd"][0])
    return r


def train_ms(obstacle, steps=5):
    Y, X, Z, ms = 128, 64, 64, 16
    sc = k3.Scene3D(Y, X, Z, device=DEV, active=mask(Y, X, Z, obstacle))
    net = k3.MarsMoon3D(seed=3, device=DEV)
    w = net.get_weights()
    w[22] = w[22] * 0.01
    net.set_weights(w)
    tr = k3.Karman3DTrainer(net, sc, 1, ms, (0.2, 0.2, 0.2), synthetic.STD_RE, use_graph=True)
    re = synthetic.reynolds(1).float().to(DEV)
    with torch.no_grad():
        st = tr.sim.step(*state(Y, X, Z, 11), re)
        gs, gts = st, []
        for _ in range(ms):
            gs = tr.sim.step(*gs, re)
            gts.append(tuple(t.clone() for t in gs[1:]))
    tr.fwd_bwd(*st, re, gts)                        # warm-up + capture
    torch.cuda.synchronize()
    us = timed(lambda: tr.fwd_bwd(*st, re, gts), steps)
    r = {"solver": sc.pressure_solver, "obstacle": obstacle, "sol16_step_ms": us / 1e3, "loss": float(tr._loss)}
    if sc.pressure_solver == "cg":
        r["iterations_fwd_last"] = int(tr.sim.solve_info["iterations"][0])
        r["iterations_bwd_last"] = int(tr.sim.solve_info["iterations_bwd"][0])
    return r


def main():
    out = {"tool": "k3d_pcg_time", "reps": REPS, "cg_max_iter": k3.CG_MAX_ITER3D, "cg_rtol": 1e-6, "cg_atol": 1e-9}
    out["sphere128_direct"] = scene_run(128, 64, 64, "sphere", "direct", True, REPS)
    out["sphere128_cg"] = scene_run(128, 64, 64, "sphere", "cg", True, REPS)
    out["cylinder128_cg"] = scene_run(128, 64, 64, "cylinder", "auto", True, REPS)
    out["sphere256_cg"] = scene_run(256, 128, 128, "sphere", "auto", False, max(3, REPS // 4))
    out["train_sphere128_direct"] = train_ms("sphere")
    out["train_cylinder128_cg"] = train_ms("cylinder")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
