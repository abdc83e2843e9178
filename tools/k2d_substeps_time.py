#!/usr/bin/env python
"""karman-2d diffusion substeps: what n substeps cost, and whether fusing them pays: one JSON line, also written to
profiles/k2d_substeps_time.json.  256 x 128, B = 2, default sphere (direct solve), one process.

1. The forward step (ops.karman_step_saved) and the adjoint (ops.karman_step_large_bwd) for n in {1, 2, 4, 8, 16}, as ratios to the
   plain call (no keyword) of the same process.  HIP events around ROUND calls in a row; the plain call and the n-substep call ALTERNATE
   window by window; per form the median over the repetitions and the spread (max - min) / median.  n = 1 issues the plain call's
   launches: its ratio is the noise floor.
2. The pre-diffusion alone (ops.karman_diffuse_sub) of 7 and 15 substeps (n = 8, 16): fused (chunk = S_MAX = 8: one and two launches)
   against chained single-substep launches (chunk = 1), alternated the same way.
Usage: python tools/k2d_substeps_time.py [reps]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "k2d_substeps_time.json")
Y, X, B = 256, 128, 2
NS = (1, 2, 4, 8, 16)
ROUND = 20          # calls per timed window (a single step is tens of microseconds of kernels)


def window(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ROUND):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / ROUND


def spread(ts):
    m = statistics.median(ts)
    return {"median_us": m, "min_us": min(ts), "max_us": max(ts), "spread": (max(ts) - min(ts)) / m}


def alternated(forms, reps):
    """{name: spread} of callables timed in alternating windows (three warm-up rounds)"""
    ts = {k: [] for k in forms}
    for it in range(3 + reps):
        for k, fn in forms.items():
            t = window(fn)
            if it >= 3:
                ts[k].append(t)
    return {k: spread(v) for k, v in ts.items()}


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import numpy as np
    import torch
    import sol_oracle as o
    from sol_amd import ops
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    g = o.KarmanGeometry(Y, X)
    mk = ops.SceneMasks(g.active, g.inflow, g.bc_mask, g.bc_mask, "cuda")
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk)
    gen = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=gen)
    d, vy, vx = torch.rand(B, Y, X, generator=gen).cuda(), (1.0 + 0.1 * rn(B, Y + 1, X)).cuda(), (0.1 * rn(B, Y, X + 1)).cuda()
    re = torch.tensor([float(np.float32(X * X / a)) for a in (0.85, 0.6)], device="cuda")      # alpha beyond the single stencil's bound
    gy, gx = rn(B, Y + 1, X).cuda(), rn(B, Y, X + 1).cuda()
    ws_f = torch.empty((ops.large_workspace_bytes(cfg, mk) + 3) // 4, dtype=torch.float32, device="cuda")
    ws_b = torch.empty((ops.large_bwd_workspace_bytes(cfg, mk) + 3) // 4, dtype=torch.float32, device="cuda")
    out = {"tool": "k2d_substeps_time", "grid": [Y, X], "B": B, "solver": mk.pressure_solver, "reps": reps, "calls_per_window": ROUND,
           "device": torch.cuda.get_device_name(0), "s_max": ops.diffuse_sub_max(), "step": {}, "pre_diffusion": {}}
    with torch.no_grad():
        for n in NS:
            _, svy, svx = ops.karman_step_saved(d, vy, vx, re, cfg, mk, ws_f, diffusion_substeps=n)
            _, py, px = ops.karman_step_saved(d, vy, vx, re, cfg, mk, ws_f)
            r = alternated({"fwd_plain": lambda: ops.karman_step_saved(d, vy, vx, re, cfg, mk, ws_f),
                            "fwd_n": lambda: ops.karman_step_saved(d, vy, vx, re, cfg, mk, ws_f, diffusion_substeps=n),
                            "bwd_plain": lambda: ops.karman_step_large_bwd(py, px, re, gy, gx, cfg, mk, ws_b),
                            "bwd_n": lambda: ops.karman_step_large_bwd(svy, svx, re, gy, gx, cfg, mk, ws_b, diffusion_substeps=n)}, reps)
            r["ratio_fwd"] = r["fwd_n"]["median_us"] / r["fwd_plain"]["median_us"]
            r["ratio_bwd"] = r["bwd_n"]["median_us"] / r["bwd_plain"]["median_us"]
            out["step"]["n=%d" % n] = r
        for n in (8, 16):
            ws = torch.empty((ops.diffuse_sub_workspace_bytes(cfg, n, 1) + 3) // 4, dtype=torch.float32, device="cuda")
            a = ops.karman_diffuse_sub(vy, vx, re, cfg, n, workspace=ws)
            b = ops.karman_diffuse_sub(vy, vx, re, cfg, n, chunk=1, workspace=ws)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            r = alternated({"fused": lambda: ops.karman_diffuse_sub(vy, vx, re, cfg, n, workspace=ws),
                            "chained": lambda: ops.karman_diffuse_sub(vy, vx, re, cfg, n, chunk=1, workspace=ws)}, reps)
            r["ratio_fused_over_chained"] = r["fused"]["median_us"] / r["chained"]["median_us"]
            out["pre_diffusion"]["%d_substeps" % (n - 1)] = r
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
