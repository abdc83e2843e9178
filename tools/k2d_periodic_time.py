#!/usr/bin/env python
"""karman-2d periodic boundaries: what a periodic x axis costs against the open step on the same grid.  One JSON line,
also written to profiles/k2d_periodic_time.json.  256 x 128 at B = 2 and 128 x 64 at B = 6 (multi_launch), no obstacle, one process; HIP
events around ROUND calls in a row; the two forms -- boundaries "open" and ("open", "periodic") -- ALTERNATE window by window; per form
the median over the repetitions and the spread (max - min) / median; the shader clock the box held is recorded before and after.

Per grid:
  fwd       the forward step (ops.karman_step_saved)
  bwd       the velocity adjoint (ops.karman_step_large_bwd)
  solve     the pressure solve alone (ops.karman_pressure_solve_large) -- the periodic scene's products accumulate in fp64 (k_p_gemm)
  trainer   one LargeGridTrainer step (mars_moon, msteps = 2, captured)
The open scene has no obstacle either, so it has no direct blob and runs the CG solve: the open forms are therefore ALSO timed on the
default sphere (direct solve, "open_sphere"), and the periodic forms twice: empty ("periodic": the box blob, nS = 0) and with the same
sphere ("periodic_sphere": the same one-window capacitance part) -- the like-for-like partner.  "ratio_*": a periodic median over
open_sphere's; "noise": the largest spread of the three.  A ratio inside 1 +- noise is within what the windows resolve.
Usage: python tools/k2d_periodic_time.py [reps]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "k2d_periodic_time.json")
GRIDS = ((256, 128, 2, False), (128, 64, 6, True))
ROUND = 20


def window(fn, rounds=ROUND):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(rounds):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / rounds


def spread(ts):
    m = statistics.median(ts)
    return {"median_us": m, "min_us": min(ts), "max_us": max(ts), "spread": (max(ts) - min(ts)) / m}


def alternated(forms, reps, rounds=ROUND):
    ts = {k: [] for k in forms}
    for it in range(3 + reps):
        for k, fn in forms.items():
            t = window(fn, rounds)
            if it >= 3:
                ts[k].append(t)
    return {k: spread(v) for k, v in ts.items()}


def clocks():
    """rocm-smi's clock lines (read only): the clock the box held"""
    import subprocess
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
        return [l.strip() for l in r.stdout.splitlines() if "sclk" in l or "mclk" in l]
    except Exception as e:
        return ["unavailable: %s" % e]


def ratios(r):
    r["ratio_periodic_over_open_sphere"] = r["periodic"]["median_us"] / r["open_sphere"]["median_us"]
    r["ratio_periodic_sphere_over_open_sphere"] = r["periodic_sphere"]["median_us"] / r["open_sphere"]["median_us"]      # the same obstacle on both sides
    r["noise"] = max(r[k]["spread"] for k in ("periodic", "periodic_sphere", "open_sphere"))
    r["within_noise"] = abs(r["ratio_periodic_sphere_over_open_sphere"] - 1.0) <= r["noise"]
    return r


def measure(Y, X, B, ml, reps):
    import numpy as np
    import torch
    import sol_oracle as o
    import sol_amd
    from sol_amd import ops, schedule2d
    g = o.geometry(Y, X)
    empty = np.ones((Y, X))
    mk = {"open_sphere": ops.SceneMasks(g.active, g.inflow, g.bc_mask, g.bc_mask, "cuda", multi_launch=ml),
          "periodic": ops.SceneMasks(empty, g.inflow, g.bc_mask, g.bc_mask, "cuda", multi_launch=ml, boundaries=("open", "periodic")),
          "periodic_sphere": ops.SceneMasks(g.active, g.inflow, g.bc_mask, g.bc_mask, "cuda", multi_launch=ml, boundaries=("open", "periodic"))}
    assert all(m.pressure_solver == "direct" for m in mk.values())
    cfg = {k: ops.karman_cfg(B, Y, X, g.dx, masks=m) for k, m in mk.items()}
    gen = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=gen)
    d, vy, vx = torch.rand(B, Y, X, generator=gen).cuda(), (1.0 + 0.1 * rn(B, Y + 1, X)).cuda(), (0.1 * rn(B, Y, X + 1)).cuda()
    vx[:, :, -1] = vx[:, :, 0]
    re = torch.tensor([o.RE_TRAIN[i % 6] for i in range(B)], dtype=torch.float32, device="cuda")
    gy, gx, rhs = rn(B, Y + 1, X).cuda(), rn(B, Y, X + 1).cuda(), rn(B, Y, X).cuda()
    ws = lambda n: torch.empty((int(n) + 3) // 4, dtype=torch.float32, device="cuda")
    out = {"grid": [Y, X], "B": B, "multi_launch": ml, "nS": {k: int(m.direct_header[5]) for k, m in mk.items()}}
    with torch.no_grad():
        forms = {"fwd": {}, "bwd": {}, "solve": {}}
        for k, m in mk.items():
            c = cfg[k]
            ws_s, ws_f, ws_b = ws(ops.large_workspace_bytes(c, m)), ws(ops.large_workspace_bytes(c, m, saved=True)), ws(ops.large_bwd_workspace_bytes(c, m))
            _, sy, sx = ops.karman_step_saved(d, vy, vx, re, c, m, ws_f)
            forms["fwd"][k] = lambda c=c, m=m, w=ws_f: ops.karman_step_saved(d, vy, vx, re, c, m, w)
            forms["bwd"][k] = lambda c=c, m=m, w=ws_b, sy=sy, sx=sx: ops.karman_step_large_bwd(sy, sx, re, gy, gx, c, m, w)
            forms["solve"][k] = lambda c=c, m=m, w=ws_s: ops.karman_pressure_solve_large(rhs, c, m, w)
        for name, f in forms.items():
            out[name] = ratios(alternated(f, reps))
    ms = 2
    net = lambda: sol_amd.model_mars_moon(cin=3, cout=2, seed=0)
    args = (d, vy, vx, re, torch.stack([vy] * ms).contiguous(), torch.stack([vx] * ms).contiguous())
    kw = dict(multi_launch=ml, any_width=schedule2d.row_pitch(Y, X) != X)
    tr = {"open_sphere": sol_amd.LargeGridTrainer(net(), B, Y, X, ms, (0.2, 0.2), o.STD_RE, masks=mk["open_sphere"], **kw),
          "periodic": sol_amd.LargeGridTrainer(net(), B, Y, X, ms, (0.2, 0.2), o.STD_RE, masks=mk["periodic"], obstacles=[], **kw),
          "periodic_sphere": sol_amd.LargeGridTrainer(net(), B, Y, X, ms, (0.2, 0.2), o.STD_RE, masks=mk["periodic_sphere"], **kw)}
    for t in tr.values():
        t.fwd_bwd(*args)
        assert t._graph is not None
    out["trainer_step"] = dict(ratios(alternated({k: (lambda t=t: t.fwd_bwd(*args)) for k, t in tr.items()}, reps, rounds=5)), msteps=ms)
    return out


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import torch
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    out = {"tool": "k2d_periodic_time", "reps": reps, "calls_per_window": ROUND, "device": torch.cuda.get_device_name(0),
           "clocks_before": clocks(), "grids": []}
    for Y, X, B, ml in GRIDS:
        out["grids"].append(measure(Y, X, B, ml, reps))
    out["clocks"] = clocks()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
