#!/usr/bin/env python
"""karman-3d periodic spanwise boundaries: what a periodic z axis costs against the open step at 128 x 64 x 64, B = 1.  One
JSON line, also written to profiles/k3d_periodic_time.json.  One process; HIP events around ROUND calls in a row; the three scenes --
"open_cylinder" (Scene3D(pressure_solver="direct_extruded")), "periodic_cylinder" (the same obstacle, boundaries="periodic-z": the
like-for-like partner) and "periodic_empty" (no obstacle, the dense periodic blob with nS = 0) -- ALTERNATE window by window; per scene
the median over the repetitions and the spread (max - min) / median; the shader clock the box held is recorded before and after.

  fwd        the forward step (Karman3DFlow._fwd, saving the post-diffusion velocity)
  bwd_window the velocity adjoint with the LDS-window scatter (option k3d_adj_tile = 1)
  bwd_global the velocity adjoint with global atomics (k3d_adj_tile = 0)
  solve      the pressure solve alone -- a periodic blob's six transform products run with fp64 accumulators (sol_periodic_gemm) where an
             open blob at this grid runs the matrix-core transforms
  trainer    one captured Karman3DTrainer step (SOL-2)
"stencil": fwd minus solve, the launches of csrc/karman3d_periodic.hip against the open ones -- a difference of two windows: the solve-alone
call carries two copy launches and gaps of its own, so it understates the stencil of a scene whose solve is short (DESIGN 4.8 attributes by
launch from a kernel trace instead).  "ratio_*": a periodic median over
open_cylinder's; "noise": the largest spread of the three.  A ratio inside 1 +- noise is within what the windows resolve.
Usage: python tools/k3d_periodic_time.py [reps]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "k3d_periodic_time.json")
GRID, B = (128, 64, 64), 1
ROUND = 20
SCENES = ("open_cylinder", "periodic_cylinder", "periodic_empty")


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
    for k in SCENES[1:]:
        r["ratio_%s_over_open_cylinder" % k] = r[k]["median_us"] / r["open_cylinder"]["median_us"]
    r["noise"] = max(r[k]["spread"] for k in SCENES)
    r["within_noise"] = abs(r["ratio_periodic_cylinder_over_open_cylinder"] - 1.0) <= r["noise"]
    return r


def measure(reps):
    import numpy as np
    import torch
    import sol_oracle3d as o
    from sol_amd import _lib, karman3d as k3
    Y, X, Z = GRID
    act, inflow = k3.cylinder_arrays3d(Y, X, Z)
    sc = {"open_cylinder": k3.Scene3D(Y, X, Z, active=act, inflow=inflow, pressure_solver="direct_extruded"),
          "periodic_cylinder": k3.Scene3D(Y, X, Z, active=act, inflow=inflow, pressure_solver="direct_extruded", boundaries="periodic-z"),
          "periodic_empty": k3.Scene3D(Y, X, Z, active=np.ones(GRID), inflow=inflow, pressure_solver="direct", boundaries="periodic-z")}
    sims = {k: k3.Karman3DFlow(s, B) for k, s in sc.items()}
    gen = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=gen)
    d = torch.rand(B, Y, X, Z, generator=gen).cuda()
    vy, vx, vz = (1.0 + 0.1 * rn(B, Y + 1, X, Z)).cuda(), (0.1 * rn(B, Y, X + 1, Z)).cuda(), (0.1 * rn(B, Y, X, Z + 1)).cuda()
    vz[..., -1] = vz[..., 0]
    re = torch.tensor([o.RE_TRAIN[2]], dtype=torch.float32, device="cuda")
    gy, gx, gz, rhs = rn(B, Y + 1, X, Z).cuda(), rn(B, Y, X + 1, Z).cuda(), rn(B, Y, X, Z + 1).cuda(), rn(B, Y, X, Z).cuda()
    out = {"grid": list(GRID), "B": B, "header": {k: [int(v) for v in s.direct_header[:7]] for k, s in sc.items()}}
    with torch.no_grad():
        forms = {"fwd": {}, "bwd_window": {}, "bwd_global": {}, "solve": {}}
        for k, sim in sims.items():
            saved = [torch.empty_like(t) for t in (vy, vx, vz)]
            sim._fwd(d, vy, vx, vz, re, saved=saved)
            forms["fwd"][k] = lambda sim=sim, sv=saved: sim._fwd(d, vy, vx, vz, re, saved=sv)
            forms["bwd_window"][k] = forms["bwd_global"][k] = lambda sim=sim, sv=saved: sim._bwd(sv, re, gy, gx, gz)
            forms["solve"][k] = lambda sim=sim: sim.pressure_solve(rhs)
        for name, f in forms.items():
            old = _lib.get_option("k3d_adj_tile")
            _lib.set_option("k3d_adj_tile", 0 if name == "bwd_global" else 1)
            try:
                out[name] = ratios(alternated(f, reps))
            finally:
                _lib.set_option("k3d_adj_tile", old)
    out["stencil_us"] = {k: out["fwd"][k]["median_us"] - out["solve"][k]["median_us"] for k in SCENES}
    ms = 2
    gts = [(vy, vx, vz)] * ms
    tr = {}
    for k, s in sc.items():
        net = k3.MarsMoon3D(device="cuda")
        w = net.get_weights()
        w[22] = w[22] * 0.05
        net.set_weights(w)
        tr[k] = k3.Karman3DTrainer(net, s, B, ms, (0.2, 0.25, 0.3), o.STD_RE, use_graph=True)
        tr[k].fwd_bwd(d, vy, vx, vz, re, gts)
        assert tr[k]._graph is not None
    out["trainer_step"] = dict(ratios(alternated({k: (lambda t=t: t.fwd_bwd(d, vy, vx, vz, re, gts)) for k, t in tr.items()}, reps, rounds=3)), msteps=ms)
    return out


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import torch
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    out = {"tool": "k3d_periodic_time", "reps": reps, "calls_per_window": ROUND, "device": torch.cuda.get_device_name(0), "clocks_before": clocks()}
    out.update(measure(reps))
    out["clocks"] = clocks()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
