#!/usr/bin/env python
"""karman-2d MacCormack advection: what advection="mac_cormack" costs: one JSON line, also written to
profiles/k2d_maccormack_time.json.  256 x 128, B = 2, default sphere (direct solve), one process.

1. The forward step (ops.karman_step_saved), the velocity adjoint (ops.karman_step_large_bwd) and the velocity + density adjoint
   (+ ops.karman_density_bwd) under mac_cormack as ratios to the plain calls (no keyword) of the same process.  HIP events around ROUND
   calls in a row; the forms ALTERNATE window by window; per form the median over the repetitions and the spread (max - min) / median.
   "semi_lagrangian" spelled out issues the plain call's launches: its ratio is the noise floor, and the plain forms' spread is what a
   comparison with another build of the library has to stay within.
2. The stage alone (ops.karman_advect): tiled (option k2d_mc_tile = 1, one launch) against two launches (0), and k_l_advect.
3. A LargeGridTrainer step (mars_moon, B = 1, two unrolled steps, captured) with and without.
Usage: python tools/k2d_maccormack_time.py [reps]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "k2d_maccormack_time.json")
Y, X, B = 256, 128, 2
ROUND = 20          # calls per timed window (a single step is tens of microseconds of kernels)


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
    """{name: spread} of callables timed in alternating windows (three warm-up rounds)"""
    ts = {k: [] for k in forms}
    for it in range(3 + reps):
        for k, fn in forms.items():
            t = window(fn, rounds)
            if it >= 3:
                ts[k].append(t)
    return {k: spread(v) for k, v in ts.items()}


def clocks():
    """rocm-smi's clock lines (read only), as tools/k2d_buoyancy_time.py records them: the clock the box held"""
    import subprocess
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
        return [l.strip() for l in r.stdout.splitlines() if "sclk" in l or "mclk" in l]
    except Exception as e:
        return ["unavailable: %s" % e]


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import torch
    import sol_oracle as o
    import sol_amd
    from sol_amd import _lib, ops
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    MC, SL = dict(advection="mac_cormack"), dict(advection="semi_lagrangian")
    g = o.KarmanGeometry(Y, X)
    mk = ops.SceneMasks(g.active, g.inflow, g.bc_mask, g.bc_mask, "cuda")
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk)
    gen = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=gen)
    d, vy, vx = torch.rand(B, Y, X, generator=gen).cuda(), (1.0 + 0.1 * rn(B, Y + 1, X)).cuda(), (0.1 * rn(B, Y, X + 1)).cuda()
    re = torch.tensor([o.RE_TRAIN[0], o.RE_TRAIN[1]], dtype=torch.float32, device="cuda")
    gd, gy, gx = rn(B, Y, X).cuda(), rn(B, Y + 1, X).cuda(), rn(B, Y, X + 1).cuda()
    ws = lambda n: torch.empty((int(n) + 3) // 4, dtype=torch.float32, device="cuda")
    ph = ops.StepPhysics.of(**MC)
    ws_f, ws_b, ws_d = ws(ops.large_workspace_bytes(cfg, mk, ph, saved=True)), ws(ops.large_bwd_workspace_bytes(cfg, mk, ph)), ws(ops.density_bwd_workspace_bytes(cfg, ph))
    out = {"tool": "k2d_maccormack_time", "grid": [Y, X], "B": B, "solver": mk.pressure_solver, "reps": reps, "calls_per_window": ROUND,
           "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        _, sy, sx = ops.karman_step_saved(d, vy, vx, re, cfg, mk, ws_f, **MC)
        _, py, px = ops.karman_step_saved(d, vy, vx, re, cfg, mk, ws_f)

        def both(svy, svx, kw):
            oy, ox = ops.karman_step_large_bwd(svy, svx, re, gy, gx, cfg, mk, ws_b, **kw)
            return ops.karman_density_bwd(d, svy, svx, re, gd, cfg, mk, oy, ox, ws_d, **kw)

        r = alternated({"fwd_plain": lambda: ops.karman_step_saved(d, vy, vx, re, cfg, mk, ws_f),
                        "fwd_sl": lambda: ops.karman_step_saved(d, vy, vx, re, cfg, mk, ws_f, **SL),
                        "fwd_mc": lambda: ops.karman_step_saved(d, vy, vx, re, cfg, mk, ws_f, **MC),
                        "bwd_plain": lambda: ops.karman_step_large_bwd(py, px, re, gy, gx, cfg, mk, ws_b),
                        "bwd_sl": lambda: ops.karman_step_large_bwd(py, px, re, gy, gx, cfg, mk, ws_b, **SL),
                        "bwd_mc": lambda: ops.karman_step_large_bwd(sy, sx, re, gy, gx, cfg, mk, ws_b, **MC),
                        "bwd_dens_plain": lambda: both(py, px, {}),
                        "bwd_dens_mc": lambda: both(sy, sx, MC)}, reps)
        for k in ("fwd", "bwd"):
            r["ratio_%s_mc" % k] = r[k + "_mc"]["median_us"] / r[k + "_plain"]["median_us"]
            r["ratio_%s_sl" % k] = r[k + "_sl"]["median_us"] / r[k + "_plain"]["median_us"]
        r["ratio_bwd_dens_mc"] = r["bwd_dens_mc"]["median_us"] / r["bwd_dens_plain"]["median_us"]
        out["step"] = r
        # the stage alone: tiled against two launches
        act, infl = mk.active, mk.inflow
        ws_a = ws(ops.large_workspace_bytes(cfg, mk, ph))        # (holds the stage's part and more)

        def two():
            _lib.set_option("k2d_mc_tile", 0)
            try:
                return ops.karman_advect(d, py, px, cfg, act, infl, workspace=ws_a, **MC)
            finally:
                _lib.set_option("k2d_mc_tile", 1)

        a, b = ops.karman_advect(d, py, px, cfg, act, infl, workspace=ws_a, **MC), two()
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        r = alternated({"tiled": lambda: ops.karman_advect(d, py, px, cfg, act, infl, workspace=ws_a, **MC), "two_launch": two,
                        "semi_lagrangian": lambda: ops.karman_advect(d, py, px, cfg, act, infl)}, reps)
        r["ratio_tiled_over_two_launch"] = r["tiled"]["median_us"] / r["two_launch"]["median_us"]
        out["stage"] = r
    # a LargeGridTrainer step with and without
    ms = 2
    net = lambda: sol_amd.model_mars_moon(cin=3, cout=2, seed=0)
    args = (d[:1].contiguous(), vy[:1].contiguous(), vx[:1].contiguous(), re[:1].contiguous(),
            torch.stack([vy[:1]] * ms).contiguous(), torch.stack([vx[:1]] * ms).contiguous())
    tr = {k: sol_amd.LargeGridTrainer(net(), 1, Y, X, ms, (0.2, 0.2), o.STD_RE, **kw) for k, kw in (("plain", {}), ("mac_cormack", MC))}
    r = alternated({k: (lambda t=t: t.fwd_bwd(*args)) for k, t in tr.items()}, reps, rounds=5)
    r["ratio"] = r["mac_cormack"]["median_us"] / r["plain"]["median_us"]
    out["trainer_step"] = dict(r, msteps=ms, B=1)
    out["clocks"] = clocks()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
