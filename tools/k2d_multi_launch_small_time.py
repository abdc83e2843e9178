#!/usr/bin/env python
"""karman-2d multi_launch on the one-workgroup grids: what the multi-launch path costs where the fused one-workgroup
kernels would serve, and whether the one-launch direct solve (option k2d_solve_one_wg, csrc/karman_solve_small.hip) beats the chain of
GEMM launches.  One JSON line, also written to profiles/k2d_multi_launch_small_time.json.  64 x 32 at B = 3 and 128 x 64 at B = 6,
default sphere, one process; HIP events around ROUND calls in a row; the forms ALTERNATE window by window; per form the median over the
repetitions and the spread (max - min) / median; the shader clock the box held is recorded.

Per grid:
  solve         the pressure solve alone (ops.karman_pressure_solve_large on multi_launch masks): chain (option 0) against one launch (1)
  fwd / bwd     the forward step (ops.karman_step_saved) and the velocity adjoint: fused one-workgroup (default masks: sol_karman_step_fwd /
                sol_karman_step_bwd), multi-launch with the chain, multi-launch with the one-launch solve
  trainer       a plain-physics SOL-4 training step, captured: SolTrainer against LargeGridTrainer(multi_launch=True) with the chain and
                with the one-launch solve -- the price of the options on these grids
"one_launch_wins": the one-launch solve's median is below the chain's at BOTH grids; the default of k2d_solve_one_wg follows it.
Usage: python tools/k2d_multi_launch_small_time.py [reps]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "k2d_multi_launch_small_time.json")
GRIDS = ((64, 32, 3), (128, 64, 6))
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
    """{name: spread} of callables timed in alternating windows (three warm-up rounds)"""
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


def with_option(value, fn):
    from sol_amd import _lib

    def run():
        old = _lib.get_option("k2d_solve_one_wg")
        _lib.set_option("k2d_solve_one_wg", value)
        try:
            return fn()
        finally:
            _lib.set_option("k2d_solve_one_wg", old)
    return run


def measure(Y, X, B, reps):
    import torch
    import sol_oracle as o
    import sol_amd
    from sol_amd import _lib, ops
    g = o.geometry(Y, X)
    fused = ops.SceneMasks(g.active, g.inflow, g.bc_mask, g.bc_mask, "cuda")
    multi = ops.SceneMasks(g.active, g.inflow, g.bc_mask, g.bc_mask, "cuda", multi_launch=True)
    assert not fused.large and multi.large and fused.pressure_solver == multi.pressure_solver == "direct"
    cf, cm = ops.karman_cfg(B, Y, X, g.dx, masks=fused), ops.karman_cfg(B, Y, X, g.dx, masks=multi)
    gen = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=gen)
    d, vy, vx = torch.rand(B, Y, X, generator=gen).cuda(), (1.0 + 0.1 * rn(B, Y + 1, X)).cuda(), (0.1 * rn(B, Y, X + 1)).cuda()
    re = torch.tensor([o.RE_TRAIN[i % 6] for i in range(B)], dtype=torch.float32, device="cuda")
    gy, gx, rhs = rn(B, Y + 1, X).cuda(), rn(B, Y, X + 1).cuda(), rn(B, Y, X).cuda()
    ws = lambda n: torch.empty((int(n) + 3) // 4, dtype=torch.float32, device="cuda")
    ws_s, ws_f, ws_b = ws(ops.large_workspace_bytes(cm, multi)), ws(ops.large_workspace_bytes(cm, multi, saved=True)), ws(ops.large_bwd_workspace_bytes(cm, multi))
    out = {"grid": [Y, X], "B": B, "window": int(multi.direct_header[7]), "SP": int(multi.direct_header[6])}
    with torch.no_grad():
        solve = lambda: ops.karman_pressure_solve_large(rhs, cm, multi, ws_s)
        r = alternated({"chain": with_option(0, solve), "one_launch": with_option(1, solve)}, reps)
        r["ratio_one_launch_over_chain"] = r["one_launch"]["median_us"] / r["chain"]["median_us"]
        out["solve"] = r
        _, sy, sx = ops.karman_step_saved(d, vy, vx, re, cf, fused)
        fwd_m = lambda: ops.karman_step_saved(d, vy, vx, re, cm, multi, ws_f)
        bwd_m = lambda: ops.karman_step_large_bwd(sy, sx, re, gy, gx, cm, multi, ws_b)
        r = alternated({"fwd_fused": lambda: ops.karman_step_saved(d, vy, vx, re, cf, fused),
                        "fwd_multi_chain": with_option(0, fwd_m), "fwd_multi_one_launch": with_option(1, fwd_m),
                        "bwd_fused": lambda: ops._step_bwd(sy, sx, re, gy, gx, cf, fused, None),
                        "bwd_multi_chain": with_option(0, bwd_m), "bwd_multi_one_launch": with_option(1, bwd_m)}, reps)
        for k in ("fwd", "bwd"):
            for form in ("chain", "one_launch"):
                r["ratio_%s_multi_%s_over_fused" % (k, form)] = r["%s_multi_%s" % (k, form)]["median_us"] / r[k + "_fused"]["median_us"]
        out["step"] = r
    # a plain-physics SOL-4 training step, captured (the option is read when the graph is captured)
    ms = 4
    net = lambda: sol_amd.model_mars_moon(cin=3, cout=2, seed=0)
    args = (d, vy, vx, re, torch.stack([vy] * ms).contiguous(), torch.stack([vx] * ms).contiguous())
    forms = {"sol_trainer": sol_amd.SolTrainer(net(), fused, B, Y, X, ms, g.dx, (0.2, 0.2), o.STD_RE)}
    for name, v in (("large_grid_chain", 0), ("large_grid_one_launch", 1)):
        _lib.set_option("k2d_solve_one_wg", v)
        tr = sol_amd.LargeGridTrainer(net(), B, Y, X, ms, (0.2, 0.2), o.STD_RE, multi_launch=True)
        tr.fwd_bwd(*args)
        assert tr._graph is not None
        forms[name] = tr
    r = alternated({k: (lambda t=t: t.fwd_bwd(*args)) for k, t in forms.items()}, reps, rounds=5)
    for name in ("large_grid_chain", "large_grid_one_launch"):
        r["ratio_%s_over_sol_trainer" % name] = r[name]["median_us"] / r["sol_trainer"]["median_us"]
    out["trainer_step"] = dict(r, msteps=ms)
    return out


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import torch
    from sol_amd import _lib
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    default = _lib.get_option("k2d_solve_one_wg")
    out = {"tool": "k2d_multi_launch_small_time", "reps": reps, "calls_per_window": ROUND, "device": torch.cuda.get_device_name(0),
           "default_k2d_solve_one_wg": default, "clocks_before": clocks(), "grids": []}
    for Y, X, B in GRIDS:
        out["grids"].append(measure(Y, X, B, reps))
        _lib.set_option("k2d_solve_one_wg", default)
    out["one_launch_wins"] = all(gr["solve"]["ratio_one_launch_over_chain"] < 1.0 for gr in out["grids"])
    out["clocks"] = clocks()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
