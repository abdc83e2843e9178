#!/usr/bin/env python
"""karman-2d gradient with respect to the Reynolds number: what re_grad adds to a backward pass, one JSON line, also written
to profiles/k2d_re_bwd_time.json.

In ONE process, on a spun-up state with fixed random cotangents, each pair ALTERNATED (a, b, a, b: a drift of the clock hits both):
  * 256 x 128, B = 2, the default sphere (direct solve): sol_karman_step_bwd_large_re against sol_karman_step_bwd_large, and
    sol_karman_density_bwd_re against sol_karman_density_bwd;
  * 64 x 32, B = 3: the staged adjoint with g_re (what re_grad runs on a one-workgroup grid) against the fused one-workgroup adjoint
    (sol_karman_step_bwd, what runs without the flag) -- the price of leaving the fused kernel alone;
and the kernel split of the two _re calls (sol_prof_begin / sol_prof_end: device time per kernel, us per call).  HIP events around eager
calls.  No threshold: the file records what was measured, on whatever clock the box held ("clocks": rocm-smi's lines after the runs); compare the numbers of one file with each other and with nothing else.
Usage: python tools/k2d_re_bwd_time.py [reps]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch          # noqa: E402
from sol_amd import _lib, fluid, karman, ops   # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
DEV = "cuda"


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def alternated(a, b, reps, rounds=4):
    """us per call of a and of b, `rounds` blocks of each in turn; the minimum over the blocks of each"""
    a(), b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(a, reps))
        tb.append(timed(b, reps))
    return min(ta), min(tb)


def clocks():
    """rocm-smi's clock lines (read only), as tools/k2d_large_rollout_time.py records them"""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
        return [l.strip() for l in r.stdout.splitlines() if "sclk" in l or "mclk" in l]
    except Exception as e:
        return ["unavailable: %s" % e]


def scene(Y, X, B):
    dom = fluid.Domain([Y, X], box=fluid.box[0:200, 0:100])
    active, inflow = karman.KarmanFlow().scene_arrays(dom)
    bc, _ = karman.velocity_bc_masks(Y, X)
    mk = ops.SceneMasks(active, inflow, bc.reshape(Y + 1, X), bc.reshape(Y + 1, X), DEV)
    cfg = ops.karman_cfg(B, Y, X, dom.dx[1], masks=mk)
    re = torch.full((B,), 1.6e5, device=DEV)
    gen = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=gen)
    st = (torch.rand(B, Y, X, generator=gen).to(DEV), (1.0 + 0.1 * rn(B, Y + 1, X)).to(DEV), (0.1 * rn(B, Y, X + 1)).to(DEV))
    fwd = lambda *s: ops.karman_step_saved(*s, re, cfg, mk)
    with torch.no_grad():
        st = fwd(*st)[0]                  # spun-up state
        st = fwd(*st)[0]
        _, svy, svx = fwd(*st)
    gen = torch.Generator().manual_seed(3)
    w = (torch.randn(B, Y, X, generator=gen).to(DEV), torch.randn(B, Y + 1, X, generator=gen).to(DEV), torch.randn(B, Y, X + 1, generator=gen).to(DEV))
    return mk, cfg, re, st, svy, svx, w


def main():
    r = {"tool": "k2d_re_bwd_time", "reps": REPS, "device": torch.cuda.get_device_name(0)}
    # 256 x 128, B = 2: the _re adjoints against the plain ones
    Y, X, B = 256, 128, 2
    mk, cfg, re, st, svy, svx, w = scene(Y, X, B)
    ws_v = torch.empty((ops.large_bwd_workspace_bytes(cfg, mk, re=True) + 3) // 4, dtype=torch.float32, device=DEV)
    ws_d = torch.empty((ops.density_bwd_workspace_bytes(cfg, re=True) + 3) // 4, dtype=torch.float32, device=DEV)
    vel = lambda: ops.karman_step_large_bwd(svy, svx, re, w[1], w[2], cfg, mk, ws_v)
    vel_re = lambda: ops.karman_step_large_bwd_re(svy, svx, re, w[1], w[2], st[1], st[2], cfg, mk, workspace=ws_v)
    dens = lambda: ops.karman_density_bwd(st[0], svy, svx, re, w[0], cfg, mk, workspace=ws_d)
    dens_re = lambda: ops.karman_density_bwd_re(st[0], svy, svx, re, w[0], st[1], st[2], cfg, mk, workspace=ws_d)
    big = {"grid": [Y, X], "B": B, "solver": mk.pressure_solver}
    big["velocity_bwd_re_us"], big["velocity_bwd_us"] = alternated(vel_re, vel, REPS)
    big["density_bwd_re_us"], big["density_bwd_us"] = alternated(dens_re, dens, REPS)
    big["velocity_re_minus_plain_us"] = big["velocity_bwd_re_us"] - big["velocity_bwd_us"]
    big["density_re_minus_plain_us"] = big["density_bwd_re_us"] - big["density_bwd_us"]
    for key, fn in (("velocity_re_kernels_us", vel_re), ("density_re_kernels_us", dens_re)):
        torch.cuda.synchronize()
        preps = min(REPS, 50)                                              # (every launch carries two events)
        with _lib.profile() as p:
            for _ in range(preps):
                fn()
        big[key] = {k: round(v[1] / preps, 3) for k, v in sorted(p.kernels.items(), key=lambda kv: -kv[1][1])}
    r["large"] = big
    # 64 x 32, B = 3: the staged adjoint (re_grad) against the fused one-workgroup adjoint (the default)
    Y, X, B = 64, 32, 3
    mk, cfg, re, st, svy, svx, w = scene(Y, X, B)
    ws_s = torch.empty((ops.large_bwd_workspace_bytes(cfg, mk, re=True) + 3) // 4, dtype=torch.float32, device=DEV)
    staged = lambda: ops.karman_step_large_bwd_re(svy, svx, re, w[1], w[2], st[1], st[2], cfg, mk, workspace=ws_s)
    fused = lambda: ops._step_bwd(svy, svx, re, w[1], w[2], cfg, mk, None)
    small = {"grid": [Y, X], "B": B, "solver": mk.pressure_solver}
    small["staged_bwd_re_us"], small["fused_bwd_us"] = alternated(staged, fused, REPS)
    small["staged_over_fused"] = small["staged_bwd_re_us"] / small["fused_bwd_us"]
    r["one_workgroup"] = small
    r["clocks"] = clocks()
    line = json.dumps(r)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "k2d_re_bwd_time.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
