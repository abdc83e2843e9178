#!/usr/bin/env python
"""Large-grid Burgers step: forward and adjoint: one JSON line, also written to profiles/burgers_large_bwd_time.json.

At 128 x 128 (the reference's hi-res setting, dx = 0.25, dt = 0.1, nu = 0.1), B = 5 and B = 1, in ONE process on a smooth random
state: the forward sequence (ops.burgers_step_large under no_grad: five launches) and the adjoint sequence
(ops.burgers_step_large_bwd with a fixed random cotangent: seven launches) in us, HIP events around eager calls; and the kernel split
of both (sol_prof_begin / sol_prof_end: per-kernel device time summed over the repetitions, us per call of the sequence).  The file
also states whether the scatter kernel alone takes longer than the adjoint's four circulant products together -- the condition under
which it would be routed through an LDS window.
Usage: python tools/burgers_large_bwd_time.py [reps]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch          # noqa: E402
from sol_amd import _lib, ops, synthetic   # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
DEV = "cuda"
Y = X = 128
DT, NU, DX = 0.1, 0.1, 32.0 / 128


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


def run(B, reps):
    gen = torch.Generator().manual_seed(3)
    sm = lambda *s: synthetic._smooth(torch.randn(*s, generator=gen, dtype=torch.float64)).float().to(DEV)
    vy, vx, fy, fx = 0.8 * sm(B, Y + 1, X), 0.8 * sm(B, Y, X + 1), 0.2 * sm(B, Y + 1, X), 0.2 * sm(B, Y, X + 1)
    wy, wx = torch.randn(B, Y + 1, X, generator=gen).to(DEV), torch.randn(B, Y, X + 1, generator=gen).to(DEV)
    cfg = _lib.BurgersCfg(B, Y, X, DX, DT)
    circ = ops.burgers_circ(Y, X, DT * NU, DEV)
    ws = torch.empty((ops.burgers_large_workspace_bytes(cfg) + 3) // 4, dtype=torch.float32, device=DEV)
    fwd = lambda: ops.burgers_step_large(vy, vx, fy, fx, cfg, circ, ws)
    bwd = lambda: ops.burgers_step_large_bwd(vy, vx, wy, wx, cfg, circ, ws)
    r = {"grid": [Y, X], "B": B}
    with torch.no_grad():
        r["step_fwd_us"] = timed(fwd, reps)
        r["step_bwd_us"] = timed(bwd, reps)
    r["bwd_over_fwd"] = r["step_bwd_us"] / r["step_fwd_us"]
    for key, fn in (("bwd_kernels_us", bwd), ("fwd_kernels_us", fwd)):
        torch.cuda.synchronize()
        with torch.no_grad(), _lib.profile() as p:
            for _ in range(reps):
                fn()
        r[key] = {k: round(v[1] / reps, 3) for k, v in sorted(p.kernels.items(), key=lambda kv: -kv[1][1])}
        r[key.replace("_us", "_launches")] = int(sum(v[0] for v in p.kernels.values()) // reps)
    k = r["bwd_kernels_us"]
    r["scatter_us"] = k["k_burgers_adv_large_bwd"]
    r["four_products_us"] = round(sum(v for n, v in k.items() if "k_burgers_circ_large" in n), 3)
    r["lds_window_needed"] = r["scatter_us"] > r["four_products_us"]
    return r


def main():
    out = {"tool": "burgers_large_bwd_time", "reps": REPS, "dt": DT, "nu": NU, "dx": DX, "scatter": "global int64 atomics",
           "device": torch.cuda.get_device_name(0)}
    for B in (5, 1):
        out["B%d" % B] = run(B, REPS)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "burgers_large_bwd_time.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
