#!/usr/bin/env python
"""Circular padding of the karman-2d correction network: what conv_padding="circular" costs against "zeros" on the same
periodic scene.  One JSON line, also written to profiles/k2d_circular_net_time.json.  One process; HIP events around ROUND calls in a
row; the two forms ALTERNATE window by window; per form the median over the repetitions and the spread (max - min) / median; the shader
clock the box held is recorded before and after (rocm-smi, read only).

Cases (B = 2, mars_moon, no obstacle), with the rows the network runs in:
  256x128_x   x periodic: zeros dense rows of 128; circular rows of 192 (132 pixels: one extra 64-pixel tile)
  256x124_x   x periodic: zeros any_width rows of 128; circular rows of 128 (no extra tile)
  256x128_y   y periodic: zeros 256 rows of 128; circular 260 rows of 128
Per case:
  trainer   one captured LargeGridTrainer step (msteps = 2)
  rollout   one captured LargeGridRollout step
"ratio": the circular median over the zeros median; "noise": the larger spread of the two.  A ratio inside 1 +- noise is within what the
windows resolve.  "halo": the sol_conv_halo launch alone on a [2, 256, 192, 32] buffer (x periodic, W = 128), wrap and zero, per launch.
"halo_launches": sol_conv_halo launches per network forward / backward pass (counted with _lib.profile on an eager pass).
Usage: python tools/k2d_circular_net_time.py [reps]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "k2d_circular_net_time.json")
CASES = (("256x128_x", 256, 128, ("open", "periodic")), ("256x124_x", 256, 124, ("open", "periodic")), ("256x128_y", 256, 128, ("periodic", "open")))
B, MS, ROUND = 2, 2, 5


def window(fn, rounds):
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
    r = {k: spread(v) for k, v in ts.items()}
    r["ratio"] = r["circular"]["median_us"] / r["zeros"]["median_us"]
    r["noise"] = max(r["circular"]["spread"], r["zeros"]["spread"])
    r["within_noise"] = abs(r["ratio"] - 1.0) <= r["noise"]
    return r


def clocks():
    """rocm-smi's clock lines (read only): the clock the box held"""
    import subprocess
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
        return [l.strip() for l in r.stdout.splitlines() if "sclk" in l or "mclk" in l]
    except Exception as e:
        return ["unavailable: %s" % e]


def measure(name, Y, X, bnd, reps):
    import numpy as np
    import torch
    import sol_oracle as o
    import sol_amd
    from sol_amd import _lib, ops, schedule2d
    g = o.geometry(Y, X)
    mk = ops.SceneMasks(np.ones((Y, X)), g.inflow, g.bc_mask, g.bc_mask, "cuda", multi_launch=False, boundaries=bnd)
    per = mk.periodic
    gen = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=gen)
    d, vy, vx = torch.rand(B, Y, X, generator=gen).cuda(), (1.0 + 0.1 * rn(B, Y + 1, X)).cuda(), (0.1 * rn(B, Y, X + 1)).cuda()
    vy, vx = ops.karman_seam_sync(vy, vx, per)
    re = torch.tensor([o.RE_TRAIN[i % 6] for i in range(B)], dtype=torch.float32, device="cuda")
    args = (d, vy, vx, re, torch.stack([vy] * MS).contiguous(), torch.stack([vx] * MS).contiguous())
    net = lambda: sol_amd.model_mars_moon(cin=3, cout=2, seed=0)
    aw = schedule2d.row_pitch(Y, X) != X
    out = {"case": name, "grid": [Y, X], "B": B, "boundaries": list(bnd), "zeros_any_width": aw}
    tr = {k: sol_amd.LargeGridTrainer(net(), B, Y, X, MS, (0.2, 0.2), o.STD_RE, masks=mk, obstacles=[], any_width=aw and k == "zeros", conv_padding=k)
          for k in ("zeros", "circular")}
    for t in tr.values():
        t.fwd_bwd(*args)
        assert t._graph is not None
    out["rows"] = {k: [t._sched.HB, t._sched.P, t._sched.WV] for k, t in tr.items()}
    out["trainer"] = dict(alternated({k: (lambda t=t: t.fwd_bwd(*args)) for k, t in tr.items()}, reps), msteps=MS)
    ro = {k: sol_amd.LargeGridRollout(net(), mk, B, Y, X, g.dx, (0.2, 0.2), o.STD_RE, any_width=aw and k == "zeros", conv_padding=k)
          for k in ("zeros", "circular")}
    st = [t.clone() for t in (d, vy, vx)]
    for r in ro.values():
        r.run(*st, re, 1)
        assert r._graph is not None
    steps = 4 * ROUND
    out["rollout"] = alternated({k: (lambda r=r: r.run(*[t.clone() for t in (d, vy, vx)], re, steps)) for k, r in ro.items()}, reps, rounds=1)
    for k in ("zeros", "circular"):
        for f in ("median_us", "min_us", "max_us"):
            out["rollout"][k][f] /= steps
    out["rollout"]["steps_per_window"] = steps
    # the halo launches of one eager network pass
    sch = schedule2d.NetSchedule2D(net(), B, Y, X, padding="circular", periodic=per)
    x, gy = rn(B, Y, X, 3).cuda(), rn(B, Y, X, 2).cuda()
    with torch.no_grad():
        sch.begin_step()
        with _lib.profile() as pf:
            _, state = sch.forward(x)
        fwd = sum(c for n, (c, _) in pf.kernels.items() if "k_conv_halo" in n)
        with _lib.profile() as pb:
            sch.backward(state, gy)
        bwd = sum(c for n, (c, _) in pb.kernels.items() if "k_conv_halo" in n)
    out["halo_launches"] = {"forward": fwd, "backward": bwd,
                            "halo_us_forward": sum(t for n, (_, t) in pf.kernels.items() if "k_conv_halo" in n),
                            "halo_us_backward": sum(t for n, (_, t) in pb.kernels.items() if "k_conv_halo" in n),
                            "all_us_forward": sum(t for _, t in pf.kernels.values()), "all_us_backward": sum(t for _, t in pb.kernels.values())}
    return out


def halo_alone(reps):
    import torch
    from sol_amd import ops
    buf = torch.randn(2, 256, 192, 32, device="cuda")
    r = {}
    for mode in ("wrap", "zero"):
        ts = [window(lambda: ops.conv_halo(buf, 256, 128, (False, True), mode), 200) for _ in range(3 + reps)][3:]
        r[mode] = spread(ts)
    r["buffer"] = [2, 256, 192, 32]
    return r


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import torch
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 11
    out = {"tool": "k2d_circular_net_time", "reps": reps, "calls_per_window": ROUND, "device": torch.cuda.get_device_name(0),
           "clocks_before": clocks(), "cases": []}
    for name, Y, X, bnd in CASES:
        out["cases"].append(measure(name, Y, X, bnd, reps))
    out["halo"] = halo_alone(reps)
    out["clocks"] = clocks()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
