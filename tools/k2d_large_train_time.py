#!/usr/bin/env python
"""karman-2d training on large grids: the wide-row 5x5 weight gradient against the W = 64 kernel at equal pixel
count, and the training step at 256 x 128: one JSON line, also written to profiles/k2d_large_train_time.json.

1. Weight gradient, 32 -> 32 channels, split precision (sol_conv5x5_bwd_weight, the launch alone and launch + reduce): [B=2, H=256,
   W=128] (two column tiles per row block, x halo from the neighbouring tile) and, as the yardstick, [B=4, H=256, W=64] -- the same
   pixels, the same FLOP, the same number of workgroups.  HIP events around every call, the two shapes ALTERNATE call by call in one
   process; per shape the median over the repetitions and the spread (max - min) / median.  The wide form stages 68 / 64 of the x
   pixels: expected within +6.25 % plus the spread of the yardstick.
2. Training step, SOL-4, mars_moon, LargeGridTrainer.train_step (forward, reverse sweep, Adam), ms per step by HIP events:
   default sphere (direct solve) B = 1 and 6, captured and eager; two cylinders (CG solve), B = 1, eager.
3. --split: `rocprofv3 --kernel-trace --stats` runs of their own per configuration (fresh child processes running `--trace NAME N`:
   the set-up plus N eager steps, and the set-up alone, which is taken off), kernel time per step summed into solver / convolutions
   / weight gradient / other (tools/rocpd_stats.py reads the same rocpd database).  Merged into the JSON of an earlier plain run.
Usage: python tools/k2d_large_train_time.py [reps]              timings (1, 2)
       python tools/k2d_large_train_time.py --split             kernel split (3)"""
import glob
import json
import os
import sqlite3
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "k2d_large_train_time.json")
Y, X, MS = 256, 128, 4
TWO = ["sphere:50,50,10", "sphere:120,50,10"]
CONFIGS = {"sphere_direct_B1": (None, 1), "sphere_direct_B6": (None, 6), "two_cylinders_cg_B1": (TWO, 1)}
TRACE_STEPS = 3
GROUPS = (("weight_gradient", ("bww",)), ("convolutions", ("conv5x5", "k_pack", "pack_jobs")),
          ("solver", ("k_l_", "k_lb_", "pcg_", "k_large", "karman")))


def events():
    import torch
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def spread(ts):
    m = statistics.median(ts)
    return {"median_us": m, "min_us": min(ts), "max_us": max(ts), "spread": (max(ts) - min(ts)) / m}


def bww_compare(reps):
    import torch
    from sol_amd import _lib
    from sol_amd._lib import check, ptr, stream
    lib = _lib.load()
    gen = torch.Generator().manual_seed(5)
    shapes = {"wide_2x256x128": (2, 256, 128), "w64_4x256x64": (4, 256, 64)}
    data, times = {}, {k: {"bww": [], "bww_reduce": []} for k in shapes}
    for k, (B, H, W) in shapes.items():
        x = torch.randn(B, H, W, 32, generator=gen).to("cuda")
        dz = (torch.randn(B, H, W, 32, generator=gen) * 1e-2).to("cuda")
        part = torch.zeros(lib.sol_conv5x5_bwd_weight_ws_floats(B, H, W, 32, 32), dtype=torch.float32, device="cuda")
        dw, db = torch.empty(5, 5, 32, 32, device="cuda"), torch.empty(32, device="cuda")
        data[k] = (x, dz, part, dw, db, B, H, W)

    def call(k, reduce):
        x, dz, part, dw, db, B, H, W = data[k]
        check(lib.sol_conv5x5_bwd_weight(stream(), ptr(x), ptr(dz), ptr(part), B, H, W, 32, 32))
        if reduce:
            check(lib.sol_conv5x5_bwd_weight_reduce(stream(), ptr(part), ptr(dw), ptr(db), B, H, W, 32, 32, 0))

    for it in range(5 + reps):                       # five warm-up rounds
        for reduce in (False, True):
            for k in shapes:                         # alternate the two shapes call by call
                e0, e1 = events()
                e0.record()
                call(k, reduce)
                e1.record()
                torch.cuda.synchronize()
                if it >= 5:
                    times[k]["bww_reduce" if reduce else "bww"].append(e0.elapsed_time(e1) * 1e3)
    r = {"layer": "32->32", "conv_precision": int(_lib.get_option("conv_precision")), "reps": reps,
         "workgroups": {k: int(B * H // 8 * max(1, W // 64)) for k, (B, H, W) in shapes.items()}}
    for k in shapes:
        r[k] = {m: spread(ts) for m, ts in times[k].items()}
    for m in ("bww", "bww_reduce"):
        r["ratio_wide_over_w64_" + m] = r["wide_2x256x128"][m]["median_us"] / r["w64_4x256x64"][m]["median_us"]
    r["expected_bound"] = 1.0625 + r["w64_4x256x64"]["bww"]["spread"]
    return r


def make_trainer(name, use_graph):
    import torch
    import sol_amd
    specs, B = CONFIGS[name]
    net = sol_amd.model_mars_moon(cin=3, cout=2, seed=0)
    w = net.get_weights()                            # small last layer: an untrained corrector fed back through the solver (bench.py)
    w[22] = w[22] * 0.01
    net.set_weights(w)
    kw = {} if specs is None else {"obstacles": sol_amd.parse_obstacles(specs)}
    tr = sol_amd.LargeGridTrainer(net, B, Y, X, MS, (0.2, 0.2), 1e4, use_graph=use_graph, **kw)
    gen = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=gen)
    d, vy, vx = torch.rand(B, Y, X, generator=gen).to("cuda"), (1.0 + 0.1 * rn(B, Y + 1, X)).to("cuda"), (0.1 * rn(B, Y, X + 1)).to("cuda")
    re = torch.full((B,), 1.6e5, device="cuda")
    from sol_amd import ops
    dom = tr.dom
    mk = tr.sim._masks(dom, tr.bcv, tr.bcm, tr.device)
    cfg = ops.karman_cfg(B, Y, X, dom.dx[1], masks=mk)
    gy, gx = [], []
    with torch.no_grad():
        d, vy, vx = ops.karman_step_large(d, vy, vx, re, cfg, mk)       # spun up in the scene
        s = (d, vy + 0.05 * (vy - 1.0), vx * 1.05)
        for _ in range(MS):
            s = ops.karman_step_large(*s, re, cfg, mk)
            gy.append(s[1])
            gx.append(s[2])
    return tr, (d, vy, vx, re, torch.stack(gy), torch.stack(gx))


def train_time(name, use_graph, reps):
    import torch
    tr, batch = make_trainer(name, use_graph)
    for _ in range(3):
        tr.train_step(*batch, 1e-6)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = events()
        e0.record()
        tr.train_step(*batch, 1e-6)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    r = {"ms_per_step": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "solver": tr.pressure_solver_used}
    if tr.solve_info:
        r["iterations_fwd"] = tr.solve_info["iterations"].tolist()
        r["iterations_bwd"] = tr.solve_info["iterations_bwd"].tolist()
    return r


def trace_child(name, steps):
    import torch
    tr, batch = make_trainer(name, False)
    for _ in range(steps):                           # (the first one builds the schedule; every step issues the same kernels)
        tr.train_step(*batch, 1e-6)
    torch.cuda.synchronize()


def traced(name, steps):
    """{kernel: (launches, ns)} of a child that sets the configuration up (scene, spin-up, ground truth) and runs `steps` eager steps"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "trace", "--", sys.executable, os.path.abspath(__file__), "--trace", name, str(steps)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        dbs = glob.glob(os.path.join(tmp, "**", "*.db"), recursive=True)
        if p.returncode != 0 or not dbs:
            raise RuntimeError("rocprofv3 run of %s failed (%d):\n%s" % (name, p.returncode, p.stdout[-2000:]))
        return {k: (n, d) for k, n, d in sqlite3.connect(dbs[0]).execute("select name, count(*), sum(duration) from kernels group by name")}


def split(name):
    # the set-up's own launches (five solver steps among them) are traced alone and taken off
    full, setup = traced(name, TRACE_STEPS), traced(name, 0)
    rows = [(k, n - setup.get(k, (0, 0))[0], max(0, d - setup.get(k, (0, 0))[1])) for k, (n, d) in full.items()]
    r = {g: 0.0 for g, _ in GROUPS}
    r["other"] = 0.0
    top = {}
    for kname, n, dur in rows:
        grp = next((g for g, keys in GROUPS if any(k in kname for k in keys)), "other")
        r[grp] += dur / 1e6 / TRACE_STEPS
        top[kname[:60]] = round(dur / 1e6 / TRACE_STEPS, 4)
    r = {k + "_ms": round(v, 4) for k, v in r.items()}
    r["kernel_ms_per_step"] = round(sum(v for v in r.values()), 4)
    r["launches_per_step"] = int(sum(n for _, n, _ in rows) // TRACE_STEPS)
    r["largest_kernels_ms"] = dict(sorted(top.items(), key=lambda kv: -kv[1])[:8])
    return r


def main():
    args = sys.argv[1:]
    if args[:1] == ["--trace"]:
        sys.path.insert(0, ROOT)
        return trace_child(args[1], int(args[2]))
    if args[:1] == ["--split"]:
        with open(OUT) as f:
            out = json.loads(f.read())
        out["kernel_split_eager"] = {name: split(name) for name in CONFIGS}
    else:
        sys.path.insert(0, ROOT)
        import torch
        reps = int(args[0]) if args else 20
        out = {"tool": "k2d_large_train_time", "reps": reps, "grid": [Y, X], "msteps": MS, "network": "mars_moon",
               "device": torch.cuda.get_device_name(0), "weight_gradient": bww_compare(reps), "train_step": {}}
        for name in CONFIGS:
            for use_graph in ((True, False) if "cg" not in name else (False,)):
                out["train_step"]["%s_%s" % (name, "graph" if use_graph else "eager")] = train_time(name, use_graph, reps)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
