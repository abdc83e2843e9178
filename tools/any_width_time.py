#!/usr/bin/env python
"""What training on a ragged row width costs: one LargeGridTrainer training step at 256 x 96 with any_width=True
(rows pitched to 128 pixels, column-masked convolutions) against the same batch, unroll and network at 256 x 128 without the flag --
both launch the same 64-pixel tiles in the network, so the padded step may exceed the yardstick by its pad / crop copies only (its
solver step is the SMALLER one: 96 columns).  One JSON line, also written to profiles/any_width_time.json.

Conventions of tools/k2d_large_train_time.py: SOL-4, mars_moon with a small last layer, B = 1, default sphere (direct solve), HIP
events around train_step (forward, reverse sweep, Adam), three warm-up steps; the two trainers ALTERNATE step by step in one process.
Per configuration the median and the p10 / p90 of the timed steps; `difference_ms` = padded median - yardstick median stands beside
`yardstick_p10_p90_ms`, the run-to-run spread it has to be read against.  The network's share alone (the part both grids share tile
for tile) comes from the launch profiler over one eager step: kernel time of the convolution / pack / weight-gradient launches, and
the names of the column-masked instantiations that ran (none on the yardstick grid).
Usage: python tools/any_width_time.py [reps]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "any_width_time.json")
Y, MS, B = 256, 4, 1
GRIDS = {"padded_256x96": (96, True), "yardstick_256x128": (128, False)}


def make(X, any_width, use_graph):
    import torch
    import sol_amd
    from sol_amd import ops
    net = sol_amd.model_mars_moon(cin=3, cout=2, seed=0)
    w = net.get_weights()                            # small last layer: an untrained corrector fed back through the solver (bench.py)
    w[22] = w[22] * 0.01
    net.set_weights(w)
    tr = sol_amd.LargeGridTrainer(net, B, Y, X, MS, (0.2, 0.2), 1e4, use_graph=use_graph, any_width=any_width)
    gen = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=gen)
    d, vy, vx = torch.rand(B, Y, X, generator=gen).to("cuda"), (1.0 + 0.1 * rn(B, Y + 1, X)).to("cuda"), (0.1 * rn(B, Y, X + 1)).to("cuda")
    re = torch.full((B,), 1.6e5, device="cuda")
    mk = tr.sim._masks(tr.dom, tr.bcv, tr.bcm, tr.device)
    cfg = ops.karman_cfg(B, Y, X, tr.dom.dx[1], masks=mk)
    gy, gx = [], []
    with torch.no_grad():
        d, vy, vx = ops.karman_step_large(d, vy, vx, re, cfg, mk)       # spun up in the scene
        s = (d, vy + 0.05 * (vy - 1.0), vx * 1.05)
        for _ in range(MS):
            s = ops.karman_step_large(*s, re, cfg, mk)
            gy.append(s[1])
            gx.append(s[2])
    return tr, (d, vy, vx, re, torch.stack(gy), torch.stack(gx))


def pct(ts, q):
    ts = sorted(ts)
    return ts[min(len(ts) - 1, max(0, int(round(q * (len(ts) - 1)))))]


def timed(use_graph, reps):
    import torch
    runs = {k: make(X, aw, use_graph) for k, (X, aw) in GRIDS.items()}
    for _ in range(3):
        for tr, batch in runs.values():
            tr.train_step(*batch, 1e-6)
    torch.cuda.synchronize()
    ts = {k: [] for k in runs}
    for _ in range(reps):
        for k, (tr, batch) in runs.items():          # alternate the two grids step by step
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tr.train_step(*batch, 1e-6)
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    r = {k: {"median_ms": statistics.median(v), "p10_ms": pct(v, 0.1), "p90_ms": pct(v, 0.9), "min_ms": min(v), "max_ms": max(v)} for k, v in ts.items()}
    y = r["yardstick_256x128"]
    r["difference_ms"] = r["padded_256x96"]["median_ms"] - y["median_ms"]
    r["yardstick_p10_p90_ms"] = y["p90_ms"] - y["p10_ms"]
    r["solver"] = runs["padded_256x96"][0].pressure_solver_used
    return r


def network_kernel_time():
    """kernel time per eager step of the network's launches (convolutions, packs, weight gradient + reduce) per grid, and which
    column-masked instantiations ran: launch profiler"""
    import torch
    from sol_amd import _lib
    out = {}
    for k, (X, aw) in GRIDS.items():
        tr, batch = make(X, aw, False)
        for _ in range(2):
            tr.fwd_bwd(*batch)
        torch.cuda.synchronize()
        with _lib.profile() as p:
            tr.fwd_bwd(*batch)
        net = sum(us for name, (n, us) in p.kernels.items() if "conv5x5" in name or "pack" in name or "bww" in name)
        # (the forward / backward-data kernels only: the trailing `true` of the weight-gradient kernels is their wide-row form)
        masked = sorted(name for name in p.kernels if "conv5x5" in name and "bww" not in name and name.replace(" ", "").rstrip(")").endswith("true>")
                        and "dx<1,1,true>" not in name.replace(" ", ""))
        out[k] = {"network_kernels_ms": net / 1e3, "library_launches": int(sum(n for n, _ in p.kernels.values())), "masked_instantiations": masked}
    return out


def main():
    sys.path.insert(0, ROOT)
    import torch
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    out = {"tool": "any_width_time", "reps": reps, "msteps": MS, "batch": B, "network": "mars_moon", "device": torch.cuda.get_device_name(0),
           "wasted_tile_fraction": 1.0 - 96.0 / 128.0,
           "train_step_graph": timed(True, reps), "train_step_eager": timed(False, reps), "eager_step_kernel_time": network_kernel_time()}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
