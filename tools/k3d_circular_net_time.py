#!/usr/bin/env python
"""Circular z padding of the karman-3d correction network: what conv_padding="circular" costs against "zeros" on the periodic
cylinder at 128 x 64 x 64, B = 1.  One JSON line, also written to profiles/k3d_circular_net_time.json.  One process; HIP events around
ROUND calls in a row; the two forms ALTERNATE window by window; per form the median over the repetitions and the spread (max - min) /
median; the shader clock the box held is recorded before and after (rocm-smi, read only).

  trainer   one captured Karman3DTrainer step (SOL-2)
  rollout   one Karman3DRollout step (solver step, network, correction, seam sync)
  network   the roll-out's forward schedule alone (NetSchedule3D(train=False).forward)
"ratio": the circular median over the zeros median; "noise": the larger spread of the two.  "rows": HB over Z, what the circular network's
buffers [B, Y, HB, X, C] hold against the zero-padded network's [B, Y, X, Z, C] -- the ratio to expect of the convolution launches, before
the halo launches.  "entries": one sol_conv3d_halo (32 channels, wrap and zero), sol_conv3d_circ_pack and sol_conv3d_circ_unpack (3
channels) launch alone on the buffers of this grid, per launch.  "own_launches": the feature's own launches per network forward /
backward pass with their summed time (counted with _lib.profile on an eager pass).
Usage: python tools/k3d_circular_net_time.py [reps]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "k3d_circular_net_time.json")
GRID, B, MS = (128, 64, 64), 1, 2
FORMS = ("zeros", "circular")


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


def alternated(forms, reps, rounds):
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
    r["calls_per_window"] = rounds
    return r


def clocks():
    """rocm-smi's clock lines (read only): the clock the box held"""
    import subprocess
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
        return [l.strip() for l in r.stdout.splitlines() if "sclk" in l or "mclk" in l]
    except Exception as e:
        return ["unavailable: %s" % e]


def measure(reps):
    import torch
    import sol_oracle3d as o
    from sol_amd import _lib, karman3d as k3
    from sol_amd._lib import check, ptr, stream
    from sol_amd.schedule3d import NetSchedule3D
    Y, X, Z = GRID
    HB = k3.circular_rows3d(X, Z)
    act, inflow = k3.cylinder_arrays3d(Y, X, Z)
    sc = k3.Scene3D(Y, X, Z, active=act, inflow=inflow, pressure_solver="direct_extruded", boundaries="periodic-z")
    gen = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=gen)
    d = torch.rand(B, Y, X, Z, generator=gen).cuda()
    vy, vx, vz = (1.0 + 0.1 * rn(B, Y + 1, X, Z)).cuda(), (0.1 * rn(B, Y, X + 1, Z)).cuda(), (0.1 * rn(B, Y, X, Z + 1)).cuda()
    vz[..., -1] = vz[..., 0]
    re = torch.tensor([o.RE_TRAIN[2]], dtype=torch.float32, device="cuda")
    gts = [(vy, vx, vz)] * MS
    std = (0.2, 0.25, 0.3)

    def net():
        n = k3.MarsMoon3D(device="cuda")
        w = n.get_weights()
        w[22] = w[22] * 0.05
        n.set_weights(w)
        return n

    out = {"grid": list(GRID), "B": B, "rows": {"Z": Z, "HB": HB, "ratio": HB / Z}}
    tr = {k: k3.Karman3DTrainer(net(), sc, B, MS, std, o.STD_RE, use_graph=True, conv_padding=k) for k in FORMS}
    for t in tr.values():
        t.fwd_bwd(d, vy, vx, vz, re, gts)
        assert t._graph is not None
    out["trainer"] = dict(alternated({k: (lambda t=t: t.fwd_bwd(d, vy, vx, vz, re, gts)) for k, t in tr.items()}, reps, 3), msteps=MS)
    del tr
    ro = {k: k3.Karman3DRollout(net(), sc, B, std, o.STD_RE, conv_padding=k) for k in FORMS}
    with torch.no_grad():
        out["rollout"] = alternated({k: (lambda r=r: r.step(d, vy, vx, vz, re)) for k, r in ro.items()}, reps, 10)
        feat = rn(B, Y, X, Z, 4).cuda()
        out["network"] = alternated({k: (lambda r=r: r.sch.forward(feat)) for k, r in ro.items()}, reps, 10)
    del ro
    # the feature's own launches of one eager pass
    own = lambda p: {n.strip("()").replace(" ", ""): [c, t] for n, (c, t) in p.kernels.items() if "k_conv3d_circ" in n or "k_conv3d_halo" in n}
    sch = NetSchedule3D(net(), B, Y, X, Z, padding="circular")
    gy = rn(B, Y, X, Z, 3).cuda()
    with torch.no_grad():
        sch.begin_step()
        _, state = sch.forward(feat)
        sch.backward(state, gy)                                # (warm: allocator pools, the weight-gradient partials)
        with _lib.profile() as pf:
            _, state = sch.forward(feat)
        with _lib.profile() as pb:
            sch.backward(state, gy)
    out["own_launches"] = {"forward": own(pf), "backward": own(pb),
                           "own_us_forward": sum(t for _, t in own(pf).values()), "own_us_backward": sum(t for _, t in own(pb).values()),
                           "all_us_forward": sum(t for _, t in pf.kernels.values()), "all_us_backward": sum(t for _, t in pb.kernels.values())}
    del sch, state
    # one launch of each entry alone
    lib = _lib.load()
    h32, x4, b4, b3, y3 = (torch.randn(*s, device="cuda") for s in ((B, Y, HB, X, 32), (B, Y, X, Z, 4), (B, Y, HB, X, 4), (B, Y, HB, X, 3), (B, Y, X, Z, 3)))
    calls = {"halo_wrap_c32": lambda: check(lib.sol_conv3d_halo(stream(), ptr(h32), B * Y, Z, HB, X, 32, 0)),
             "halo_zero_c32": lambda: check(lib.sol_conv3d_halo(stream(), ptr(h32), B * Y, Z, HB, X, 32, 1)),
             "pack_wrap": lambda: check(lib.sol_conv3d_circ_pack(stream(), ptr(x4), ptr(b4), B, Y, X, Z, HB, 4, 0)),
             "unpack_c3": lambda: check(lib.sol_conv3d_circ_unpack(stream(), ptr(b3), ptr(y3), B, Y, X, Z, HB, 3))}
    out["entries"] = {k: spread([window(fn, 200) for _ in range(3 + reps)][3:]) for k, fn in calls.items()}
    out["entries"]["buffer"] = [B, Y, HB, X]
    return out


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import torch
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 11
    out = {"tool": "k3d_circular_net_time", "reps": reps, "device": torch.cuda.get_device_name(0), "clocks_before": clocks()}
    out.update(measure(reps))
    out["clocks"] = clocks()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
