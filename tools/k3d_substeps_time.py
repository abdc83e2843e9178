#!/usr/bin/env python
"""karman-3d diffusion substeps: what n substeps cost, and whether fusing them pays: one JSON line, also written to
profiles/k3d_substeps_time.json.  128 x 64 x 64, B = 1, the default sphere (direct solve), one process, on a spun-up state.

1. The forward step (Karman3DFlow._fwd_sub with saved_*) and the velocity adjoint (sol_karman3d_step_bwd on the scaled cfg, then the
   pre-diffusion on its result) for n in {1, 2, 4, 8}, as ratios to the plain launches (Karman3DFlow._fwd / ._bwd: the launches of a
   simulator built without the keyword) in the same process.  HIP events around ROUND calls in a row; the plain call and the n-substep
   call ALTERNATE window by window (a drift of the clock hits both); per form the median over the repetitions and the spread
   (max - min) / median.  n = 1 issues the plain call's launches: its ratio is the noise floor.
2. The pre-diffusion alone (karman3d.diffuse_sub) of m substeps for every m <= S_MAX: ONE fused launch (chunk = m) against m chained
   single-substep launches (chunk = 1), alternated the same way, the bits asserted equal.  This is the number that decides the default
   chunk (karman3d.DIFFUSE_SUB_CHUNK3D).
No threshold: the file records what was measured, on whatever clock the box held ("clocks": rocm-smi's lines after the runs, read
only); compare the numbers of one file with each other and with nothing else.
Usage: python tools/k3d_substeps_time.py [reps]"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "k3d_substeps_time.json")
Y, X, Z, B = 128, 64, 64, 1
NS = (1, 2, 4, 8)
ROUND = 10          # calls per timed window


def window(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ROUND):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / ROUND


def spread(ts):
    m = statistics.median(ts)
    return {"median_us": m, "min_us": min(ts), "max_us": max(ts), "spread": (max(ts) - min(ts)) / m}


def alternated(forms, reps):
    """{name: spread} of callables timed in alternating windows (three warm-up rounds)"""
    ts = {k: [] for k in forms}
    for it in range(3 + reps):
        for k, fn in forms.items():
            t = window(fn)
            if it >= 3:
                ts[k].append(t)
    return {k: spread(v) for k, v in ts.items()}


def clocks():
    """rocm-smi's clock lines (read only), as tools/k3d_buoyancy_time.py records them"""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
        return [l.strip() for l in r.stdout.splitlines() if "sclk" in l or "mclk" in l]
    except Exception as e:
        return ["unavailable: %s" % e]


def main():
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import sol_amd        # noqa: F401
    from sol_amd import karman3d as k3
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    dev = "cuda"
    sc = k3.Scene3D(Y, X, Z, device=dev)
    plain = k3.Karman3DFlow(sc, B)
    smax = k3.diffuse_sub_max3d()
    re = torch.tensor([float(np.float32(X * X / 0.45))], device=dev)          # alpha beyond the single stencil's bound 1/6
    gen = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)
    st = (torch.rand(B, Y, X, Z, generator=gen, dtype=torch.float32).to(dev), (1.0 + 0.1 * rn(B, Y + 1, X, Z)).to(dev),
          (0.1 * rn(B, Y, X + 1, Z)).to(dev), (0.1 * rn(B, Y, X, Z + 1)).to(dev))
    warm = k3.Karman3DFlow(sc, B, diffusion_substeps=3)
    with torch.no_grad():
        for _ in range(2):                                                     # spun-up state (three substeps: the stable count at this alpha)
            st = warm.step(*st, re)
    wv = [rn(*t.shape).to(dev) for t in st[1:]]
    out = {"tool": "k3d_substeps_time", "grid": [Y, X, Z], "B": B, "solver": sc.pressure_solver, "reps": reps, "calls_per_window": ROUND,
           "device": torch.cuda.get_device_name(0), "s_max": smax, "default_chunk": k3.DIFFUSE_SUB_CHUNK3D, "step": {}, "pre_diffusion": {}}
    with torch.no_grad():
        psaved = [torch.empty_like(t) for t in st[1:]]
        plain._fwd(*st, re, psaved)
        for n in NS:
            sim = k3.Karman3DFlow(sc, B, diffusion_substeps=n)
            saved = [torch.empty_like(t) for t in st[1:]]
            sim._fwd_sub(*st, re, saved, nsub=n)

            def bwd_n(sim=sim, saved=saved, n=n):
                return k3.diffuse_sub(sim, *sim._bwd(saved, re, *wv, nsub=n), re, n)

            r = alternated({"fwd_plain": lambda: plain._fwd(*st, re, psaved),
                            "fwd_n": lambda: sim._fwd_sub(*st, re, saved, nsub=n),
                            "bwd_plain": lambda: plain._bwd(psaved, re, *wv),
                            "bwd_n": bwd_n}, reps)
            r["ratio_fwd"] = r["fwd_n"]["median_us"] / r["fwd_plain"]["median_us"]
            r["ratio_bwd"] = r["bwd_n"]["median_us"] / r["bwd_plain"]["median_us"]
            out["step"]["n=%d" % n] = r
        v = st[1:]
        for m in range(1, smax + 1):
            a = k3.diffuse_sub(plain, *v, re, m + 1, chunk=m)
            b = k3.diffuse_sub(plain, *v, re, m + 1, chunk=1)
            assert all(torch.equal(x, y) for x, y in zip(a, b))
            r = alternated({"fused": lambda: k3.diffuse_sub(plain, *v, re, m + 1, chunk=m),
                            "chained": lambda: k3.diffuse_sub(plain, *v, re, m + 1, chunk=1)}, reps)
            r["ratio_fused_over_chained"] = r["fused"]["median_us"] / r["chained"]["median_us"]
            out["pre_diffusion"]["%d_substeps" % m] = r
    out["clocks"] = clocks()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
