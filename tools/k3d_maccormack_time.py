#!/usr/bin/env python
"""karman-3d MacCormack advection: what the scheme adds to a forward step, to its adjoints and to a training step, one JSON
line, also written to profiles/k3d_maccormack_time.json.

At 128 x 64 x 64, B = 1, the default sphere (direct solve), in ONE process and on a spun-up state, each pair ALTERNATED (a, b, a, b: a
drift of the clock hits both), HIP events around eager calls:
  * forward: Karman3DFlow._fwd with adv = 1.0 and saved_* (sol_karman3d_step_fwd_adv: k3m_hat + k3m_out in place of k3_advect) against
    the plain call;
  * the velocity adjoint with fixed random cotangents (sol_karman3d_step_bwd_adv: clear, k3m_hat, k3m_vel_adj, k3m_gh, then the plain
    scatter on g_h) against the plain one;
  * the velocity adjoint followed by the density adjoint (sol_karman3d_density_bwd_adv) against the plain pair;
  * a Karman3DTrainer SOL-2 fwd_bwd (mars_moon3d, captured graph) with and without the scheme;
and the kernel split of the MacCormack forward step and of the two adjoints, next to the plain ones (sol_prof_begin / sol_prof_end:
device time per kernel, us per call) -- the stage kernels' own times and how many plain k3_advect launches the forward stage costs.
Reported as ratios to the plain calls.  No threshold: the file records what was measured, on whatever clock the box held ("clocks":
rocm-smi's lines after the runs); compare the numbers of one file with each other and with nothing else.
Usage: python tools/k3d_maccormack_time.py [reps]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch          # noqa: E402
import sol_amd        # noqa: E402,F401
from sol_amd import _lib                 # noqa: E402
from sol_amd import karman3d as k3       # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
DEV = "cuda"
Y, X, Z, B = 128, 64, 64, 1
S = 1.0


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
    """rocm-smi's clock lines (read only), as tools/k3d_buoyancy_time.py records them"""
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
        return [l.strip() for l in r.stdout.splitlines() if "sclk" in l or "mclk" in l]
    except Exception as e:
        return ["unavailable: %s" % e]


def kernels(fn, reps):
    torch.cuda.synchronize()
    with _lib.profile() as p:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    return {k: round(tot / reps, 3) for k, (calls, tot) in sorted(p.kernels.items())}


def main():
    sc = k3.Scene3D(Y, X, Z, device=DEV)
    sim = k3.Karman3DFlow(sc, B, advection="mac_cormack", correction_strength=S)      # (sizes the workspace for every _adv call)
    re = torch.full((B,), 1.6e5, device=DEV)
    gen = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)
    st = (torch.rand(B, Y, X, Z, generator=gen, dtype=torch.float32).to(DEV), (1.0 + 0.1 * rn(B, Y + 1, X, Z)).to(DEV),
          (0.1 * rn(B, Y, X + 1, Z)).to(DEV), (0.1 * rn(B, Y, X, Z + 1)).to(DEV))
    saved = [torch.empty_like(t) for t in st[1:]]
    with torch.no_grad():
        for _ in range(2):                                                     # spun-up state
            st = sim._fwd(*st, re, adv=S)
        sim._fwd(*st, re, saved, adv=S)
    wd, wv = rn(B, Y, X, Z).to(DEV), [rn(*t.shape).to(DEV) for t in saved]
    fwd_m = lambda: sim._fwd(*st, re, saved, adv=S)
    fwd_p = lambda: sim._fwd(*st, re, saved)
    bwd_m = lambda: sim._bwd(saved, re, *wv, adv=S)
    bwd_p = lambda: sim._bwd(saved, re, *wv)
    both_m = lambda: k3.density_bwd(sim, st[0], saved, re, wd, sim._bwd(saved, re, *wv, adv=S), adv=S)
    both_p = lambda: k3.density_bwd(sim, st[0], saved, re, wd, sim._bwd(saved, re, *wv))
    both_m(), both_p()                                                         # (any workspace growth happens outside the timed calls)

    r = {"tool": "k3d_maccormack_time", "reps": REPS, "device": torch.cuda.get_device_name(0), "scene": "sphere",
         "solver": sc.pressure_solver, "grid": [Y, X, Z], "B": B, "correction_strength": S}
    with torch.no_grad():
        r["forward_maccormack_us"], r["forward_plain_us"] = alternated(fwd_m, fwd_p, REPS)
        r["adjoint_velocity_maccormack_us"], r["adjoint_velocity_plain_us"] = alternated(bwd_m, bwd_p, REPS)
        r["adjoint_velocity_density_maccormack_us"], r["adjoint_velocity_density_plain_us"] = alternated(both_m, both_p, REPS)
        r["forward_ratio"] = r["forward_maccormack_us"] / r["forward_plain_us"]
        r["adjoint_velocity_ratio"] = r["adjoint_velocity_maccormack_us"] / r["adjoint_velocity_plain_us"]
        r["adjoint_velocity_density_ratio"] = r["adjoint_velocity_density_maccormack_us"] / r["adjoint_velocity_density_plain_us"]
        preps = min(REPS, 20)                                                  # (every launch carries two events)
        r["forward_maccormack_kernels_us"] = kernels(fwd_m, preps)
        r["forward_plain_kernels_us"] = kernels(fwd_p, preps)
        r["adjoint_maccormack_kernels_us"] = kernels(both_m, preps)
        r["adjoint_plain_kernels_us"] = kernels(both_p, preps)
        km, kp = r["forward_maccormack_kernels_us"], r["forward_plain_kernels_us"]
        plain_adv = kp.get("k3_advect", kp.get("k3_advect_tile"))
        r["forward_stage_us"] = {"k3m_hat": km.get("k3m_hat"), "k3m_out": km.get("k3m_out"), "plain_advect": plain_adv}
        r["forward_stage_in_plain_advect_launches"] = (km["k3m_hat"] + km["k3m_out"]) / plain_adv
    # a training step: Karman3DTrainer, mars_moon3d, SOL-2, B = 1, captured graph, fwd_bwd only
    ms = 2
    gts = [tuple(t.clone() for t in saved) for _ in range(ms)]
    trainers = []
    for adv in (dict(advection="mac_cormack", correction_strength=S), {}):
        net = k3.MarsMoon3D(seed=0, device=DEV)
        tr = k3.Karman3DTrainer(net, sc, B, ms, (0.2, 0.2, 0.2), 1.0e6, use_graph=True, **adv)
        trainers.append(lambda tr=tr: tr.fwd_bwd(*st, re, gts))
    r["trainer_maccormack_us"], r["trainer_plain_us"] = alternated(trainers[0], trainers[1], max(3, REPS // 6))
    r["trainer_ratio"] = r["trainer_maccormack_us"] / r["trainer_plain_us"]
    r["trainer"] = {"net": "mars_moon3d", "msteps": ms, "use_graph": True}
    r["clocks"] = clocks()
    line = json.dumps(r)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "k3d_maccormack_time.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
