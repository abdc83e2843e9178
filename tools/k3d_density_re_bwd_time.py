#!/usr/bin/env python
"""karman-3d density adjoint and Reynolds-number gradient: what they add to a backward pass, one JSON line, also written to
profiles/k3d_density_re_bwd_time.json.

At 128 x 64 x 64, B = 1, the default sphere (direct solve), in ONE process and on a spun-up state, HIP events around eager calls: the plain
velocity adjoint (sol_karman3d_step_bwd, the code path that exists without the opt-in flags), sol_karman3d_step_bwd_re, the density adjoint
alone (karman3d.density_bwd on the saved state with a fixed random cotangent) with both scatter forms (LDS window, option
k3d_dens_adj_tile = 1, and global atomics only) and its _re form; and the kernel split of the density adjoint with the reduction
(sol_prof_begin / sol_prof_end: device time per kernel, us per call).  No threshold: the file records what was measured, on whatever clock
the box held; compare the new calls to the velocity adjoint of the same file and to nothing else.

--parent LIB: a library built from the parent commit (tools/ab_lib.py builds variants the same way).  The plain sol_karman3d_step_bwd is
then timed alternately through this build and through LIB in the same process ("parent_ab": rounds of (this, parent) us and the medians):
the default path launches the same kernels, so the two agree within the alternation's own spread unless an existing kernel was touched.
Usage: python tools/k3d_density_re_bwd_time.py [reps] [--parent LIB]"""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch          # noqa: E402
from sol_amd import _lib   # noqa: E402
from sol_amd import karman3d as k3   # noqa: E402
from sol_amd._lib import ptr, stream   # noqa: E402

ARGS = [a for a in sys.argv[1:]]
PARENT = None
if "--parent" in ARGS:
    i = ARGS.index("--parent")
    PARENT = ARGS[i + 1]
    ARGS = ARGS[:i] + ARGS[i + 2:]
REPS = int(ARGS[0]) if ARGS else 30
DEV = "cuda"
Y, X, Z, B = 128, 64, 64, 1
ROUNDS = 7


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


def main():
    sc = k3.Scene3D(Y, X, Z, device=DEV)
    sim = k3.Karman3DFlow(sc, B, density_grad=True, re_grad=True)
    re = torch.full((B,), 1.6e5, device=DEV)
    gen = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=gen)
    st = (torch.rand(B, Y, X, Z, generator=gen).to(DEV), (1.0 + 0.1 * rn(B, Y + 1, X, Z)).to(DEV), (0.1 * rn(B, Y, X + 1, Z)).to(DEV),
          (0.1 * rn(B, Y, X, Z + 1)).to(DEV))
    with torch.no_grad():
        for _ in range(2):                                                   # spun-up state
            st = sim.step(*st, re)
        saved = [torch.empty_like(t) for t in st[1:]]
        sim._fwd(*st, re, saved)
    gen = torch.Generator().manual_seed(3)
    wd = torch.randn(B, Y, X, Z, generator=gen).to(DEV)
    wv = [torch.randn(t.shape, generator=gen).to(DEV) for t in saved]
    vel_in = list(st[1:])
    vel = lambda: sim._bwd(saved, re, *wv)
    vel_re = lambda: sim._bwd(saved, re, *wv, vel_in=vel_in)
    dens = lambda: k3.density_bwd(sim, st[0], saved, re, wd)
    dens_re = lambda: k3.density_bwd(sim, st[0], saved, re, wd, vel_in=vel_in)
    dens_re()                                                                # (grows the workspace once, outside the timed calls)
    vel_re()
    r = {"tool": "k3d_density_re_bwd_time", "reps": REPS, "device": torch.cuda.get_device_name(0), "solver": sc.pressure_solver,
         "grid": [Y, X, Z], "B": B}
    r["step_bwd_us"] = timed(vel, REPS)
    r["step_bwd_re_us"] = timed(vel_re, REPS)
    r["density_bwd_us"] = timed(dens, REPS)
    r["density_bwd_re_us"] = timed(dens_re, REPS)
    _lib.set_option("k3d_dens_adj_tile", 0)
    try:
        r["density_bwd_global_atomics_us"] = timed(dens, REPS)
    finally:
        _lib.set_option("k3d_dens_adj_tile", 1)
    r["step_bwd_again_us"] = timed(vel, REPS)                                # the yardstick once more: did the box move meanwhile?
    for key in ("step_bwd_re", "density_bwd", "density_bwd_re", "density_bwd_global_atomics"):
        r[key + "_over_step_bwd"] = round(r[key + "_us"] / r["step_bwd_us"], 4)
    torch.cuda.synchronize()
    preps = min(REPS, 30)                                                    # (every launch carries two events)
    with _lib.profile() as p:
        for _ in range(preps):
            dens_re()
    r["density_bwd_re_kernels_us"] = {k: round(v[1] / preps, 3) for k, v in sorted(p.kernels.items(), key=lambda kv: -kv[1][1])}
    r["density_bwd_re_launches"] = int(sum(v[0] for v in p.kernels.values()) // preps)
    r["parent_ab"] = None
    if PARENT:
        # the parent commit's library beside this one in the same process: the plain adjoint through both, alternately, same buffers
        plib = C.CDLL(os.path.abspath(PARENT))
        for name in ("sol_karman3d_step_bwd", "sol_karman3d_step_bwd_workspace_bytes"):
            getattr(plib, name).restype, getattr(plib, name).argtypes = _lib._SIGS[name]
        nb = plib.sol_karman3d_step_bwd_workspace_bytes(C.byref(sim.cfg))
        ws = torch.empty((nb + 3) // 4, dtype=torch.float32, device=DEV)
        gi = [torch.empty_like(t) for t in saved]
        hdr = sc.direct_header.ctypes.data_as(C.c_void_p)

        def through(lib):
            def call():
                rc = lib.sol_karman3d_step_bwd(C.byref(sim.cfg), stream(), ptr(saved[0]), ptr(saved[1]), ptr(saved[2]), ptr(re), ptr(sc.active),
                                               ptr(sc.velBCyMask), sc.bc_stride, ptr(wv[0]), ptr(wv[1]), ptr(wv[2]), ptr(gi[0]), ptr(gi[1]), ptr(gi[2]),
                                               hdr, ptr(ws), nb)
                assert rc == 0
            return call

        this, parent = through(sim.lib), through(plib)
        this()
        mine = [t.clone() for t in gi]
        parent()
        torch.cuda.synchronize()
        same = all(torch.equal(a, b) for a, b in zip(mine, gi))
        rounds = [(timed(this, REPS), timed(parent, REPS)) for _ in range(ROUNDS)]
        a, b = [x[0] for x in rounds], [x[1] for x in rounds]
        r["parent_ab"] = {"rounds_us": [[round(x, 2), round(y, 2)] for x, y in rounds], "this_median_us": round(statistics.median(a), 2),
                          "parent_median_us": round(statistics.median(b), 2), "this_spread_us": round(max(a) - min(a), 2),
                          "parent_spread_us": round(max(b) - min(b), 2), "gradients_bit_equal": bool(same)}
    line = json.dumps(r)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "k3d_density_re_bwd_time.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
