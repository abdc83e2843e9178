#!/usr/bin/env python
"""Host cost of the karman-3d step's Python layer, this tree against ANOTHER TREE (an export of another commit) on one library: for a
change of karman3d.py / torch_ops.py that moves no kernel, only the eager calls can move (a captured trainer replays a graph and never
sees the Python layer).
    python tools/k3d_step_physics_time.py OTHER_ROOT [rounds] [--own-libs] [--out profiles/k3d_step_physics_refactor_speed.json]      (on the GPU box)
Per round one fresh process per tree, the other tree first, alternating; both load THIS tree's library (SOL_HIP_LIB) -- with --own-libs
each tree loads the library built in its own tree (a change that touches the C sources' default path).  Each process
times, on karman3d_adjoint_cases' 16_comb scene (B = 2, 16 x 8 x 8) and at 32 x 16 x 16 with B = 1 (the default sphere, direct solve):
the no-grad Karman3DFlow.step; step + backward in the plain, the density_grad + re_grad and the buoyant diffusion_substeps = 3 modes;
one eager manual Karman3DTrainer.fwd_bwd (msteps = 2).  A host clock around CALLS calls that end in a device synchronise, the median of
WINDOWS windows per process.  Per metric: every round's figure of both trees, the other tree's own max - min as the margin, and whether
this tree's median exceeds the other's by no more than it.  No threshold is built in: the file records what was measured."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"16x8x8_B2": (2, 16, 8, 8), "32x16x16_B1": (1, 32, 16, 16)}
FORCE = (0.3, -0.2, 0.15)
CALLS, WINDOWS, WARM = 20, 7, 2


def child(root):
    for p in (os.path.join(ROOT, "oracle"), root):
        sys.path.insert(0, p)
    import torch
    import sol_amd
    import sol_oracle3d as o
    from sol_amd import karman3d as k3
    assert os.path.realpath(sol_amd.__file__).startswith(os.path.realpath(root) + os.sep), (sol_amd.__file__, root)
    f32 = lambda t: t.to(device="cuda", dtype=torch.float32).contiguous()

    def timed(fn):
        ts = []
        for it in range(WARM + WINDOWS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            torch.cuda.synchronize()
            if it >= WARM:
                ts.append((time.perf_counter() - t0) * 1e6 / CALLS)
        return statistics.median(ts)

    res = {}
    for tag, (B, Y, X, Z) in SHAPES.items():
        scene = k3.Scene3D(Y, X, Z, device="cuda")
        d, v = o.synthetic_state(B, Y, X, Z, 13)
        st = [f32(t) for t in (d, *v)] + [f32(torch.tensor(o.RE_TRAIN[:B]))]
        w = [torch.randn_like(t) for t in st[:4]]

        def step_bwd(sim, re_grad):
            def fn():
                h = [t.clone().requires_grad_(True) for t in st[:4]] + [st[4].clone().requires_grad_(re_grad)]
                out = sim.step(*h)
                terms = [(a * b).sum() for a, b in zip(out, w) if a.requires_grad]
                torch.autograd.grad(sum(terms), [t for t in h if t.requires_grad], allow_unused=True)
            return fn

        plain = k3.Karman3DFlow(scene, B)
        with torch.no_grad():
            res[tag + ":step_nograd_us"] = timed(lambda: plain.step(*st))
        res[tag + ":step_bwd_plain_us"] = timed(step_bwd(plain, False))
        res[tag + ":step_bwd_density_re_us"] = timed(step_bwd(k3.Karman3DFlow(scene, B, density_grad=True, re_grad=True), True))
        res[tag + ":step_bwd_buoyant_n3_us"] = timed(step_bwd(k3.Karman3DFlow(scene, B, buoyancy=FORCE, diffusion_substeps=3), False))
        tr = k3.Karman3DTrainer(k3.MarsMoon3D(seed=4, device="cuda"), scene, B, 2, (0.2, 0.25, 0.3), o.STD_RE)
        gts = [tuple(f32(c) for c in o.synthetic_state(B, Y, X, Z, 500 + i)[1]) for i in range(2)]
        res[tag + ":trainer_fwd_bwd_manual_us"] = timed(lambda: tr.fwd_bwd(*st, gts))
    print(json.dumps(res))


def main():
    args = sys.argv[1:]
    dst = None
    if "--out" in args:
        k = args.index("--out")
        dst = args[k + 1]
        del args[k:k + 2]
    own_libs = "--own-libs" in args          # each tree loads the library built in ITS tree: a change of the C sources whose default path must
    if own_libs:                             # cost what it did (the other tree's library must have been built)
        args.remove("--own-libs")
    if not 1 <= len(args) <= 2:
        sys.exit(__doc__)
    other, rounds = os.path.abspath(args[0]), int(args[1]) if len(args) > 1 else 6
    env = dict(os.environ, SOL_HIP_LIB=os.path.join(ROOT, "solver-in-the-loop_amd", "lib", "libsol_hip.so"))
    if own_libs:
        del env["SOL_HIP_LIB"]
    runs = {"other": {}, "this": {}}
    for r in range(rounds):
        for name, root in (("other", other), ("this", ROOT)):
            o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            if o.returncode != 0:
                print(o.stdout[-1500:], o.stderr[-3000:])
                sys.exit("the child of the %s tree (%s) failed" % (name, root))
            for k, t in json.loads(o.stdout.strip().splitlines()[-1]).items():
                runs[name].setdefault(k, []).append(t)
        print("round %d done" % (r + 1), flush=True)
    metrics, outside = {}, []
    for k in sorted(runs["this"]):
        a, b = runs["other"][k], runs["this"][k]
        margin = max(a) - min(a)
        inside = statistics.median(b) - statistics.median(a) <= margin
        metrics[k] = {"other": a, "this": b, "other_median": statistics.median(a), "this_median": statistics.median(b), "other_margin": margin, "inside": inside}
        outside += [] if inside else [k]
        print("%-44s other %9.1f us  this %9.1f us  margin %7.1f  %s" % (k, statistics.median(a), statistics.median(b), margin, "inside" if inside else "OUTSIDE"))
    summary = {"tool": "tools/k3d_step_physics_time.py", "rounds": rounds, "calls_per_window": CALLS, "windows_per_process": WINDOWS,
               "method": __doc__.split("\n", 5)[5], "outside_margin": outside, "metrics": metrics}
    if dst is not None:
        with open(dst, "w") as f:
            json.dump(summary, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    if "--child" in sys.argv:
        child(sys.argv[sys.argv.index("--child") + 1])
    else:
        main()
