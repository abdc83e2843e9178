#!/usr/bin/env python
"""Does the Python layer of ANOTHER TREE of this package (an export of another commit) drive the 2-D Karman step to the SAME BITS and
the SAME LAUNCHES as this tree?  For a change of ops.py / torch_ops.py / trainer.py / karman.py that must not move a result.
    python tools/tree_bitcompare.py OTHER_ROOT [--suite 3d] [--own-libs] [--out verdicts.json]        (on the GPU box; --suite 3d: the 3-D step, child3d below)
Each tree is imported in a fresh child process from its own root, through the package's public names only (and _lib.profile for the
census); both load THIS tree's library (SOL_HIP_LIB), so the C sources of the two trees must be the same -- or, with --own-libs, each
tree loads the library built in its own tree: a change of the C sources that must leave these cases (the default paths) alone.  The cases come from the
tables of this tree's GPU tests (tests/buoyancy_cases.py: sphere_130 direct, two_144 cg and direct_scattered, B = 2) and one
one-workgroup grid, 32 x 16.  Per large-grid scene: force in {none, (0, 0), FORCES[1]} x advection in {semi_lagrangian, mac_cormack
s = 0.5} x diffusion_substeps in {1, 2}, each through karman_step_large under autograd (density_grad x re_grad x the cotangent sets
velocity / density / both / none) and through the direct calls karman_step_saved + karman_step_large_bwd / _bwd_re / _bwd_buoy +
karman_density_bwd / _re, plus torch.ops.sol.karman_step_adv / karman_step_bwd and the no-grad extras (feat, out, p_guess).  Per case:
the SHA-1 of every output and gradient, info's iteration counts and the kernel census (name -> launches) of the eager calls.
One verdict per case; exit status 1 if any differs."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 0.5
KINDS = ("vel", "dens", "both", "none")


def child(root):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, root)
    import torch
    import sol_amd
    from sol_amd import _lib, ops, torch_ops
    assert os.path.realpath(sol_amd.__file__).startswith(os.path.realpath(root) + os.sep), (sol_amd.__file__, root)
    import buoyancy_cases as bc
    import sol_oracle as o
    from large2d_scenes import CG_RTOL, f32, masks, state, cotangent_at
    from density_adjoint_cases import w_dens

    def sha(t):
        return None if t is None else hashlib.sha1(t.detach().float().cpu().numpy().tobytes()).hexdigest()[:16]

    def counts(info):
        return {k: v.tolist() for k, v in sorted(info.items())}

    out = {}

    def record(name, fn):
        """fn(info) -> tensors; the case's hashes, info's counts and the census of its launches"""
        info = {}
        torch.cuda.synchronize()
        with _lib.profile() as p:
            res = fn(info)
        out[name] = {"sha": [sha(t) for t in res], "info": counts(info), "census": {k: v[0] for k, v in sorted(p.kernels.items())}}

    def autograd_case(step, d, vy, vx, re, w, kind, re_grad):
        def fn(info):
            h = [t.clone().requires_grad_(True) for t in (d, vy, vx)] + [re.clone().requires_grad_(re_grad)]
            outs = step(*h, info)
            terms = [(a * b).sum() for a, b, use in zip(outs, w, (kind in ("dens", "both"), kind in ("vel", "both"), kind in ("vel", "both")))
                     if use and a.requires_grad]
            leaves = [t for t in h if t.requires_grad]
            g = torch.autograd.grad(sum(terms), leaves, allow_unused=True) if terms else [None] * len(leaves)
            return list(outs) + list(g)
        return fn

    def physics():
        for force in (None, (0.0, 0.0), bc.FORCES[1]):
            for adv in ({}, {"advection": "mac_cormack", "correction_strength": S}):
                for n in (1, 2):
                    yield "f%s_%s_n%d" % ("none" if force is None else "%g,%g" % force, "mc" if adv else "sl", n), force, adv, n

    for scene, solver in (("sphere_130", "direct"), ("two_144", "cg"), ("two_144", "direct_scattered")):
        Y, X, _, order, _ = bc.SCENES[scene]
        g = bc.geometry_of(scene)
        mk = masks(g, solver)
        cfg = ops.karman_cfg(bc.B, Y, X, g.dx, masks=mk, cg_rtol=CG_RTOL, inflow_order=order)
        d, vy, vx, re = (f32(t) for t in bc.start_state(scene))
        w = tuple(f32(t) for t in bc.cotangents(scene, "both"))
        pick = lambda kind: (w[0] if kind in ("dens", "both") else None, w[1] if kind in ("vel", "both") else None, w[2] if kind in ("vel", "both") else None)
        tag = "%s_%s/" % (scene, solver)
        for pname, force, adv, n in physics():
            kw = dict(buoyancy=force, diffusion_substeps=n, **adv)
            # karman_step_large under autograd
            for dg in (False, True):
                for rg in (False, True):
                    for kind in KINDS:
                        step = lambda a, b, c, r, info: ops.karman_step_large(a, b, c, r, cfg, mk, info=info, density_grad=dg, re_grad=rg, **kw)
                        record(tag + "autograd/%s/dens%d_re%d/%s" % (pname, dg, rg, kind), autograd_case(step, d, vy, vx, re, w, kind, rg))
            # the direct calls
            saved = {}

            def fwd(info):
                st, svy, svx = ops.karman_step_saved(d, vy, vx, re, cfg, mk, info=info, **kw)
                saved["v"] = (svy, svx)
                return st + (svy, svx)
            with torch.no_grad():
                record(tag + "direct/%s/saved" % pname, fwd)
                svy, svx = saved["v"]
                py, px = ops.karman_diffuse_sub(vy, vx, re, cfg, n)          # the input velocity the re adjoints take
                sc = ops.diffusion_sub_cfg(cfg, n)                           # the cfg the density adjoint's launches run on
                bkw = dict(diffusion_substeps=n, **adv)
                if force is None:
                    record(tag + "direct/%s/bwd" % pname, lambda info: ops.karman_step_large_bwd(svy, svx, re, w[1], w[2], cfg, mk, info=info, **bkw))
                    record(tag + "direct/%s/bwd_re" % pname,
                           lambda info: ops.karman_step_large_bwd_re(svy, svx, re, w[1], w[2], py, px, cfg, mk, info=info, **bkw))
                    if n == 1 and not adv:
                        record(tag + "direct/%s/bwd_re_accumulate" % pname,
                               lambda info: ops.karman_step_large_bwd_re(svy, svx, re, w[1], w[2], py, px, cfg, mk, g_re=torch.ones_like(re), info=info))
                    for acc in (False, True):
                        gv = lambda: [t.clone() for t in w[1:]] if acc else [None, None]
                        record(tag + "direct/%s/density_bwd_acc%d" % (pname, acc),
                               lambda info: ops.karman_density_bwd(d, svy, svx, re, w[0], sc, mk, *gv(), **adv))
                        record(tag + "direct/%s/density_bwd_re_acc%d" % (pname, acc),
                               lambda info: ops.karman_density_bwd_re(d, svy, svx, re, w[0], py, px, sc, mk, *gv(), torch.ones_like(re) if acc else None, **adv))
                else:
                    for kind in KINDS:
                        wd, wy, wx = pick(kind)
                        for vel_in in (None, (py, px)):
                            record(tag + "direct/%s/bwd_buoy_%s_re%d" % (pname, kind, vel_in is not None),
                                   lambda info: ops.karman_step_large_bwd_buoy(d, svy, svx, re, wy, wx, wd, cfg, mk, force, vel_in=vel_in, info=info, **bkw))
                # the no-grad extras
                feat = torch.zeros(bc.B, Y, X, 4, dtype=torch.float32, device=d.device)
                bufs = tuple(torch.zeros_like(t) for t in (d, vy, vx))
                record(tag + "nograd/%s/feat_out" % pname,
                       lambda info: ops.karman_step_large(d, vy, vx, re, cfg, mk, info=info, feat=feat, feat_scale=(5.0, 4.0, 1e-5), out=bufs, **kw) + (feat,))
                if solver == "cg":
                    guess = torch.zeros(bc.B, Y, X, dtype=torch.float32, device=d.device)
                    for k in range(2):          # cold guess, then the first call's pressure as the guess
                        record(tag + "nograd/%s/p_guess%d" % (pname, k),
                               lambda info: ops.karman_step_large(d, vy, vx, re, cfg, mk, info=info, p_guess=guess, **kw) + (guess,))
        # the torch.ops surface: the composition of everything once, and the velocity adjoint op
        h = torch_ops.register_scene(cfg, mk)
        fy, fx = bc.FORCES[1]
        step = lambda a, b, c, r, info: torch.ops.sol.karman_step_adv(a, b, c, r, h, 1, S, 2, True, True, fy, fx)
        record(tag + "torch_ops/karman_step_adv", autograd_case(step, d, vy, vx, re, w, "both", True))
        with torch.no_grad():
            _, svy, svx = ops.karman_step_saved(d, vy, vx, re, cfg, mk)
            record(tag + "torch_ops/karman_step_bwd", lambda info: torch.ops.sol.karman_step_bwd(svy, svx, re, w[1], w[2], h))

    # one one-workgroup grid
    Y, X, B = 32, 16, 2
    g = o.KarmanGeometry(Y, X)
    mk = masks(g)
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk)
    d, vy, vx, re = (f32(t) for t in state(B, Y, X, 11, g))
    w = (f32(w_dens(B, Y, X, g)),) + tuple(f32(t) for t in cotangent_at(B, Y, X))
    for n in (1, 3):
        for dg in (False, True):
            for rg in (False, True):
                for kind in KINDS:
                    step = lambda a, b, c, r, info: ops.karman_step(a, b, c, r, cfg, mk, info, density_grad=dg, re_grad=rg, diffusion_substeps=n)
                    record("small_32x16/autograd/n%d/dens%d_re%d/%s" % (n, dg, rg, kind), autograd_case(step, d, vy, vx, re, w, kind, rg))
        with torch.no_grad():
            record("small_32x16/nograd/n%d" % n, lambda info: ops.karman_step(d, vy, vx, re, cfg, mk, info, diffusion_substeps=n))
            def fwd(info):
                st, svy, svx = ops.karman_step_saved(d, vy, vx, re, cfg, mk, info=info, diffusion_substeps=n)
                return st + (svy, svx)
            record("small_32x16/saved/n%d" % n, fwd)
    h = torch_ops.register_scene(cfg, mk)
    for op, args in (("karman_step", ()), ("karman_step_dens", ()), ("karman_step_re", (True,)), ("karman_step_sub", (3, True, True))):
        step = lambda a, b, c, r, info: getattr(torch.ops.sol, op)(a, b, c, r, h, *args)
        record("small_32x16/torch_ops/" + op, autograd_case(step, d, vy, vx, re, w, "both", True))
    with torch.no_grad():
        _, svy, svx = ops.karman_step_saved(d, vy, vx, re, cfg, mk)
        record("small_32x16/torch_ops/karman_step_bwd", lambda info: torch.ops.sol.karman_step_bwd(svy, svx, re, w[1], w[2], h))
    print(json.dumps(out))


def child3d(root):
    """--suite 3d: the same question for the 3-D step (karman3d.py / torch_ops.py).  Scenes: tests/karman3d_adjoint_cases.py 16_comb (B = 2,
    16 x 8 x 8, direct), diffusion_substeps3d_cases.CG_CASE's wall mask at that shape with the CG solve, and 20_comb (B = 1, 20 x 10 x 10).
    Per scene, force in {none, (0, 0, 0), FORCES[1]} x diffusion_substeps in {1, 3}: Karman3DFlow.step under autograd (density_grad x
    re_grad x the cotangent sets), the direct calls as the tests make them (_fwd / _fwd_sub with `saved`, _bwd with and without vel_in /
    g_re / buoyancy / g_d, density_bwd with and without g_v / vel_in / g_re), every torch.ops.sol.karman3d_step* op with and without a
    gradient and karman3d_density_bwd, the fused feature output, two steps of Karman3DRollout (the 16 x 8 x 8 scenes); then one Karman3DTrainer.fwd_bwd at
    buoyancy3d_cases.TRAINER_SHAPE (msteps = 2, the golden weights) for both schedules x force x substeps, eager, and one use_graph replay
    of the manual schedule (hashes only: a capture takes no per-launch events).  Per case: SHA-1s, solve_info's counts, kernel census."""
    for p in (os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), root):
        sys.path.insert(0, p)
    import torch
    import sol_amd
    from sol_amd import _lib, torch_ops
    from sol_amd import karman3d as k3
    assert os.path.realpath(sol_amd.__file__).startswith(os.path.realpath(root) + os.sep), (sol_amd.__file__, root)
    import buoyancy3d_cases as bc
    import diffusion_substeps3d_cases as dc
    import make_golden as mg
    import sol_oracle3d as o
    from large2d_scenes import DEV, f32

    ZERO, STD_V = (0.0, 0.0, 0.0), (0.2, 0.25, 0.3)
    out = {}

    def sha(t):
        return None if t is None else hashlib.sha1(t.detach().float().cpu().numpy().tobytes()).hexdigest()[:16]

    def record(name, fn, sims=(), census=True):
        """fn() -> tensors; the case's hashes, the solve_info counts of `sims` and the census of its launches"""
        for s in sims:
            s.solve_info = {}
        torch.cuda.synchronize()
        if census:
            with _lib.profile() as p:
                res = fn()
                torch.cuda.synchronize()
        else:
            res = fn()
            torch.cuda.synchronize()
        assert name not in out, name
        out[name] = {"sha": [sha(t) for t in res], "info": {"%d.%s" % (i, k): v.tolist() for i, s in enumerate(sims) for k, v in sorted(s.solve_info.items())},
                     "census": {k: v[0] for k, v in sorted(p.kernels.items())} if census else {}}

    def autograd_case(step, st, w, kind, re_grad):
        def fn():
            h = [t.clone().requires_grad_(True) for t in st[:4]] + [st[4].clone().requires_grad_(re_grad)]
            outs = step(*h)
            use = (kind in ("dens", "both"),) + (kind in ("vel", "both"),) * 3
            terms = [(a * b).sum() for a, b, u in zip(outs, w, use) if u and a.requires_grad]
            leaves = [t for t in h if t.requires_grad]
            g = torch.autograd.grad(sum(terms), leaves, allow_unused=True) if terms else [None] * len(leaves)
            return list(outs) + list(g)
        return fn

    def golden_net():
        net = k3.MarsMoon3D(device=DEV)
        net.set_weights([q.detach().numpy() for q in mg.k3d_params()])
        return net

    for name in ("16_comb", dc.CG_CASE[0], "20_comb"):
        c = dc.case(name)
        wall = name == dc.CG_CASE[0]
        B, Y, X, Z = c["shape"]
        g = dc.geometry(name)
        scene = k3.Scene3D(Y, X, Z, device=DEV, active=g.active, inflow=g.inflow, pressure_solver="cg" if wall else "auto")
        d, v, re = dc.state(name)
        st = tuple(f32(t) for t in (d, *v, re))
        w = tuple(f32(t) for t in (dc.w_dens(name), *dc.w_vel(name)))
        wd, wv = w[0], w[1:]
        ones = lambda: torch.ones(B, dtype=torch.float32, device=DEV)
        for force, n in ((f, n) for f in (None, ZERO, bc.FORCES[1]) for n in (1, 3)):
            tag = "%s/f%s_n%d/" % (name, "none" if force is None else "%g,%g,%g" % force, n)
            mk = lambda **kw: k3.Karman3DFlow(scene, B, dt=c["dt"], buoyancy=force, diffusion_substeps=n, cg_rtol=1e-7, **c["kw"], **kw)
            for dg in (False, True):
                for rg in (False, True):
                    sim = mk(density_grad=dg, re_grad=rg)
                    for kind in KINDS:
                        record(tag + "autograd/dens%d_re%d/%s" % (dg, rg, kind), autograd_case(sim.step, st, w, kind, rg), [sim])
            # the direct calls, on a simulator without physics of its own: the force and the count are named per call
            plain = k3.Karman3DFlow(scene, B, dt=c["dt"], cg_rtol=1e-7, **c["kw"])
            fkw = {} if force is None else {"buoyancy": force}
            with torch.no_grad():
                vel = k3.diffuse_sub(plain, *st[1:4], st[4], n)
                saved, saved2 = ([torch.empty_like(t) for t in vel] for _ in range(2))
                record(tag + "direct/fwd", lambda: plain._fwd(st[0], *vel, st[4], saved, nsub=n, **fkw) + tuple(saved), [plain])
                record(tag + "direct/fwd_sub", lambda: plain._fwd_sub(*st, saved2, nsub=n, **fkw) + tuple(saved2), [plain])
                record(tag + "direct/bwd", lambda: plain._bwd(saved, st[4], *wv, nsub=n), [plain])
                record(tag + "direct/bwd_re", lambda: plain._bwd(saved, st[4], *wv, vel_in=vel, nsub=n), [plain])
                record(tag + "direct/bwd_re_acc", lambda: plain._bwd(saved, st[4], *wv, vel_in=vel, g_re=ones(), nsub=n), [plain])
                if force is not None:
                    for gd, vin in ((None, None), (wd, None), (None, vel), (wd, vel)):
                        record(tag + "direct/bwd_buoy_gd%d_re%d" % (gd is not None, vin is not None),
                               lambda: plain._bwd(saved, st[4], *wv, vel_in=vin, buoyancy=force, g_d=gd, nsub=n), [plain])
                gv = lambda: [t.clone() for t in wv]
                record(tag + "direct/density_bwd", lambda: k3.density_bwd(plain, st[0], saved, st[4], wd, nsub=n), [plain])
                record(tag + "direct/density_bwd_acc", lambda: k3.density_bwd(plain, st[0], saved, st[4], wd, g_v=gv(), nsub=n), [plain])
                record(tag + "direct/density_bwd_re", lambda: k3.density_bwd(plain, st[0], saved, st[4], wd, vel_in=vel, nsub=n), [plain])
                record(tag + "direct/density_bwd_re_acc",
                       lambda: k3.density_bwd(plain, st[0], saved, st[4], wd, g_v=gv(), vel_in=vel, g_re=ones(), nsub=n), [plain])
            # the torch.ops surface on a simulator with this physics (the first three run its count and no force)
            sim = mk()
            h = torch_ops.register_scene3d(sim)
            f = ZERO if force is None else force
            t3 = torch.ops.sol
            for op, step in (("karman3d_step", lambda *a: t3.karman3d_step(*a, h)), ("karman3d_step_dens", lambda *a: t3.karman3d_step_dens(*a, h)),
                             ("karman3d_step_re", lambda *a: t3.karman3d_step_re(*a, h, True)),
                             ("karman3d_step_buoy", lambda *a: t3.karman3d_step_buoy(*a, h, *f, True)),
                             ("karman3d_step_sub", lambda *a: t3.karman3d_step_sub(*a, h, n, True, True, *f))):
                record(tag + "torch_ops/%s/grad" % op, autograd_case(step, st, w, "both", True), [sim])
                with torch.no_grad():
                    record(tag + "torch_ops/%s/nograd" % op, lambda: step(*st), [sim])
            with torch.no_grad():
                record(tag + "torch_ops/karman3d_density_bwd", lambda: t3.karman3d_density_bwd(st[0], *saved, st[4], wd, h), [sim])
                feat = torch.zeros(B, Y, X, Z, 4, dtype=torch.float32, device=DEV)
                record(tag + "nograd/feat_out", lambda: sim.step(*st, feat_out=feat, feat_scale=(5.0, 4.0, 3.0, 1e-5)) + (feat,), [sim])
                if Z % 8 == 0:                                      # (the network's thin-layer launches refuse 20 x 10 x 10)
                    ro = k3.Karman3DRollout(golden_net(), scene, B, STD_V, o.STD_RE, dt=c["dt"], buoyancy=force, diffusion_substeps=n, cg_rtol=1e-7, **c["kw"])
                    record(tag + "rollout/two_steps", lambda: ro.step(*ro.step(*st[:4], st[4]), st[4]), [ro.sim])

    # the trainer
    p = bc.trainer_problem()
    B, Y, X, Z = bc.TRAINER_SHAPE
    scene = k3.Scene3D(Y, X, Z, device=DEV)

    def trainer_case(schedule, force, n, use_graph):
        tr = k3.Karman3DTrainer(golden_net(), scene, B, 2, bc.TRAINER_STD_V, o.STD_RE, use_graph=use_graph, schedule=schedule, buoyancy=force,
                                diffusion_substeps=n)

        def fn():
            for _ in range(2 if use_graph else 1):                  # (graph: the second call is a pure replay)
                tr._grads.zero_()
                loss = tr.fwd_bwd(p["d"], *p["v"], p["re"], p["gts"])
            return [loss.clone(), tr.loss_steps.clone(), tr.grads.clone()] + [t.clone() for t in tr.final]
        record("trainer/%s/f%d_n%d%s" % (schedule, force is not None, n, "/graph" if use_graph else ""), fn, [tr.sim], census=not use_graph)

    for schedule in ("manual", "autograd"):
        for force in (None, bc.TRAINER_FORCE):
            for n in (1, 3):
                trainer_case(schedule, force, n, False)
    trainer_case("manual", bc.TRAINER_FORCE, 3, True)
    print(json.dumps(out))


def main():
    args = sys.argv[1:]
    dst = None
    if "--out" in args:
        k = args.index("--out")
        dst = args[k + 1]
        del args[k:k + 2]
    suite = "2d"
    if "--suite" in args:
        k = args.index("--suite")
        suite = args[k + 1]
        del args[k:k + 2]
    own_libs = "--own-libs" in args          # each tree loads the library built in ITS tree: for a change of the C sources that must not move
    if own_libs:                             # the cases of this tool (the default paths); the other tree's library must have been built
        args.remove("--own-libs")
    if len(args) != 1 or suite not in ("2d", "3d"):
        sys.exit(__doc__)
    other = os.path.abspath(args[0])
    env = dict(os.environ, SOL_HIP_LIB=os.path.join(ROOT, "solver-in-the-loop_amd", "lib", "libsol_hip.so"))
    if own_libs:
        del env["SOL_HIP_LIB"]
    res = {}
    for name, root in (("other", other), ("this", ROOT)):
        o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child" if suite == "2d" else "--child3d", root], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if o.returncode != 0:
            print(o.stdout[-1500:], o.stderr[-3000:])
            sys.exit("the child of the %s tree (%s) failed" % (name, root))
        res[name] = json.loads(o.stdout.strip().splitlines()[-1])
        print("%s tree: %d cases" % (name, len(res[name])), flush=True)
    cases = sorted(set(res["other"]) | set(res["this"]))
    verdicts = {c: "identical" if res["other"].get(c) == res["this"].get(c) else "DIFFERS" for c in cases}
    bad = [c for c in cases if verdicts[c] != "identical"]
    for c in bad:
        print("DIFFERS %s\n   other %s\n   this  %s" % (c, json.dumps(res["other"].get(c)), json.dumps(res["this"].get(c))))
    launches = sum(sum(v["census"].values()) for v in res["this"].values())
    summary = {"tool": "tree_bitcompare", "suite": suite, "cases": len(cases), "identical": len(cases) - len(bad), "differs": bad,
               "launches_compared": launches, "verdicts": verdicts}
    print("%d cases, %d identical (sha of every output and gradient, info counts, kernel census), %d differ" % (len(cases), len(cases) - len(bad), len(bad)))
    if dst is not None:
        with open(dst, "w") as f:
            json.dump(summary, f, indent=1, sort_keys=True)
            f.write("\n")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    if "--child" in sys.argv:
        child(sys.argv[sys.argv.index("--child") + 1])
    elif "--child3d" in sys.argv:
        child3d(sys.argv[sys.argv.index("--child3d") + 1])
    else:
        main()
