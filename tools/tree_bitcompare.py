#!/usr/bin/env python
"""Does the Python layer of ANOTHER TREE of this package (an export of another commit) drive the 2-D Karman step to the SAME BITS and
the SAME LAUNCHES as this tree?  For a change of ops.py / torch_ops.py / trainer.py / karman.py that must not move a result.
    python tools/tree_bitcompare.py OTHER_ROOT [--out verdicts.json]        (on the GPU box)
Each tree is imported in a fresh child process from its own root, through the package's public names only (and _lib.profile for the
census); both load THIS tree's library (SOL_HIP_LIB), so the C sources of the two trees must be the same.  The cases come from the
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


def main():
    args = sys.argv[1:]
    dst = None
    if "--out" in args:
        k = args.index("--out")
        dst = args[k + 1]
        del args[k:k + 2]
    if len(args) != 1:
        sys.exit(__doc__)
    other = os.path.abspath(args[0])
    env = dict(os.environ, SOL_HIP_LIB=os.path.join(ROOT, "solver-in-the-loop_amd", "lib", "libsol_hip.so"))
    res = {}
    for name, root in (("other", other), ("this", ROOT)):
        o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
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
    summary = {"tool": "tree_bitcompare", "cases": len(cases), "identical": len(cases) - len(bad), "differs": bad,
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
    else:
        main()
