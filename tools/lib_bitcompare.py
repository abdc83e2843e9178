#!/usr/bin/env python
"""Does a library variant (tools/ab_lib.py --build NAME ...) compute the SAME BITS as the product library?  Two karman-2d training steps
(loss, gradient, final state), the CG pressure solves (the 2-D large step eager and replayed, its solve alone, the 3-D step and its
adjoint: fields and cg_info) and the adjoints' fixed-point scatter with the LDS window and with global atomics only (the 2-D large-grid
adjoint, direct on the default sphere and CG on two cylinders, B = 2; the 3-D direct-solve adjoint at 128 x 64 x 64, B = 1) and every
host path that sizes and carves a workspace at the smallest shapes of the GPU tests (the large-grid 2-D step through its six forward entry
points and its adjoints with each solver, the Burgers large step and adjoint, the 3-D density and Re adjoints) per library in fresh processes (SOL_HIP_LIB), SHA-1 of every result, one verdict per leg.
    python tools/lib_bitcompare.py NAME [NAME2 ...]        (on the GPU box)"""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--child" in sys.argv:
    sys.path.insert(0, ROOT)
    import torch
    import sol_amd
    import bench
    dev = torch.device("cuda", 0)
    sha = lambda t: hashlib.sha1(t.detach().float().cpu().numpy().tobytes()).hexdigest()[:16]
    out = {}
    for (B, Y, X, ms) in ((6, 128, 64, 32), (3, 64, 32, 4)):
        wl = bench.Workload(sol_amd, dev, B, Y, X, ms, 0, use_graph=False)
        tr = wl.trainer
        loss = tr.fwd_bwd(wl.d0, wl.vy0, wl.vx0, wl.re, wl.gt_vy, wl.gt_vx, want_final=True)
        torch.cuda.synchronize()
        g = tr.grads
        g = torch.cat([t.flatten() for t in g]) if isinstance(g, (list, tuple)) else g
        out["%dx%dx%d_ms%d" % (B, Y, X, ms)] = {"loss": float(loss).hex(), "grad": sha(g), "final": [sha(t) for t in tr.final]}
    # the CG pressure solves (csrc/pcg.hip): the 2-D large step on two cylinders eager and replayed from a graph, its solve alone,
    # and the 3-D cylinder forward + adjoint step
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import sol_oracle3d as o3
    from sol_amd import fluid, karman, karman3d, ops
    B, Y, X = 2, 256, 128
    dom = fluid.Domain([Y, X], box=fluid.box[0:200, 0:100])
    active, inflow = karman.KarmanFlow(obstacles=karman.parse_obstacles(["sphere:50,50,10", "sphere:120,50,10"])).scene_arrays(dom)
    bc = karman.velocity_bc_masks(Y, X)[0].reshape(Y + 1, X)
    mk = ops.SceneMasks(active, inflow, bc, bc, dev, pressure_solver="cg")
    cfg = ops.karman_cfg(B, Y, X, dom.dx[1], masks=mk, cg_max_iter=600)
    gen = torch.Generator().manual_seed(1)
    d0, vy0, vx0 = (t.to(dev) for t in (torch.rand(B, Y, X, generator=gen), 1.0 + 0.1 * torch.randn(B, Y + 1, X, generator=gen),
                                        0.1 * torch.randn(B, Y, X + 1, generator=gen)))
    re = torch.full((B,), 1.6e5, device=dev)
    ws = torch.empty((ops.large_workspace_bytes(cfg, mk) + 3) // 4, dtype=torch.float32, device=dev)
    cg = lambda outs, info: [sha(t) for t in outs] + [info["iterations"].tolist(), info["converged"].tolist()]
    with torch.no_grad():
        d, vy, vx = ops.karman_step_large(d0, vy0, vx0, re, cfg, mk, ws)         # spun up: divergence free, in the scene
        info = {}
        out["cg2d_step_eager"] = cg(ops.karman_step_large(d, vy, vx, re, cfg, mk, ws, info), info)
        s, gr, info = torch.cuda.Stream(), torch.cuda.CUDAGraph(), {}
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.cuda.graph(gr, stream=s):
            outs = ops.karman_step_large(d, vy, vx, re, cfg, mk, ws, info)
        torch.cuda.current_stream().wait_stream(s)
        gr.replay()
        torch.cuda.synchronize()
        out["cg2d_step_replayed"] = cg(outs, info)
        info = {}
        rhs = -((vy0[:, 1:] - vy0[:, :-1]) + (vx0[:, :, 1:] - vx0[:, :, :-1]))   # -div of the unprojected field
        out["cg2d_solve"] = cg([ops.pressure_solve_large(rhs, cfg, mk, info=info)], info)
    B, Y, X, Z = 2, 32, 16, 16
    g3 = o3.geometry(Y, X, Z, obstacle="cylinder")
    sim = karman3d.Karman3DFlow(karman3d.Scene3D(Y, X, Z, device=dev, active=g3.active, inflow=g3.inflow, pressure_solver="cg"), B)
    d, v = o3.synthetic_state(B, Y, X, Z, 41)
    v = [t.float().to(dev).requires_grad_(True) for t in v]
    outs = sim.step(d.float().to(dev), *v, torch.tensor(o3.RE_TRAIN[:B], dtype=torch.float32, device=dev))
    sum((t * (k + 1.0)).sum() for k, t in enumerate(outs[1:])).backward()
    out["cg3d_fwd_adjoint"] = [sha(t) for t in list(outs) + [t.grad for t in v]] + \
        [sim.solve_info[k].tolist() for k in ("iterations", "converged", "iterations_bwd", "converged_bwd")]
    # the fixed-point scatter of the adjoints (csrc/fixed_scatter.hpp), both forms of each: input gradients (and iterations_bwd with CG)
    from sol_amd import _lib

    def tiled(option, fn):
        res = []
        for tile in (1, 0):
            _lib.set_option(option, tile)
            try:
                res.append(fn())
            finally:
                _lib.set_option(option, 1)
        return res

    def adjoint2d(specs):
        B, Y, X = 2, 256, 128
        dom = fluid.Domain([Y, X], box=fluid.box[0:200, 0:100])
        active, inflow = karman.KarmanFlow(obstacles=None if specs is None else karman.parse_obstacles(specs)).scene_arrays(dom)
        bc = karman.velocity_bc_masks(Y, X)[0].reshape(Y + 1, X)
        mk = ops.SceneMasks(active, inflow, bc, bc, dev)
        cfg = ops.karman_cfg(B, Y, X, dom.dx[1], masks=mk, cg_max_iter=600)
        with torch.no_grad():
            st = ops.karman_step_large(d0, vy0, vx0, re, cfg, mk)               # spun up in this scene
        gen = torch.Generator().manual_seed(3)
        w = [torch.randn(t.shape, generator=gen).to(dev) for t in st[1:]]

        def run():
            v, info = [t.clone().requires_grad_(True) for t in st[1:]], {}
            outs = ops.karman_step_large(st[0], v[0], v[1], re, cfg, mk, info=info)
            g = torch.autograd.grad(outs[1:], v, w)
            return [mk.pressure_solver] + [sha(t) for t in g] + ([info["iterations_bwd"].tolist()] if "iterations_bwd" in info else [])
        return tiled("k2d_adj_tile", run)
    out["adj2d_sphere_direct"] = adjoint2d(None)
    out["adj2d_two_cylinders_cg"] = adjoint2d(["sphere:50,50,10", "sphere:120,50,10"])

    B, Y, X, Z = 1, 128, 64, 64
    sim = karman3d.Karman3DFlow(karman3d.Scene3D(Y, X, Z, device=dev, pressure_solver="direct"), B)
    d, v3 = o3.synthetic_state(B, Y, X, Z, 41)
    re3 = torch.tensor(o3.RE_TRAIN[:B], dtype=torch.float32, device=dev)
    with torch.no_grad():
        st3 = sim.step(d.float().to(dev), *(t.float().to(dev) for t in v3), re3)
    gen = torch.Generator().manual_seed(3)
    w3 = [torch.randn(t.shape, generator=gen).to(dev) for t in st3[1:]]

    def run3d():
        v = [t.clone().requires_grad_(True) for t in st3[1:]]
        outs = sim.step(st3[0], *v, re3)
        return [sha(t) for t in torch.autograd.grad(outs[1:], v, w3)]
    out["adj3d_direct_128x64x64"] = tiled("k3d_adj_tile", run3d)

    # every host path that sizes and carves a workspace (csrc/carve.hpp), at the smallest shapes of the GPU tests (tests/buoyancy_cases.py,
    # tests/karman3d_adjoint_cases.py, test_gpu_burgers_large_adjoint.py): the six forward entry points of the large-grid 2-D step with
    # each solver, the velocity, density and Re adjoints, the Burgers large step and adjoint, the 3-D density and Re adjoints
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import buoyancy_cases as bc
    import karman3d_adjoint_cases as kc
    from large2d_scenes import CG_RTOL, f32, masks
    shas = lambda ts: [sha(t) for t in ts]
    force = bc.FORCES[1]
    for name, solver in (("sphere_130", "direct"), ("two_144", "cg"), ("two_144", "direct_scattered")):
        Y, X, _, order, _ = bc.SCENES[name]
        g = bc.geometry_of(name)
        mk = masks(g, solver)
        cfg = ops.karman_cfg(bc.B, Y, X, g.dx, masks=mk, cg_rtol=CG_RTOL, inflow_order=order)
        d, vy, vx, re = (f32(t) for t in bc.start_state(name))
        wd, wy, wx = (f32(t) for t in bc.cotangents(name, "both"))
        leg, info = {}, {}
        with torch.no_grad():
            feat = torch.zeros(bc.B, Y, X, 4, dtype=torch.float32, device=dev)
            leg["step"] = shas(ops.karman_step_large(d, vy, vx, re, cfg, mk, info=info, feat=feat, feat_scale=(5.0, 4.0, 1e-5)) + (feat,))
            leg["step_buoy"] = shas(ops.karman_step_large(d, vy, vx, re, cfg, mk, feat=feat, feat_scale=(5.0, 4.0, 1e-5), buoyancy=force) + (feat,))
            if solver == "cg":
                guess = torch.zeros(bc.B, Y, X, dtype=torch.float32, device=dev)
                for k in range(2):          # cold guess, then the first call's pressure as the guess
                    leg["step_warm%d" % k] = shas(ops.karman_step_large(d, vy, vx, re, cfg, mk, info=info, p_guess=guess) + (guess,)) + [info["iterations"].tolist()]
            st, svy, svx = ops.karman_step_saved(d, vy, vx, re, cfg, mk)
            leg["saved"] = shas(st + (svy, svx))
            sb, sby, sbx = ops.karman_step_saved(d, vy, vx, re, cfg, mk, buoyancy=force)
            leg["saved_buoy"] = shas(sb + (sby, sbx))
        leg["bwd"] = shas(ops.karman_step_large_bwd(svy, svx, re, wy, wx, cfg, mk))
        leg["bwd_re"] = shas(ops.karman_step_large_bwd_re(svy, svx, re, wy, wx, vy, vx, cfg, mk))
        leg["density_bwd"] = shas(ops.karman_density_bwd(d, svy, svx, re, wd, cfg, mk))
        leg["density_bwd_re"] = shas(ops.karman_density_bwd_re(d, svy, svx, re, wd, vy, vx, cfg, mk))
        leg["bwd_buoy"] = shas(ops.karman_step_large_bwd_buoy(d, sby, sbx, re, wy, wx, wd, cfg, mk, force))
        leg["bwd_buoy_re"] = shas(ops.karman_step_large_bwd_buoy(d, sby, sbx, re, wy, wx, wd, cfg, mk, force, vel_in=(vy, vx)))
        out["large2d_%s_%s" % (name, solver)] = leg

    for Y, X in ((70, 36), (24, 100)):
        gen = torch.Generator().manual_seed(3)
        rn = lambda *s: torch.randn(*s, generator=gen).to(dev)
        vy, vx, fy, fx, wy, wx = (a * rn(2, Y + 1, X) if k % 2 == 0 else a * rn(2, Y, X + 1) for k, a in enumerate((0.3, 0.3, 0.2, 0.2, 1.0, 1.0)))
        cfg, circ = sol_amd._lib.BurgersCfg(2, Y, X, 32.0 / Y, 0.1), ops.burgers_circ(Y, X, 0.01)
        with torch.no_grad():
            fwd = ops.burgers_step_large(vy, vx, fy, fx, cfg, circ)
        out["burgers_large_%dx%d" % (Y, X)] = shas(fwd + tuple(ops.burgers_step_large_bwd(vy, vx, wy, wx, cfg, circ)))

    for name, solver in (("16_comb", "direct"), ("16_comb", "cg"), ("20_comb", "direct")):
        c = kc.case(name)
        _, Y, X, Z = c["shape"]
        sim = karman3d.Karman3DFlow(karman3d.Scene3D(Y, X, Z, device=dev, pressure_solver=solver), c["shape"][0], dt=c["dt"],
                                    density_grad=True, re_grad=True, **c["kw"])
        d, v, re = kc.state(name)
        hs = [f32(t).requires_grad_(True) for t in (d, *v, re)]
        outs = sim.step(*hs)
        ((outs[0] * f32(kc.w_dens(name))).sum() + sum((a * f32(w)).sum() for a, w in zip(outs[1:], kc.w_vel(name)))).backward()
        out["adj3d_density_re_%s_%s" % (name, solver)] = shas(list(outs) + [h.grad for h in hs])
    print(json.dumps(out))
    sys.exit(0)
names = ["product"] + [a for a in sys.argv[1:] if not a.startswith("--")]
res = {}
for n in names:
    env = dict(os.environ)
    if n != "product":
        env["SOL_HIP_LIB"] = os.path.join(ROOT, "solver-in-the-loop_amd", "lib", "libsol_%s.so" % n)
    o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        res[n] = json.loads(o.stdout.strip().splitlines()[-1])
    except Exception:
        print(o.stdout[-1500:], o.stderr[-1500:])
        raise
    print(n, json.dumps(res[n]), flush=True)
for n in names[1:]:
    for leg in res["product"]:
        print("%-10s %-20s %s" % (n, leg, "BIT-IDENTICAL to product" if res[n].get(leg) == res["product"][leg] else "DIFFERS from product"))
