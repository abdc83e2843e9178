"""Buoyancy on the large-grid karman-2d step, on the GPU (pytest -m gpu): csrc/karman_buoyancy.hip behind ops.karman_step_large /
karman_step_saved / karman_step_large_bwd_buoy, KarmanFlow(buoyancy=...), torch.ops.sol.karman_step_buoy, LargeGridTrainer and
LargeGridRollout, against the float64 reference of buoyancy_cases.py (the oracle's stages + the face average of the definition).

Tolerances are the suite's (large2d_scenes): TOL_FIELD = 1e-5 on fields, TOL_GRAD = 1e-4 relative L2 on gradients, CG_RTOL = 1e-7 for
solves compared with the reference.  The inputs are fixed (state seed 11; seed 13 for the two-step chain) and conditioned on the
reference ALONE: test_karman2d_buoyancy_cpu.py measures the reference in float32 against float64 on every case below -- fields 1.8e-6,
gradients 7.7e-6 (one step with a velocity cotangent: after leaving out at most TRIM = 0.1 % of the entries, the trimmed metric of the
large-grid adjoint tests, buoyancy_cases.needs_trim; untrimmed everywhere else), g_re 2.7e-5.  The trainer problem (256 x 128, B = 1,
three steps, mars_moon, F = (0.981, 0)) measured the same way on the CPU: loss 1.6e-6, per-step losses 1.8e-6, weight gradient
5.7e-6; without the force the loss is 5000x and the gradient 39x the buoyant one, so an ignored force cannot pass."""
import os
import sys

import numpy as np
import pytest
import torch

import sol_amd
import sol_oracle as o
from sol_amd import _lib, fluid, karman, ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buoyancy_cases as bc
from large2d_scenes import CG_RTOL, DEV, TOL_FIELD, TOL_GRAD, TRIM, f32, masks, rel, trimmed_rel

pytestmark = pytest.mark.gpu
B = bc.B
FS = (1.0 / 0.2, 1.0 / 0.25, 1.0 / o.STD_RE)          # feature scales (1 / std)
RUNS = [(n, s) for n in ("sphere_130", "two_144", "before_160") for s in bc.SCENES[n][4]]


def setup(name, solver, **kw):
    Y, X, _, order, _ = bc.SCENES[name]
    g = bc.geometry_of(name)
    mk = masks(g, solver)
    assert mk.pressure_solver == solver and mk.large
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk, cg_rtol=CG_RTOL, inflow_order=order, **kw)
    return g, mk, cfg


def device_state(name, steps=1):
    return tuple(f32(t) for t in bc.start_state(name, steps=steps))


def check(got, ref, trimmed, what, names=("g_d", "g_vy", "g_vx")):
    """large2d_scenes.check_grads for (g_d, g_vy, g_vx): every figure printed before it is asserted"""
    for name, a, b in zip(names, got, ref):
        full = rel(a, b)
        if trimmed:
            v, k, worst = trimmed_rel(a, b)
            print("%s %s: rel L2 %.3e untrimmed, %.3e after leaving out %d of %d entries (largest deviation left out %.3e)"
                  % (what, name, full, v, k, b.numel(), worst))
            assert k <= int(TRIM * b.numel())
            assert v < TOL_GRAD, (what, name, v, full)
        else:
            print("%s %s: rel L2 %.3e" % (what, name, full))
            assert full < TOL_GRAD, (what, name, full)


# ---- 1. forward against the reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("force", bc.FORCES, ids=["fy", "fyx"])
@pytest.mark.parametrize("name,solver", RUNS)
def test_forward_against_the_reference(name, solver, force):
    g, mk, cfg = setup(name, solver)
    Y, X = bc.SCENES[name][:2]
    d, vy, vx, re = device_state(name)
    ref = bc.reference(name, force, "both")[0]
    feat = torch.full((B, Y, X, 4), 9.0, dtype=torch.float32, device=DEV)
    info = {}
    with torch.no_grad():
        out = ops.karman_step_large(d, vy, vx, re, cfg, mk, info=info, feat=feat, feat_scale=FS, buoyancy=force)
        plain = ops.karman_step_large(d, vy, vx, re, cfg, mk)
        saved, svy, svx = ops.karman_step_saved(d, vy, vx, re, cfg, mk, buoyancy=force)
    errs = [rel(a, b) for a, b in zip(out, ref)]
    print("forward %s %s F=%s: d %.3e vy %.3e vx %.3e; the force moves vy by %.2f" % ((name, solver, force) + tuple(errs) + (rel(out[1], plain[1]),)))
    assert max(errs) < TOL_FIELD, errs
    if solver == "cg":
        assert info["converged"].tolist() == [1] * B
    # the fused features: to_feature of the new velocity times the scales, channel 3 zero
    rf = torch.stack([ref[1][:, :Y] * FS[0], ref[2][:, :, :X] * FS[1], (bc.start_state(name)[3] * FS[2]).reshape(B, 1, 1).expand(B, Y, X)], dim=-1)
    assert rel(feat[..., :3], rf) < TOL_FIELD and not feat[..., 3].any()
    # the saved form issues the same launches: the same bits; the density is the plain step's (the force does not touch it)
    for a, b in zip(saved, out):
        assert torch.equal(a, b)
    assert torch.equal(out[0], plain[0]) and rel(out[1], plain[1]) > 0.05


# ---- 2. F = (0, 0) through the new entry points: the plain entry points' bits --------------------------------------------------------------
@pytest.mark.parametrize("name,solver", [("sphere_130", "direct"), ("two_144", "cg")])
def test_zero_force_gives_the_plain_bits_forward_and_backward(name, solver):
    g, mk, cfg = setup(name, solver)
    Y, X = bc.SCENES[name][:2]
    d, vy, vx, re = device_state(name)
    wd, wy, wx = (f32(t) for t in bc.cotangents(name, "both"))
    z = (0.0, 0.0)
    f0, f1 = (torch.zeros(B, Y, X, 4, dtype=torch.float32, device=DEV) for _ in range(2))
    with torch.no_grad():
        a = ops.karman_step_large(d, vy, vx, re, cfg, mk, feat=f0, feat_scale=FS, buoyancy=z)
        b = ops.karman_step_large(d, vy, vx, re, cfg, mk, feat=f1, feat_scale=FS)
        sa, say, sax = ops.karman_step_saved(d, vy, vx, re, cfg, mk, buoyancy=z)
        sb, sby, sbx = ops.karman_step_saved(d, vy, vx, re, cfg, mk)
    for x, y in zip(a + (f0,) + sa + (say, sax), b + (f1,) + sb + (sby, sbx)):
        assert torch.equal(x, y)
    got = ops.karman_step_large_bwd_buoy(d, say, sax, re, wy, wx, wd, cfg, mk, z)
    py, px = ops.karman_step_large_bwd(sby, sbx, re, wy, wx, cfg, mk)
    ref = ops.karman_density_bwd(d, sby, sbx, re, wd, cfg, mk, py, px)
    got_re = ops.karman_step_large_bwd_buoy(d, say, sax, re, wy, wx, wd, cfg, mk, z, vel_in=(vy, vx))
    qy, qx, q_re = ops.karman_step_large_bwd_re(sby, sbx, re, wy, wx, vy, vx, cfg, mk)
    ref_re = ops.karman_density_bwd_re(d, sby, sbx, re, wd, vy, vx, cfg, mk, qy, qx, q_re)
    torch.cuda.synchronize()
    for x, y in zip(got + got_re, ref + ref_re):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())


# ---- 3. the stand-alone pair: transposes of each other, the ghost ring, the spelling -------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere_130", "two_144"])
@pytest.mark.parametrize("f", [(0.981, 0.0), (0.3, -0.2), (0.0, 0.7)])
def test_add_and_add_bwd_are_transposes(name, f):
    Y, X = bc.SCENES[name][:2]
    g = bc.geometry_of(name)
    act = f32(g.active)
    gen = torch.Generator().manual_seed(17)
    d = torch.randn(B, Y, X, generator=gen, dtype=torch.float32)
    gy, gx = torch.randn(B, Y + 1, X, generator=gen, dtype=torch.float32), torch.randn(B, Y, X + 1, generator=gen, dtype=torch.float32)
    gd = torch.randn(B, Y, X, generator=gen, dtype=torch.float32)
    vy, vx = ops.karman_buoyancy_add(f32(d), torch.zeros(B, Y + 1, X, dtype=torch.float32, device=DEV),
                                     torch.zeros(B, Y, X + 1, dtype=torch.float32, device=DEV), act, f)
    back = ops.karman_buoyancy_add_bwd(f32(gy), f32(gx), act, f, f32(gd))
    back0 = ops.karman_buoyancy_add_bwd(f32(gy), f32(gx), act, f)
    dot = lambda a, b: float((a.double().cpu() * b.double().cpu()).sum())
    lhs, rhs = dot(vy, gy) + dot(vx, gx), dot(d, back0)
    print("<add(d), g> = %.9e, <d, add_bwd(g)> = %.9e (%s F=%s)" % (lhs, rhs, name, f))
    assert abs(lhs - rhs) < 1e-6 * abs(lhs) and abs(lhs) > 1.0          # (seeded inputs: |lhs| is 10 .. 100 here)
    assert rel(back, back0.double().cpu() + gd.double()) < 1e-6          # g_d_out is added, NULL counts as zero
    # against the definition in float64
    ty, tx = bc.add_term(d.double(), g, f)
    assert rel(vy, ty) < 1e-6 and rel(vx, tx) < 1e-6


def test_add_on_the_border_pins_the_ghost_ring_the_end_faces_and_the_spelling():
    """Density in the first and last row and column only, an obstacle in the grid: face rows 0 and Y and face columns 0 and X average
    with the zero ghost ring; every face equals fl(v + fl(fl(f) * fl(0.5f * (d0 + d1)))) * mask bit for bit (the spelling in sol_hip.h)."""
    Y, X = 130, 65
    g = bc.geometry_of("sphere_130")
    gen = torch.Generator().manual_seed(5)
    d = torch.zeros(1, Y, X, dtype=torch.float32)
    for sl in ((0, slice(None)), (Y - 1, slice(None)), (slice(None), 0), (slice(None), X - 1)):
        d[0][sl] = torch.rand(d[0][sl].shape, generator=gen, dtype=torch.float32) + 0.5
    vy0, vx0 = torch.randn(1, Y + 1, X, generator=gen, dtype=torch.float32), torch.randn(1, Y, X + 1, generator=gen, dtype=torch.float32)
    f = (0.981, -0.37)
    vy, vx = ops.karman_buoyancy_add(f32(d), f32(vy0), f32(vx0), f32(g.active), f)
    dz = torch.nn.functional.pad(d, (1, 1, 1, 1))
    f32s = [torch.tensor(v, dtype=torch.float32) for v in f]
    my, mx = torch.as_tensor(g.my, dtype=torch.float32), torch.as_tensor(g.mx, dtype=torch.float32)
    ey = (vy0 + f32s[0] * (0.5 * (dz[:, :-1, 1:-1] + dz[:, 1:, 1:-1]))) * my          # float32 tensors: one rounding per operation
    ex = (vx0 + f32s[1] * (0.5 * (dz[:, 1:-1, :-1] + dz[:, 1:-1, 1:]))) * mx
    assert torch.equal(vy.cpu(), ey) and torch.equal(vx.cpu(), ex)
    # the end faces see half of the border cell (the other half is the ghost ring's zero)
    assert torch.equal(vy.cpu()[0, 0], vy0[0, 0] + f32s[0] * (0.5 * d[0, 0])) and torch.equal(vy.cpu()[0, Y], vy0[0, Y] + f32s[0] * (0.5 * d[0, Y - 1]))
    assert torch.equal(vx.cpu()[0, :, 0], vx0[0, :, 0] + f32s[1] * (0.5 * d[0, :, 0])) and torch.equal(vx.cpu()[0, :, X], vx0[0, :, X] + f32s[1] * (0.5 * d[0, :, X - 1]))
    assert float((vy.cpu() - vy0 * my).abs()[0, 2:Y - 1, 1:X - 1].max()) == 0.0          # the interior holds no density: untouched but for the mask
    # transpose: a cotangent on the four end rows / columns alone reaches exactly the border cells
    gy, gx = torch.zeros(1, Y + 1, X, dtype=torch.float32), torch.zeros(1, Y, X + 1, dtype=torch.float32)
    gy[0, 0], gy[0, Y], gx[0, :, 0], gx[0, :, X] = 1.0, 2.0, 3.0, 4.0
    back = ops.karman_buoyancy_add_bwd(f32(gy), f32(gx), f32(g.active), f).cpu()
    exp = torch.zeros(1, Y, X, dtype=torch.float64)
    exp[0, 0] += 0.5 * f[0] * 1.0
    exp[0, Y - 1] += 0.5 * f[0] * 2.0
    exp[0, :, 0] += 0.5 * f[1] * 3.0
    exp[0, :, X - 1] += 0.5 * f[1] * 4.0
    assert rel(back, exp) < 1e-6 and not back[0, 1:Y - 1, 1:X - 1].any()


# ---- 4. the adjoint against the reference's autograd -------------------------------------------------------------------------------------
def hip_grad(name, solver, force, kind, re_grad=False, info=None):
    g, mk, cfg = setup(name, solver)
    d, vy, vx, re = device_state(name)
    leaves = [t.requires_grad_(True) for t in ((d, vy, vx, re) if re_grad else (d, vy, vx))]
    out = ops.karman_step_large(d, vy, vx, re, cfg, mk, info=info, re_grad=re_grad, buoyancy=force)
    assert all(t.requires_grad for t in out)                     # the density is in the graph without density_grad
    wd, wy, wx = bc.cotangents(name, kind)
    loss = 0.0
    if wd is not None:
        loss = loss + (out[0] * f32(wd)).sum()
    if wy is not None:
        loss = loss + (out[1] * f32(wy)).sum() + (out[2] * f32(wx)).sum()
    loss.backward()
    torch.cuda.synchronize()
    return tuple(t.detach() for t in out), tuple(torch.zeros_like(t) if t.grad is None else t.grad for t in leaves)


@pytest.mark.parametrize("kind", ["vel", "dens", "both"])
@pytest.mark.parametrize("force", bc.FORCES, ids=["fy", "fyx"])
@pytest.mark.parametrize("name,solver", [("sphere_130", "direct"), ("two_144", "cg"), ("before_160", "direct")])
def test_adjoint_against_the_references_autograd(name, solver, force, kind):
    ref_out, ref_g = bc.reference(name, force, kind)
    info = {}
    out, got = hip_grad(name, solver, force, kind, info=info)
    assert max(rel(a, b) for a, b in zip(out, ref_out)) < TOL_FIELD
    check(got, ref_g, bc.needs_trim(kind, 1), "%s %s F=%s %s" % (name, solver, force, kind))
    if kind == "vel":            # a velocity-only loss still yields a density gradient, and a large one
        ratio = float(got[0].double().norm() / got[1].double().norm())
        print("velocity-only loss: |g_d| / |g_vy| = %.3f" % ratio)
        assert ratio > 0.01
    if solver == "cg":           # a density-only loss runs no pressure solve
        assert ("iterations_bwd" in info) == (kind != "dens"), info
        assert kind == "dens" or info["converged_bwd"].tolist() == [1] * B


@pytest.mark.parametrize("name,solver,force", [("sphere_130", "direct", bc.FORCES[0]), ("sphere_130", "direct", bc.FORCES[1]),
                                               ("two_144", "cg", bc.FORCES[0])])
def test_adjoint_with_the_reynolds_number_gradient(name, solver, force):
    ref_out, ref_g = bc.reference(name, force, "both", 1, True)
    out, got = hip_grad(name, solver, force, "both", re_grad=True)
    plain = hip_grad(name, solver, force, "both")[1]
    check(got[:3], ref_g[:3], True, "%s %s F=%s re_grad" % (name, solver, force))
    e = rel(got[3], ref_g[3])
    print("g_re %s against the reference %s: %.3e" % (got[3].tolist(), ref_g[3].tolist(), e))
    assert e < TOL_GRAD
    for a, b in zip(got[:3], plain):          # the _re twin issues the plain launches: the same bits
        assert torch.equal(a, b)


def test_torch_op_karman_step_buoy():
    from sol_amd import torch_ops
    name, force = "sphere_130", bc.FORCES[1]
    g, mk, cfg = setup(name, "direct")
    h = torch_ops.register_scene(cfg, mk)
    d, vy, vx, re = device_state(name)
    leaves = [t.requires_grad_(True) for t in (d, vy, vx)]
    out = torch.ops.sol.karman_step_buoy(d, vy, vx, re, h, force[0], force[1])
    wd, wy, wx = (f32(t) for t in bc.cotangents(name, "both"))
    ((out[0] * wd).sum() + (out[1] * wy).sum() + (out[2] * wx).sum()).backward()
    ref_out, ref_g = hip_grad(name, "direct", force, "both")
    for a, b in zip(tuple(out) + tuple(t.grad for t in leaves), ref_out + ref_g):
        assert torch.equal(a.detach(), b)
    with torch.no_grad():
        ng = torch.ops.sol.karman_step_buoy(d, vy, vx, re, h, force[0], force[1])
    assert all(torch.equal(a, b) for a, b in zip(ng, ref_out))


# ---- 5. two chained KarmanFlow.step calls: the density gradient crosses a step boundary ---------------------------------------------------
@pytest.mark.parametrize("force", bc.FORCES, ids=["fy", "fyx"])
def test_two_chained_flow_steps_against_the_reference(force):
    name = "sphere_130"
    Y, X = bc.SCENES[name][:2]
    ref_out, ref_g = bc.reference(name, force, "both", 2)
    d, vy, vx, re = device_state(name, steps=2)
    leaves = [t.requires_grad_(True) for t in (d, vy, vx)]
    dom = fluid.Domain([Y, X], box=fluid.box[0:200, 0:100])
    vel = fluid.StaggeredGrid([vy.reshape(B, Y + 1, X, 1), vx.reshape(B, Y, X + 1, 1)], dom.box)
    s = fluid.Fluid(dom, density=d.reshape(B, Y, X, 1), velocity=vel, batch_size=B)
    sim = karman.KarmanFlow(buoyancy=force) if force[1] else karman.KarmanFlow(buoyancy_factor=0.1, gravity=(-9.81, 0.0))
    assert sim._buoyancy == pytest.approx(force)
    bcv, bcm = karman.velocity_bc_masks(Y, X, batch_size=B)
    for _ in range(2):
        s = sim.step(s, re=bc.start_state(name, steps=2)[3].tolist(), res=X, velBCy=bcv, velBCyMask=bcm)
    od, oy, ox = s.density.data.reshape(B, Y, X), s.velocity.data[0].data.reshape(B, Y + 1, X), s.velocity.data[1].data.reshape(B, Y, X + 1)
    errs = [rel(a, b) for a, b in zip((od, oy, ox), ref_out)]
    print("two chained steps F=%s: fields %s" % (force, errs))
    assert max(errs) < TOL_FIELD
    wd, wy, wx = (f32(t) for t in bc.cotangents(name, "both"))
    ((od * wd).sum() + (oy * wy).sum() + (ox * wx).sum()).backward()
    torch.cuda.synchronize()
    check(tuple(t.grad for t in leaves), ref_g, False, "two chained KarmanFlow.step F=%s" % (force,))


# ---- 6. bits --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,solver", [("sphere_130", "direct"), ("two_144", "cg")])
def test_backward_is_bit_reproducible_eager_captured_and_tile_vs_global(name, solver):
    force = bc.FORCES[1]
    g, mk, cfg = setup(name, solver, cg_max_iter=400)
    d, vy, vx, re = device_state(name)
    wd, wy, wx = (f32(t) for t in bc.cotangents(name, "both"))
    with torch.no_grad():
        _, svy, svx = ops.karman_step_saved(d, vy, vx, re, cfg, mk, buoyancy=force)
    run = lambda **kw: ops.karman_step_large_bwd_buoy(d, svy, svx, re, wy, wx, wd, cfg, mk, force, **kw)
    first, second = run(), run()
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
    for opt in ("k2d_adj_tile", "k2d_dens_adj_tile"):
        _lib.set_option(opt, 0)
        try:
            glob = run()
            torch.cuda.synchronize()
        finally:
            _lib.set_option(opt, 1)
        for a, b in zip(glob, first):
            assert torch.equal(a, b), opt
    if solver != "direct":
        return
    # replayed from a captured graph (kernel nodes only: sol_graph_check inside capture_graph)
    ws = torch.empty((ops.large_bwd_workspace_bytes(cfg, mk) + 3) // 4, dtype=torch.float32, device=DEV)
    wsd = torch.empty((ops.density_bwd_workspace_bytes(cfg) + 3) // 4, dtype=torch.float32, device=DEV)
    cap = {}

    def body():
        cap["g"] = run(workspace=ws, density_workspace=wsd)

    torch.cuda.synchronize()
    graph = _lib.capture_graph(body, "buoyant large-grid adjoint")
    for _ in range(2):
        for t in cap["g"]:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(cap["g"], first):
            assert torch.equal(a, b)


# ---- 7. poisoning ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,solver", [("sphere_130", "direct"), ("two_144", "cg")])
def test_a_non_finite_velocity_cotangent_poisons_its_simulation_alone(name, solver):
    force = bc.FORCES[0]
    g, mk, cfg = setup(name, solver, cg_max_iter=400)          # (the poisoned simulation's solve cannot converge: a budget it may spend)
    Y, X = bc.SCENES[name][:2]
    d, vy, vx, re = device_state(name)
    wd, wy, wx = (f32(t) for t in bc.cotangents(name, "both"))
    with torch.no_grad():
        _, svy, svx = ops.karman_step_saved(d, vy, vx, re, cfg, mk, buoyancy=force)
    clean = ops.karman_step_large_bwd_buoy(d, svy, svx, re, wy, wx, wd, cfg, mk, force, vel_in=(vy, vx))
    bad = wy.clone()
    bad[0, Y // 3, X // 2] = float("inf")
    got = ops.karman_step_large_bwd_buoy(d, svy, svx, re, bad, wx, wd, cfg, mk, force, vel_in=(vy, vx))
    torch.cuda.synchronize()
    for a, b in zip(got, clean):                     # g_d_in, g_vy_in, g_vx_in, g_re
        assert bool(torch.isnan(a[0]).all()), "simulation 0 is not NaN throughout"
        assert torch.equal(a[1], b[1]) and bool(torch.isfinite(a[1]).all())


# ---- 8. LargeGridTrainer(buoyancy=...) -------------------------------------------------------------------------------------------------------
def _net_of(p):
    net = sol_amd.model_mars_moon(cin=3, cout=2, seed=0)
    net.set_weights([q.detach().numpy() for q in p["params"]])
    return net


def _batch(p):
    return (f32(p["d"]), f32(p["vy"]), f32(p["vx"]), f32(p["re"]), f32(torch.stack(p["gt_vy"])), f32(torch.stack(p["gt_vx"])))


def test_large_grid_trainer_with_buoyancy_against_the_reference_and_replayed():
    """256 x 128 (the grid of test_gpu_karman2d_large_trainer.py), B = 1, msteps = 3, mars_moon, at that file's tolerances: loss and
    per-step losses 1e-5, full weight gradient TOL_GRAD untrimmed, captured against eager 1e-6; a second replay gives the first one's bits
    (the carried density gradient is reset at the head of every run)."""
    Y, X = bc.TRAINER_GRID
    force, ms = bc.FORCES[0], 3
    p = bc.trainer_problem(force, ms)
    lref, steps_ref, gref, fin_ref = bc.trainer_reference(p, force)
    te = sol_amd.make_trainer(_net_of(p), None, 1, Y, X, ms, 100.0 / X, bc.TRAINER_STD_V, o.STD_RE, use_graph=False, buoyancy=force)
    assert isinstance(te, sol_amd.LargeGridTrainer) and te.buoyancy == force
    args = _batch(p)
    loss = float(te.fwd_bwd(*args, want_final=True))
    e_l, e_g = abs(loss - lref) / abs(lref), rel(te.grads, gref)
    e_s = [abs(a - b) / abs(b) for a, b in zip(te.loss_steps.tolist(), steps_ref)]
    e_f = [rel(a, b) for a, b in zip(te.final, fin_ref)]
    print("LargeGridTrainer(buoyancy=%s) vs float64 reference: loss %.3e, per-step %s, gradient %.3e, final state %s" % (force, e_l, e_s, e_g, e_f))
    assert e_l < 1e-5 and max(e_s) < 1e-5 and e_g < TOL_GRAD and max(e_f) < TOL_FIELD, (e_l, e_s, e_g, e_f)
    g_eager, l_eager = te.grads.clone(), te.loss_steps.clone()
    assert float(te.fwd_bwd(*args)) == loss and torch.equal(te.grads, g_eager)          # run to run: the same bits
    # without the force the same trainer computes something else entirely
    t0 = sol_amd.LargeGridTrainer(_net_of(p), 1, Y, X, ms, bc.TRAINER_STD_V, o.STD_RE, use_graph=False)
    assert t0.buoyancy is None and abs(float(t0.fwd_bwd(*args)) - lref) > 0.5 * abs(lref)
    # captured: a replay equals eager, a second replay equals the first
    tg = sol_amd.LargeGridTrainer(_net_of(p), 1, Y, X, ms, bc.TRAINER_STD_V, o.STD_RE, buoyancy=force)
    lg = float(tg.fwd_bwd(*args))
    assert tg._graph is not None
    e_g = rel(tg.grads, g_eager)
    print("captured vs eager: loss %.3e gradient %.3e" % (abs(lg - loss) / abs(loss), e_g))
    assert abs(lg - loss) <= 1e-6 * abs(loss) and e_g < 1e-6 and rel(tg.loss_steps, l_eager) < 1e-6
    g1, l1 = tg.grads.clone(), tg.loss_steps.clone()
    assert float(tg.fwd_bwd(*args)) == lg and torch.equal(tg.grads, g1) and torch.equal(tg.loss_steps, l1)


# ---- 9. LargeGridRollout(buoyancy=...) --------------------------------------------------------------------------------------------------------
def test_large_grid_rollout_with_buoyancy_three_steps_against_the_reference():
    Y, X = bc.TRAINER_GRID
    force = bc.FORCES[1]
    p = bc.trainer_problem(force, 1)
    g = p["g"]
    rd, ry, rx, re = p["d"], p["vy"], p["vx"], p["re"]
    with torch.no_grad():
        params = [q.detach() for q in p["params"]]
        for _ in range(3):
            rd, ry, rx = bc.buoyant_step(rd, ry, rx, re, g, force)
            cy, cx = o.correction(params, ry, rx, re, bc.TRAINER_STD_V, o.STD_RE)
            ry, rx = ry + cy, rx + cx
    runs = []
    for kw in (dict(use_graph=True), dict(use_graph=False)):
        ro = sol_amd.make_rollout(_net_of(p), masks(g), 1, Y, X, g.dx, bc.TRAINER_STD_V, o.STD_RE, buoyancy=force, **kw)
        assert isinstance(ro, sol_amd.LargeGridRollout) and ro.buoyancy == force
        h = tuple(f32(p[k]) for k in ("d", "vy", "vx", "re"))
        ro.run(*h, 3)
        errs = [rel(a, b) for a, b in zip(h[:3], (rd, ry, rx))]
        print("LargeGridRollout(buoyancy=%s, %s): d %.3e vy %.3e vx %.3e" % ((force, kw) + tuple(errs)))
        assert max(errs) < TOL_FIELD, errs
        runs.append(h[:3])
    assert all(torch.equal(a, b) for a, b in zip(*runs))           # the captured step includes the new launch: eager's bits
    # a CG scene with a warm start (eager): the same fields within the solve's tolerance
    ro = sol_amd.LargeGridRollout(_net_of(p), masks(g, "cg"), 1, Y, X, g.dx, bc.TRAINER_STD_V, o.STD_RE, buoyancy=force, use_graph=False,
                                  cg_warm_start=True, cg_rtol=CG_RTOL)
    h = tuple(f32(p[k]) for k in ("d", "vy", "vx", "re"))
    its = ro.run(*h, 3)
    errs = [rel(a, b) for a, b in zip(h[:3], (rd, ry, rx))]
    print("LargeGridRollout(buoyancy, CG warm start): %s, iterations %s" % (errs, its.tolist()))
    assert max(errs) < TOL_FIELD and bool(ro.solve_info["converged"].all())


# ---- 10. refusals and defaults --------------------------------------------------------------------------------------------------------------
def test_refusals_and_defaults():
    # a grid the one-workgroup kernels serve, with a force
    Y, X = 64, 32
    g = o.KarmanGeometry(Y, X)
    dom = fluid.Domain([Y, X], box=fluid.box[0:200, 0:100])
    st = fluid.Fluid(dom, density=0.0, velocity=0.0, batch_size=1)
    bcv, bcm = karman.velocity_bc_masks(Y, X, batch_size=1)
    with pytest.raises(sol_amd.SolError, match="large-grid"):
        karman.KarmanFlow(buoyancy=(0.981, 0.0)).step(st, re=[1e5], res=X, velBCy=bcv, velBCyMask=bcm)
    mk = masks(g)
    cfg = ops.karman_cfg(1, Y, X, g.dx, masks=mk)
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)
    with pytest.raises(sol_amd.SolError, match="large-grid"):
        ops.karman_step_saved(z(1, Y, X), z(1, Y + 1, X), z(1, Y, X + 1), torch.ones(1, dtype=torch.float32, device=DEV), cfg, mk, buoyancy=(0.1, 0.0))
    net = sol_amd.model_mars_moon(cin=3, cout=2, seed=0)
    with pytest.raises(ValueError, match="buoyancy"):
        sol_amd.SolTrainer(net, mk, 1, Y, X, 2, g.dx, (0.2, 0.2), o.STD_RE, buoyancy=(0.981, 0.0))
    with pytest.raises(ValueError, match="buoyancy"):
        sol_amd.GraphTrainer(net, 1, Y, X, 2, (0.2, 0.2), o.STD_RE, buoyancy=(0.981, 0.0))
    sol_amd.GraphTrainer(net, 1, Y, X, 2, (0.2, 0.2), o.STD_RE, buoyancy=None, use_graph=False)          # the default is accepted
    # buoyancy=None: the large-grid step's bits are what they are without the keyword
    name = "sphere_130"
    g, mk, cfg = setup(name, "direct")
    Yl, Xl = bc.SCENES[name][:2]
    d, vy, vx, re = device_state(name)
    with torch.no_grad():
        a = ops.karman_step_large(d, vy, vx, re, cfg, mk, buoyancy=None)
        b = ops.karman_step_large(d, vy, vx, re, cfg, mk)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    dom = fluid.Domain([Yl, Xl], box=fluid.box[0:200, 0:100])
    bcv, bcm = karman.velocity_bc_masks(Yl, Xl, batch_size=B)
    outs = []
    for sim in (karman.KarmanFlow(), karman.KarmanFlow(buoyancy=None), karman.KarmanFlow(buoyancy_factor=0.0)):
        vel = fluid.StaggeredGrid([vy.reshape(B, Yl + 1, Xl, 1), vx.reshape(B, Yl, Xl + 1, 1)], dom.box)
        s = sim.step(fluid.Fluid(dom, density=d.reshape(B, Yl, Xl, 1), velocity=vel, batch_size=B), re=re.tolist(), res=Xl, velBCy=bcv, velBCyMask=bcm)
        outs.append((s.density.data.reshape(B, Yl, Xl), s.velocity.data[0].data.reshape(B, Yl + 1, Xl), s.velocity.data[1].data.reshape(B, Yl, Xl + 1)))
        assert not outs[-1][0].requires_grad
    for got in outs:
        assert all(torch.equal(x, y) for x, y in zip(got, b))


# ---- 11. scripts: --buoyancy travels with the data -------------------------------------------------------------------------------------
def test_scripts_generate_train_apply_with_buoyancy(tmp_path):
    """karman.py -r 128 --buoyancy 0.3,-0.2 twice (default sphere, direct solve) -> karman_train.py for a few steps -> karman_apply.py,
    neither given the flag: the force is recorded in params.pickle, picked up from the set, recorded in dataStats.pickle and picked up
    from there; a contradicting flag is refused; the generated frames differ from a run without the force."""
    import importlib.util
    import pickle
    from sol_amd import scene
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    sys.path.insert(0, sdir)

    def load(name):
        spec = importlib.util.spec_from_file_location("sol_script_buoy_" + name, os.path.join(sdir, name + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m

    Y, X = 256, 128
    for re_nr in (1.6e5, 3.2e5):
        hi = load("karman").main(["-o", str(tmp_path / "hi"), "-r", "128", "-t", "7", "-s", "1", "--re", str(re_nr), "--buoyancy", "0.3,-0.2"])
    with open(hi + "/params.pickle", "rb") as f:
        assert pickle.load(f)["buoyancy"] == (0.3, -0.2)
    plain = load("karman").main(["-o", str(tmp_path / "plain"), "-r", "128", "-t", "7", "-s", "1", "--re", "3.2e5"])
    with open(plain + "/params.pickle", "rb") as f:
        assert pickle.load(f)["buoyancy"] is None
    # (the inflow has filled a few rows by frame 5: the force has something to act on)
    a, b = (scene.read_zipped_array(os.path.join(p, "velo_000005.npz")) for p in (hi, plain))
    assert np.isfinite(a).all() and np.abs(a - b).max() > 1e-3
    tf = str(tmp_path / "tf")
    train = ["--train", str(tmp_path / "hi"), "-s", "1", "-n", "2", "-b", "1", "-t", "5", "-m", "2", "-e", "1", "--lr", "1e-4", "--tf", tf, "--seed", "0"]
    with pytest.raises(SystemExit, match="contradicts"):
        load("karman_train").main(train + ["--buoyancy", "0.5"])
    loss = load("karman_train").main(train)
    assert loss is not None and np.isfinite(loss)
    with open(tf + "/dataStats.pickle", "rb") as f:
        assert pickle.load(f)["buoyancy"] == (0.3, -0.2)
    run = load("karman_apply").main(["-o", str(tmp_path / "run"), "-r", "128", "-t", "3", "-s", "1", "--stats", tf + "/dataStats.pickle",
                                     "--model", tf + "/model.pt"])
    for i in range(3):
        for name in ("denTf", "velTf", "corTf"):
            assert np.isfinite(scene.read_zipped_array(os.path.join(run, "%s_%06d.npz" % (name, i)))).all(), (name, i)
