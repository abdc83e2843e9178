"""Diffusion substeps of the karman-2d step, on the GPU (pytest -m gpu): csrc/karman_diffuse_sub.hip behind ops.karman_diffuse_sub, the
diffusion_substeps= keyword of ops.karman_step / karman_step_large / karman_step_saved and the adjoints, KarmanFlow(diffusion_substeps=),
torch.ops.sol.karman_step_sub, LargeGridTrainer, LargeGridRollout and scripts/karman.py, against the float64 reference of
diffusion_substeps_cases.py (n - 1 explicit substeps of alpha / n, then the oracle's step at re * n).

Tolerances are the suite's (large2d_scenes): TOL_FIELD = 1e-5 on fields, TOL_GRAD = 1e-4 relative L2 on gradients, CG_RTOL = 1e-7 for
solves compared with the reference, the trimmed gradient metric (at most TRIM = 0.1 % of the entries left out) where a velocity cotangent
passes one step's advection adjoint (diffusion_substeps_cases.needs_trim).  The Reynolds numbers make the single stencil unstable
(alpha = 0.85 / 0.6 / 0.42 per simulation), so an ignored parameter cannot pass: the v_y of the step's output moves by 2.5 .. 10 % against
n = 1 (a thousand times the field tolerance), and after 40 steps the single stencil has blown up.  The inputs are fixed (state seed 11;
seed 13 for the two-step chain, as in the buoyancy suite) and conditioned on the reference ALONE: test_karman2d_diffusion_substeps_cpu.py
measures the reference in float32 against float64 on every case below -- pre-diffusion 1.4e-7, fields 1.8e-6, gradients 1.7e-5 (trimmed
where a velocity cotangent passes one step's advection adjoint; 8.4e-5 untrimmed), g_re 2.6e-5, the trainer problem (144 x 72, B = 1,
two steps, mars_moon, n = 4) loss 8.7e-7 and weight gradient 3.6e-7, with n = 1 a loss 45x off; four roll-out steps 1.9e-6 -- and pins
them.  Measured on an MI355X with this file: pre-diffusion 2.3e-7, |<Mx, y> - <x, My>| at most 3.1e-9 of |Mx||y|; forward fields
1.1e-6 (buoyant 1.6e-6); gradients 9.4e-7 untrimmed, g_d 1.4e-7, g_re 6.9e-6 (5.5e-5 at 32 x 16); trainer loss 1.1e-6, weight
gradient 6.1e-7, captured = eager bit for bit; roll-out of four steps 6.7e-7; stability: max|v| 1.55 -> 1.008 with n = 4, 1.9e6 with
n = 1."""
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
import diffusion_substeps_cases as dc
from large2d_scenes import CG_RTOL, DEV, TOL_FIELD, TOL_GRAD, TRIM, f32, masks, rel, trimmed_rel

pytestmark = pytest.mark.gpu
B = dc.B
FS = (1.0 / 0.2, 1.0 / 0.25, 1.0 / o.STD_RE)
RUNS = [(n, s) for n in ("sphere_130", "two_144", "before_160") for s in bc.SCENES[n][4]]
MOVED = 0.01          # v_y of the output against n = 1, relative L2: the CPU twin measures 0.025 .. 0.104 on the cases below and pins > 0.02


def setup(name, solver, **kw):
    Y, X, _, order, _ = bc.SCENES[name]
    g = bc.geometry_of(name)
    mk = masks(g, solver)
    assert mk.pressure_solver == solver and mk.large
    return g, mk, ops.karman_cfg(B, Y, X, g.dx, masks=mk, cg_rtol=CG_RTOL, inflow_order=order, **kw)


def device_state(name, steps=1):
    return tuple(f32(t) for t in dc.start_state(name, steps=steps))


def check(got, ref, trimmed, what, names=("g_d", "g_vy", "g_vx")):
    for name, a, b in zip(names, got, ref):
        full = rel(a, b)
        if trimmed and name != "g_d":
            v, k, worst = trimmed_rel(a, b)
            print("%s %s: rel L2 %.3e untrimmed, %.3e after leaving out %d of %d entries (largest deviation left out %.3e)"
                  % (what, name, full, v, k, b.numel(), worst))
            assert k <= int(TRIM * b.numel())
            assert v < TOL_GRAD, (what, name, v, full)
        else:
            print("%s %s: rel L2 %.3e" % (what, name, full))
            assert full < TOL_GRAD, (what, name, full)


def pre_cfg(Y, X):
    return ops.karman_cfg(dc.PRE_B, Y, X, 100.0 / X)


# ---- 1. the pre-diffusion alone -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", dc.PRE_N)
@pytest.mark.parametrize("Y,X", dc.PRE_SHAPES)
def test_pre_diffusion_against_float64_and_chunks_give_equal_bits(Y, X, n):
    vy, vx, re = (f32(t) for t in dc.pre_inputs(Y, X))
    cfg = pre_cfg(Y, X)
    assert ops.diffuse_sub_max() == 8
    fused = ops.karman_diffuse_sub(vy, vx, re, cfg, n)
    c8 = ops.karman_diffuse_sub(vy, vx, re, cfg, n, chunk=8)
    c3 = ops.karman_diffuse_sub(vy, vx, re, cfg, n, chunk=3)
    c1 = ops.karman_diffuse_sub(vy, vx, re, cfg, n, chunk=1)
    torch.cuda.synchronize()
    ref = dc.pre_reference(Y, X, n)
    errs = [rel(a, b) for a, b in zip(fused, ref)]
    print("pre-diffusion %dx%d n=%d against float64: vy %.3e vx %.3e" % (Y, X, n, errs[0], errs[1]))
    assert max(errs) < TOL_FIELD
    for other in (c8, c3, c1):
        assert torch.equal(other[0], fused[0]) and torch.equal(other[1], fused[1])
    assert rel(fused[0], vy) > 0.05                      # it does something


SYM_BOUND = 4 * 1e-8          # |<Mx, y> - <x, My>| / (|Mx| |y|): the CPU twin's float32 figure (6.5e-9 at worst, pinned below 1e-8) times 4


@pytest.mark.parametrize("n", dc.PRE_N)
@pytest.mark.parametrize("Y,X", dc.PRE_SHAPES)
def test_pre_diffusion_is_its_own_transpose(Y, X, n):
    xy, xx, re = dc.pre_inputs(Y, X, seed=21)
    yy, yx, _ = dc.pre_inputs(Y, X, seed=22)
    cfg = pre_cfg(Y, X)
    mx = ops.karman_diffuse_sub(f32(xy), f32(xx), f32(re), cfg, n)
    my = ops.karman_diffuse_sub(f32(yy), f32(yx), f32(re), cfg, n)
    dot = lambda a, b: float((a.double().cpu() * b.double().cpu()).sum())
    lhs, rhs = dot(mx[0], yy) + dot(mx[1], yx), dot(xy, my[0]) + dot(xx, my[1])
    scale = float(np.sqrt((dot(mx[0], mx[0]) + dot(mx[1], mx[1])) * (dot(yy, yy) + dot(yx, yx))))
    print("<Mx, y> = %.9e, <x, My> = %.9e, |Mx||y| = %.3e (%dx%d n=%d)" % (lhs, rhs, scale, Y, X, n))
    assert abs(lhs - rhs) < SYM_BOUND * scale


# ---- 2. the forward step against the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", dc.STEP_N)
@pytest.mark.parametrize("name,solver", RUNS)
def test_forward_against_the_reference(name, solver, n):
    g, mk, cfg = setup(name, solver)
    Y, X = bc.SCENES[name][:2]
    d, vy, vx, re = device_state(name)
    ref = dc.reference(name, n)[0]
    feat = torch.full((B, Y, X, 4), 9.0, dtype=torch.float32, device=DEV)
    info = {}
    with torch.no_grad():
        out = ops.karman_step_large(d, vy, vx, re, cfg, mk, info=info, feat=feat, feat_scale=FS, diffusion_substeps=n)
        plain = ops.karman_step_large(d, vy, vx, re, cfg, mk)
        saved, svy, svx = ops.karman_step_saved(d, vy, vx, re, cfg, mk, diffusion_substeps=n)
    errs = [rel(a, b) for a, b in zip(out, ref)]
    moved = rel(out[1], plain[1])
    print("forward %s %s n=%d: d %.3e vy %.3e vx %.3e; against n = 1 vy moves by %.3f" % ((name, solver, n) + tuple(errs) + (moved,)))
    assert max(errs) < TOL_FIELD, errs
    if solver == "cg":
        assert info["converged"].tolist() == [1] * B
    rf = torch.stack([ref[1][:, :Y] * FS[0], ref[2][:, :, :X] * FS[1], (dc.start_state(name)[3] * FS[2]).reshape(B, 1, 1).expand(B, Y, X)], dim=-1)
    assert rel(feat[..., :3], rf) < TOL_FIELD and not feat[..., 3].any()
    for a, b in zip(saved, out):
        assert torch.equal(a, b)
    assert moved > MOVED


def test_forward_with_buoyancy_against_the_reference():
    name, n = "sphere_130", 5
    g, mk, cfg = setup(name, "direct")
    d, vy, vx, re = device_state(name)
    ref = dc.reference(name, n, force=dc.FORCE)[0]
    with torch.no_grad():
        out = ops.karman_step_large(d, vy, vx, re, cfg, mk, buoyancy=dc.FORCE, diffusion_substeps=n)
    errs = [rel(a, b) for a, b in zip(out, ref)]
    print("buoyant forward n=%d: %s" % (n, errs))
    assert max(errs) < TOL_FIELD


# ---- 3. diffusion_substeps = 1: the plain calls' bits -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,solver", [("sphere_130", "direct"), ("two_144", "cg")])
def test_one_substep_gives_the_plain_bits_forward_and_backward(name, solver):
    g, mk, cfg = setup(name, solver)
    Y, X = bc.SCENES[name][:2]
    d, vy, vx, re = device_state(name)
    wd, wy, wx = (f32(t) for t in bc.cotangents(name, "both"))
    with torch.no_grad():
        a = ops.karman_step_large(d, vy, vx, re, cfg, mk, diffusion_substeps=1)
        b = ops.karman_step_large(d, vy, vx, re, cfg, mk)
        sa, say, sax = ops.karman_step_saved(d, vy, vx, re, cfg, mk, diffusion_substeps=1)
        sb, sby, sbx = ops.karman_step_saved(d, vy, vx, re, cfg, mk)
        py, px = ops.karman_diffuse_sub(vy, vx, re, cfg, 1)
    assert py.data_ptr() == vy.data_ptr() and px.data_ptr() == vx.data_ptr()          # no launch
    for x, y in zip(a + sa + (say, sax), b + sb + (sby, sbx)):
        assert torch.equal(x, y)
    got = ops.karman_step_large_bwd(say, sax, re, wy, wx, cfg, mk, diffusion_substeps=1)
    ref = ops.karman_step_large_bwd(sby, sbx, re, wy, wx, cfg, mk)
    got_re = ops.karman_step_large_bwd_re(say, sax, re, wy, wx, vy, vx, cfg, mk, diffusion_substeps=1)
    ref_re = ops.karman_step_large_bwd_re(sby, sbx, re, wy, wx, vy, vx, cfg, mk)
    # the autograd surface, every mode: KarmanFlow-level keyword 1 against no keyword
    grads = []
    for kw in (dict(diffusion_substeps=1), dict()):
        leaves = [t.clone().requires_grad_(True) for t in (d, vy, vx, re)]
        out = ops.karman_step_large(*leaves, cfg, mk, density_grad=True, re_grad=True, **kw)
        ((out[0] * wd).sum() + (out[1] * wy).sum() + (out[2] * wx).sum()).backward()
        grads.append(tuple(t.detach() for t in out) + tuple(t.grad for t in leaves))
    torch.cuda.synchronize()
    for x, y in zip(got + got_re + grads[0], ref + ref_re + grads[1]):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())
    # the buoyant adjoint, the torch op and KarmanFlow with the count 1
    f = dc.FORCE
    with torch.no_grad():
        _, fay, fax = ops.karman_step_saved(d, vy, vx, re, cfg, mk, buoyancy=f, diffusion_substeps=1)
        _, fby, fbx = ops.karman_step_saved(d, vy, vx, re, cfg, mk, buoyancy=f)
    bu = ops.karman_step_large_bwd_buoy(d, fay, fax, re, wy, wx, wd, cfg, mk, f, vel_in=(vy, vx), diffusion_substeps=1)
    bu_ref = ops.karman_step_large_bwd_buoy(d, fby, fbx, re, wy, wx, wd, cfg, mk, f, vel_in=(vy, vx))
    from sol_amd import torch_ops
    h = torch_ops.register_scene(cfg, mk)
    op_grads = []
    for op in (lambda *a: torch.ops.sol.karman_step_sub(*a, h, 1, True, True), lambda *a: torch.ops.sol.karman_step_re(*a, h, True)):
        leaves = [t.clone().requires_grad_(True) for t in (d, vy, vx, re)]
        out = op(*leaves)
        ((out[0] * wd).sum() + (out[1] * wy).sum() + (out[2] * wx).sum()).backward()
        op_grads.append(tuple(t.detach() for t in out) + tuple(t.grad for t in leaves))
    bcv, bcm = karman.velocity_bc_masks(Y, X, batch_size=B)
    order = bc.SCENES[name][3]
    flows = []
    for kw in (dict(diffusion_substeps=1), dict()):
        sim = karman.KarmanFlow(pressure_solver=solver, cg_rtol=CG_RTOL, inflow_order=order, obstacles=_obstacles(name), **kw)
        with torch.no_grad():
            flows.append(flow_fields(sim.step(flow_state(d, vy, vx, Y, X), re=re, res=X, velBCy=bcv, velBCyMask=bcm), Y, X))
    torch.cuda.synchronize()
    for x, y in zip(bu + op_grads[0] + flows[0], bu_ref + op_grads[1] + flows[1]):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())
    for x, y in zip(flows[0], b):
        assert torch.equal(x, y)


def _obstacles(name):
    from large2d_scenes import SCENE_SPECS
    specs = SCENE_SPECS[bc.SCENES[name][2]]
    return None if specs is None else karman.parse_obstacles(specs)


# ---- 4. the adjoint against the reference's autograd -------------------------------------------------------------------------------------
def hip_grad(name, solver, n, kind, density=False, re_grad=False, force=None, info=None):
    g, mk, cfg = setup(name, solver)
    d, vy, vx, re = device_state(name)
    leaves = [t.requires_grad_(True) for t in ((d, vy, vx, re) if re_grad else (d, vy, vx))]
    out = ops.karman_step_large(d, vy, vx, re, cfg, mk, info=info, density_grad=density, re_grad=re_grad, buoyancy=force, diffusion_substeps=n)
    wd, wy, wx = bc.cotangents(name, kind)
    loss = 0.0
    if wd is not None:
        loss = loss + (out[0] * f32(wd)).sum()
    if wy is not None:
        loss = loss + (out[1] * f32(wy)).sum() + (out[2] * f32(wx)).sum()
    loss.backward()
    torch.cuda.synchronize()
    return tuple(t.detach() for t in out), tuple(torch.zeros_like(t) if t.grad is None else t.grad for t in leaves)


ADJ = [("sphere_130", "direct"), ("two_144", "cg")]


@pytest.mark.parametrize("n", dc.STEP_N)
@pytest.mark.parametrize("name,solver", ADJ)
def test_velocity_adjoint_against_the_references_autograd(name, solver, n):
    ref_out, ref_g = dc.reference(name, n, "vel")
    info = {}
    out, got = hip_grad(name, solver, n, "vel", info=info)
    assert max(rel(a, b) for a, b in zip(out, ref_out)) < TOL_FIELD
    check(got[1:], ref_g[1:], dc.needs_trim("vel", 1), "%s %s n=%d" % (name, solver, n), ("g_vy", "g_vx"))
    assert not got[0].any()                              # the density is a passive tracer in the plain mode
    if solver == "cg":
        assert info["converged_bwd"].tolist() == [1] * B
    again = hip_grad(name, solver, n, "vel")[1]          # the backward pass run twice: equal bits
    for a, b in zip(got, again):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name,solver", ADJ)
def test_density_and_reynolds_number_gradients_against_the_reference(name, solver):
    n = 5
    ref_out, ref_g = dc.reference(name, n, "both", 1, True)
    out, got = hip_grad(name, solver, n, "both", density=True, re_grad=True)
    assert max(rel(a, b) for a, b in zip(out, ref_out)) < TOL_FIELD
    check(got[:3], ref_g[:3], dc.needs_trim("both", 1), "%s %s n=%d density + re" % (name, solver, n))
    e = rel(got[3], ref_g[3])
    print("g_re %s against the reference %s: %.3e" % (got[3].tolist(), ref_g[3].tolist(), e))
    assert e < TOL_GRAD
    # a density-only loss under density_grad, without re
    ref_d = dc.reference(name, n, "dens")[1]
    got_d = hip_grad(name, solver, n, "dens", density=True)[1]
    check(got_d, ref_d, False, "%s %s n=%d density-only loss" % (name, solver, n))
    again = hip_grad(name, solver, n, "both", density=True, re_grad=True)[1]
    for a, b in zip(got, again):
        assert torch.equal(a, b)


def test_buoyancy_and_reynolds_number_gradient_together():
    name, n = "sphere_130", 5
    ref_out, ref_g = dc.reference(name, n, "both", 1, True, dc.FORCE)
    out, got = hip_grad(name, "direct", n, "both", re_grad=True, force=dc.FORCE)
    assert max(rel(a, b) for a, b in zip(out, ref_out)) < TOL_FIELD
    check(got[:3], ref_g[:3], True, "buoyant n=%d re_grad" % n)
    e = rel(got[3], ref_g[3])
    print("buoyant g_re %s against the reference %s: %.3e" % (got[3].tolist(), ref_g[3].tolist(), e))
    assert e < TOL_GRAD


# ---- 5. one-workgroup grids ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Y,X", dc.SMALL)
def test_one_workgroup_grids_forward_and_backward(Y, X):
    n = dc.SMALL_N
    g, st = dc.small_state(Y, X)
    mk = masks(g)
    assert not mk.large
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk, cg_rtol=CG_RTOL)
    wy, wx = (f32(t) for t in dc.small_cotangents(Y, X))
    for re_grad in (False, True):
        ref_out, ref_g = dc.small_reference(Y, X, n, re_grad)
        d, vy, vx, re = (f32(t) for t in st)
        leaves = [t.requires_grad_(True) for t in ((vy, vx, re) if re_grad else (vy, vx))]
        out = ops.karman_step(d, vy, vx, re, cfg, mk, re_grad=re_grad, diffusion_substeps=n)
        with torch.no_grad():
            plain = ops.karman_step(d, vy, vx, re, cfg, mk)
            ng = ops.karman_step(d, vy, vx, re, cfg, mk, diffusion_substeps=n)
        errs = [rel(a, b) for a, b in zip(out, ref_out)]
        print("%dx%d n=%d re_grad=%s: fields %s, against n = 1 vy moves by %.3f" % (Y, X, n, re_grad, errs, rel(out[1], plain[1])))
        assert max(errs) < TOL_FIELD and rel(out[1], plain[1]) > MOVED
        assert all(torch.equal(a.detach(), b) for a, b in zip(out, ng))
        ((out[1] * wy).sum() + (out[2] * wx).sum()).backward()
        torch.cuda.synchronize()
        check([t.grad for t in leaves[:2]], ref_g[:2], True, "%dx%d n=%d re_grad=%s" % (Y, X, n, re_grad), ("g_vy", "g_vx"))
        if re_grad:
            e = rel(leaves[2].grad, ref_g[2])
            print("g_re %s against the reference %s: %.3e" % (leaves[2].grad.tolist(), ref_g[2].tolist(), e))
            assert e < TOL_GRAD


# ---- 6. surfaces ---------------------------------------------------------------------------------------------------------------------------
def flow_state(d, vy, vx, Y, X):
    dom = fluid.Domain([Y, X], box=fluid.box[0:200, 0:100])
    vel = fluid.StaggeredGrid([vy.reshape(B, Y + 1, X, 1), vx.reshape(B, Y, X + 1, 1)], dom.box)
    return fluid.Fluid(dom, density=d.reshape(B, Y, X, 1), velocity=vel, batch_size=B)


def flow_fields(s, Y, X):
    return s.density.data.reshape(B, Y, X), s.velocity.data[0].data.reshape(B, Y + 1, X), s.velocity.data[1].data.reshape(B, Y, X + 1)


def test_karman_flow_and_the_torch_op_give_the_ops_calls_bits():
    from sol_amd import torch_ops
    name, n = "sphere_130", 5
    Y, X = bc.SCENES[name][:2]
    g, mk, cfg = setup(name, "direct")
    wd, wy, wx = (f32(t) for t in bc.cotangents(name, "both"))
    ref_out, ref_g = hip_grad(name, "direct", n, "both", density=True, re_grad=True)
    # torch.ops.sol.karman_step_sub
    h = torch_ops.register_scene(cfg, mk)
    d, vy, vx, re = device_state(name)
    leaves = [t.requires_grad_(True) for t in (d, vy, vx, re)]
    out = torch.ops.sol.karman_step_sub(d, vy, vx, re, h, n, True, True)
    ((out[0] * wd).sum() + (out[1] * wy).sum() + (out[2] * wx).sum()).backward()
    for a, b in zip(tuple(out) + tuple(t.grad for t in leaves), ref_out + ref_g):
        assert torch.equal(a.detach(), b)
    with torch.no_grad():
        ng = torch.ops.sol.karman_step_sub(d, vy, vx, re, h, n)
    assert all(torch.equal(a, b) for a, b in zip(ng, ref_out))
    # KarmanFlow(diffusion_substeps=n): backward() fills the gradients
    d, vy, vx, re = device_state(name)
    leaves = [t.requires_grad_(True) for t in (d, vy, vx, re)]
    sim = karman.KarmanFlow(diffusion_substeps=n, density_grad=True, re_grad=True, cg_rtol=CG_RTOL)
    bcv, bcm = karman.velocity_bc_masks(Y, X, batch_size=B)
    s = sim.step(flow_state(d, vy, vx, Y, X), re=re, res=X, velBCy=bcv, velBCyMask=bcm)
    od, oy, ox = flow_fields(s, Y, X)
    ((od * wd).sum() + (oy * wy).sum() + (ox * wx).sum()).backward()
    torch.cuda.synchronize()
    for a, b in zip((od, oy, ox) + tuple(t.grad for t in leaves), ref_out + ref_g):
        assert a is not None and torch.equal(a.detach(), b)


def test_two_chained_flow_steps_against_the_reference():
    name, n = "sphere_130", 2
    Y, X = bc.SCENES[name][:2]
    ref_out, ref_g = dc.reference(name, n, "both", 2)
    d, vy, vx, re = device_state(name, steps=2)
    leaves = [t.requires_grad_(True) for t in (d, vy, vx)]
    sim = karman.KarmanFlow(diffusion_substeps=n, density_grad=True, cg_rtol=CG_RTOL)
    bcv, bcm = karman.velocity_bc_masks(Y, X, batch_size=B)
    s = flow_state(d, vy, vx, Y, X)
    for _ in range(2):
        s = sim.step(s, re=re.tolist(), res=X, velBCy=bcv, velBCyMask=bcm)
    out = flow_fields(s, Y, X)
    errs = [rel(a, b) for a, b in zip(out, ref_out)]
    print("two chained steps n=%d: fields %s" % (n, errs))
    assert max(errs) < TOL_FIELD
    wd, wy, wx = (f32(t) for t in bc.cotangents(name, "both"))
    ((out[0] * wd).sum() + (out[1] * wy).sum() + (out[2] * wx).sum()).backward()
    torch.cuda.synchronize()
    check(tuple(t.grad for t in leaves), ref_g, dc.needs_trim("both", 2), "two chained KarmanFlow.step n=%d" % n)


# ---- 7. LargeGridTrainer(diffusion_substeps=) ----------------------------------------------------------------------------------------------
def _net_of(p):
    net = sol_amd.model_mars_moon(cin=3, cout=2, seed=0)
    net.set_weights([q.detach().numpy() for q in p["params"]])
    return net


def test_large_grid_trainer_against_the_reference_and_replayed():
    """144 x 72 (the smallest grid LargeGridTrainer accepts, any_width=True), B = 1, two steps, mars_moon, n = 4, at the tolerances of
    test_gpu_karman2d_large_trainer.py: loss and per-step losses 1e-5, full weight gradient TOL_GRAD, captured against eager 1e-6."""
    Y, X = dc.TRAINER_GRID
    n, ms = dc.TRAINER_N, 2
    p = dc.trainer_problem(ms)
    lref, steps_ref, gref, fin_ref = dc.trainer_reference(p, n)
    te = sol_amd.make_trainer(_net_of(p), None, 1, Y, X, ms, 100.0 / X, dc.TRAINER_STD_V, o.STD_RE, use_graph=False, any_width=True,
                              diffusion_substeps=n)
    assert isinstance(te, sol_amd.LargeGridTrainer) and te.diffusion_substeps == n
    args = (f32(p["d"]), f32(p["vy"]), f32(p["vx"]), f32(p["re"]), f32(torch.stack(p["gt_vy"])), f32(torch.stack(p["gt_vx"])))
    loss = float(te.fwd_bwd(*args, want_final=True))
    e_l, e_g = abs(loss - lref) / abs(lref), rel(te.grads, gref)
    e_s = [abs(a - b) / abs(b) for a, b in zip(te.loss_steps.tolist(), steps_ref)]
    e_f = [rel(a, b) for a, b in zip(te.final, fin_ref)]
    print("LargeGridTrainer(diffusion_substeps=%d) vs float64 reference: loss %.3e, per-step %s, gradient %.3e, final state %s" % (n, e_l, e_s, e_g, e_f))
    assert e_l < 1e-5 and max(e_s) < 1e-5 and e_g < TOL_GRAD and max(e_f) < TOL_FIELD, (e_l, e_s, e_g, e_f)
    g_eager, l_eager = te.grads.clone(), te.loss_steps.clone()
    # with n = 1 the same trainer computes something else (the CPU twin measures how far: TRAINER_N1_PIN)
    t1 = sol_amd.LargeGridTrainer(_net_of(p), 1, Y, X, ms, dc.TRAINER_STD_V, o.STD_RE, use_graph=False, any_width=True)
    assert t1.diffusion_substeps == 1 and abs(float(t1.fwd_bwd(*args)) - lref) > 0.05 * abs(lref)
    tg = sol_amd.LargeGridTrainer(_net_of(p), 1, Y, X, ms, dc.TRAINER_STD_V, o.STD_RE, any_width=True, diffusion_substeps=n)
    lg = float(tg.fwd_bwd(*args))
    assert tg._graph is not None
    e_g = rel(tg.grads, g_eager)
    print("captured vs eager: loss %.3e gradient %.3e" % (abs(lg - loss) / abs(loss), e_g))
    assert abs(lg - loss) <= 1e-6 * abs(loss) and e_g < 1e-6 and rel(tg.loss_steps, l_eager) < 1e-6
    g1 = tg.grads.clone()
    assert float(tg.fwd_bwd(*args)) == lg and torch.equal(tg.grads, g1)


# ---- 8. LargeGridRollout(diffusion_substeps=) ----------------------------------------------------------------------------------------------
ROLLOUT_GROWTH = 1.5          # the CPU twin: the float32 reference's error after four steps is 1.02 x its error after one (pinned < 1.5)


def test_large_grid_rollout_equals_the_hand_composition_and_matches_the_reference():
    from sol_amd.schedule2d import NetSchedule2D
    Y, X = dc.TRAINER_GRID
    n, steps = dc.TRAINER_N, 4
    p = dc.trainer_problem(2)
    g = p["g"]
    ref = dc.rollout_reference(p, n, steps)
    runs = []
    for kw in (dict(use_graph=True), dict(use_graph=False)):
        ro = sol_amd.make_rollout(_net_of(p), masks(g), 1, Y, X, g.dx, dc.TRAINER_STD_V, o.STD_RE, any_width=True, diffusion_substeps=n, **kw)
        assert isinstance(ro, sol_amd.LargeGridRollout) and ro.diffusion_substeps == n
        h = tuple(f32(p[k]) for k in ("d", "vy", "vx", "re"))
        ro.run(*h, steps)
        errs = [rel(a, b) for a, b in zip(h[:3], ref)]
        print("LargeGridRollout(diffusion_substeps=%d, %s) after %d steps: d %.3e vy %.3e vx %.3e" % ((n, kw, steps) + tuple(errs)))
        assert max(errs) < ROLLOUT_GROWTH * TOL_FIELD, errs
        runs.append(h[:3])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    # the step plus network composed by hand: the same bits
    mk = masks(g)
    cfg = ops.karman_cfg(1, Y, X, g.dx, masks=mk)
    net = _net_of(p)
    sched = NetSchedule2D(net, 1, Y, X, train=False, any_width=True)
    fs = (1.0 / dc.TRAINER_STD_V[0], 1.0 / dc.TRAINER_STD_V[1], 1.0 / o.STD_RE)
    d, vy, vx, re = (f32(p[k]) for k in ("d", "vy", "vx", "re"))
    feat = torch.zeros(1, Y, X, 4, dtype=torch.float32, device=DEV)
    with torch.no_grad():
        sched.begin_step()
        for _ in range(steps):
            d, vy, vx = ops.karman_step_large(d, vy, vx, re, cfg, mk, feat=feat, feat_scale=fs, diffusion_substeps=n)
            out, _ = sched.forward(feat)
            ops.karman_correct(out, vy, vx, dc.TRAINER_STD_V)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((d, vy, vx), runs[0]))


# ---- 9. stability --------------------------------------------------------------------------------------------------------------------------
def test_four_substeps_stay_bounded_where_the_single_stencil_blows_up():
    """32 x 16, alpha = 0.85, 40 steps without a network (the CPU twin's float64 run: n = 4 ends at about the initial max|v|, n = 1 beyond 1e3)"""
    S = dc.STABILITY
    Y, X = S["Y"], S["X"]
    g = o.KarmanGeometry(Y, X)
    mk = masks(g)
    cfg = ops.karman_cfg(1, Y, X, g.dx, masks=mk)
    from large2d_scenes import state
    d0, vy0, vx0, _ = state(1, Y, X, dc.SEED, g)
    re = f32(torch.tensor([float(np.float32(X * X / S["alpha"]))]))
    first = max(float(vy0.abs().max()), float(vx0.abs().max()))
    last = {}
    for n in (S["n"], 1):
        d, vy, vx = f32(d0), f32(vy0), f32(vx0)
        with torch.no_grad():
            for _ in range(S["steps"]):
                d, vy, vx = ops.karman_step(d, vy, vx, re, cfg, mk, diffusion_substeps=n)
        v = torch.cat([vy.reshape(-1), vx.reshape(-1)])
        last[n] = float(v.abs().max()) if bool(torch.isfinite(v).all()) else float("inf")
    print("max|v| initially %.3f; after %d steps: n = %d %.3f, n = 1 %.3e" % (first, S["steps"], S["n"], last[S["n"]], last[1]))
    assert last[S["n"]] < 2 * first and last[1] > 1e3


# ---- 10. the scripts -----------------------------------------------------------------------------------------------------------------------
def _script(name):
    import importlib.util
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    if sdir not in sys.path:
        sys.path.insert(0, sdir)
    spec = importlib.util.spec_from_file_location("sol_script_sub_" + name, os.path.join(sdir, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_training_script_takes_the_count_from_the_set_and_records_it(tmp_path):
    """karman.py -r 80 --diffusion-substeps 4 twice -> karman_train.py for two steps without the flag: the count is picked up from the
    set and recorded in dataStats.pickle; a contradicting flag is refused"""
    import pickle
    for re_nr in (8000.0, 16000.0):
        _script("karman").main(["-o", str(tmp_path / "set"), "-r", "80", "-t", "7", "-s", "1", "--re", str(re_nr), "--diffusion-substeps", "4"])
    tf = str(tmp_path / "tf")
    train = ["--train", str(tmp_path / "set"), "-s", "1", "-n", "2", "-b", "1", "-t", "5", "-m", "2", "-e", "1", "--lr", "1e-4", "--tf", tf, "--seed", "0",
             "--any-width"]
    with pytest.raises(SystemExit, match="contradicts"):
        _script("karman_train").main(train + ["--diffusion-substeps", "2"])
    loss = _script("karman_train").main(train)
    assert loss is not None and np.isfinite(loss)
    with open(tf + "/dataStats.pickle", "rb") as f:
        assert pickle.load(f)["diffusion_substeps"] == 4


def test_script_records_auto_substeps_and_its_frames_equal_the_library_step(tmp_path):
    import pickle
    from sol_amd import scene
    load = _script

    re_nr, res = 8000.0, 80
    want = ops.min_diffusion_substeps(re_nr, res)
    assert want == 4                                      # alpha = 0.8
    run = load("karman").main(["-o", str(tmp_path / "sub"), "-r", str(res), "-t", "5", "-s", "0", "--re", str(re_nr), "--diffusion-substeps", "auto"])
    with open(run + "/params.pickle", "rb") as f:
        assert pickle.load(f)["diffusion_substeps"] == want
    plain = load("karman").main(["-o", str(tmp_path / "plain"), "-r", str(res), "-t", "5", "-s", "0", "--re", str(re_nr)])
    with open(plain + "/params.pickle", "rb") as f:
        assert pickle.load(f)["diffusion_substeps"] == 1
    # a frame is KarmanFlow(diffusion_substeps=want).step applied to the previous frame
    Y, X = 2 * res, res
    frames = [scene.read_zipped_array(os.path.join(run, "velo_%06d.npz" % i)) for i in range(5)]
    dens = [scene.read_zipped_array(os.path.join(run, "dens_%06d.npz" % i)) for i in range(5)]
    assert all(np.isfinite(f).all() for f in frames)
    assert np.abs(frames[4] - scene.read_zipped_array(os.path.join(plain, "velo_000004.npz"))).max() > 1e-3
    dom = fluid.Domain([Y, X], box=fluid.box[0:200, 0:100])
    sim = karman.KarmanFlow(diffusion_substeps=want)
    bcv, bcm = karman.velocity_bc_masks(Y, X, batch_size=1)
    st = fluid.Fluid(dom, density=dens[3], velocity=frames[3], batch_size=1)
    with torch.no_grad():
        st = sim.step(st, re=[re_nr], res=res, velBCy=bcv, velBCyMask=bcm)
    assert np.array_equal(st.velocity.staggered_tensor().cpu().numpy(), frames[4])
    assert np.array_equal(st.density.data.cpu().numpy(), dens[4])
    # karman_apply.py picks the count up from the statistics file (as karman_train.py writes it): its first frame is one step of
    # LargeGridRollout(diffusion_substeps=want) from the script's start state; a contradicting flag is refused
    net = sol_amd.model_mars_moon(cin=3, cout=2, seed=0)
    net.save(str(tmp_path / "model.pt"))
    stats = {"std": (1.0, (0.2, 0.2)), "ext.std": (o.STD_RE,), "scene": None, "buoyancy": None, "diffusion_substeps": want}
    with open(tmp_path / "dataStats.pickle", "wb") as f:
        pickle.dump(stats, f)
    apply_args = ["-r", str(res), "-t", "2", "--re", str(re_nr), "--stats", str(tmp_path / "dataStats.pickle"), "--model", str(tmp_path / "model.pt"),
                  "--any-width"]
    with pytest.raises(SystemExit, match="contradicts"):
        load("karman_apply").main(["-o", str(tmp_path / "bad")] + apply_args + ["--diffusion-substeps", "2"])
    out = load("karman_apply").main(["-o", str(tmp_path / "run")] + apply_args)
    got = scene.read_zipped_array(os.path.join(out, "velTf_000001.npz"))
    g = o.KarmanGeometry(Y, X)
    ro = sol_amd.make_rollout(net, masks(g), 1, Y, X, g.dx, (0.2, 0.2), o.STD_RE, any_width=True, diffusion_substeps=want)
    vy0, vx0 = scene.split_staggered(np.asarray(frames[0], dtype=np.float32))
    d, vy, vx, re = f32(dens[0][..., 0]), f32(vy0), f32(vx0), f32([re_nr])
    ro.run(d, vy, vx, re, 1)
    exp = fluid.StaggeredGrid([vy.reshape(1, Y + 1, X, 1), vx.reshape(1, Y, X + 1, 1)]).staggered_tensor().cpu().numpy()
    assert np.array_equal(got, exp)
