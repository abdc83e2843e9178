"""MacCormack advection on the large-grid karman-2d step, on the GPU (pytest -m gpu): csrc/karman_maccormack.hip behind ops.karman_advect /
karman_advect_bwd, ops.karman_step_large / karman_step_saved and their adjoints (advection="mac_cormack"), against the float64 reference of
maccormack_cases.py (the oracle's stages and sampler + the definition in include/sol_hip.h).

Tolerances are the suite's (large2d_scenes): TOL_FIELD = 1e-5 on fields, TOL_GRAD = 1e-4 relative L2 on gradients, CG_RTOL = 1e-7.  The
limiter and the clamped edges tie exactly in places and fp32 decides a few entries the other way, so EVERY gradient comparison here uses
the trimmed metric with the cap as a condition (at most TRIM = 0.1 % of the entries left out).  The inputs are fixed and conditioned on the
reference ALONE: test_karman2d_maccormack_cpu.py measures the reference in float32 against float64 on every case below and pins it."""
import os
import sys

import pytest
import torch

import sol_amd
import sol_oracle as o
from sol_amd import _lib, ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buoyancy_cases as bc
import maccormack_cases as mc
from large2d_scenes import CG_RTOL, DEV, TOL_FIELD, TOL_GRAD, TRIM, f32, masks, rel, trimmed_rel

pytestmark = pytest.mark.gpu
B = mc.B
MC = dict(advection="mac_cormack")
RUNS = [(n, s) for n in ("sphere_130", "two_144", "before_160") for s in bc.SCENES[n][4]]


def setup(name, solver, **kw):
    Y, X, _, order, _ = bc.SCENES[name]
    g = bc.geometry_of(name)
    mk = masks(g, solver)
    assert mk.pressure_solver == solver and mk.large
    return g, mk, ops.karman_cfg(B, Y, X, g.dx, masks=mk, cg_rtol=CG_RTOL, inflow_order=order, **kw)


def check(got, ref, what, names=("g_d", "g_vy", "g_vx"), tol=TOL_GRAD):
    """every gradient by the trimmed metric, the cap a condition; every figure printed before it is asserted"""
    for name, a, b in zip(names, got, ref):
        v, k, worst = trimmed_rel(a, b)
        print("%s %s: rel L2 %.3e untrimmed, %.3e after leaving out %d of %d entries (largest deviation left out %.3e)"
              % (what, name, rel(a, b), v, k, b.numel(), worst))
        assert k <= int(TRIM * b.numel())
        assert v < tol, (what, name, v)


class option:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = _lib.get_option(self.name)
        _lib.set_option(self.name, self.value)

    def __exit__(self, *exc):
        _lib.set_option(self.name, self.old)


# ---- 1. the stage alone, forward --------------------------------------------------------------------------------------------------------
def stage_setup(Y, X, order, cfl=None):
    g = mc.stage_geometry(Y, X)
    cfg = ops.karman_cfg(mc.STAGE_B, Y, X, g.dx, inflow_order=order)
    return g, cfg, tuple(f32(t) for t in mc.stage_inputs(Y, X, cfl))


STAGE_CASES = [(Y, X, s, order, None) for (Y, X) in mc.STAGE_SHAPES for s in mc.STRENGTHS for order in ("after", "before")]
STAGE_CASES += [(130, 65, 1.0, "after", 6.0)]          # departure points beyond the halo of the tiled form


@pytest.mark.parametrize("Y,X,s,order,cfl", STAGE_CASES)
def test_advect_alone_against_float64_and_tiled_equals_two_launch(Y, X, s, order, cfl):
    g, cfg, (d, cy, cx, _, _, _) = stage_setup(Y, X, order, cfl)
    ref, _, reverted = mc.stage_reference(Y, X, s, order, cfl)
    act, infl = f32(g.active), f32(g.inflow)
    assert _lib.get_option("k2d_mc_tile") == 1
    out = ops.karman_advect(d, cy, cx, cfg, act, infl, correction_strength=s, **MC)
    with option("k2d_mc_tile", 0):
        two = ops.karman_advect(d, cy, cx, cfg, act, infl, correction_strength=s, **MC)
    plain = ops.karman_advect(d, cy, cx, cfg, act, infl)
    sl = mc.stage_reference(Y, X, s, order, cfl, "semi_lagrangian")[0]
    torch.cuda.synchronize()
    errs = [rel(a, b) for a, b in zip(out, ref)]
    print("advect %dx%d s=%s %s cfl=%s: d %.3e ay %.3e ax %.3e; reverted %s; differs from semi-Lagrangian by %.2f"
          % ((Y, X, s, order, cfl) + tuple(errs) + (["%.3f" % r for r in reverted], rel(out[0], plain[0]))))
    for a, b in zip(out, two):
        assert torch.equal(a, b)
    assert max(rel(a, b) for a, b in zip(plain, sl)) < TOL_FIELD
    assert rel(out[0], plain[0]) > 0.05                     # a surface that ignored the keyword could not pass
    assert max(errs) < TOL_FIELD, errs


# ---- 2. no new extrema; the blob keeps its peak ---------------------------------------------------------------------------------------------
def test_no_new_extrema_and_the_blob_keeps_its_peak():
    Y, X = mc.BLOB["Y"], mc.BLOB["X"]
    cfg = ops.karman_cfg(1, Y, X, 1.0)
    d, cy, cx = (f32(t) for t in mc.blob_inputs())
    act, zero = torch.ones(Y, X, dtype=torch.float32, device=DEV), torch.zeros(Y, X, dtype=torch.float32, device=DEV)
    dm, ds = d, d
    for _ in range(mc.BLOB["steps"]):
        nxt = ops.karman_advect(dm, cy, cx, cfg, act, zero, **MC)[0]
        assert float(nxt.max()) <= float(dm.max()) and float(nxt.min()) >= min(0.0, float(dm.min()))
        dm = nxt
        ds = ops.karman_advect(ds, cy, cx, cfg, act, zero)[0]
    peak, ref, plain = float(dm.max()), mc.blob_peak("mac_cormack"), float(ds.max())
    print("blob peak after %d steps: mac_cormack %.6f (float64 %.6f), semi_lagrangian %.6f" % (mc.BLOB["steps"], peak, ref, plain))
    assert abs(peak - ref) < 1e-4 * ref
    assert peak > 2.0 * plain
    # seeded noise, s = 1, no inflow: within the input's range (and the ghost ring's zero)
    g, cfg, (d, cy, cx, _, _, _) = stage_setup(130, 65, "after")
    out = ops.karman_advect(d, cy, cx, cfg, f32(g.active), torch.zeros(130, 65, dtype=torch.float32, device=DEV), **MC)[0]
    assert float(out.max()) <= float(d.max()) and float(out.min()) >= min(0.0, float(d.min()))


# ---- 3. the stage alone, adjoint ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Y,X,s,order,cfl", STAGE_CASES)
def test_advect_bwd_against_autograd_tiled_equals_global_and_is_reproducible(Y, X, s, order, cfl):
    g, cfg, (d, cy, cx, gd, gy, gx) = stage_setup(Y, X, order, cfl)
    _, ref, _ = mc.stage_reference(Y, X, s, order, cfl)
    act, infl = f32(g.active), f32(g.inflow)
    run = lambda **kw: ops.karman_advect_bwd(d, cy, cx, cfg, act, infl, gd, gy, gx, correction_strength=s, **MC, **kw)
    got, again, glob = run(), run(), run(tile=False)
    torch.cuda.synchronize()
    check(got, ref, "advect_bwd %dx%d s=%s %s cfl=%s" % (Y, X, s, order, cfl), ("g_d", "g_cy", "g_cx"))
    for a, b, c in zip(got, again, glob):
        assert torch.equal(a, b) and torch.equal(a, c) and bool(torch.isfinite(a).all())


def test_advect_bwd_semi_lagrangian_against_autograd():
    Y, X = 40, 24
    g, cfg, (d, cy, cx, gd, gy, gx) = stage_setup(Y, X, "after")
    ref = mc.stage_reference(Y, X, 1.0, "after", None, "semi_lagrangian")[1]
    got = ops.karman_advect_bwd(d, cy, cx, cfg, f32(g.active), f32(g.inflow), gd, gy, gx)
    check(got, ref, "advect_bwd semi_lagrangian", ("g_d", "g_cy", "g_cx"))


@pytest.mark.parametrize("which", ["density", "velocity"])
def test_a_nan_cotangent_poisons_its_simulation_alone(which):
    Y, X = 40, 24
    g, cfg, (d, cy, cx, gd, gy, gx) = stage_setup(Y, X, "after")
    act, infl = f32(g.active), f32(g.inflow)
    clean = ops.karman_advect_bwd(d, cy, cx, cfg, act, infl, gd, gy, gx, **MC)
    gd, gy = gd.clone(), gy.clone()
    (gd if which == "density" else gy)[1, 7, 5] = float("nan")
    got = ops.karman_advect_bwd(d, cy, cx, cfg, act, infl, gd, gy, gx, **MC)
    torch.cuda.synchronize()
    for a, b in zip(got, clean):
        assert bool(torch.isnan(a[1]).all())
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])


# ---- 4. the full step forward -----------------------------------------------------------------------------------------------------------------
def device_state(name, **kw):
    return tuple(f32(t) for t in mc.start_state(name, **kw))


@pytest.mark.parametrize("name,solver", RUNS)
def test_step_forward_against_the_reference(name, solver):
    g, mk, cfg = setup(name, solver)
    d, vy, vx, re = device_state(name)
    ref = mc.reference(name)[0]
    info = {}
    with torch.no_grad():
        out = ops.karman_step_large(d, vy, vx, re, cfg, mk, info=info, **MC)
        plain = ops.karman_step_large(d, vy, vx, re, cfg, mk)
        saved, svy, svx = ops.karman_step_saved(d, vy, vx, re, cfg, mk, **MC)
        with option("k2d_mc_tile", 0):
            two = ops.karman_step_large(d, vy, vx, re, cfg, mk, **MC)
    errs = [rel(a, b) for a, b in zip(out, ref)]
    print("forward %s %s: d %.3e vy %.3e vx %.3e; differs from the plain step by d %.3f vx %.3f"
          % ((name, solver) + tuple(errs) + (rel(out[0], plain[0]), rel(out[2], plain[2]))))
    assert max(errs) < TOL_FIELD, errs
    if solver == "cg":
        assert info["converged"].tolist() == [1] * B
    for a, b, c in zip(saved, out, two):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert rel(out[0], plain[0]) > 0.03 and rel(out[2], plain[2]) > 0.03


@pytest.mark.parametrize("s,cfl", [(0.5, None), (1.0, 2.5), (1.0, 6.0)])
def test_step_forward_at_half_strength_and_high_cfl(s, cfl):
    name = "sphere_130"
    g, mk, cfg = setup(name, "direct")
    d, vy, vx, re = device_state(name, cfl=cfl)
    ref = mc.reference(name, s, cfl=cfl)[0]
    with torch.no_grad():
        out = ops.karman_step_large(d, vy, vx, re, cfg, mk, correction_strength=s, **MC)
    errs = [rel(a, b) for a, b in zip(out, ref)]
    print("forward s=%s cfl=%s:" % (s, cfl), errs)
    assert max(errs) < TOL_FIELD, errs


# ---- 5. the adjoint against the reference's autograd ---------------------------------------------------------------------------------------------
def hip_grad(name, solver, kind, steps=1, s=1.0, force=None, n=1, re_grad=False, cfl=None, density_grad=True):
    g, mk, cfg = setup(name, solver)
    d, vy, vx, re = device_state(name, steps=steps, cfl=cfl)
    leaves = [t.requires_grad_(True) for t in ((d, vy, vx, re) if re_grad else (d, vy, vx))]
    out = (d, vy, vx)
    for _ in range(steps):
        out = ops.karman_step_large(*out, re, cfg, mk, density_grad=density_grad, re_grad=re_grad, buoyancy=force, diffusion_substeps=n,
                                    correction_strength=s, **MC)
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
@pytest.mark.parametrize("name,solver", RUNS)
def test_adjoint_against_the_references_autograd(name, solver, kind):
    ref_out, ref_g, _ = mc.reference(name, 1.0, kind)
    out, got = hip_grad(name, solver, kind)
    assert max(rel(a, b) for a, b in zip(out, ref_out)) < TOL_FIELD
    check(got, ref_g, "adjoint %s %s %s" % (name, solver, kind))
    assert float(got[1].abs().max()) > 0


@pytest.mark.parametrize("name,solver", [("sphere_130", "direct"), ("two_144", "cg"), ("before_160", "direct")])
def test_two_chained_steps_against_the_references_autograd(name, solver):
    ref_out, ref_g, _ = mc.reference(name, 1.0, "both", 2)
    out, got = hip_grad(name, solver, "both", steps=2)
    assert max(rel(a, b) for a, b in zip(out, ref_out)) < TOL_FIELD
    check(got, ref_g, "two steps %s %s" % (name, solver))


@pytest.mark.parametrize("s,cfl", [(0.5, None), (1.0, 2.5), (1.0, 6.0)])
def test_adjoint_at_half_strength_and_high_cfl(s, cfl):
    ref_out, ref_g, _ = mc.reference("sphere_130", s, "both", cfl=cfl)
    out, got = hip_grad("sphere_130", "direct", "both", s=s, cfl=cfl)
    check(got, ref_g, "adjoint s=%s cfl=%s" % (s, cfl))


def test_a_velocity_only_loss_without_density_grad_leaves_the_density_out():
    ref_g = mc.reference("sphere_130", 1.0, "vel")[1]
    g, mk, cfg = setup("sphere_130", "direct")
    d, vy, vx, re = device_state("sphere_130")
    vy.requires_grad_(True), vx.requires_grad_(True)
    out = ops.karman_step_large(d, vy, vx, re, cfg, mk, **MC)
    assert not out[0].requires_grad
    wy, wx = (f32(t) for t in bc.cotangents("sphere_130", "vel")[1:])
    ((out[1] * wy).sum() + (out[2] * wx).sum()).backward()
    check((vy.grad, vx.grad), ref_g[1:], "velocity mode", ("g_vy", "g_vx"))
    # the staged entry points by hand give the autograd function's bits
    with torch.no_grad():
        _, svy, svx = ops.karman_step_saved(d, vy, vx, re, cfg, mk, **MC)
        hy, hx = ops.karman_step_large_bwd(svy, svx, re, wy, wx, cfg, mk, **MC)
    assert torch.equal(hy, vy.grad) and torch.equal(hx, vx.grad)


# ---- 6. composition -----------------------------------------------------------------------------------------------------------------------
def test_with_a_buoyancy_force():
    ref_out, ref_g, _ = mc.reference("sphere_130", 1.0, "both", force=mc.FORCE)
    out, got = hip_grad("sphere_130", "direct", "both", force=mc.FORCE)
    assert max(rel(a, b) for a, b in zip(out, ref_out)) < TOL_FIELD
    check(got, ref_g, "with buoyancy")


def test_with_diffusion_substeps_and_re_grad():
    # (144 x 72: the scene on which the reference's own float32 g_re holds, 2.4e-6 -- the CPU twin; g_re is one number per simulation and
    # cannot be trimmed, and at 130 x 65 a few faces that fp32 torch decides the other way move it by 2e-4)
    ref_out, ref_g, _ = mc.reference("two_144", 1.0, "both", n=mc.NSUB, re_grad=True)
    out, got = hip_grad("two_144", "cg", "both", n=mc.NSUB, re_grad=True)
    assert max(rel(a, b) for a, b in zip(out, ref_out)) < TOL_FIELD
    check(got[:3], ref_g[:3], "with substeps and re_grad")
    e = rel(got[3], ref_g[3])
    print("g_re: rel %.3e" % e, got[3].tolist(), ref_g[3].tolist())
    assert e < TOL_GRAD


def test_with_force_substeps_and_re_grad_together():
    ref_out, ref_g, _ = mc.reference("two_144", 1.0, "both", force=mc.FORCE, n=mc.NSUB, re_grad=True)
    out, got = hip_grad("two_144", "cg", "both", force=mc.FORCE, n=mc.NSUB, re_grad=True)
    assert max(rel(a, b) for a, b in zip(out, ref_out)) < TOL_FIELD
    check(got[:3], ref_g[:3], "all three")
    assert rel(got[3], ref_g[3]) < TOL_GRAD


# ---- 7. the default keyword gives the bits of a call without it ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,solver", [("sphere_130", "direct"), ("two_144", "cg")])
def test_semi_lagrangian_gives_the_bits_of_a_call_without_the_keyword(name, solver):
    g, mk, cfg = setup(name, solver)
    d, vy, vx, re = device_state(name)
    wd, wy, wx = (f32(t) for t in bc.cotangents(name, "both"))
    SL = dict(advection="semi_lagrangian", correction_strength=0.5)
    with torch.no_grad():
        a = ops.karman_step_large(d, vy, vx, re, cfg, mk, **SL)
        b = ops.karman_step_large(d, vy, vx, re, cfg, mk)
        sa, say, sax = ops.karman_step_saved(d, vy, vx, re, cfg, mk, **SL)
        sb, sby, sbx = ops.karman_step_saved(d, vy, vx, re, cfg, mk)
    for x, y in zip(a + sa + (say, sax), b + sb + (sby, sbx)):
        assert torch.equal(x, y)
    ga = ops.karman_density_bwd(d, say, sax, re, wd, cfg, mk, *ops.karman_step_large_bwd(say, sax, re, wy, wx, cfg, mk, **SL), **SL)
    gb = ops.karman_density_bwd(d, sby, sbx, re, wd, cfg, mk, *ops.karman_step_large_bwd(sby, sbx, re, wy, wx, cfg, mk))
    ra = ops.karman_step_large_bwd_re(say, sax, re, wy, wx, vy, vx, cfg, mk, **SL)
    rb = ops.karman_step_large_bwd_re(sby, sbx, re, wy, wx, vy, vx, cfg, mk)
    torch.cuda.synchronize()
    for x, y in zip(ga + ra, gb + rb):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())
    # the autograd function, default keyword against none
    grads = []
    for kw in (SL, {}):
        leaves = [t.clone().requires_grad_(True) for t in (d, vy, vx)]
        out = ops.karman_step_large(*leaves, re, cfg, mk, density_grad=True, **kw)
        ((out[0] * wd).sum() + (out[1] * wy).sum() + (out[2] * wx).sum()).backward()
        grads.append([t.grad for t in leaves])
    for x, y in zip(*grads):
        assert torch.equal(x, y)


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_a_one_workgroup_grid_refuses_mac_cormack():
    Y, X = 64, 32
    g = o.KarmanGeometry(Y, X)
    mk = masks(g)
    assert not mk.large
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk)
    d, vy, vx = (torch.zeros(B, *s, dtype=torch.float32, device=DEV) for s in ((Y, X), (Y + 1, X), (Y, X + 1)))
    re = torch.full((B,), 1e5, dtype=torch.float32, device=DEV)
    for call in (lambda: ops.karman_step_large(d, vy, vx, re, cfg, mk, **MC), lambda: ops.karman_step_saved(d, vy, vx, re, cfg, mk, **MC),
                 lambda: ops.karman_step_large_bwd(vy, vx, re, vy, vx, cfg, mk, **MC)):
        with pytest.raises(sol_amd.SolError, match="multi-launch"):
            call()


# ---- 7b. KarmanFlow and the torch op give the ops call's bits -----------------------------------------------------------------------------------
def _obstacles(name):
    from large2d_scenes import SCENE_SPECS
    from sol_amd import karman
    specs = SCENE_SPECS[bc.SCENES[name][2]]
    return None if specs is None else karman.parse_obstacles(specs)


def flow_state(d, vy, vx, Y, X):
    from sol_amd import fluid
    dom = fluid.Domain([Y, X], box=fluid.box[0:200, 0:100])
    vel = fluid.StaggeredGrid([vy.reshape(B, Y + 1, X, 1), vx.reshape(B, Y, X + 1, 1)])
    return fluid.Fluid(dom, density=d.reshape(B, Y, X, 1), velocity=vel, batch_size=B)


def flow_fields(st, Y, X):
    return (st.density.data.reshape(B, Y, X), st.velocity.data[0].data.reshape(B, Y + 1, X), st.velocity.data[1].data.reshape(B, Y, X + 1))


@pytest.mark.parametrize("name,solver", [("sphere_130", "direct"), ("two_144", "cg")])
def test_karman_flow_and_the_torch_op_give_the_ops_bits(name, solver):
    from sol_amd import karman, torch_ops
    g, mk, cfg = setup(name, solver)
    Y, X, order = bc.SCENES[name][0], bc.SCENES[name][1], bc.SCENES[name][3]
    d, vy, vx, re = device_state(name)
    wd, wy, wx = (f32(t) for t in bc.cotangents(name, "both"))
    bcv, bcm = karman.velocity_bc_masks(Y, X, batch_size=B)
    h = torch_ops.register_scene(cfg, mk)
    s = 0.75

    def run(step):
        leaves = [t.clone().requires_grad_(True) for t in (d, vy, vx)]
        out = step(*leaves)
        ((out[0] * wd).sum() + (out[1] * wy).sum() + (out[2] * wx).sum()).backward()
        return tuple(t.detach() for t in out) + tuple(t.grad for t in leaves)

    for adv, code in (("mac_cormack", 1), ("semi_lagrangian", 0)):
        kw = dict(advection=adv, correction_strength=s)
        sim = karman.KarmanFlow(pressure_solver=solver, cg_rtol=CG_RTOL, inflow_order=order, obstacles=_obstacles(name), density_grad=True, **kw)
        a = run(lambda *t: ops.karman_step_large(*t, re, cfg, mk, density_grad=True, **kw))
        b = run(lambda *t: torch.ops.sol.karman_step_adv(*t, re, h, code, s, 1, True))
        c = run(lambda *t: flow_fields(sim.step(flow_state(*t, Y, X), re=re, res=X, velBCy=bcv, velBCyMask=bcm), Y, X))
        torch.cuda.synchronize()
        for x, y, z in zip(a, b, c):
            assert torch.equal(x, y) and torch.equal(x, z) and bool(torch.isfinite(x).all())
        if code == 0:          # ... and of the calls without the keyword
            e = run(lambda *t: torch.ops.sol.karman_step_dens(*t, re, h))
            for x, y in zip(a, e):
                assert torch.equal(x, y)
        else:
            mac = a
    assert rel(mac[2], a[2]) > 0.02


# ---- 8. LargeGridTrainer / LargeGridRollout -----------------------------------------------------------------------------------------------------
def _net_of(p):
    net = sol_amd.model_mars_moon(cin=3, cout=2, seed=0)
    net.set_weights([q.detach().numpy() for q in p["params"]])
    return net


def test_large_grid_trainer_against_the_reference_and_replayed():
    """144 x 72 (the smallest grid LargeGridTrainer accepts, any_width=True), B = 1, two steps, mars_moon, at the tolerances of the
    substeps trainer test: loss and per-step losses 1e-5, full weight gradient TOL_GRAD, captured against eager 1e-6."""
    Y, X = mc.TRAINER_GRID
    ms = 2
    p = mc.trainer_problem(ms)
    lref, steps_ref, gref, fin_ref = mc.trainer_reference(p)
    te = sol_amd.make_trainer(_net_of(p), None, 1, Y, X, ms, 100.0 / X, mc.TRAINER_STD_V, o.STD_RE, use_graph=False, any_width=True, **MC)
    assert isinstance(te, sol_amd.LargeGridTrainer) and te.advection == dict(advection="mac_cormack", correction_strength=1.0)
    args = (f32(p["d"]), f32(p["vy"]), f32(p["vx"]), f32(p["re"]), f32(torch.stack(p["gt_vy"])), f32(torch.stack(p["gt_vx"])))
    loss = float(te.fwd_bwd(*args, want_final=True))
    e_l, e_g = abs(loss - lref) / abs(lref), rel(te.grads, gref)
    e_s = [abs(a - b) / abs(b) for a, b in zip(te.loss_steps.tolist(), steps_ref)]
    e_f = [rel(a, b) for a, b in zip(te.final, fin_ref)]
    print("LargeGridTrainer(mac_cormack) vs float64 reference: loss %.3e, per-step %s, gradient %.3e, final state %s" % (e_l, e_s, e_g, e_f))
    assert e_l < 1e-5 and max(e_s) < 1e-5 and e_g < TOL_GRAD and max(e_f) < TOL_FIELD, (e_l, e_s, e_g, e_f)
    g_eager, l_eager = te.grads.clone(), te.loss_steps.clone()
    # the plain trainer computes something else
    t1 = sol_amd.LargeGridTrainer(_net_of(p), 1, Y, X, ms, mc.TRAINER_STD_V, o.STD_RE, use_graph=False, any_width=True)
    l1 = float(t1.fwd_bwd(*args))
    print("semi_lagrangian trainer on the same problem: loss %.4e against %.4e" % (l1, lref))
    assert t1.advection == {} and abs(l1 - lref) > 0.05 * abs(lref)
    tg = sol_amd.LargeGridTrainer(_net_of(p), 1, Y, X, ms, mc.TRAINER_STD_V, o.STD_RE, any_width=True, **MC)
    lg = float(tg.fwd_bwd(*args))
    assert tg._graph is not None
    e_g = rel(tg.grads, g_eager)
    print("captured vs eager: loss %.3e gradient %.3e" % (abs(lg - loss) / abs(loss), e_g))
    assert abs(lg - loss) <= 1e-6 * abs(loss) and e_g < 1e-6 and rel(tg.loss_steps, l_eager) < 1e-6
    g1 = tg.grads.clone()
    assert float(tg.fwd_bwd(*args)) == lg and torch.equal(tg.grads, g1)


def test_large_grid_rollout_equals_the_hand_composition_and_matches_the_reference():
    from sol_amd.schedule2d import NetSchedule2D
    Y, X = mc.TRAINER_GRID
    steps = 4
    p = mc.trainer_problem(2)
    g = p["g"]
    ref = mc.rollout_reference(p, steps)
    runs = []
    for kw in (dict(use_graph=True), dict(use_graph=False)):
        ro = sol_amd.make_rollout(_net_of(p), masks(g), 1, Y, X, g.dx, mc.TRAINER_STD_V, o.STD_RE, any_width=True, **MC, **kw)
        assert isinstance(ro, sol_amd.LargeGridRollout) and ro.advection["advection"] == "mac_cormack"
        h = tuple(f32(p[k]) for k in ("d", "vy", "vx", "re"))
        ro.run(*h, steps)
        errs = [rel(a, b) for a, b in zip(h[:3], ref)]
        print("LargeGridRollout(mac_cormack, %s) after %d steps: d %.3e vy %.3e vx %.3e" % ((kw, steps) + tuple(errs)))
        assert max(errs) < 1.5 * TOL_FIELD, errs           # the growth factor of the substeps roll-out test
        runs.append(h[:3])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    mk = masks(g)
    cfg = ops.karman_cfg(1, Y, X, g.dx, masks=mk)
    sched = NetSchedule2D(_net_of(p), 1, Y, X, train=False, any_width=True)
    fs = (1.0 / mc.TRAINER_STD_V[0], 1.0 / mc.TRAINER_STD_V[1], 1.0 / o.STD_RE)
    d, vy, vx, re = (f32(p[k]) for k in ("d", "vy", "vx", "re"))
    feat = torch.zeros(1, Y, X, 4, dtype=torch.float32, device=DEV)
    with torch.no_grad():
        sched.begin_step()
        for _ in range(steps):
            d, vy, vx = ops.karman_step_large(d, vy, vx, re, cfg, mk, feat=feat, feat_scale=fs, **MC)
            out, _ = sched.forward(feat)
            ops.karman_correct(out, vy, vx, mc.TRAINER_STD_V)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((d, vy, vx), runs[0]))


# ---- 9b. refusals on the device's side ----------------------------------------------------------------------------------------------------------
def test_karman_flow_on_a_one_workgroup_grid_and_the_small_grid_factories_refuse():
    from sol_amd import fluid, karman
    Y, X = 64, 32
    sim = karman.KarmanFlow(**MC)
    dom = fluid.Domain([Y, X], box=fluid.box[0:200, 0:100])
    st = fluid.Fluid(dom, density=torch.zeros(1, Y, X, 1).numpy(), velocity=torch.zeros(1, Y + 1, X + 1, 2).numpy(), batch_size=1)
    bcv, bcm = karman.velocity_bc_masks(Y, X, batch_size=1)
    with pytest.raises(sol_amd.SolError, match="KarmanFlow: the mac_cormack advection is built on the multi-launch"):
        sim.step(st, re=[1e5], res=X, velBCy=bcv, velBCyMask=bcm)
    g = o.KarmanGeometry(Y, X)
    net = sol_amd.model_mars_moon(cin=3, cout=2, seed=0)
    with pytest.raises(ValueError, match="advection='mac_cormack'"):
        sol_amd.make_trainer(net, masks(g), 1, Y, X, 2, g.dx, (0.2, 0.2), o.STD_RE, **MC)
    with pytest.raises(ValueError, match="advection='mac_cormack'"):
        sol_amd.make_trainer(sol_amd.model.MODELS["mercury"](3, 2, 0, DEV), masks(g), 1, Y, X, 2, g.dx, (0.2, 0.2), o.STD_RE, **MC)
    with pytest.raises(ValueError, match="make_rollout: the mac_cormack advection"):
        sol_amd.make_rollout(net, masks(g), 1, Y, X, g.dx, (0.2, 0.2), o.STD_RE, **MC)


# ---- 10. the scripts ------------------------------------------------------------------------------------------------------------------------
def _script(name):
    import importlib.util
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    if sdir not in sys.path:
        sys.path.insert(0, sdir)
    spec = importlib.util.spec_from_file_location("sol_script_mc_" + name, os.path.join(sdir, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_scripts_record_the_advection_and_pick_it_up(tmp_path):
    """karman.py -r 80 --advection mac_cormack --mc-strength 0.75 records it and its frames are the library step's; karman_train.py takes
    it from the set, records it in dataStats.pickle and refuses a contradicting flag"""
    import pickle
    import numpy as np
    from sol_amd import fluid, karman, scene
    res = 80
    Y, X = 2 * res, res
    runs = [_script("karman").main(["-o", str(tmp_path / "set"), "-r", str(res), "-t", "7", "-s", "0", "--re", str(re_nr), "--advection", "mac_cormack",
                                    "--mc-strength", "0.75"]) for re_nr in (8000.0e2, 16000.0e2)]
    with open(runs[0] + "/params.pickle", "rb") as f:
        pk = pickle.load(f)
    assert pk["advection"] == "mac_cormack" and pk["correction_strength"] == 0.75
    plain = _script("karman").main(["-o", str(tmp_path / "plain"), "-r", str(res), "-t", "7", "-s", "0", "--re", "8e5"])
    with open(plain + "/params.pickle", "rb") as f:
        pk = pickle.load(f)
    assert pk["advection"] == "semi_lagrangian" and pk["correction_strength"] == 1.0
    frames = [scene.read_zipped_array(os.path.join(runs[0], "velo_%06d.npz" % i)) for i in range(7)]
    dens = [scene.read_zipped_array(os.path.join(runs[0], "dens_%06d.npz" % i)) for i in range(7)]
    assert np.abs(frames[6] - scene.read_zipped_array(os.path.join(plain, "velo_000006.npz"))).max() > 1e-3
    dom = fluid.Domain([Y, X], box=fluid.box[0:200, 0:100])
    sim = karman.KarmanFlow(advection="mac_cormack", correction_strength=0.75)
    bcv, bcm = karman.velocity_bc_masks(Y, X, batch_size=1)
    st = fluid.Fluid(dom, density=dens[5], velocity=frames[5], batch_size=1)
    with torch.no_grad():
        st = sim.step(st, re=[8000.0e2], res=res, velBCy=bcv, velBCyMask=bcm)
    assert np.array_equal(st.velocity.staggered_tensor().cpu().numpy(), frames[6])
    assert np.array_equal(st.density.data.cpu().numpy(), dens[6])
    tf = str(tmp_path / "tf")
    train = ["--train", str(tmp_path / "set"), "-s", "1", "-n", "2", "-b", "1", "-t", "5", "-m", "2", "-e", "1", "--lr", "1e-4", "--tf", tf, "--seed", "0",
             "--any-width"]
    with pytest.raises(SystemExit, match="contradicts"):
        _script("karman_train").main(train + ["--advection", "semi_lagrangian"])
    with pytest.raises(SystemExit, match="contradicts"):
        _script("karman_train").main(train + ["--mc-strength", "0.5"])
    loss = _script("karman_train").main(train)
    assert loss is not None and np.isfinite(loss)
    with open(tf + "/dataStats.pickle", "rb") as f:
        stats = pickle.load(f)
    assert stats["advection"] == "mac_cormack" and stats["correction_strength"] == 0.75
