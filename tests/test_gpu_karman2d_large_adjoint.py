"""Adjoint of the large-grid karman-2d step on the GPU (pytest -m gpu): sol_karman_step_bwd_large (csrc/karman_large_bwd.hip) behind
ops.karman_step_large, KarmanFlow.step and torch.ops.sol.karman_step, for the direct and the CG pressure solve, against the float64
oracle's autograd, against central differences of the HIP forward step, bit reproducibility (eager, captured, tile window vs. global
atomics), and that the forward path did not move.

Tolerances are the suite's: fields 1e-5, gradients 1e-4 relative L2, cg_rtol 1e-7 for oracle comparisons.  The step's gradient is
discontinuous where a departure point crosses a cell boundary (floorf): fp32 and float64 decide a handful of faces differently, and
each such face moves a few gradient entries by O(1).  Measured with the oracle alone (float32 against float64, 256 x 128, B = 2) the
untrimmed metric keeps a 5x margin on the default sphere and the plate (state seed 11) but not on the two-cylinder scene, where 99 %
of the squared error sits in 20 entries.  There the TRIMMED metric is asserted: each gradient component may leave out at most 0.1 %
of its entries (those with the largest absolute deviation); one boundary row (128 faces per simulation) or column (256) is already
more than that hides."""
import os
import sys

import numpy as np
import pytest
import torch

import sol_amd
import sol_oracle as o
from sol_amd import _lib, fluid, karman, ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from large2d_scenes import (CG_RTOL, DEV, PLATE, TOL_FIELD, TOL_GRAD, TRIM, TWO, active_of, check_grads, f32, geometry, masks, rel, state,
                            trimmed_rel)

pytestmark = pytest.mark.gpu
Y, X = 256, 128


def scene_of(specs):
    """(oracle geometry, specs) of the default sphere (None) or a list of obstacle specs"""
    return o.KarmanGeometry(Y, X) if specs is None else geometry(Y, X, active_of(specs, Y, X))


def cotangent(B):
    gen = torch.Generator().manual_seed(3)
    return (torch.randn(B, Y + 1, X, generator=gen, dtype=torch.float64).float().double(),
            torch.randn(B, Y, X + 1, generator=gen, dtype=torch.float64).float().double())


def oracle_grad(st, g, w, steps=1, **kw):
    d, vy, vx, re = st
    ry, rx = vy.clone().requires_grad_(True), vx.clone().requires_grad_(True)
    cd, cy, cx = d, ry, rx
    for _ in range(steps):
        cd, cy, cx = o.karman_step(cd, cy, cx, re, g, **kw)
    ((cy * w[0]).sum() + (cx * w[1]).sum()).backward()
    return (cd.detach(), cy.detach(), cx.detach()), (ry.grad, rx.grad)


def hip_grad(st, g, mk, w, info=None, **kw):
    """one differentiable ops.karman_step_large + backward of sum <out, w> -> (outputs, (g_vy, g_vx))"""
    d, vy, vx, re = st
    B = d.shape[0]
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk, **kw)
    hy, hx = f32(vy).requires_grad_(True), f32(vx).requires_grad_(True)
    out = ops.karman_step_large(f32(d), hy, hx, f32(re), cfg, mk, info=info)
    assert out[1].requires_grad and out[2].requires_grad and not out[0].requires_grad
    ((out[1] * f32(w[0])).sum() + (out[2] * f32(w[1])).sum()).backward()
    torch.cuda.synchronize()
    return tuple(t.detach() for t in out), (hy.grad, hx.grad)


def fluid_of(st, B):
    dom = fluid.Domain([Y, X], box=fluid.box[0:200, 0:100])
    hy, hx = f32(st[1]).requires_grad_(True), f32(st[2]).requires_grad_(True)
    vel = fluid.StaggeredGrid([hy.reshape(B, Y + 1, X, 1), hx.reshape(B, Y, X + 1, 1)], dom.box)
    return fluid.Fluid(dom, density=f32(st[0]).reshape(B, Y, X, 1), velocity=vel, batch_size=B), hy, hx


def flow_out(s, B):
    return s.velocity.data[0].data.reshape(B, Y + 1, X), s.velocity.data[1].data.reshape(B, Y, X + 1)


# ---- 1. direct solve against the oracle ------------------------------------------------------------------------------------------
def test_direct_adjoint_against_the_oracle():
    B = 2
    g = scene_of(None)
    mk = masks(g)
    assert mk.pressure_solver == "direct" and mk.large
    st = state(B, Y, X, 11, g)
    w = cotangent(B)
    ref_out, ref_g = oracle_grad(st, g, w)
    out, got = hip_grad(st, g, mk, w)
    for a, b in zip(out, ref_out):
        assert rel(a, b) < TOL_FIELD, rel(a, b)
    check_grads(got, ref_g, False, "ops.karman_step_large, direct")

    # the same through KarmanFlow.step on a Fluid
    sim = karman.KarmanFlow()
    bcv, bcm = karman.velocity_bc_masks(Y, X, batch_size=B)
    fl, hy, hx = fluid_of(st, B)
    oy, ox = flow_out(sim.step(fl, re=st[3].tolist(), res=X, velBCy=bcv, velBCyMask=bcm), B)
    assert sim.pressure_solver_used == "direct"
    assert rel(oy, ref_out[1]) < TOL_FIELD and rel(ox, ref_out[2]) < TOL_FIELD
    ((oy * f32(w[0])).sum() + (ox * f32(w[1])).sum()).backward()
    check_grads((hy.grad, hx.grad), ref_g, False, "KarmanFlow.step, direct")

    # ... and through torch.ops.sol.karman_step
    from sol_amd import torch_ops
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk)
    h = torch_ops.register_scene(cfg, mk)
    ty, tx = f32(st[1]).requires_grad_(True), f32(st[2]).requires_grad_(True)
    td, oy, ox = torch.ops.sol.karman_step(f32(st[0]), ty, tx, f32(st[3]), h)
    assert rel(td, ref_out[0]) < TOL_FIELD and rel(oy, ref_out[1]) < TOL_FIELD and rel(ox, ref_out[2]) < TOL_FIELD
    ((oy * f32(w[0])).sum() + (ox * f32(w[1])).sum()).backward()
    check_grads((ty.grad, tx.grad), ref_g, False, "torch.ops.sol.karman_step, direct")
    with torch.no_grad():
        nd, ny, nx = torch.ops.sol.karman_step(f32(st[0]), f32(st[1]), f32(st[2]), f32(st[3]), h)
    assert torch.equal(ny, oy.detach()) and torch.equal(nx, ox.detach())


def test_direct_adjoint_dirichlet0_against_the_oracle():
    B = 2
    g = scene_of(None)
    mk = masks(g)
    st = state(B, Y, X, 11, g)
    w = cotangent(B)
    ref_out, ref_g = oracle_grad(st, g, w, grad_pad="dirichlet0")
    out, got = hip_grad(st, g, mk, w, grad_pad="dirichlet0")
    for a, b in zip(out, ref_out):
        assert rel(a, b) < TOL_FIELD, rel(a, b)
    check_grads(got, ref_g, False, "direct, dirichlet0")


# ---- 2. CG solve against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("specs,seed,trimmed", [(PLATE, 11, False), (TWO, 11, True), (TWO, 5, True)],
                         ids=["plate_11", "two_cylinders_11", "two_cylinders_5"])
def test_cg_adjoint_against_the_oracle(specs, seed, trimmed):
    B = 2
    g = scene_of(specs)
    mk = masks(g)
    assert mk.pressure_solver == "cg" and mk.direct is None
    st = state(B, Y, X, seed, g)
    w = cotangent(B)
    ref_out, ref_g = oracle_grad(st, g, w)
    info = {}
    out, got = hip_grad(st, g, mk, w, info, cg_rtol=CG_RTOL)
    for a, b in zip(out, ref_out):
        assert rel(a, b) < TOL_FIELD, rel(a, b)
    assert info["converged"].tolist() == [1] * B and info["converged_bwd"].tolist() == [1] * B, info
    assert int(info["iterations_bwd"].min()) >= 1
    check_grads(got, ref_g, trimmed, "CG %s seed %d" % (specs, seed))


# ---- 3. CG adjoint == direct adjoint on the default scene -------------------------------------------------------------------------
def test_cg_adjoint_equals_direct_adjoint_on_the_default_scene():
    B = 2
    g = scene_of(None)
    m_dir, m_cg = masks(g, "direct"), masks(g, "cg")
    assert m_dir.pressure_solver == "direct" and m_cg.pressure_solver == "cg"
    d, vy, vx, re = state(B, Y, X, 11, g)
    w = cotangent(B)
    c_dir = ops.karman_cfg(B, Y, X, g.dx, masks=m_dir)
    c_cg = ops.karman_cfg(B, Y, X, g.dx, masks=m_cg, cg_rtol=CG_RTOL)
    hy, hx = f32(vy).requires_grad_(True), f32(vx).requires_grad_(True)
    # the same saved state for both adjoints: the post-diffusion velocity the differentiable forward call kept
    out = ops.karman_step_large(f32(d), hy, hx, f32(re), c_dir, m_dir)
    svy, svx, _ = out[1].grad_fn.saved_tensors
    info = {}
    g_dir = ops.karman_step_large_bwd(svy, svx, f32(re), f32(w[0]), f32(w[1]), c_dir, m_dir)
    g_cg = ops.karman_step_large_bwd(svy, svx, f32(re), f32(w[0]), f32(w[1]), c_cg, m_cg, info=info)
    torch.cuda.synchronize()
    assert info["converged_bwd"].tolist() == [1] * B
    errs = [rel(a, b) for a, b in zip(g_cg, g_dir)]
    print("CG adjoint against direct adjoint:", errs)
    assert max(errs) < 1e-5, errs


# ---- 4. three chained steps through KarmanFlow.step -------------------------------------------------------------------------------
@pytest.mark.parametrize("specs,trimmed", [(None, False), (TWO, True)], ids=["default", "two_cylinders"])
def test_three_chained_steps_against_the_oracle(specs, trimmed):
    B = 2
    g = scene_of(specs)
    st = state(B, Y, X, 11, g)
    w = cotangent(B)
    ref_out, ref_g = oracle_grad(st, g, w, steps=3)
    sim = karman.KarmanFlow(cg_rtol=CG_RTOL) if specs is None else karman.KarmanFlow(obstacles=karman.parse_obstacles(specs), cg_rtol=CG_RTOL)
    bcv, bcm = karman.velocity_bc_masks(Y, X, batch_size=B)
    fl, hy, hx = fluid_of(st, B)
    s = fl
    for _ in range(3):
        s = sim.step(s, re=st[3].tolist(), res=X, velBCy=bcv, velBCyMask=bcm)
    assert sim.pressure_solver_used == ("direct" if specs is None else "cg")
    oy, ox = flow_out(s, B)
    assert rel(oy, ref_out[1]) < TOL_FIELD and rel(ox, ref_out[2]) < TOL_FIELD, (rel(oy, ref_out[1]), rel(ox, ref_out[2]))
    ((oy * f32(w[0])).sum() + (ox * f32(w[1])).sum()).backward()
    torch.cuda.synchronize()
    if specs is not None:
        assert sim.solve_info["converged_bwd"].tolist() == [1] * B and sim.solve_info["converged"].tolist() == [1] * B
    check_grads((hy.grad, hx.grad), ref_g, trimmed, "three steps, %s" % (specs or "default"))


# ---- 5. adjoint identity by central differences (independent of oracle/) ---------------------------------------------------------
def test_adjoint_identity_by_central_differences():
    """<J u, w> = <u, J^T w> for the CG step at 256 x 128 with two cylinders (HIP forward on both sides)."""
    B = 1
    g = scene_of(TWO)
    mk = masks(g)
    assert mk.pressure_solver == "cg"
    d, vy, vx, re = state(B, Y, X, 11, g)
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk, cg_rtol=CG_RTOL)
    d0, v, hre = f32(d), [f32(vy), f32(vx)], f32(re)
    gen = torch.Generator().manual_seed(23)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)
    smooth = lambda t: torch.nn.functional.avg_pool2d(t[:, None], 5, 1, 2)[:, 0]
    u = [smooth(rn(*t.shape)).to(DEV) for t in v]
    w = [rn(*t.shape).to(DEV) for t in v]
    a = [t.clone().requires_grad_(True) for t in v]
    info = {}
    out = ops.karman_step_large(d0, a[0], a[1], hre, cfg, mk, info=info)
    sum((o_ * w_).sum() for o_, w_ in zip(out[1:], w)).backward()
    assert info["converged"].tolist() == [1] and info["converged_bwd"].tolist() == [1]
    dot = lambda xs, ys: float(sum((x.double() * y.double()).sum() for x, y in zip(xs, ys)))
    rhs = dot([t.grad for t in a], u)
    res = {}
    for eps in (2e-2, 1e-2, 5e-3):
        with torch.no_grad():
            p = ops.karman_step_large(d0, *[t + eps * du for t, du in zip(v, u)], hre, cfg, mk)[1:]
            m = ops.karman_step_large(d0, *[t - eps * du for t, du in zip(v, u)], hre, cfg, mk)[1:]
        res[eps] = dot([x.double() - y.double() for x, y in zip(p, m)], w) / (2 * eps)
    torch.cuda.synchronize()
    scale = dot([t.grad for t in a], [t.grad for t in a]) ** 0.5 * dot(u, u) ** 0.5
    print("adjoint identity 2-D large CG: <u, J^T w> = %.6e, <J u, w> by central differences %s, |u||J^T w| = %.3e" % (rhs, res, scale))
    assert min(abs(x - rhs) for x in res.values()) < 2e-3 * abs(rhs) + 2e-4 * scale, (rhs, res, scale)


# ---- 6. bit reproducibility -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["direct", "cg"])
def test_adjoint_is_bit_reproducible_eager_captured_and_tile_vs_global(solver):
    B = 2
    g = scene_of(None if solver == "direct" else TWO)
    mk = masks(g)
    assert mk.pressure_solver == solver
    d, vy, vx, re = state(B, Y, X, 11, g)
    w = cotangent(B)
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk, cg_max_iter=400)          # (a budget small enough to capture; the scene converges inside it)
    hd, hre, hw = f32(d), f32(re), [f32(w[0]), f32(w[1])]
    hy, hx = f32(vy).requires_grad_(True), f32(vx).requires_grad_(True)
    info = {}
    out = ops.karman_step_large(hd, hy, hx, hre, cfg, mk, info=info)
    svy, svx, _ = out[1].grad_fn.saved_tensors
    runs = []
    for _ in range(2):
        i2 = {}
        runs.append(ops.karman_step_large_bwd(svy, svx, hre, hw[0], hw[1], cfg, mk, info=i2))
        if solver == "cg":
            assert i2["converged_bwd"].tolist() == [1] * B, i2
    torch.cuda.synchronize()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert bool(torch.isfinite(runs[0][0]).all()) and float(runs[0][0].abs().max()) > 0
    # through autograd: the same bits
    ((out[1] * hw[0]).sum() + (out[2] * hw[1]).sum()).backward()
    # (the products' backward hands w itself to the step: same cotangent bits)
    assert torch.equal(hy.grad, runs[0][0]) and torch.equal(hx.grad, runs[0][1])
    # all-global-atomics form of the scatter
    _lib.set_option("k2d_adj_tile", 0)
    try:
        glob = ops.karman_step_large_bwd(svy, svx, hre, hw[0], hw[1], cfg, mk)
        torch.cuda.synchronize()
    finally:
        _lib.set_option("k2d_adj_tile", 1)
    assert torch.equal(glob[0], runs[0][0]) and torch.equal(glob[1], runs[0][1])
    # replayed from a captured graph (no host synchronisation, the full cg_max_iter budget)
    nb = sol_amd.load().sol_karman_step_bwd_large_workspace_bytes(__import__("ctypes").byref(cfg))
    ws = torch.empty((nb + 3) // 4, dtype=torch.float32, device=DEV)
    cap = {}

    def body():
        cap["g"] = ops.karman_step_large_bwd(svy, svx, hre, hw[0], hw[1], cfg, mk, workspace=ws)

    torch.cuda.synchronize()
    graph = _lib.capture_graph(body, "large-grid adjoint (%s)" % solver)
    for _ in range(2):
        cap["g"][0].zero_(); cap["g"][1].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap["g"][0], runs[0][0]) and torch.equal(cap["g"][1], runs[0][1])


# ---- 7. nothing existing moved ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["direct", "cg"])
def test_forward_bits_unchanged_nonfinite_cotangent_and_budget_report(solver):
    B = 2
    g = scene_of(None if solver == "direct" else TWO)
    mk = masks(g)
    d, vy, vx, re = state(B, Y, X, 11, g)
    w = cotangent(B)
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk)
    hd, hre = f32(d), f32(re)
    with torch.no_grad():
        i0 = {}
        plain = ops.karman_step_large(hd, f32(vy), f32(vx), hre, cfg, mk, info=i0)
    hy, hx = f32(vy).requires_grad_(True), f32(vx).requires_grad_(True)
    i1 = {}
    out = ops.karman_step_large(hd, hy, hx, hre, cfg, mk, info=i1)
    for a, b in zip(out, plain):
        assert torch.equal(a.detach(), b)
    if solver == "cg":
        assert torch.equal(i0["iterations"], i1["iterations"]) and i1["converged"].tolist() == [1] * B
    else:
        assert i0 == {} and i1 == {}
    # a non-finite cotangent in simulation 0: its input gradient is NaN everywhere, simulation 1 stays finite
    wy, wx = f32(w[0]).clone(), f32(w[1]).clone()
    wy[0, 100, 60] = float("inf")
    svy, svx, _ = out[1].grad_fn.saved_tensors
    gy, gx = ops.karman_step_large_bwd(svy, svx, hre, wy, wx, cfg, mk)
    torch.cuda.synchronize()
    assert bool(torch.isnan(gy[0]).all()) and bool(torch.isnan(gx[0]).all())
    assert bool(torch.isfinite(gy[1]).all()) and bool(torch.isfinite(gx[1]).all())
    if solver == "cg":
        # a backward budget of two iterations: reported, not converged, finite
        c2 = ops.karman_cfg(B, Y, X, g.dx, masks=mk, cg_max_iter=2)
        i2 = {}
        gy, gx = ops.karman_step_large_bwd(svy, svx, hre, f32(w[0]), f32(w[1]), c2, mk, info=i2)
        torch.cuda.synchronize()
        assert i2["converged_bwd"].tolist() == [0] * B and i2["iterations_bwd"].tolist() == [2] * B, i2
        assert bool(torch.isfinite(gy).all()) and bool(torch.isfinite(gx).all())


# ---- 8. the trainers refuse a large domain at construction ------------------------------------------------------------------------
def test_graph_trainer_refuses_a_large_domain():
    net = sol_amd.model_mars_moon(cin=3, cout=2, seed=0, device=DEV)
    with pytest.raises(ValueError, match="W <= 64"):
        sol_amd.GraphTrainer(net, 1, Y, X, 2, (0.2, 0.25), o.STD_RE)
