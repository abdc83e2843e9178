"""Adjoint of the karman-2d marker density on the GPU (pytest -m gpu): sol_karman_density_bwd (csrc/karman_density_bwd.hip) behind
ops.karman_step / ops.karman_step_large(density_grad=True), KarmanFlow(density_grad=True).step and torch.ops.sol.karman_step_dens, on the
one-workgroup grids (32 x 16, 64 x 32) and on the smallest large grid (130 x 65: ragged tile row and column, direct solve), against the
float64 oracle's autograd, against the linearity of the density path (no oracle), bit reproducibility (eager, captured, LDS window against
global atomics, CFL 5.3), poisoning by a non-finite cotangent, and that the defaults did not move.

Tolerances are the suite's (large2d_scenes.py): fields 1e-5, gradients 1e-4 relative L2.  The inputs are fixed (density_adjoint_cases.py
says why, test_karman2d_density_adjoint_cpu.py pins it): with them the oracle's own float32 run matches float64 untrimmed, so the metric
asserted here, trimmed_rel with the suite's cap of 0.1 % of a component's entries, only has to absorb a cell that the KERNEL's fp32
rounding decides differently; the untrimmed value is printed beside it."""
import os
import sys

import pytest
import torch

from sol_amd import _lib, fluid, karman, ops, torch_ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from density_adjoint_cases import SEED, oracle_case, scene, w_dens
from large2d_scenes import DEV, TOL_FIELD, TOL_GRAD, TRIM, cfl_scaled, cotangent_at, f32, masks, rel, state, trimmed_rel

pytestmark = pytest.mark.gpu
NAMES = ("g_d", "g_vy", "g_vx")


def check_fields(out, ref, what):
    for name, a, b in zip(("d", "vy", "vx"), out, ref):
        e = rel(a, b)
        print("%s %s_out: rel L2 %.3e" % (what, name, e))
        assert e < TOL_FIELD, (what, name, e)


def check_grads(got, ref, what):
    for name, a, b in zip(NAMES, got, ref):
        v, k, worst = trimmed_rel(a, b, TRIM)
        print("%s %s: rel L2 %.3e untrimmed, %.3e after leaving out %d of %d entries (largest deviation left out %.3e)"
              % (what, name, rel(a, b), v, k, b.numel(), worst))
        assert k <= int(TRIM * b.numel())
        assert v < TOL_GRAD, (what, name, v)


def leaves(st):
    return tuple(f32(t).requires_grad_(True) for t in st[:3])


def step_ops(hd, hy, hx, re, cfg, mk, info=None, density_grad=True):
    if mk.large:
        return ops.karman_step_large(hd, hy, hx, f32(re), cfg, mk, info=info, density_grad=density_grad)
    return ops.karman_step(hd, hy, hx, f32(re), cfg, mk, info, density_grad=density_grad)


def flow_step(sim, s, re, B, Y, X):
    bcv, bcm = karman.velocity_bc_masks(Y, X, batch_size=B)
    return sim.step(s, re=re.tolist(), res=X, velBCy=bcv, velBCyMask=bcm)


def fluid_of(hd, hy, hx, B, Y, X):
    dom = fluid.Domain([Y, X], box=fluid.box[0:200, 0:100])
    vel = fluid.StaggeredGrid([hy.reshape(B, Y + 1, X, 1), hx.reshape(B, Y, X + 1, 1)], dom.box)
    return fluid.Fluid(dom, density=hd.reshape(B, Y, X, 1), velocity=vel, batch_size=B)


def fluid_out(s, B, Y, X):
    return s.density.data.reshape(B, Y, X), s.velocity.data[0].data.reshape(B, Y + 1, X), s.velocity.data[1].data.reshape(B, Y, X + 1)


def backward(out, w_d, w_v=None):
    loss = (out[0] * f32(w_d)).sum()
    if w_v is not None:
        loss = loss + (out[1] * f32(w_v[0])).sum() + (out[2] * f32(w_v[1])).sum()
    loss.backward()
    torch.cuda.synchronize()


def grads_of(hs):
    return tuple(torch.zeros_like(h) if h.grad is None else h.grad for h in hs)


# ---- 1. against the oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("api,Y,X,B", [("ops", 32, 16, 2), ("torch_ops", 64, 32, 3), ("flow", 130, 65, 2)])
def test_density_adjoint_against_the_oracle(api, Y, X, B):
    g = scene(Y, X)
    mk = masks(g)
    assert mk.large == (Y == 130) and mk.pressure_solver == "direct"
    st = state(B, Y, X, SEED, g)
    w_d = w_dens(B, Y, X, g)
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk)
    ref_out, ref_g = oracle_case(Y, X, B)
    # density-only loss <d_out, w_d> through the surface under test
    hs = leaves(st)
    info = {}
    if api == "ops":
        out = step_ops(*hs, st[3], cfg, mk, info)
    elif api == "torch_ops":
        out = torch.ops.sol.karman_step_dens(*hs, f32(st[3]), torch_ops.register_scene(cfg, mk))
    else:
        sim = karman.KarmanFlow(density_grad=True)
        out = fluid_out(flow_step(sim, fluid_of(*hs, B, Y, X), st[3], B, Y, X), B, Y, X)
        assert sim.pressure_solver_used == "direct"
    assert all(t.requires_grad for t in out)
    check_fields(out, ref_out, "%s %dx%d" % (api, Y, X))
    backward(out, w_d)
    assert "iterations_bwd" not in info            # a density-only loss runs no velocity adjoint, hence no pressure solve
    dens = grads_of(hs)
    check_grads(dens, ref_g, "%s %dx%d density-only" % (api, Y, X))
    if Y == 32:
        return
    # combined loss with velocity cotangents, through ops.*
    w_v = cotangent_at(B, Y, X)
    ref_out, ref_g = oracle_case(Y, X, B, with_velocity=True)
    hs = leaves(st)
    backward(step_ops(*hs, st[3], cfg, mk), w_d, w_v)
    comb = grads_of(hs)
    check_grads(comb, ref_g, "ops %dx%d combined" % (Y, X))
    # ... its velocity part = the default path's result for the same velocity cotangents + the density part of an accumulate = 0 call,
    # bit for bit; its density part = the density-only one
    hv = leaves(st)
    plain = step_ops(*hv, st[3], cfg, mk, density_grad=False)
    svy, svx, _ = plain[1].grad_fn.saved_tensors
    ((plain[1] * f32(w_v[0])).sum() + (plain[2] * f32(w_v[1])).sum()).backward()
    part = ops.karman_density_bwd(f32(st[0]), svy, svx, f32(st[3]), f32(w_d), cfg, mk)
    torch.cuda.synchronize()
    assert hv[0].grad is None
    assert torch.equal(comb[1], hv[1].grad + part[1]) and torch.equal(comb[2], hv[2].grad + part[2])
    assert torch.equal(comb[0], part[0]) and torch.equal(comb[0], dens[0])
    assert torch.equal(part[1], dens[1]) and torch.equal(part[2], dens[2])


def test_inflow_before_against_the_oracle():
    Y, X, B = 130, 65, 2
    g = scene(Y, X)
    mk = masks(g)
    st = state(B, Y, X, SEED, g)
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk, inflow_order="before")
    ref_out, ref_g = oracle_case(Y, X, B, inflow_order="before")
    hs = leaves(st)
    out = step_ops(*hs, st[3], cfg, mk)
    check_fields(out, ref_out, "inflow before")
    backward(out, w_dens(B, Y, X, g))
    check_grads(grads_of(hs), ref_g, "inflow before")


# ---- 2. three chained steps -----------------------------------------------------------------------------------------------------------
def test_three_chained_steps_against_the_oracle():
    Y, X, B = 64, 32, 2
    g = scene(Y, X)
    st = state(B, Y, X, SEED, g)
    ref_out, ref_g = oracle_case(Y, X, B, steps=3, with_velocity=True)
    hs = leaves(st)
    sim = karman.KarmanFlow(density_grad=True)
    s = fluid_of(*hs, B, Y, X)
    for _ in range(3):
        s = flow_step(sim, s, st[3], B, Y, X)
    out = fluid_out(s, B, Y, X)
    check_fields(out, ref_out, "three steps")
    backward(out, w_dens(B, Y, X, g), cotangent_at(B, Y, X))
    check_grads(grads_of(hs), ref_g, "three steps")


# ---- 3. linearity of the density path (no oracle, no kinks) ------------------------------------------------------------------------
@pytest.mark.parametrize("cfl", [None, 5.3])
def test_density_gradient_is_the_transpose_of_the_affine_density_map(cfl):
    """d_out is affine in d_in at a fixed velocity: <w, step(d1) - step(d2)> = <g_d, d1 - d2>.  At CFL 5.3 the scatter's targets leave the
    LDS halo and the domain."""
    Y, X, B = 130, 65, 2
    g = scene(Y, X)
    mk = masks(g)
    st = state(B, Y, X, SEED, g)
    if cfl is not None:
        st, reached = cfl_scaled(st, g, cfl)
        assert abs(reached - cfl) < 0.05
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk)
    gen = torch.Generator().manual_seed(29)
    d1, d2 = f32(st[0]), f32(torch.rand(B, Y, X, generator=gen, dtype=torch.float64))
    w = f32(torch.randn(B, Y, X, generator=gen, dtype=torch.float64))
    h1 = d1.clone().requires_grad_(True)
    o1 = step_ops(h1, f32(st[1]), f32(st[2]), st[3], cfg, mk)
    (o1[0] * w).sum().backward()
    with torch.no_grad():
        o2 = step_ops(d2, f32(st[1]), f32(st[2]), st[3], cfg, mk)
    torch.cuda.synchronize()
    dout = o1[0].detach().double() - o2[0].double()
    lhs = float((w.double() * dout).sum())
    rhs = float((h1.grad.double() * (d1.double() - d2.double())).sum())
    bound = 1e-5 * float(w.double().norm()) * float(dout.norm())
    print("linearity at CFL %s: <w, dout> = %.9e, <g_d, din> = %.9e, difference %.3e, bound %.3e" % (cfl, lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs) > 10 * bound                    # the identity is not met by two vanishing sides
    assert abs(lhs - rhs) <= bound


# ---- 4. bit reproducibility ----------------------------------------------------------------------------------------------------------
def test_density_adjoint_is_bit_reproducible_eager_captured_and_tile_vs_global():
    Y, X, B = 130, 65, 2
    g = scene(Y, X)
    mk = masks(g)
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk)
    st0 = state(B, Y, X, SEED, g)
    hw = f32(w_dens(B, Y, X, g))
    for st in (st0, cfl_scaled(st0, g, 5.3)[0]):
        hd, hre = f32(st[0]), f32(st[3])
        with torch.no_grad():
            _, svy, svx = ops.karman_step_large_saved(hd, f32(st[1]), f32(st[2]), hre, cfg, mk)
        runs = [ops.karman_density_bwd(hd, svy, svx, hre, hw, cfg, mk) for _ in range(2)]
        torch.cuda.synchronize()
        for a, b in zip(*runs):
            assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
        _lib.set_option("k2d_dens_adj_tile", 0)
        try:
            glob = ops.karman_density_bwd(hd, svy, svx, hre, hw, cfg, mk)
            torch.cuda.synchronize()
        finally:
            _lib.set_option("k2d_dens_adj_tile", 1)
        for a, b in zip(glob, runs[0]):
            assert torch.equal(a, b)
    # (the spun-up state again) accumulate = 1 onto a buffer = one fp32 add per face onto what was there
    base = [torch.full_like(svy, 0.25), torch.full_like(svx, -3.0)]
    acc = ops.karman_density_bwd(hd, svy, svx, hre, hw, cfg, mk, base[0].clone(), base[1].clone())
    assert torch.equal(acc[1], base[0] + runs[0][1]) and torch.equal(acc[2], base[1] + runs[0][2]) and torch.equal(acc[0], runs[0][0])
    # one linear capture of the accumulate = 0 call, replayed twice
    nb = ops.density_bwd_workspace_bytes(cfg)
    ws = torch.empty((nb + 3) // 4, dtype=torch.float32, device=DEV)
    cap = {}

    def body():
        cap["g"] = ops.karman_density_bwd(hd, svy, svx, hre, hw, cfg, mk, workspace=ws)

    torch.cuda.synchronize()
    graph = _lib.capture_graph(body, "density adjoint")
    for _ in range(2):
        for t in cap["g"]:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(cap["g"], runs[0]):
            assert torch.equal(a, b)


# ---- 5. a non-finite cotangent poisons its simulation only ---------------------------------------------------------------------------
def test_nonfinite_cotangent_poisons_its_simulation_only():
    Y, X, B = 130, 65, 2
    g = scene(Y, X)
    mk = masks(g)
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk)
    st = state(B, Y, X, SEED, g)
    hd, hre, hw = f32(st[0]), f32(st[3]), f32(w_dens(B, Y, X, g))
    with torch.no_grad():
        _, svy, svx = ops.karman_step_large_saved(hd, f32(st[1]), f32(st[2]), hre, cfg, mk)
    clean = ops.karman_density_bwd(hd, svy, svx, hre, hw, cfg, mk)
    bad = hw.clone()
    bad[1, 100, 30] = float("inf")
    got = ops.karman_density_bwd(hd, svy, svx, hre, bad, cfg, mk)
    # ... and added onto a finite velocity adjoint
    acc = ops.karman_density_bwd(hd, svy, svx, hre, bad, cfg, mk, torch.ones_like(svy), torch.ones_like(svx))
    torch.cuda.synchronize()
    for res in (got, acc):
        for name, t in zip(NAMES, res):
            assert bool(torch.isnan(t[1]).all()), name
    for a, b in zip(got, clean):
        assert torch.equal(a[0], b[0]) and bool(torch.isfinite(b).all())


# ---- 6. the defaults did not move ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Y,X", [(64, 32), (130, 65)])
def test_defaults_keep_the_density_out_of_the_graph(Y, X):
    B = 2
    g = scene(Y, X)
    mk = masks(g)
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk)
    st = state(B, Y, X, SEED, g)
    hs = leaves(st)
    plain = step_ops(*hs, st[3], cfg, mk, density_grad=False)
    assert not plain[0].requires_grad and plain[1].requires_grad and plain[2].requires_grad
    optin = step_ops(*leaves(st), st[3], cfg, mk)
    assert all(t.requires_grad for t in optin)
    for a, b in zip(plain, optin):
        assert torch.equal(a.detach(), b.detach())
    # through KarmanFlow, and nothing requires a gradient: the opt-in changes nothing
    sim = karman.KarmanFlow()
    out = fluid_out(flow_step(sim, fluid_of(*hs, B, Y, X), st[3], B, Y, X), B, Y, X)
    assert not out[0].requires_grad and out[1].requires_grad
    for a, b in zip(out, plain):
        assert torch.equal(a.detach(), b.detach())
    none = step_ops(f32(st[0]), f32(st[1]), f32(st[2]), st[3], cfg, mk)
    assert not any(t.requires_grad for t in none)
    torch.cuda.synchronize()
