"""Buoyancy of the karman-3d step on the GPU (pytest -m gpu): k3_buoyancy / k3b_buoyancy_adj (csrc/karman3d_buoyancy.hip) behind
sol_karman3d_buoyancy_add(_bwd), sol_karman3d_step_fwd_buoy, sol_karman3d_step_bwd_buoy(_re), Karman3DFlow(buoyancy=...).step,
torch.ops.sol.karman3d_step_buoy, Karman3DTrainer / Karman3DRollout (buoyancy=...) and scripts/karman3d.py --buoyancy -- against the
float64 reference of buoyancy3d_cases.py (composed from the 3-D oracle's own stages), against the exact transpose identity of the term,
bit reproducibility, poisoning by a non-finite cotangent, and that nothing moves with the force off.

Shapes are the smallest at which each piece can go wrong: 1 x 1 x 1, 3 x 5 x 7 (ragged), 16 x 8 x 8 with B = 2, 9 x 8 x 130 (three lane
trips along z) for the term; 16 x 8 x 8 with B = 2, 20 x 10 x 10 (advection tiles that end inside the grid) and 32 x 16 x 16 with the
velocity x 3.5 for the step.  Metric: max |a - b| / max |b| (buoyancy3d_cases.maxrel), untrimmed.  Bounds: the float32-against-float64
distance of the reference itself, pinned by test_karman3d_buoyancy_cpu.py (FIELD_PIN 3e-6, GRAD_PIN 1e-5, RE_PIN 4e-5), times MARGIN = 5,
the ratio the 3-D adjoint tests keep between their tolerance and their own pin: fields 1.5e-5, gradients 5e-5, g_re 2e-4."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

import sol_oracle3d as o
from sol_amd import _lib, torch_ops
from sol_amd import karman3d as k3
from sol_amd._lib import check, ptr, stream

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buoyancy3d_cases as bc
import karman3d_adjoint_cases as kc
from large2d_scenes import DEV, TOL_FIELD, TOL_GRAD, f32, rel

pytestmark = pytest.mark.gpu

TOL_F, TOL_G, TOL_RE = bc.FIELD_PIN * bc.MARGIN, bc.GRAD_PIN * bc.MARGIN, bc.RE_PIN * bc.MARGIN
ZERO = (0.0, 0.0, 0.0)


@functools.lru_cache(maxsize=None)
def scene_of(shape, solver="auto", obstacle="sphere"):
    _, Y, X, Z = shape
    g = o.geometry(Y, X, Z, obstacle=obstacle)
    return k3.Scene3D(Y, X, Z, device=DEV, active=g.active, inflow=g.inflow, pressure_solver=solver)


def sim_of(name, force, solver="auto", obstacle="sphere", **kw):
    c = kc.case(name)
    if solver == "cg":
        kw.setdefault("cg_rtol", 1e-7)
    return k3.Karman3DFlow(scene_of(c["shape"], solver, obstacle), c["shape"][0], dt=c["dt"], buoyancy=force, **c["kw"], **kw)


def leaves(name, re_leaf=True):
    d, v, re = kc.state(name)
    return [f32(t).requires_grad_(True) for t in (d, *v)] + [f32(re).requires_grad_(re_leaf)]


def chain(step, hs, steps=1):
    cur = hs[:4]
    for _ in range(steps):
        cur = step(*cur, hs[4])
    return cur


def backward(name, out, kind):
    loss = 0.0
    if kind in ("dens", "both"):
        loss = loss + (out[0] * f32(kc.w_dens(name))).sum()
    if kind in ("vel", "both"):
        loss = loss + sum((a * f32(w)).sum() for a, w in zip(out[1:], kc.w_vel(name)))
    loss.backward()
    torch.cuda.synchronize()


def grads_of(hs):
    return tuple(torch.zeros_like(h) if h.grad is None else h.grad for h in hs)


def check_fields(out, ref, what):
    errs = [bc.maxrel(a, b) for a, b in zip(out, ref)]
    print("%s fields (d, vy, vx, vz): %s  bound %.1e" % (what, ["%.2e" % e for e in errs], TOL_F))
    assert max(errs) < TOL_F, (what, errs)
    return max(errs)


def check_grads(got, ref, what, with_re):
    errs = [bc.maxrel(a, b) for a, b in zip(got[:4], ref[:4])]
    print("%s gradients (g_d, g_vy, g_vx, g_vz): %s  bound %.1e" % (what, ["%.2e" % e for e in errs], TOL_G))
    assert max(errs) < TOL_G, (what, errs)
    if with_re:
        e = bc.maxrel(got[4], ref[4])
        print("%s g_re: %.2e  bound %.1e  (%s against %s)" % (what, e, TOL_RE, got[4].tolist(), ref[4].tolist()))
        assert e < TOL_RE, (what, "g_re", e)


def interior_level(out, active):
    """max |div| over interior active cells, relative to max |v|"""
    v = tuple(t.detach().double().cpu() for t in out[1:])
    div = o.divergence(v)
    inner = torch.zeros_like(div[0])
    inner[1:-1, 1:-1, 1:-1] = 1.0
    return float((div * inner * torch.as_tensor(np.asarray(active))).abs().max()) / max(float(t.abs().max()) for t in v)


# ---- 1. the term alone, against float64, and its exact transpose ---------------------------------------------------------------------
def term_inputs(shape):
    B, Y, X, Z = shape
    act = bc.wall_mask(Y, X, Z)
    gen = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).float().double()
    fshapes = ((B, Y + 1, X, Z), (B, Y, X + 1, Z), (B, Y, X, Z + 1))
    return act, r(B, Y, X, Z), tuple(r(*s) for s in fshapes), tuple(r(*s) for s in fshapes)


def term_add(act, d, v, f):
    B, Y, X, Z = d.shape
    out = [t.clone() for t in v]
    check(_lib.load().sol_karman3d_buoyancy_add(stream(), B, Y, X, Z, ptr(act), ptr(d), f[0], f[1], f[2], ptr(out[0]), ptr(out[1]), ptr(out[2])))
    return out


def term_add_bwd(act, g, f, gd=None):
    B, Y, X, Z = g[0].shape[0], g[1].shape[1], g[0].shape[2], g[0].shape[3]
    out = torch.full((B, Y, X, Z), float("nan"), dtype=torch.float32, device=DEV)
    check(_lib.load().sol_karman3d_buoyancy_add_bwd(stream(), B, Y, X, Z, ptr(act), ptr(g[0]), ptr(g[1]), ptr(g[2]), f[0], f[1], f[2], ptr(gd), ptr(out)))
    return out


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 3, 5, 7), (2, 16, 8, 8), (1, 9, 8, 130)])
def test_the_term_alone_against_float64_and_its_exact_transpose(shape):
    """Worst measured over the four shapes: forward 4.4e-8 of max (|v| + |term|) (bound 4 x 2^-24 = 2.4e-7), transpose 5.3e-8 of its magnitude
    (bound 9 x 2^-24 = 5.4e-7), <add(d), w> against <d, add_bwd(w)> 6.0e-8 of sum |add(d) w| (1 x 1 x 1; the larger shapes 2e-10 .. 5e-9;
    bound 1e-6)."""
    act, d, v, w = term_inputs(shape)
    masks = bc.face_masks(act)
    f = (0.3, -0.2, 0.15)
    hact, hd, hv, hw = f32(act), f32(d), [f32(t) for t in v], [f32(t) for t in w]
    eps = 2.0 ** -24
    # forward: (v + f avg(d)) mask, three roundings of the fp32 spelling (the average, the product, the sum)
    got = term_add(hact, hd, hv, f)
    torch.cuda.synchronize()
    f32f = [float(np.float32(c)) for c in f]
    term = bc.add_term(d, masks, f32f)
    for c in range(3):
        ref = torch.as_tensor(masks[c]) * v[c] + term[c]
        scale = float((v[c].abs() + term[c].abs()).max())
        e = float((got[c].double().cpu() - ref).abs().max())
        print("term %s component %d: max error %.2e of %.2e (%.2e relative, bound %.2e)" % (shape, c, e, scale, e / scale, 4 * eps))
        assert e <= 4 * eps * scale, (shape, c, e)          # three roundings, each within eps of (|v| + |term|); 4 covers the second-order terms
        assert float((got[c].double().cpu() - torch.as_tensor(masks[c]) * v[c]).abs().max()) > 0          # the term is there
    # a zero component leaves that component's faces bit-identical (masked faces included)
    part = term_add(hact, hd, hv, (0.3, 0.0, 0.15))
    assert torch.equal(part[1], hv[1]) and torch.equal(part[0], got[0]) and torch.equal(part[2], got[2])
    none = term_add(hact, hd, hv, ZERO)
    assert all(torch.equal(a, b) for a, b in zip(none, hv))
    # transpose against float64, with and without g_d_out
    gd = f32(torch.as_tensor(np.random.default_rng(3).standard_normal(d.shape)))
    for base in (None, gd):
        gs = term_add_bwd(hact, hw, f, base)
        ref = bc.add_term_transpose(w, masks, f32f) + (0.0 if base is None else base.double().cpu())
        mag = sum(abs(fc) * 0.5 * 2 * float(wc.abs().max()) for fc, wc in zip(f32f, w)) + (0.0 if base is None else float(base.abs().max()))
        e = float((gs.double().cpu() - ref).abs().max())
        print("transpose %s (g_d_out %s): max error %.2e of %.2e (%.2e relative, bound %.2e)" % (shape, base is not None, e, mag, e / mag, 9 * eps))
        assert e <= 9 * eps * mag, (shape, e)             # per component the pair sum, the product and the running sum (masks and halves are exact)
    # <add(d) - add(0), w> = <d, add_bwd(w)> to fp32 round-off: both sides from the kernels, summed in float64
    zero_v = [torch.zeros_like(t) for t in hv]
    lin = term_add(hact, hd, zero_v, f)
    gs = term_add_bwd(hact, hw, f)
    torch.cuda.synchronize()
    lhs = sum(float((a.double() * b.double()).sum()) for a, b in zip(lin, hw))
    rhs = float((hd.double() * gs.double()).sum())
    mag = sum(float((a.double() * b.double()).abs().sum()) for a, b in zip(lin, hw))
    print("transpose identity %s: <add(d), w> = %.9e, <d, add_bwd(w)> = %.9e, difference %.2e of %.2e" % (shape, lhs, rhs, abs(lhs - rhs), mag))
    assert mag > 0 and abs(lhs - rhs) <= 1e-6 * mag


# ---- 2. force off equals today ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,obstacle", [("direct", "sphere"), ("cg", "cylinder")])
def test_force_off_equals_today_bit_for_bit(solver, obstacle):
    name = "16_comb"
    plain = sim_of(name, None, solver, obstacle, density_grad=True, re_grad=True)
    zero = sim_of(name, ZERO, solver, obstacle, density_grad=True, re_grad=True)
    assert plain.cg == (solver == "cg") and plain.buoyancy is None and zero.buoyancy is None
    res = []
    for sim in (plain, zero):
        hs = leaves(name)
        out = chain(sim.step, hs)
        backward(name, out, "both")
        res.append(([t.detach() for t in out], grads_of(hs)))
    for a, b in zip(res[0][0] + list(res[0][1]), res[1][0] + list(res[1][1])):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    # the _buoy entry points with a zero force: the plain call's bits, forward (with saved_* and with feat_out) and adjoint (with and without re)
    d, v, re = kc.state(name)
    st = [f32(t) for t in (d, *v, re)]
    fs = [1.0 / 0.2, 1.0 / 0.25, 1.0 / 0.3, 1.0 / o.STD_RE]
    fwd = []
    for force in (None, ZERO):
        saved = [torch.empty_like(t) for t in st[1:4]]
        feat = torch.zeros(*st[0].shape, 4, dtype=torch.float32, device=DEV)
        with torch.no_grad():
            out = plain._fwd(*st, saved, buoyancy=force)
            outf = plain._fwd(*st, None, feat, fs, buoyancy=force)
        fwd.append(list(out) + saved + list(outf) + [feat])
    for a, b in zip(*fwd):
        assert torch.equal(a, b)
    saved = fwd[0][4:7]
    wv = [f32(t) for t in kc.w_vel(name)]
    base = plain._bwd(saved, st[4], *wv)
    got = plain._bwd(saved, st[4], *wv, buoyancy=ZERO, g_d=None)
    base_re = plain._bwd(saved, st[4], *wv, vel_in=st[1:4])
    wd = f32(kc.w_dens(name))
    got_re = plain._bwd(saved, st[4], *wv, vel_in=st[1:4], buoyancy=ZERO, g_d=wd)
    torch.cuda.synchronize()
    assert len(got) == 4 and len(got_re) == 5
    assert all(torch.equal(a, b) for a, b in zip(base, got)) and all(torch.equal(a, b) for a, b in zip(base_re, got_re))
    assert torch.equal(got[3], torch.zeros_like(got[3])) and torch.equal(got_re[4], wd)          # g_dsum = g_d_out (NULL: zero)


# ---- 3. forward step against the reference ---------------------------------------------------------------------------------------------
FWD = [(n, fi, "direct", 0) for n in bc.FORWARD_CASES for fi in (0, 1)]
FWD += [(n, 1, "direct", 1) for n in ("16_comb", "16_before", "20_comb", "32_x35")]
FWD += [("16_comb", 0, "cg", 0), ("16_dirichlet", 1, "cg", 0), ("32_x35", 1, "cg", 1)]


@pytest.mark.parametrize("name,fi,solver,tile", FWD)
def test_forward_step_against_the_reference(name, fi, solver, tile):
    """Worst measured: 1.5e-6 over the fields of this test and of the adjoint tests below (the CG cases 4.1e-7 at 16 x 8 x 8, 9.7e-7 at
    32 x 16 x 16) against the bound 1.5e-5; interior divergence level of the buoyant step 0.64 .. 1.47 times the plain step's (bound 3)."""
    force = bc.FORCES[fi]
    ref_out, _ = bc.reference(name, force, "dens", 1)
    sim = sim_of(name, force, solver)
    plain = sim_of(name, None, solver)
    assert sim.cg == (solver == "cg") and sim.buoyancy == force
    d, v, re = kc.state(name)
    st = [f32(t) for t in (d, *v, re)]
    prev = _lib.get_option("k3d_tile")
    _lib.set_option("k3d_tile", tile)
    try:
        with torch.no_grad():
            out = sim.step(*st)
            base = plain.step(*st)
        torch.cuda.synchronize()
    finally:
        _lib.set_option("k3d_tile", prev)
    check_fields(out, ref_out, "%s F=%s %s tile=%d" % (name, force, solver, tile))
    assert torch.equal(out[0], base[0])                       # the density is advected by the post-diffusion velocity: the force does not touch it
    assert bc.maxrel(out[1], base[1]) > 1e-2                  # ... and the velocity does feel it
    if solver == "cg":
        assert bool((sim.solve_info["converged"] == 1).all()), sim.solve_info
    # interior divergence at the plain step's level: the solve's residual scales with the magnitude of the field it projects, so the two
    # are compared relative to max |v_out|; 3 = room for round-off to fall differently on two right-hand sides
    act = kc.geometry(name).active
    lb, lp = interior_level(out, act), interior_level(base, act)
    print("interior divergence / max|v|: buoyant %.2e, plain %.2e (ratio %.2f)" % (lb, lp, lb / lp))
    assert lb <= 3.0 * lp, (lb, lp)


# ---- 4. adjoint against the reference's autograd ------------------------------------------------------------------------------------------
ADJ = [(n, fi, k, s, r) for n in bc.ADJOINT_CASES for fi in (0, 1) for k in bc.KINDS for s in (1, 2) for r in (False, True)]


def run_adjoint(name, force, kind, steps, re_grad, solver="auto"):
    sim = sim_of(name, force, solver, re_grad=re_grad)
    hs = leaves(name, re_leaf=re_grad)
    out = chain(sim.step, hs, steps)
    assert all(t.requires_grad for t in out)
    backward(name, out, kind)
    return sim, out, hs


@pytest.mark.parametrize("name,fi,kind,steps,re_grad", ADJ)
def test_adjoint_against_the_references_autograd(name, fi, kind, steps, re_grad):
    """Worst measured over the 48 cases: g_d, g_v* 3.4e-7 against the bound 5e-5; g_re 5.1e-6 against 2e-4."""
    force = bc.FORCES[fi]
    ref_out, ref_g = bc.reference(name, force, kind, steps)
    sim, out, hs = run_adjoint(name, force, kind, steps, re_grad)
    what = "%s F=%s %s steps=%d re=%s" % (name, force, kind, steps, re_grad)
    check_fields(out, ref_out, what)
    got = grads_of(hs)
    assert all(h.grad is not None for h in hs[:4]) and (hs[4].grad is not None) == re_grad
    check_grads(got, ref_g, what, with_re=re_grad)
    assert all(float(t.abs().max()) > 0 for t in got[:4])          # a velocity-only loss reaches the density, a density-only loss the velocity
    if kind == "dens" and steps == 2 and not re_grad:
        # ... through the projection: the force-off step's density-only gradient (density advection alone) is far away
        hp = leaves(name, re_leaf=False)
        backward(name, chain(sim_of(name, None, density_grad=True).step, hp, steps), kind)
        for c in (1, 2, 3):
            assert bc.maxrel(hp[c].grad, ref_g[c]) > 100 * TOL_G, c


def test_adjoint_on_a_cg_scene_against_the_references_autograd():
    """Measured: fields 2.5e-7, gradients 2.2e-7, g_re 3.9e-6 (bounds 1.5e-5, 5e-5, 2e-4)."""
    name, force, kind, steps = "16_comb", bc.FORCES[1], "both", 2
    ref_out, ref_g = bc.reference(name, force, kind, steps)
    sim, out, hs = run_adjoint(name, force, kind, steps, True, solver="cg")
    assert sim.cg and bool((sim.solve_info["converged"] == 1).all()) and bool((sim.solve_info["converged_bwd"] == 1).all()), sim.solve_info
    check_fields(out, ref_out, "cg " + name)
    check_grads(grads_of(hs), ref_g, "cg " + name, with_re=True)


# ---- 5. bit reproducibility ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.ADJOINT_CASES)
def test_bit_reproducible_twice_and_with_either_scatter(name):
    force = bc.FORCES[1]

    def run():
        _, out, hs = run_adjoint(name, force, "both", 2, True)
        return [t.detach() for t in out] + list(grads_of(hs))

    first, second = run(), run()
    for a, b in zip(first, second):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
    for opt in ("k3d_adj_tile", "k3d_dens_adj_tile"):
        assert _lib.get_option(opt) == 1
        _lib.set_option(opt, 0)
        try:
            glob = run()
        finally:
            _lib.set_option(opt, 1)
        for a, b in zip(glob, first):
            assert torch.equal(a, b), opt


# ---- 6. a non-finite velocity cotangent poisons its simulation only --------------------------------------------------------------------
def test_nonfinite_velocity_cotangent_poisons_its_simulation_only():
    name, force = "16_comb", bc.FORCES[1]
    sim = sim_of(name, force, re_grad=True)
    wv = [f32(t) for t in kc.w_vel(name)]
    wd = f32(kc.w_dens(name))
    bad = [t.clone() for t in wv]
    bad[2][1, 5, 3, 4] = float("nan")
    res = []
    for w in (wv, bad):
        hs = leaves(name)
        out = chain(sim.step, hs)
        ((out[0] * wd).sum() + sum((a * b).sum() for a, b in zip(out[1:], w))).backward()
        torch.cuda.synchronize()
        res.append(grads_of(hs))
    clean, got = res
    for n, a, b in zip(bc.NAMES, got, clean):
        assert bool(torch.isnan(a[1]).all()), n
        assert torch.equal(a[0], b[0]) and bool(torch.isfinite(b).all()), n
    # the entry point itself: every g_dsum of the poisoned simulation is NaN, the other simulation's are the clean call's bits
    d, v, re = kc.state(name)
    st = [f32(t) for t in (d, *v, re)]
    saved = [torch.empty_like(t) for t in st[1:4]]
    with torch.no_grad():
        sim._fwd(*st, saved, buoyancy=force)
    a = sim._bwd(saved, st[4], *wv, buoyancy=force, g_d=wd)
    b = sim._bwd(saved, st[4], *bad, buoyancy=force, g_d=wd)
    torch.cuda.synchronize()
    assert bool(torch.isnan(b[3][1]).all()) and torch.equal(b[3][0], a[3][0]) and bool(torch.isfinite(a[3]).all())


# ---- 7. torch.ops.sol.karman3d_step_buoy ---------------------------------------------------------------------------------------------------
def test_torch_op_is_registered_differentiable_and_equals_the_step():
    name, force = "16_comb", bc.FORCES[1]
    assert hasattr(torch.ops.sol, "karman3d_step_buoy")
    sim = sim_of(name, force, re_grad=True)
    host = sim_of(name, None)                                   # the op takes the force per call: a scene registered without one
    h = torch_ops.register_scene3d(host)
    res = []
    for step in (sim.step, lambda *a: torch.ops.sol.karman3d_step_buoy(*a, h, *force, True)):
        hs = leaves(name)
        out = chain(step, hs, 2)
        assert all(t.requires_grad for t in out)
        backward(name, out, "both")
        res.append([t.detach() for t in out] + list(grads_of(hs)))
        assert hs[4].grad is not None
    for a, b in zip(*res):
        assert torch.equal(a, b) and float(a.abs().max()) > 0
    # re_grad off: re stays data; no gradient wanted at all: the no-grad forward, same bits
    hs = leaves(name)
    out = torch.ops.sol.karman3d_step_buoy(*hs, h, *force)
    backward(name, out, "vel")
    assert hs[4].grad is None and hs[0].grad is not None
    with torch.no_grad():
        st = [t.detach() for t in hs]
        plain_out = torch.ops.sol.karman3d_step_buoy(*st, h, *force)
        ref = sim.step(*st)
    assert not any(t.requires_grad for t in plain_out) and all(torch.equal(a, b) for a, b in zip(plain_out, ref))
    # a force of (0, 0, 0): the plain step with the density in the graph
    dens = sim_of(name, None, density_grad=True)
    res = []
    for step in (dens.step, lambda *a: torch.ops.sol.karman3d_step_buoy(*a, h, 0.0, 0.0, 0.0)):
        hs = leaves(name, re_leaf=False)
        out = chain(step, hs)
        assert out[0].requires_grad
        backward(name, out, "both")
        res.append([t.detach() for t in out] + list(grads_of(hs[:4])))
    for a, b in zip(*res):
        assert torch.equal(a, b)


# ---- 8. trainer ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trainer_run(force, schedule="manual", use_graph=False):
    """one fwd_bwd of a fresh Karman3DTrainer on bc.trainer_problem (use_graph: a second call, the pure replay) -> (loss, per-step losses,
    gradient, final state, parameter offsets).  Cached: shared by the tests below, never modified."""
    p = bc.trainer_problem()
    B, Y, X, Z = bc.TRAINER_SHAPE
    net = k3.MarsMoon3D(device=DEV)
    net.set_weights([q.detach().numpy() for q in p["params"]])
    tr = k3.Karman3DTrainer(net, scene_of(bc.TRAINER_SHAPE), B, 2, bc.TRAINER_STD_V, o.STD_RE, use_graph=use_graph, schedule=schedule, buoyancy=force)
    assert tr.buoyancy == (force if force is not None and any(force) else None)
    for _ in range(2 if use_graph else 1):                      # (graph: the second call is a pure replay)
        tr._grads.zero_()
        loss = tr.fwd_bwd(p["d"], *p["v"], p["re"], p["gts"])
    torch.cuda.synchronize()
    assert (tr._graph is not None) == use_graph
    return float(loss), tr.loss_steps.clone(), tr.grads.clone(), [t.clone() for t in tr.final], net.offsets


def test_trainer_sol2_against_the_reference():
    """SOL-2 at 32 x 16 x 16, B = 2, force (0.981, 0, 0): the recipe and tolerances of test_karman3d_trainer_sol2_against_oracle (loss 1e-5,
    gradient TOL_GRAD relative L2, per layer 3 TOL_GRAD) with the buoyant step in the reference's unrolled loss; per-step losses 1e-5, final
    state (density included) TOL_FIELD relative L2.  Measured: loss 3.3e-9, per-step losses 3.7e-8, gradient 1.2e-6 (worst layer 1.9e-5), final
    state 6.0e-7; the force-off trainer's gradient is 1.01 (relative L2) away from the buoyant reference."""
    force = bc.TRAINER_FORCE
    loss, losses, gref, fin = bc.trainer_reference(force)
    man = trainer_run(force)
    e = [abs(float(a) - b) / abs(b) for a, b in zip(man[1], losses)]
    eg = rel(man[2], gref)
    off = man[4]
    per = [rel(man[2][off[k]:off[k + 1]], gref[off[k]:off[k + 1]]) for k in range(len(o.mars_moon3d_param_shapes()))]
    ef = [rel(a, b) for a, b in zip(man[3], fin)]
    print("trainer: loss %.9e against %.9e (%.2e), per-step %s, gradient %.2e (worst layer %.2e), final state %s" % (
        man[0], loss, abs(man[0] - loss) / abs(loss), ["%.2e" % x for x in e], eg, max(per), ["%.2e" % x for x in ef]))
    assert abs(man[0] - loss) < 1e-5 * abs(loss), (man[0], loss)
    assert max(e) < 1e-5, e
    assert eg < TOL_GRAD, eg
    assert max(per) < 3 * TOL_GRAD, per
    assert max(ef) < TOL_FIELD, ef
    # the force is in the gradient: the force-off trainer's (today's launches) is far beyond the tolerance away
    offr = trainer_run(None)
    away = rel(offr[2], gref)
    print("force-off gradient against the buoyant reference: %.2e" % away)
    assert away > 100 * TOL_GRAD
    zero = trainer_run(ZERO)
    assert zero[0] == offr[0] and torch.equal(zero[2], offr[2]) and all(torch.equal(a, b) for a, b in zip(zero[3], offr[3]))


def test_trainer_manual_schedule_equals_autograd():
    """the hand-written reverse sweep (density cotangent carried from step to step) against the torch-autograd composition of the buoyant
    step: fp32 round-off, the bounds of test_karman3d_manual_schedule_equals_autograd_composition.  Measured: loss and per-step losses equal,
    gradient 2.4e-7, final state 5.2e-7."""
    man, aut = trainer_run(bc.TRAINER_FORCE), trainer_run(bc.TRAINER_FORCE, schedule="autograd")
    print("manual against autograd: loss %.2e, per-step %.2e, gradient %.2e, final %s" % (
        abs(man[0] - aut[0]) / abs(aut[0]), rel(man[1], aut[1]), rel(man[2], aut[2]), ["%.2e" % rel(a, b) for a, b in zip(man[3], aut[3])]))
    assert abs(man[0] - aut[0]) < 2e-6 * abs(aut[0]) and rel(man[1], aut[1]) < 2e-6
    assert rel(man[2], aut[2]) < 2e-5
    assert all(rel(a, b) < 2e-6 for a, b in zip(man[3], aut[3]))


@pytest.mark.parametrize("schedule", ["manual", "autograd"])
def test_trainer_graph_replay_equals_eager(schedule):
    """use_graph=True captures kernel nodes only (_lib.capture_graph runs sol_graph_check and refuses anything else); the second replay
    equals the eager run bit for bit"""
    eager, gr = trainer_run(bc.TRAINER_FORCE, schedule=schedule), trainer_run(bc.TRAINER_FORCE, schedule=schedule, use_graph=True)
    assert gr[0] == eager[0] and torch.equal(gr[1], eager[1]) and torch.equal(gr[2], eager[2])
    assert all(torch.equal(a, b) for a, b in zip(gr[3], eager[3]))
    assert float(gr[2].abs().max()) > 0


# ---- 9. roll-out and the script --------------------------------------------------------------------------------------------------------------
def test_rollout_against_the_reference_rollout():
    """3 steps at 16 x 8 x 8, B = 2, the golden small-weight network.  Bound: three steps, each within the one-step field bound (the step map
    does not amplify differences at these CFL numbers): 3 x 1.5e-5.  Worst measured 2.6e-7."""
    import make_golden as mg
    name, force, n = "16_comb", bc.FORCES[1], 3
    d, v, re = kc.state(name)
    g = kc.geometry(name)
    params = mg.k3d_params()
    std_v, std_re = (0.2, 0.25, 0.3), o.STD_RE
    dr, vr = bc.rollout_reference(params, d, v, re, g, std_v, std_re, force, n)
    d0, v0 = bc.rollout_reference(params, d, v, re, g, std_v, std_re, ZERO, n)
    net = k3.MarsMoon3D(device=DEV)
    net.set_weights([p.numpy() for p in params])
    B = d.shape[0]
    ro = k3.Karman3DRollout(net, scene_of(kc.case(name)["shape"]), B, std_v, std_re, buoyancy=force)
    assert ro.buoyancy == force
    out = ro.run(f32(d), *[f32(t) for t in v], f32(re), n)
    torch.cuda.synchronize()
    errs = [bc.maxrel(a, b) for a, b in zip(out, (dr, *vr))]
    print("roll-out, %d steps: %s (bound %.1e)" % (n, ["%.2e" % e for e in errs], n * TOL_F))
    assert max(errs) < n * TOL_F, errs
    assert bc.maxrel(vr[0], v0[0]) > 1e-2                                    # the force is in the flow


def test_karman3d_script_with_buoyancy(tmp_path):
    """scripts/karman3d.py --buoyancy 0.981 -r 8: the frames differ from the run without the flag; the force is recorded and read back"""
    import importlib.util
    import pickle
    import sol_amd
    from sol_amd import scene as sc_io
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    sys.path.insert(0, sdir)
    spec = importlib.util.spec_from_file_location("sol_script_karman3d_buoy", os.path.join(sdir, "karman3d.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    common = ["-r", "8", "-t", "5", "--re", "1.6e5"]
    plain = mod.main(common + ["-o", str(tmp_path / "plain")])
    buoy = mod.main(common + ["-o", str(tmp_path / "buoy"), "--buoyancy", "0.981"])
    a, b = (sc_io.read_zipped_array(p + "/velo_000004.npz") for p in (plain, buoy))
    assert a.shape == b.shape == (1, 17, 9, 9, 3) and np.isfinite(b).all()
    assert np.abs(a - b).max() > 1e-2 * np.abs(a).max()
    rec = [pickle.load(open(p + "/params.pickle", "rb"))["buoyancy"] for p in (plain, buoy)]
    assert rec[0] is None and rec[1] == (0.981, 0.0, 0.0)
    # --train-sol with the force: recorded with the model, and a --model roll-out picks it up (a contradicting flag is refused)
    force = (0.3, -0.2, 0.15)
    tr = mod.main(["-r", "8", "-t", "6", "--re", "1.6e5", "-o", str(tmp_path / "train"), "--buoyancy", "0.3,-0.2,0.15", "--train-sol", "2", "--train-steps", "1"])
    model = tr + "/model3d.pt"
    assert tuple(torch.load(model, map_location="cpu")["buoyancy"]) == force
    ro = mod.main(common + ["-o", str(tmp_path / "ro"), "--model", model])
    assert tuple(pickle.load(open(ro + "/params.pickle", "rb"))["buoyancy"]) == force
    c = sc_io.read_zipped_array(ro + "/velo_000004.npz")
    assert np.isfinite(c).all() and np.abs(c - a).max() > 1e-2 * np.abs(a).max()
    with pytest.raises(SystemExit, match="contradicts"):
        mod.main(common + ["-o", str(tmp_path / "bad"), "--model", model, "--buoyancy", "0.5"])
