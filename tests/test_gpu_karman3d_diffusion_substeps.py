"""Diffusion substeps of the karman-3d step on the GPU (pytest -m gpu): k3_diffuse_sub (csrc/karman3d_diffuse_sub.hip) behind
sol_karman3d_diffuse_sub, karman3d.diffuse_sub, Karman3DFlow(diffusion_substeps=n).step, torch.ops.sol.karman3d_step_sub,
Karman3DTrainer / Karman3DRollout (diffusion_substeps=n) -- against the float64 reference of diffusion_substeps3d_cases.py (n - 1 explicit
substeps of o.laplace_replicate, then the oracle's step at re * n) at Reynolds numbers where the single stencil is unstable (alpha = 0.45,
0.3 > 1/6), bit equality of every chunking, the adjoint identity, n = 1 against the default constructor, the feature channel, stability,
and the rejection of bad arguments.

Shapes are the smallest at which each piece can go wrong: 16 x 8 x 8 (the minimum grid), 20 x 10 x 10, 18 x 10 x 70 (Z > 64, Z + 1 odd:
three tiles along z) and 17 x 11 x 37 (ends inside a tile on every axis) for the pre-diffusion; the 3-D adjoint suite's cases for the step.
Metric: max |a - b| / max |b| (maxrel), untrimmed, no element left out.  Bounds: the float32-against-float64 distance of the reference
itself, pinned by test_karman3d_diffusion_substeps_cpu.py (PRE_PIN 1.3e-6, FIELD_PIN 2.7e-6, GRAD_PIN 8e-6, RE_PIN 1e-5), times MARGIN = 5:
pre-diffusion 6.5e-6, fields 1.35e-5, gradients 4e-5, g_re 5e-5."""
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
from sol_amd._lib import ptr, stream

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buoyancy3d_cases as bc
import diffusion_substeps3d_cases as dc
from large2d_scenes import DEV, f32, rel

pytestmark = pytest.mark.gpu

TOL_PRE, TOL_F, TOL_G, TOL_RE = dc.PRE_PIN * dc.MARGIN, dc.FIELD_PIN * dc.MARGIN, dc.GRAD_PIN * dc.MARGIN, dc.RE_PIN * dc.MARGIN
S_MAX = k3.diffuse_sub_max3d()


@functools.lru_cache(maxsize=None)
def scene_of(shape, solver="auto", wall=False):
    Y, X, Z = shape
    g = dc.wall_geometry(Y, X, Z) if wall else o.geometry(Y, X, Z)
    return k3.Scene3D(Y, X, Z, device=DEV, active=g.active, inflow=g.inflow, pressure_solver=solver)


def sim_of(name, n, force=None, **kw):
    c = dc.case(name)
    wall = name == "16_wall"
    if wall:
        kw.setdefault("cg_rtol", 1e-7)
    return k3.Karman3DFlow(scene_of(c["shape"][1:], "cg" if wall else "auto", wall), c["shape"][0], dt=c["dt"], buoyancy=force,
                           diffusion_substeps=n, **c["kw"], **kw)


def leaves(name, re_leaf=True):
    d, v, re = dc.state(name)
    return [f32(t).requires_grad_(True) for t in (d, *v)] + [f32(re).requires_grad_(re_leaf)]


def chain(step, hs, steps=1):
    cur = hs[:4]
    for _ in range(steps):
        cur = step(*cur, hs[4])
    return cur


def backward(name, out):
    loss = (out[0] * f32(dc.w_dens(name))).sum() + sum((a * f32(w)).sum() for a, w in zip(out[1:], dc.w_vel(name)))
    loss.backward()
    torch.cuda.synchronize()


def grads_of(hs):
    return tuple(torch.zeros_like(h) if h.grad is None else h.grad for h in hs)


def check_fields(out, ref, what):
    errs = [dc.maxrel(a, b) for a, b in zip(out, ref)]
    print("%s fields (d, vy, vx, vz): %s  bound %.2e" % (what, ["%.2e" % e for e in errs], TOL_F))
    assert max(errs) < TOL_F, (what, errs)


def check_grads(got, ref, what, with_re):
    errs = [dc.maxrel(a, b) for a, b in zip(got[:4], ref[:4])]
    print("%s gradients (g_d, g_vy, g_vx, g_vz): %s  bound %.1e" % (what, ["%.2e" % e for e in errs], TOL_G))
    assert max(errs) < TOL_G, (what, errs)
    if with_re:
        e = dc.maxrel(got[4], ref[4])
        print("%s g_re: %.2e  bound %.1e  (%s against %s)" % (what, e, TOL_RE, got[4].tolist(), ref[4].tolist()))
        assert e < TOL_RE, (what, "g_re", e)


# ---- 1. the pre-diffusion alone against float64 --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pre_sim(shape):
    """a simulator of an empty box of any shape (the pre-diffusion reads the grid, dt and res alone)"""
    Y, X, Z = shape
    sc = k3.Scene3D(Y, X, Z, device=DEV, active=np.ones(shape), inflow=np.zeros(shape), pressure_solver="cg")
    return k3.Karman3DFlow(sc, dc.PRE_B)


@pytest.mark.parametrize("shape", dc.PRE_SHAPES)
def test_pre_diffusion_alone_against_float64(shape):
    """nsub - 1 = 1 (one substep), S_MAX (exactly one full launch), S_MAX + 1 (two launches), 2 S_MAX + 1 (three: the ping-pong parity);
    B = 3 with distinct re (alpha 0.45, 0.3, 0.9)"""
    sim = pre_sim(shape)
    v, re = dc.pre_inputs(shape)
    hv, hre = [f32(t) for t in v], f32(re)
    for m in (1, S_MAX, S_MAX + 1, 2 * S_MAX + 1):
        for chunk in (S_MAX, None):                             # the fused path (1, 1, 2, 3 launches) and the default chunk
            got = k3.diffuse_sub(sim, *hv, hre, m + 1, chunk=chunk)
            torch.cuda.synchronize()
            ref = dc.pre_reference(shape, m + 1)
            errs = [dc.maxrel(a, b) for a, b in zip(got, ref)]
            print("pre-diffusion %s m=%d chunk=%s: %s  bound %.2e" % (shape, m, chunk, ["%.2e" % e for e in errs], TOL_PRE))
            assert max(errs) < TOL_PRE, (shape, m, chunk, errs)
            assert all(g.data_ptr() != h.data_ptr() for g, h in zip(got, hv))
    same = k3.diffuse_sub(sim, *hv, hre, 1)                     # nsub = 1: the inputs, no launch
    assert all(a is b for a, b in zip(same, hv))
    assert all(torch.equal(a, f32(b)) for a, b in zip(hv, v))     # inputs untouched


# ---- 2. one launch of m substeps = m launches of one substep, bit for bit ----------------------------------------------------------------
def test_every_chunking_gives_equal_bits():
    shape = (17, 11, 37)                                         # ragged tiles on every axis
    sim = pre_sim(shape)
    v, re = dc.pre_inputs(shape)
    hv, hre = [f32(t) for t in v], f32(re)
    for m in range(1, 2 * S_MAX + 2):
        one = k3.diffuse_sub(sim, *hv, hre, m + 1, chunk=1)
        for chunk in range(2, S_MAX + 1):
            got = k3.diffuse_sub(sim, *hv, hre, m + 1, chunk=chunk)
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(got, one)), (m, chunk)
        dflt = k3.diffuse_sub(sim, *hv, hre, m + 1)
        assert all(torch.equal(a, b) for a, b in zip(dflt, one)), m
    assert bool(torch.isfinite(one[0]).all()) and dc.maxrel(one[0], hv[0]) > 0.05


# ---- 3. step surfaces against the reference: fields --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", dc.FIELD_CASES)
def test_step_fields_against_the_reference(name, n):
    ref = dc.reference(name, n)[0]
    sim = sim_of(name, n)
    host = sim_of(name, 1)                                      # the op names the count per call: a simulator registered without one
    h = torch_ops.register_scene3d(host)
    d, v, re = dc.state(name)
    st = [f32(t) for t in (d, *v, re)]
    with torch.no_grad():
        out = sim.step(*st)
        op = torch.ops.sol.karman3d_step_sub(*st, h, n)
        plain = host.step(*st)
    torch.cuda.synchronize()
    check_fields(out, ref, "%s n=%d" % (name, n))
    assert all(torch.equal(a, b) for a, b in zip(out, op))
    assert dc.maxrel(plain[1], ref[1]) > 0.01                   # a surface that ignored the count computes something else entirely


# ---- 4. step surfaces against the reference: gradients ----------------------------------------------------------------------------------
def run_adjoint(name, n, steps, force, surface="flow", re_grad=True):
    if surface == "flow":
        sim = sim_of(name, n, force, density_grad=True, re_grad=re_grad)
        step = sim.step
    else:
        sim = sim_of(name, 1)
        h = torch_ops.register_scene3d(sim)
        f = force or (0.0, 0.0, 0.0)
        step = lambda *a: torch.ops.sol.karman3d_step_sub(*a, h, n, True, re_grad, *f)
    hs = leaves(name, re_leaf=re_grad)
    out = chain(step, hs, steps)
    assert all(t.requires_grad for t in out)
    backward(name, out)
    return sim, out, hs


@pytest.mark.parametrize("name,n,steps,force", dc.GRAD_CASES)
def test_step_gradients_against_the_references_autograd(name, n, steps, force):
    """density, velocity and both cotangents in the loss, g_re asserted on every row; with buoyancy (0.3, -0.2, 0.15); two chained steps"""
    ref_out, ref_g = dc.reference(name, n, steps, force)
    what = "%s n=%d steps=%d F=%s" % (name, n, steps, force)
    res = []
    for surface in ("flow", "op"):
        _, out, hs = run_adjoint(name, n, steps, force, surface)
        assert all(h.grad is not None for h in hs)
        res.append([t.detach() for t in out] + list(grads_of(hs)))
    check_fields(res[0][:4], ref_out, what)
    check_grads(res[0][4:], ref_g, what, with_re=True)
    for a, b in zip(*res):                                      # the op is the same launches
        assert torch.equal(a, b) and float(a.abs().max()) > 0
    # re_grad off: re stays data, the other gradients are the same bits
    _, _, hs = run_adjoint(name, n, steps, force, "flow", re_grad=False)
    assert hs[4].grad is None and all(torch.equal(a.grad, b) for a, b in zip(hs[:4], res[0][4:8]))


@pytest.mark.parametrize("name,n,steps,force", dc.GRAD_CASES_NO_RE)
def test_step_gradients_of_rows_whose_re_gradient_is_ill_conditioned(name, n, steps, force):
    """rows the CPU twin's conditioning criterion keeps out of the g_re comparison (diffusion_substeps3d_cases.GRAD_CASES_NO_RE): run with
    re_grad off -- no g_re is computed -- for their fields and their density and velocity gradients"""
    ref_out, ref_g = dc.reference(name, n, steps, force)
    _, out, hs = run_adjoint(name, n, steps, force, "flow", re_grad=False)
    what = "%s n=%d steps=%d F=%s (re_grad off)" % (name, n, steps, force)
    assert hs[4].grad is None and all(h.grad is not None for h in hs[:4])
    check_fields(out, ref_out, what)
    check_grads(grads_of(hs), ref_g, what, with_re=False)


def test_the_existing_ops_honour_the_registered_simulators_count():
    """torch.ops.sol.karman3d_step / _dens / _re / _buoy on a simulator built with diffusion_substeps = n run n substeps: the bits of
    sim.step and of karman3d_step_sub naming the count, forward and backward"""
    name, n = "20_comb", 3
    sim = sim_of(name, n, density_grad=True, re_grad=True)
    h = torch_ops.register_scene3d(sim)
    h1 = torch_ops.register_scene3d(sim_of(name, 1))
    f = dc.FORCE
    pairs = [(lambda *a: torch.ops.sol.karman3d_step(*a, h), lambda *a: torch.ops.sol.karman3d_step_sub(*a, h1, n)),
             (lambda *a: torch.ops.sol.karman3d_step_dens(*a, h), lambda *a: torch.ops.sol.karman3d_step_sub(*a, h1, n, True)),
             (lambda *a: torch.ops.sol.karman3d_step_re(*a, h, True), sim.step),
             (lambda *a: torch.ops.sol.karman3d_step_buoy(*a, h, *f, True), lambda *a: torch.ops.sol.karman3d_step_sub(*a, h1, n, True, True, *f))]
    for k, (old, new) in enumerate(pairs):
        res = []
        for step in (old, new):
            hs = leaves(name)
            out = chain(step, hs, 2)
            loss = sum((a * f32(w)).sum() for a, w in zip(out[1:], dc.w_vel(name)))
            if out[0].requires_grad:
                loss = loss + (out[0] * f32(dc.w_dens(name))).sum()
            loss.backward()
            torch.cuda.synchronize()
            res.append([t.detach() for t in out] + list(grads_of(hs)))
        for a, b in zip(*res):
            assert torch.equal(a, b), k
        assert float(res[0][5].abs().max()) > 0
    ref = dc.reference(name, n)[0]
    with torch.no_grad():
        out = torch.ops.sol.karman3d_step(*[t.detach() for t in leaves(name)], h)
    check_fields(out, ref, "karman3d_step on a simulator with n=%d" % n)


def test_another_count_leaves_the_simulators_static_workspace_alone():
    """diffuse_sub / karman3d_step_sub with a count other than the simulator's own never replace its pre-diffusion buffer (a captured graph
    holds its address): a larger need is served by a buffer of that call alone"""
    name = "20_comb"
    d, v, re = dc.state(name)
    hv, hre = [f32(t) for t in v], f32(re)
    for n in (1, 5):
        sim = sim_of(name, n)
        before = (None if sim._sub_ws is None else sim._sub_ws.data_ptr(), sim._sub_ws_bytes)
        assert (before[0] is None) == (n == 1)
        got = k3.diffuse_sub(sim, *hv, hre, 9)
        fused = k3.diffuse_sub(sim, *hv, hre, 9, chunk=S_MAX)
        torch.cuda.synchronize()
        assert (None if sim._sub_ws is None else sim._sub_ws.data_ptr(), sim._sub_ws_bytes) == before
        assert all(torch.equal(a, b) for a, b in zip(got, fused))


def test_step_gradients_on_a_cg_scene():
    name, n, steps, force = dc.CG_CASE
    ref_out, ref_g = dc.reference(name, n, steps, force)
    sim, out, hs = run_adjoint(name, n, steps, force)
    assert sim.cg and bool((sim.solve_info["converged"] == 1).all()) and bool((sim.solve_info["converged_bwd"] == 1).all()), sim.solve_info
    check_fields(out, ref_out, "cg " + name)
    check_grads(grads_of(hs), ref_g, "cg " + name, with_re=True)


# ---- 5. the substep operator is symmetric --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(20, 10, 10), (18, 10, 70)])
def test_adjoint_identity(shape):
    """<w, diffuse_sub(v)> = <diffuse_sub(w), v>, fp64 accumulation on the host; allowed gap: the float32 pre-diffusion bound of |Mv||w|"""
    sim = pre_sim(shape)
    v, re = dc.pre_inputs(shape, seed=21)
    w, _ = dc.pre_inputs(shape, seed=22)
    hv, hw, hre = [f32(t) for t in v], [f32(t) for t in w], f32(re)
    dot = lambda a, b: sum(float((x.double() * y.double()).sum()) for x, y in zip(a, b))
    for m in (1, S_MAX, 2 * S_MAX + 1):
        mv, mw = k3.diffuse_sub(sim, *hv, hre, m + 1), k3.diffuse_sub(sim, *hw, hre, m + 1)
        torch.cuda.synchronize()
        lhs, rhs = dot(hw, mv), dot(mw, hv)
        scale = float(np.sqrt(dot(mv, mv) * dot(hw, hw)))
        print("adjoint identity %s m=%d: %.9e against %.9e, gap %.2e of |Mv||w| (bound %.2e)" % (shape, m, lhs, rhs, abs(lhs - rhs) / scale, TOL_PRE))
        assert scale > 0 and abs(lhs - rhs) < TOL_PRE * scale


# ---- 6. n = 1 changes nothing ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["16_comb", "16_wall"])
def test_n_equal_one_gives_the_default_constructors_bits(name):
    c = dc.case(name)
    wall = name == "16_wall"
    kw = dict(density_grad=True, re_grad=True, **c["kw"])
    sc = scene_of(c["shape"][1:], "cg" if wall else "auto", wall)
    res = []
    for extra in ({}, {"diffusion_substeps": 1}):
        sim = k3.Karman3DFlow(sc, c["shape"][0], dt=c["dt"], **kw, **extra)
        assert sim.nsub == 1 and sim._sub_ws is None
        hs = leaves(name)
        out = chain(sim.step, hs, 2)
        backward(name, out)
        with torch.no_grad():
            plain = sim.step(*[t.detach() for t in hs])
        res.append([t.detach() for t in out] + list(grads_of(hs)) + list(plain))
    for a, b in zip(*res):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    h = torch_ops.register_scene3d(sim)
    hs = leaves(name)
    backward(name, chain(lambda *a: torch.ops.sol.karman3d_step_sub(*a, h, 1, True, True), hs, 2))
    assert all(torch.equal(a, b) for a, b in zip(grads_of(hs), res[0][4:9]))


# ---- 7. the fused features keep the true Reynolds number --------------------------------------------------------------------------------------
def test_fused_features_carry_the_true_reynolds_number():
    name, n = "16_comb", 3
    sim = sim_of(name, n)
    d, v, re = dc.state(name)
    st = [f32(t) for t in (d, *v, re)]
    std = (0.2, 0.25, 0.3, o.STD_RE)
    feat = torch.zeros(*st[0].shape, 4, dtype=torch.float32, device=DEV)
    with torch.no_grad():
        out = sim.step(*st, feat_out=feat, feat_scale=[1.0 / s for s in std])
        base = sim.step(*st)
        ref = k3.to_feature3d(out[1], out[2], out[3], st[4]) / f32(torch.tensor(std))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, base))
    want = (st[4].double() / std[3]).reshape(-1, 1, 1, 1).expand_as(feat[..., 3])
    assert dc.maxrel(feat[..., 3], want) < 2.0 ** -22           # one fp32 product: re / std_re, NOT re * n or re / n
    assert dc.maxrel(feat, ref) < 2.0 ** -22
    assert sim.cfg.res == 8.0 and sim.sub_cfg(n) is not sim.cfg and sim.sub_cfg(1) is sim.cfg      # the launches ran on a copy


# ---- 8. stability --------------------------------------------------------------------------------------------------------------------------------
def test_stability_of_forty_steps():
    """16 x 8 x 8, alpha = 0.45, 40 steps without a network: the single stencil amplifies (the reference ends at 305 in float64, 235 in
    float32), three substeps do not (1.00001)"""
    Y, X, Z = dc.STABILITY["shape"]
    d, v = o.synthetic_state(1, Y, X, Z, dc.STABILITY["seed"])
    re = f32(dc.re_of(X, 1, (dc.STABILITY["alpha"],)))
    last = {}
    for n in (1, dc.STABILITY["n"]):
        sim = k3.Karman3DFlow(scene_of((Y, X, Z)), 1, diffusion_substeps=n)
        st = [f32(d)] + [f32(t) for t in v]
        with torch.no_grad():
            for _ in range(dc.STABILITY["steps"]):
                st = list(sim.step(*st, re))
        torch.cuda.synchronize()
        last[n] = max(float(t.abs().max()) for t in st[1:])
    print("max|v| after %d steps: %s" % (dc.STABILITY["steps"], last))
    assert last[1] > 50.0 and last[dc.STABILITY["n"]] <= 1.05


# ---- 9. trainer ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trainer_run(n, schedule="manual", use_graph=False):
    """one fwd_bwd of a fresh Karman3DTrainer on dc.trainer_problem (use_graph: a second call, the pure replay) -> (loss, per-step losses,
    gradient, final state, parameter offsets).  Cached: shared by the tests below, never modified."""
    p = dc.trainer_problem()
    B, Y, X, Z = dc.TRAINER_SHAPE
    net = k3.MarsMoon3D(device=DEV)
    net.set_weights([q.detach().numpy() for q in p["params"]])
    tr = k3.Karman3DTrainer(net, scene_of((Y, X, Z)), B, 2, dc.TRAINER_STD_V, o.STD_RE, use_graph=use_graph, schedule=schedule, diffusion_substeps=n)
    assert tr.nsub == n == tr.sim.nsub
    for _ in range(2 if use_graph else 1):                      # (graph: the second call is a pure replay)
        tr._grads.zero_()
        loss = tr.fwd_bwd(p["d"], *p["v"], p["re"], p["gts"])
    torch.cuda.synchronize()
    assert (tr._graph is not None) == use_graph
    return float(loss), tr.loss_steps.clone(), tr.grads.clone(), [t.clone() for t in tr.final], net.offsets


def test_trainer_sol2_against_the_reference():
    """SOL-2 at 2 x 32 x 16 x 16, n = 4, re = 256 / (0.45, 0.3).  Bounds: MARGIN times the float32-against-float64 distance of the reference's
    own unrolled loss (diffusion_substeps3d_cases.TRAINER_*_PIN): loss and per-step losses 8e-7, gradient 1e-5 relative L2 (per layer
    2.25e-4), final state 1.5e-5 relative L2."""
    n = dc.TRAINER_N
    loss, losses, gref, fin = dc.trainer_reference(n)
    man = trainer_run(n)
    e = [abs(float(a) - b) / abs(b) for a, b in zip(man[1], losses)]
    eg = rel(man[2], gref)
    off = man[4]
    per = [rel(man[2][off[k]:off[k + 1]], gref[off[k]:off[k + 1]]) for k in range(len(o.mars_moon3d_param_shapes()))]
    ef = [rel(a, b) for a, b in zip(man[3], fin)]
    print("trainer: loss %.9e against %.9e (%.2e), per-step %s, gradient %.2e (worst layer %.2e), final state %s" % (
        man[0], loss, abs(man[0] - loss) / abs(loss), ["%.2e" % x for x in e], eg, max(per), ["%.2e" % x for x in ef]))
    M = dc.MARGIN
    assert abs(man[0] - loss) < M * dc.TRAINER_LOSS_PIN * abs(loss), (man[0], loss)
    assert max(e) < M * dc.TRAINER_LOSS_PIN, e
    assert eg < M * dc.TRAINER_GRAD_PIN, eg
    assert max(per) < M * dc.TRAINER_LAYER_PIN, per
    assert max(ef) < M * dc.TRAINER_FINAL_PIN, ef
    # the count is in the gradient: the n = 1 trainer's (today's launches) is far beyond the tolerance away (the reference's is 0.030 away)
    away = rel(trainer_run(1)[2], gref)
    print("n = 1 gradient against the n = %d reference: %.2e" % (n, away))
    assert away > 100 * M * dc.TRAINER_GRAD_PIN


def test_trainer_manual_schedule_equals_autograd():
    """the hand-written schedule (diffuse_sub before each solver launch, and on the cotangent in the reverse sweep) against the
    torch-autograd composition of Karman3DFlow.step: fp32 round-off, the bounds of the 3-D suite's manual-against-autograd tests"""
    man, aut = trainer_run(dc.TRAINER_N), trainer_run(dc.TRAINER_N, schedule="autograd")
    print("manual against autograd: loss %.2e, per-step %.2e, gradient %.2e, final %s" % (
        abs(man[0] - aut[0]) / abs(aut[0]), rel(man[1], aut[1]), rel(man[2], aut[2]), ["%.2e" % rel(a, b) for a, b in zip(man[3], aut[3])]))
    assert abs(man[0] - aut[0]) < 2e-6 * abs(aut[0]) and rel(man[1], aut[1]) < 2e-6
    assert rel(man[2], aut[2]) < 2e-5
    assert all(rel(a, b) < 2e-6 for a, b in zip(man[3], aut[3]))


@pytest.mark.parametrize("schedule", ["manual", "autograd"])
def test_trainer_graph_replay_equals_eager(schedule):
    """use_graph=True captures kernel nodes only (_lib.capture_graph runs sol_graph_check and refuses anything else); the second replay
    equals the eager run bit for bit"""
    eager, gr = trainer_run(dc.TRAINER_N, schedule=schedule), trainer_run(dc.TRAINER_N, schedule=schedule, use_graph=True)
    assert gr[0] == eager[0] and torch.equal(gr[1], eager[1]) and torch.equal(gr[2], eager[2])
    assert all(torch.equal(a, b) for a, b in zip(gr[3], eager[3]))
    assert float(gr[2].abs().max()) > 0


# ---- 10. roll-out ------------------------------------------------------------------------------------------------------------------------------------
def test_rollout_against_the_reference_rollout():
    """3 steps at 16 x 8 x 8, B = 2, n = 3, the golden small-weight network.  Bound: three steps, each within the one-step field bound (the
    step map does not amplify differences at these CFL numbers, and three substeps of alpha / 3 <= 0.15 damp them): 3 x 1.35e-5."""
    import make_golden as mg
    name, n, steps = "16_comb", 3, 3
    d, v, re = dc.state(name)
    g = dc.geometry(name)
    params = mg.k3d_params()
    std_v, std_re = (0.2, 0.25, 0.3), o.STD_RE
    dr, vr = dc.rollout_reference(params, d, v, re, g, std_v, std_re, n, steps)
    d1, v1 = dc.rollout_reference(params, d, v, re, g, std_v, std_re, 1, steps)
    net = k3.MarsMoon3D(device=DEV)
    net.set_weights([p.numpy() for p in params])
    ro = k3.Karman3DRollout(net, scene_of(dc.case(name)["shape"][1:]), d.shape[0], std_v, std_re, diffusion_substeps=n)
    assert ro.nsub == n
    out = ro.run(f32(d), *[f32(t) for t in v], f32(re), steps)
    torch.cuda.synchronize()
    errs = [dc.maxrel(a, b) for a, b in zip(out, (dr, *vr))]
    print("roll-out, %d steps: %s (bound %.2e)" % (steps, ["%.2e" % e for e in errs], steps * TOL_F))
    assert max(errs) < steps * TOL_F, errs
    assert dc.maxrel(v1[0], vr[0]) > 0.01                       # the count is in the flow


# ---- 11. bad arguments: error returns, never faults ----------------------------------------------------------------------------------------------
def test_bad_arguments_are_rejected_with_a_message_and_no_launch():
    shape = (20, 10, 10)
    sim = pre_sim(shape)
    lib = _lib.load()
    v, re = dc.pre_inputs(shape)
    hv, hre = [f32(t) for t in v], f32(re)
    out = [torch.full_like(t, 7.0) for t in hv]
    cfg = _lib.Karman3DCfg.from_buffer_copy(sim.cfg)            # the entry point takes the coefficient from the cfg it is given: the scaled one
    cfg.res = k3.diffusion_sub_res(sim.cfg.res, S_MAX + 2)
    ws = torch.zeros(lib.sol_karman3d_diffuse_sub_workspace_bytes(C.byref(cfg), S_MAX + 1, 0) // 4, dtype=torch.float32, device=DEV)
    call = lambda ins, outs, m, chunk, w, nbytes: lib.sol_karman3d_diffuse_sub(C.byref(cfg), stream(), ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), ptr(hre),
                                                                                  ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), m, chunk, ptr(w), nbytes)
    err = lambda: lib.sol_last_error()
    assert call(hv, out, 0, 0, None, 0) == -1 and b"substeps m must be in" in err()
    assert call(hv, out, 2, S_MAX + 1, None, 0) == -1 and b"chunk" in err()
    assert call(hv, [hv[0], out[1], out[2]], 2, 0, None, 0) == -1 and b"alias" in err()
    assert call(hv, [out[0], out[0], out[2]], 2, 0, None, 0) == -1 and b"buffers of their own" in err()
    assert call(hv, out, S_MAX + 1, 0, None, 0) == -1 and b"need a workspace" in err()
    assert call(hv, out, S_MAX + 1, 0, ws, 1024) == -1 and b"workspace too small" in err()
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in out) and all(torch.equal(a, f32(b)) for a, b in zip(hv, v))      # nothing was launched
    assert call(hv, out, S_MAX + 1, 0, ws, ws.numel() * 4) == 0                                                  # ... and the good call runs
    torch.cuda.synchronize()
    assert max(dc.maxrel(a, b) for a, b in zip(out, dc.pre_reference(shape, S_MAX + 2))) < TOL_PRE
    # the Python surface
    with pytest.raises(ValueError, match="chunk"):
        k3.diffuse_sub(sim, *hv, hre, 3, chunk=S_MAX + 1)
    with pytest.raises(ValueError, match="integer >= 1"):
        k3.diffuse_sub(sim, *hv, hre, 0)
    with pytest.raises(ValueError, match="are not"):
        k3.diffuse_sub(sim, hv[1], hv[0], hv[2], hre, 3)
    with pytest.raises(Exception, match="integer >= 1"):
        torch.ops.sol.karman3d_step_sub(f32(torch.zeros(1)), *hv, hre, torch_ops.register_scene3d(sim), 0)


# ---- 12. the script --------------------------------------------------------------------------------------------------------------------------------
def test_karman3d_script_with_diffusion_substeps(tmp_path):
    """scripts/karman3d.py --diffusion-substeps auto at -r 8, --re 142.2 (alpha = 0.45): three substeps, recorded with the run and with the
    model; a --model roll-out picks the count up and refuses a contradicting flag"""
    import importlib.util
    import pickle
    import sol_amd
    from sol_amd import scene as sc_io
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    sys.path.insert(0, sdir)
    spec = importlib.util.spec_from_file_location("sol_script_karman3d_sub", os.path.join(sdir, "karman3d.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    common = ["-r", "8", "-t", "6", "--re", "142.2"]
    plain = mod.main(common + ["-o", str(tmp_path / "plain")])
    tr = mod.main(common + ["-o", str(tmp_path / "sub"), "--diffusion-substeps", "auto", "--train-sol", "2", "--train-steps", "1"])
    a, b = (sc_io.read_zipped_array(p + "/velo_000005.npz") for p in (plain, tr))
    assert a.shape == b.shape == (1, 17, 9, 9, 3) and np.isfinite(b).all()
    assert np.abs(a - b).max() > 1e-2 * np.abs(b).max()
    rec = [pickle.load(open(p + "/params.pickle", "rb"))["diffusion_substeps"] for p in (plain, tr)]
    assert rec == [1, 3]
    model = tr + "/model3d.pt"
    assert torch.load(model, map_location="cpu")["diffusion_substeps"] == 3
    ro = mod.main(common + ["-o", str(tmp_path / "ro"), "--model", model])
    assert pickle.load(open(ro + "/params.pickle", "rb"))["diffusion_substeps"] == 3
    assert np.isfinite(sc_io.read_zipped_array(ro + "/velo_000005.npz")).all()
    with pytest.raises(SystemExit, match="contradicts"):
        mod.main(common + ["-o", str(tmp_path / "bad"), "--model", model, "--diffusion-substeps", "2"])
