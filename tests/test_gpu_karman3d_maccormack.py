"""MacCormack advection of the karman-3d step on the device, against the float64 reference of maccormack3d_cases.py (the definition of
include/sol_hip.h, "MACCORMACK ADVECTION on the karman-3d step", written with the oracle's own sampling).

Bounds: fields TOL_FIELD = 1e-5 (relative L2), gradients TOL_GRAD = 1e-4 in the trimmed metric of large2d_scenes with the cap TRIM = 1e-3
asserted (k <= int(TRIM n): the limiter and the clamped edges tie exactly in places and fp32 decides a few entries the other way), g_re
TOL_GRAD relative on the rows whose float32 reference holds it (all of STEP_CASES).  The cases are the ones test_karman3d_maccormack_cpu.py
admits: the reference in float32 stays within a fifth of these bounds of the reference in float64 (fields 2e-6, trimmed gradients 2e-5) on
every step row AND every stage case (the stage runs at dx = 2 for that: maccormack3d_cases.stage_geometry), the roll-out within three
times the field figure.  Bit comparisons
are torch.equal.  Trainer and roll-out: MARGIN = 5 times the pins the CPU twin measures (the 3-D convention).

Measured on an MI355X (printed by every test): the stage alone fields <= 8.7e-8, trimmed gradients <= 9.8e-8 (trimmed = untrimmed to two
digits: no entry decided the other way); the step's 16 rows fields <= 1.1e-6, trimmed gradients <= 2.3e-5 (16_lowre), g_re <= 6.1e-6;
blob peaks 0.43128 / 0.82905; trainer loss 8.9e-10, per-step losses 6.3e-8, weight gradient 7.7e-7 (worst layer 1.3e-5), final state
8.5e-7, manual against autograd 6.2e-7, the semi-Lagrangian trainer's gradient 1.5e-3 away; roll-out of three steps 6.9e-7."""
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
import diffusion_substeps3d_cases as ds
import maccormack3d_cases as mc
from large2d_scenes import DEV, f32, rel

pytestmark = pytest.mark.gpu

TOL_FIELD, TOL_GRAD, TRIM = mc.TOL_FIELD, mc.TOL_GRAD, mc.TRIM


@pytest.fixture
def options():
    """sets library options for one test and puts the old values back"""
    old = {}

    def set_(**kw):
        for k, v in kw.items():
            old.setdefault(k, _lib.get_option(k))
            _lib.set_option(k, v)
    yield set_
    for k, v in old.items():
        _lib.set_option(k, v)


def check_fields(got, ref, what, tol=TOL_FIELD):
    errs = [rel(a, b) for a, b in zip(got, ref)]
    print("%s fields: %s  bound %.1e" % (what, ["%.2e" % e for e in errs], tol))
    assert max(errs) < tol, (what, errs)


def check_grads(got, ref, what):
    """trimmed TOL_GRAD on every component, the cap asserted"""
    for name, a, b in zip(mc.NAMES, got, ref):
        if float(b.abs().max()) == 0.0:
            assert float(a.abs().max()) == 0.0, (what, name)
            continue
        t, k, worst = mc.trimmed_rel(a, b)
        print("%s %s: trimmed %.2e (untrimmed %.2e, %d of %d left out, largest %.2e)  bound %.1e" % (what, name, t, rel(a, b), k, b.numel(), worst, TOL_GRAD))
        assert k <= int(TRIM * b.numel()) and t < TOL_GRAD, (what, name, t, k)


# ---- 1. the stage alone ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stage_sim(shape, order="after", B=mc.STAGE_B):
    """a simulator whose scene is maccormack3d_cases.stage_geometry (the stage reads the grid, dx, dt, the masks and the inflow order)"""
    g = mc.stage_geometry(*shape)
    sc = k3.Scene3D(*shape, length=g.length, device=DEV, active=g.active, inflow=g.inflow, pressure_solver="cg")
    assert sc.dx == g.dx
    return k3.Karman3DFlow(sc, B, inflow_order=order)


def stage_tensors(shape, cfl=None, B=mc.STAGE_B):
    return [f32(t) for t in mc.stage_inputs(shape, cfl, B=B)]


@pytest.mark.parametrize("c", mc.STAGE_CASES, ids=[mc.stage_id(c) for c in mc.STAGE_CASES])
def test_stage_forward_and_adjoint_against_the_reference(c):
    shape, s, order, cfl = c
    ref_out, ref_g, st = mc.stage_reference(*c)
    sim = stage_sim(shape, order)
    d, cy, cx, cz, *w = stage_tensors(shape, cfl)
    out = k3.advect3d(sim, d, cy, cx, cz, s)
    g = k3.advect3d_bwd(sim, d, cy, cx, cz, *w, adv=s)
    g2 = k3.advect3d_bwd(sim, d, cy, cx, cz, *w, adv=s)
    g0 = k3.advect3d_bwd(sim, d, cy, cx, cz, *w, adv=s, tile_window=False)
    torch.cuda.synchronize()
    what = "stage " + mc.stage_id(c)
    print("%s: the limiter reverted %s" % (what, ["%.3f" % x for x in st]))
    check_fields(out, ref_out, what)
    check_grads(g, ref_g, what)
    for a, b, z in zip(g, g2, g0):                              # run twice: equal bits; LDS windows or global atomics: equal bits
        assert torch.equal(a, b) and torch.equal(a, z) and bool(torch.isfinite(a).all())
    if cfl is None and s == 1.0:
        sl = mc.stage_reference(shape, s, order, cfl, "semi_lagrangian")[0]
        assert rel(sl[0], ref_out[0]) > 0.05                     # a surface that ignored the scheme computes something else


@pytest.mark.parametrize("shape", [(20, 10, 10), (18, 10, 70)])
def test_stage_s0_and_advection0(shape):
    """s = 0 is the semi-Lagrangian stage within 1e-6; advection = 0 through the new entry is the plain stage (the step's own launch and
    scatters), against the reference's semi-Lagrangian branch, windows on and off bit-equal"""
    sim = stage_sim(shape)
    d, cy, cx, cz, *w = stage_tensors(shape)
    zero, plain = k3.advect3d(sim, d, cy, cx, cz, 0.0), k3.advect3d(sim, d, cy, cx, cz, None)
    torch.cuda.synchronize()
    ref = mc.stage_reference(shape, 1.0, scheme="semi_lagrangian")[0]
    check_fields(plain, ref, "advection = 0 %s" % (shape,))
    assert max(rel(a, b) for a, b in zip(zero, plain)) < 1e-6
    gz, gp = k3.advect3d_bwd(sim, d, cy, cx, cz, *w, adv=0.0), k3.advect3d_bwd(sim, d, cy, cx, cz, *w, adv=None)
    gp0 = k3.advect3d_bwd(sim, d, cy, cx, cz, *w, adv=None, tile_window=False)
    torch.cuda.synchronize()
    ref_g = mc.stage_reference(shape, 1.0, scheme="semi_lagrangian")[1]
    check_grads(gp, ref_g, "advection = 0 adjoint %s" % (shape,))
    assert max(rel(a, b) for a, b in zip(gz, gp)) < 1e-6 and all(torch.equal(a, b) for a, b in zip(gp, gp0))


def test_step_adjoint_options_give_equal_bits(options):
    """the step's MacCormack adjoint with the semi-Lagrangian scatters' LDS windows (options k3d_adj_tile, k3d_dens_adj_tile) off and on:
    the step entries read the options where the stage's entry takes tile_window (tested above); the fixture puts the options back"""
    row = mc.KIND_CASE
    res = []
    for tile in (1, 0):
        options(k3d_adj_tile=tile, k3d_dens_adj_tile=tile)
        _, out, hs = run_adjoint(row)
        res.append([t.detach() for t in out] + list(grads_of(hs)))
    for a, b in zip(*res):
        assert torch.equal(a, b) and float(a.abs().max()) > 0


def test_a_non_finite_cotangent_poisons_its_own_simulation_only():
    shape, B = (20, 10, 10), 2
    sim = stage_sim(shape, B=B)
    d, cy, cx, cz, *w = stage_tensors(shape, B=B)
    clean = k3.advect3d_bwd(sim, d, cy, cx, cz, *w, adv=1.0)
    for which in (0, 2):                                         # the density's cotangent, a velocity component's
        bad = [t.clone() for t in w]
        bad[which][1, 3, 4, 5] = float("inf")
        for tile in (True, False):
            got = k3.advect3d_bwd(sim, d, cy, cx, cz, *bad, adv=1.0, tile_window=tile)
            torch.cuda.synchronize()
            for a, b in zip(got, clean):
                assert torch.equal(a[0], b[0]) and bool(torch.isfinite(a[0]).all())
                assert not bool(torch.isfinite(a[1]).any())


# ---- 2. the limiter at work --------------------------------------------------------------------------------------------------------------
def test_blob_keeps_its_peak():
    """the Gaussian blob carried 40 steps by a uniform flow, the stage alone: both peaks within 1e-4 of the float64 reference's, MacCormack
    above semi-Lagrangian, the density never above its initial maximum or below 0"""
    N = mc.BLOB["N"]
    sc = k3.Scene3D(N, N, N, length=float(N), device=DEV, active=np.ones((N, N, N)), inflow=np.zeros((N, N, N)), pressure_solver="cg")
    sim = k3.Karman3DFlow(sc, 1)
    d0, c = mc.blob_inputs()
    hc = [f32(t) for t in c]
    peaks = {}
    for scheme, adv in (("semi_lagrangian", None), ("mac_cormack", 1.0)):
        d = f32(d0)
        top = float(d.max())
        lo, hi = [], []
        for _ in range(mc.BLOB["steps"]):
            d = k3.advect3d(sim, d, *hc, adv)[0]
            lo.append(d.min())
            hi.append(d.max())
        torch.cuda.synchronize()
        peaks[scheme] = float(d.max())
        assert float(torch.stack(lo).min()) >= 0.0 and float(torch.stack(hi).max()) <= top, scheme
        assert abs(peaks[scheme] - mc.blob_peak(scheme)) < 1e-4, (scheme, peaks[scheme], mc.blob_peak(scheme))
    print("blob peaks after %d steps: %s" % (mc.BLOB["steps"], peaks))
    assert peaks["mac_cormack"] > peaks["semi_lagrangian"] + 0.3


# ---- 3. the step --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene_of(shape, solver="auto", wall=False):
    Y, X, Z = shape
    g = ds.wall_geometry(Y, X, Z) if wall else o.geometry(Y, X, Z)
    return k3.Scene3D(Y, X, Z, device=DEV, active=g.active, inflow=g.inflow, pressure_solver=solver)


def sim_of(name, s, force=None, n=1, mac=True, **kw):
    c = ds.case(name)
    wall = name == "16_wall"
    if wall:
        kw.setdefault("cg_rtol", 1e-7)
    adv = dict(advection="mac_cormack", correction_strength=s) if mac else {}
    return k3.Karman3DFlow(scene_of(c["shape"][1:], "cg" if wall else "auto", wall), c["shape"][0], dt=c["dt"], buoyancy=force,
                           diffusion_substeps=n, **adv, **c["kw"], **kw)


def leaves(name, re_leaf=True):
    d, v, re = mc.state(name)
    return [f32(t).requires_grad_(True) for t in (d, *v)] + [f32(re).requires_grad_(re_leaf)]


def chain(step, hs, steps=1):
    cur = hs[:4]
    for _ in range(steps):
        cur = step(*cur, hs[4])
    return cur


def backward(name, out, kind="both"):
    loss = 0.0
    if kind in ("dens", "both"):
        loss = loss + (out[0] * f32(ds.w_dens(name))).sum()
    if kind in ("vel", "both"):
        loss = loss + sum((a * f32(w)).sum() for a, w in zip(out[1:], ds.w_vel(name)))
    loss.backward()
    torch.cuda.synchronize()


def grads_of(hs):
    return tuple(torch.zeros_like(h) if h.grad is None else h.grad for h in hs)


def run_adjoint(row, surface="flow", kind="both", density=True, re_grad=True):
    name, s, steps, force, n, _ = row
    if surface == "flow":
        sim = sim_of(name, s, force, n, density_grad=density, re_grad=re_grad)
        step = sim.step
    else:
        sim = sim_of(name, s, mac=False)                         # the op names the scheme, the count and the force per call
        h = torch_ops.register_scene3d(sim)
        f = force or (0.0, 0.0, 0.0)
        step = lambda *a: torch.ops.sol.karman3d_step_adv(*a, h, 1, s, n, density, re_grad, *f)
    hs = leaves(name, re_leaf=re_grad)
    out = chain(step, hs, steps)
    backward(name, out, kind if (density or force is not None) else "vel")
    return sim, out, hs


@pytest.mark.parametrize("row", mc.STEP_CASES, ids=[mc.case_id(r) for r in mc.STEP_CASES])
def test_step_fields_and_gradients_against_the_reference(row):
    """Karman3DFlow.step and torch.ops.sol.karman3d_step_adv (the same launches: equal bits), density_grad and re_grad on: fields, the four
    state gradients and g_re"""
    name, s, steps, force, n, with_re = row
    ref_out, ref_g, st = mc.reference(name, s, steps, force, n)
    what = mc.case_id(row)
    res = []
    for surface in ("flow", "op"):
        sim, out, hs = run_adjoint(row, surface)
        assert all(h.grad is not None for h in hs)
        res.append([t.detach() for t in out] + list(grads_of(hs)))
    if name == "16_wall":
        assert sim.cg and bool((sim.solve_info["converged"] == 1).all()) and bool((sim.solve_info["converged_bwd"] == 1).all()), sim.solve_info
    print("%s: the limiter reverted up to %.3f of an array" % (what, max(st)))
    check_fields(res[0][:4], ref_out, what)
    check_grads(res[0][4:8], ref_g[:4], what)
    if with_re:
        e = float(((res[0][8].double().cpu() - ref_g[4]).abs() / ref_g[4].abs()).max())
        print("%s g_re: %.2e  bound %.1e  (%s against %s)" % (what, e, TOL_GRAD, res[0][8].tolist(), ref_g[4].tolist()))
        assert e < TOL_GRAD, (what, "g_re", e)
    for a, b in zip(*res):
        assert torch.equal(a, b) and float(a.abs().max()) > 0
    sl = mc.reference(name, s, steps, force, n, scheme="semi_lagrangian")[0]
    assert rel(sl[0], ref_out[0]) > 10 * TOL_FIELD               # a surface that ignored the scheme misses the density


@pytest.mark.parametrize("kind", mc.KINDS)
def test_step_kinds_of_loss_and_gradient_modes(kind):
    """loss on the density, the velocity or both; density_grad / re_grad off: the density is a passive tracer, re is data, and the velocity
    gradient of a velocity loss keeps its bits"""
    row = mc.KIND_CASE
    name, s, steps, force, n, _ = row
    ref_g = mc.reference(name, s, steps, force, n, kind)[1]
    _, out, hs = run_adjoint(row, kind=kind)
    got = grads_of(hs)
    check_grads(got[:4], ref_g[:4], "%s loss on %s" % (mc.case_id(row), kind))
    e = float(((got[4].double().cpu() - ref_g[4]).abs() / ref_g[4].abs()).max())
    assert e < TOL_GRAD, ("g_re", kind, e)
    if kind == "vel":
        _, out2, hs2 = run_adjoint(row, kind=kind, density=False, re_grad=False)
        assert not out2[0].requires_grad and hs2[0].grad is None and hs2[4].grad is None
        assert all(torch.equal(a.grad, b) for a, b in zip(hs2[1:4], got[1:4]))
        _, _, hs3 = run_adjoint(row, kind=kind, density=True, re_grad=False)
        assert hs3[4].grad is None and all(torch.equal(a, b) for a, b in zip(grads_of(hs3)[:4], got[:4]))      # (no force: no density gradient)


def test_defaults_are_the_bits_they_were():
    """advection="semi_lagrangian" spelled out gives the default constructor's bits, forward and backward; the op with advection = 0 gives
    karman3d_step_sub's; an _adv entry with advection = 0 gives the _buoy entry's"""
    name = "16_comb"
    c = ds.case(name)
    sc = scene_of(c["shape"][1:])
    res = []
    for extra in ({}, {"advection": "semi_lagrangian", "correction_strength": 0.5}):
        sim = k3.Karman3DFlow(sc, c["shape"][0], dt=c["dt"], density_grad=True, re_grad=True, **extra)
        assert sim.adv is None
        hs = leaves(name)
        out = chain(sim.step, hs, 2)
        backward(name, out)
        res.append([t.detach() for t in out] + list(grads_of(hs)))
    h = torch_ops.register_scene3d(sim)
    for step in (lambda *a: torch.ops.sol.karman3d_step_adv(*a, h, 0, 1.0, 1, True, True), lambda *a: torch.ops.sol.karman3d_step_sub(*a, h, 1, True, True)):
        hs = leaves(name)
        out = chain(step, hs, 2)
        backward(name, out)
        res.append([t.detach() for t in out] + list(grads_of(hs)))
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    # the C entries: _adv with advection = 0 against _buoy, a kept force
    lib, s = sim.lib, sim.scene
    st = [t.detach() for t in leaves(name)]
    outs = []
    for entry, tail in ((lib.sol_karman3d_step_fwd_buoy, mc.FORCE), (lib.sol_karman3d_step_fwd_adv, mc.FORCE + (0, 0.5))):
        out = [torch.empty_like(t) for t in st[:4]]
        _lib.check(entry(C.byref(sim.cfg), stream(), *[ptr(t) for t in st], ptr(s.active), ptr(s.inflow), ptr(s.velBCy), ptr(s.velBCyMask), s.bc_stride,
                         *[ptr(t) for t in out], None, None, None, None, None, s.direct_header.ctypes.data_as(C.c_void_p), ptr(sim.workspace),
                         sim.workspace_bytes, *tail))
        outs.append(out)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(*outs)) and rel(outs[0][1], res[0][1]) > 1e-4


@pytest.mark.parametrize("with_re", [False, True])
def test_backward_adv_entries_with_advection0_give_the_existing_entries_bits(with_re):
    """sol_karman3d_step_bwd_adv(_re) and sol_karman3d_density_bwd_adv(_re) called directly with advection = 0: the bits of the _buoy
    entries (a force), of the plain entries (a zero force, NULL g_d_out / g_dsum) and of the plain density entries"""
    name = "16_comb"
    c = ds.case(name)
    sim = k3.Karman3DFlow(scene_of(c["shape"][1:]), c["shape"][0], dt=c["dt"])
    lib, s, B = sim.lib, sim.scene, sim.B
    st = [t.detach() for t in leaves(name)]
    saved = [torch.empty_like(t) for t in st[1:4]]
    with torch.no_grad():
        out, vel = sim._forward(k3.StepPhysics3D(), *st, saved)
        stage = k3.advect3d(sim, st[0], *saved, None)             # the stage's entry with advection = 0 IS the step's advection launch:
    assert torch.equal(stage[0], out[0])                          # its density is the step's, bit for bit (the velocity goes on to the projection)
    re, wd, wv = st[4], f32(ds.w_dens(name)), [f32(t) for t in ds.w_vel(name)]
    vin = vel if with_re else None
    hdr = s.direct_header.ctypes.data_as(C.c_void_p)
    sim._ws(max(lib.sol_karman3d_step_bwd_adv_workspace_bytes(C.byref(sim.cfg), 1, 0), lib.sol_karman3d_density_bwd_adv_workspace_bytes(C.byref(sim.cfg), 1, 0)))

    def re_tail():
        g_re = torch.empty(B, dtype=torch.float32, device=DEV)
        return ((ptr(vel[0]), ptr(vel[1]), ptr(vel[2]), ptr(g_re), 0), [g_re]) if with_re else ((), [])

    def step_bwd_adv(force, g_d, want_dsum):
        gi = [torch.empty_like(t) for t in saved]
        g_dsum = torch.empty_like(wd) if want_dsum else None
        tail, extra = re_tail()
        entry = lib.sol_karman3d_step_bwd_adv_re if with_re else lib.sol_karman3d_step_bwd_adv
        _lib.check(entry(C.byref(sim.cfg), stream(), *[ptr(t) for t in saved], ptr(re), ptr(s.active), ptr(s.velBCyMask), s.bc_stride, *[ptr(t) for t in wv],
                         *[ptr(t) for t in gi], hdr, ptr(sim.workspace), sim.workspace_bytes, *tail, *force, ptr(g_d), ptr(g_dsum), 0, 0.5))
        return gi + extra + ([g_dsum] if want_dsum else [])

    def density_bwd_adv():
        od, gi = torch.empty_like(wd), [torch.empty_like(t) for t in saved]
        tail, extra = re_tail()
        entry = lib.sol_karman3d_density_bwd_adv_re if with_re else lib.sol_karman3d_density_bwd_adv
        _lib.check(entry(C.byref(sim.cfg), stream(), ptr(st[0]), ptr(s.inflow), *[ptr(t) for t in saved], ptr(re), ptr(s.velBCyMask), s.bc_stride, ptr(wd),
                         ptr(od), *[ptr(t) for t in gi], 0, ptr(sim.workspace), sim.workspace_bytes, *tail, 0, 0.5))
        return [od] + gi + extra

    with torch.no_grad():
        pairs = [(step_bwd_adv(mc.FORCE, wd, True), sim._bwd(saved, re, *wv, vel_in=vin, buoyancy=mc.FORCE, g_d=wd)),
                 (step_bwd_adv((0.0, 0.0, 0.0), None, False), sim._bwd(saved, re, *wv, vel_in=vin)),
                 (density_bwd_adv(), list(k3.density_bwd(sim, st[0], saved, re, wd, vel_in=vin)))]
    torch.cuda.synchronize()
    for k, (got, want) in enumerate(pairs):
        assert len(got) == len(want), k
        for a, b in zip(got, want):
            assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0, k


def test_the_existing_ops_honour_the_registered_simulators_scheme():
    row = mc.KIND_CASE
    name, s = row[0], row[1]
    sim = sim_of(name, s, density_grad=True, re_grad=True)
    h = torch_ops.register_scene3d(sim)
    res = []
    for step in (lambda *a: torch.ops.sol.karman3d_step_re(*a, h, True), sim.step):
        hs = leaves(name)
        backward(name, chain(step, hs))
        res.append(grads_of(hs))
    assert all(torch.equal(a, b) and float(a.abs().max()) > 0 for a, b in zip(*res))
    check_grads(res[0][:4], mc.reference(*row[:5])[1][:4], "karman3d_step_re on a MacCormack simulator")


# ---- 4. trainer and roll-out -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trainer_run(schedule="manual", use_graph=False, mac=True):
    """one fwd_bwd of a fresh Karman3DTrainer on buoyancy3d_cases.trainer_problem with the MacCormack step (use_graph: a second call, the
    pure replay) -> (loss, per-step losses, gradient, final state, parameter offsets).  Cached: shared by the tests below, never modified."""
    p = bc.trainer_problem()
    B, Y, X, Z = mc.TRAINER_SHAPE
    net = k3.MarsMoon3D(device=DEV)
    net.set_weights([q.detach().numpy() for q in p["params"]])
    adv = dict(advection="mac_cormack", correction_strength=1.0) if mac else {}
    tr = k3.Karman3DTrainer(net, scene_of((Y, X, Z)), B, 2, mc.TRAINER_STD_V, o.STD_RE, use_graph=use_graph, schedule=schedule, **adv)
    assert tr.sim.adv == (1.0 if mac else None)
    for _ in range(2 if use_graph else 1):
        tr._grads.zero_()
        loss = tr.fwd_bwd(p["d"], *p["v"], p["re"], p["gts"])
    torch.cuda.synchronize()
    assert (tr._graph is not None) == use_graph
    return float(loss), tr.loss_steps.clone(), tr.grads.clone(), [t.clone() for t in tr.final], net.offsets


def test_trainer_sol2_against_the_reference():
    """SOL-2 at 2 x 32 x 16 x 16 with the MacCormack step.  Bounds: MARGIN times the float32-against-float64 distance of the reference's own
    unrolled loss (maccormack3d_cases.TRAINER_*_PIN)"""
    loss, losses, gref, fin = mc.trainer_reference()
    man = trainer_run()
    e = [abs(float(a) - b) / abs(b) for a, b in zip(man[1], losses)]
    eg = rel(man[2], gref)
    off = man[4]
    per = [rel(man[2][off[k]:off[k + 1]], gref[off[k]:off[k + 1]]) for k in range(len(o.mars_moon3d_param_shapes()))]
    ef = [rel(a, b) for a, b in zip(man[3], fin)]
    print("trainer: loss %.9e against %.9e (%.2e), per-step %s, gradient %.2e (worst layer %.2e), final state %s" % (
        man[0], loss, abs(man[0] - loss) / abs(loss), ["%.2e" % x for x in e], eg, max(per), ["%.2e" % x for x in ef]))
    M = mc.MARGIN
    assert abs(man[0] - loss) < M * mc.TRAINER_LOSS_PIN * abs(loss), (man[0], loss)
    assert max(e) < M * mc.TRAINER_LOSS_PIN, e
    assert eg < M * mc.TRAINER_GRAD_PIN, eg
    assert max(per) < M * mc.TRAINER_LAYER_PIN, per
    assert max(ef) < M * mc.TRAINER_FINAL_PIN, ef
    away = rel(trainer_run(mac=False)[2], gref)                  # the scheme is in the gradient: today's trainer is far beyond the tolerance away
    print("semi-Lagrangian trainer's gradient against the MacCormack reference: %.2e" % away)
    assert away > 10 * M * mc.TRAINER_GRAD_PIN


def test_trainer_manual_schedule_equals_autograd():
    man, aut = trainer_run(), trainer_run(schedule="autograd")
    print("manual against autograd: loss %.2e, per-step %.2e, gradient %.2e, final %s" % (
        abs(man[0] - aut[0]) / abs(aut[0]), rel(man[1], aut[1]), rel(man[2], aut[2]), ["%.2e" % rel(a, b) for a, b in zip(man[3], aut[3])]))
    assert abs(man[0] - aut[0]) < 2e-6 * abs(aut[0]) and rel(man[1], aut[1]) < 2e-6
    assert rel(man[2], aut[2]) < 2e-5
    assert all(rel(a, b) < 2e-6 for a, b in zip(man[3], aut[3]))


@pytest.mark.parametrize("schedule", ["manual", "autograd"])
def test_trainer_graph_replay_equals_eager(schedule):
    """use_graph=True captures kernel nodes only (_lib.capture_graph runs sol_graph_check and refuses anything else); the second replay
    equals the eager run bit for bit"""
    eager, gr = trainer_run(schedule=schedule), trainer_run(schedule=schedule, use_graph=True)
    assert gr[0] == eager[0] and torch.equal(gr[1], eager[1]) and torch.equal(gr[2], eager[2])
    assert all(torch.equal(a, b) for a, b in zip(gr[3], eager[3]))
    assert float(gr[2].abs().max()) > 0


def test_rollout_against_the_reference_rollout():
    """3 steps at 16 x 8 x 8, B = 2, s = 1, the golden small-weight network.  Bound: three steps, each within the one-step field bound"""
    import make_golden as mg
    name, s, steps = "16_comb", 1.0, 3
    d, v, re = mc.state(name)
    g = ds.geometry(name)
    params = mg.k3d_params()
    std_v, std_re = (0.2, 0.25, 0.3), o.STD_RE
    dr, vr = mc.rollout_reference(params, d, v, re, g, std_v, std_re, s, steps)
    net = k3.MarsMoon3D(device=DEV)
    net.set_weights([p.numpy() for p in params])
    ro = k3.Karman3DRollout(net, scene_of(ds.case(name)["shape"][1:]), d.shape[0], std_v, std_re, advection="mac_cormack", correction_strength=s)
    assert ro.sim.adv == s
    out = ro.run(f32(d), *[f32(t) for t in v], f32(re), steps)
    torch.cuda.synchronize()
    errs = [rel(a, b) for a, b in zip(out, (dr, *vr))]
    print("roll-out, %d steps: %s (bound %.1e)" % (steps, ["%.2e" % e for e in errs], steps * TOL_FIELD))
    assert max(errs) < steps * TOL_FIELD, errs


# ---- 5. the script ------------------------------------------------------------------------------------------------------------------------------
def test_karman3d_script_with_maccormack(tmp_path):
    """scripts/karman3d.py --advection mac_cormack --mc-strength 0.5 at -r 8: another flow than the default's, recorded with the run and
    with the model; a --model roll-out picks the scheme up and refuses a contradicting flag"""
    import importlib.util
    import pickle
    import sol_amd
    from sol_amd import scene as sc_io
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    sys.path.insert(0, sdir)
    spec = importlib.util.spec_from_file_location("sol_script_karman3d_mc", os.path.join(sdir, "karman3d.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    common = ["-r", "8", "-t", "6"]
    plain = mod.main(common + ["-o", str(tmp_path / "plain")])
    tr = mod.main(common + ["-o", str(tmp_path / "mc"), "--advection", "mac_cormack", "--mc-strength", "0.5", "--train-sol", "2", "--train-steps", "1"])
    a, b = (sc_io.read_zipped_array(p + "/velo_000005.npz") for p in (plain, tr))
    assert a.shape == b.shape == (1, 17, 9, 9, 3) and np.isfinite(b).all()
    assert np.abs(a - b).max() > 1e-4 * np.abs(b).max()
    rec = [pickle.load(open(p + "/params.pickle", "rb")) for p in (plain, tr)]
    assert [(r["advection"], r["correction_strength"]) for r in rec] == [("semi_lagrangian", 1.0), ("mac_cormack", 0.5)]
    model = tr + "/model3d.pt"
    blob = torch.load(model, map_location="cpu")
    assert (blob["advection"], blob["correction_strength"]) == ("mac_cormack", 0.5)
    ro = mod.main(common + ["-o", str(tmp_path / "ro"), "--model", model])
    r = pickle.load(open(ro + "/params.pickle", "rb"))
    assert (r["advection"], r["correction_strength"]) == ("mac_cormack", 0.5)
    assert np.isfinite(sc_io.read_zipped_array(ro + "/velo_000005.npz")).all()
    with pytest.raises(SystemExit, match="contradicts"):
        mod.main(common + ["--model", model, "--advection", "semi_lagrangian"])


# ---- 6. refusals that need a device ---------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_rejected_with_a_message_and_no_launch():
    shape = (20, 10, 10)
    sim = stage_sim(shape)
    lib, s = sim.lib, sim.scene
    d, cy, cx, cz, *w = stage_tensors(shape)
    out = [torch.full_like(t, 7.0) for t in (d, cy, cx, cz)]
    need = lib.sol_karman3d_advect_workspace_bytes(C.byref(sim.cfg), 1)
    ws = torch.zeros(need // 4, dtype=torch.float32, device=DEV)
    call = lambda ins, outs, a, st, wsp, n: lib.sol_karman3d_advect(C.byref(sim.cfg), stream(), *[ptr(t) for t in ins], ptr(s.active), ptr(s.inflow), a, st,
                                                                    *[ptr(t) for t in outs], ptr(wsp), n)
    err = lambda: lib.sol_last_error()
    ins = [d, cy, cx, cz]
    assert call(ins, out, 2, 1.0, ws, need) == -1 and b"advection must be 0" in err()
    assert call(ins, out, 1, 1.5, ws, need) == -1 and b"correction_strength must lie in [0, 1]" in err()
    assert call(ins, out, 0, -0.5, None, 0) == -1 and b"correction_strength must lie in [0, 1]" in err()
    assert call(ins, [d] + out[1:], 1, 1.0, ws, need) == -1 and b"alias" in err()
    assert call(ins, [out[0], out[1], out[1], out[3]], 1, 1.0, ws, need) == -1 and b"buffers of their own" in err()
    assert call(ins, out, 1, 1.0, None, 0) == -1 and b"needs a workspace" in err()
    assert call(ins, out, 1, 1.0, ws, need - 256) == -1 and b"workspace too small" in err()
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in out)              # nothing was launched
    assert call(ins, out, 1, 1.0, ws, need) == 0                 # ... and the good call runs
    torch.cuda.synchronize()
    check_fields(out, mc.stage_reference(shape)[0], "the good call")
    with pytest.raises(ValueError, match="are not"):
        k3.advect3d(sim, d, cx, cy, cz, 1.0)
    with pytest.raises(ValueError, match="cotangents must have the shapes"):
        k3.advect3d_bwd(sim, d, cy, cx, cz, w[0], w[2], w[1], w[3], adv=1.0)
    h = torch_ops.register_scene3d(sim)
    with pytest.raises(Exception, match="advection must be 0"):
        torch.ops.sol.karman3d_step_adv(d, cy, cx, cz, f32(torch.ones(mc.STAGE_B)), h, 3)
    with pytest.raises(Exception, match="correction_strength"):
        torch.ops.sol.karman3d_step_adv(d, cy, cx, cz, f32(torch.ones(mc.STAGE_B)), h, 1, 1.5)
    with pytest.raises(_lib.SolError, match="correction_strength must lie in"):
        sim._forward(k3.StepPhysics3D(), d, cy, cx, cz, f32(torch.ones(mc.STAGE_B)), adv=2.0)
