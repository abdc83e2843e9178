"""karman-3d direct pressure solve for obstacles extruded along z, Scene3D(pressure_solver="direct_extruded") (pytest -m gpu): the
solve alone on the cylinder of every cell of karman3d_shapes that the step takes (Z = 8, 9, 12, 32, 72 and 84; the GEMM, the LDS-fed
and the matrix-core transforms around it), against the dense direct solve, through the step and its adjoints, composed with every
opt-in of the step, and in the trainer, eager and captured.  The host side: tests/test_karman3d_extruded_cpu.py.

Tolerances are the suite's (karman3d_shapes): TOL_FIELD = 1e-5 relative L2 on fields and pressures, TOL_GRAD = 1e-4 on gradients in
the trimmed metric, CG_RTOL = 1e-7 for the CG solves this is compared with.  Bit comparisons are torch.equal.  The values measured on
an MI355X (printed by the tests) stand in the docstrings."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import sol_oracle3d as o
from sol_amd import _lib
from sol_amd import karman3d as k3
from sol_amd import precond3d as p3

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))        # make_golden.k3d_params: the golden network weights
import karman3d_shapes as ks
from karman3d_shapes import CG_RTOL, DEV, OBSTACLE, SEED, TOL_FIELD, TOL_GRAD, f32, rel, sid

pytestmark = pytest.mark.gpu
CG_MAX_ITER = 200


@functools.lru_cache(maxsize=None)
def scene(cell, solver="direct_extruded"):
    """Scene3D of the cell's cylinder on the oracle's masks; the blob's in-plane set is checked against the dense table before anything
    is launched"""
    g = ks.geometry(cell, "cylinder")
    sc = k3.Scene3D(*cell, device=DEV, active=g.active, inflow=g.inflow, pressure_solver=solver)
    assert sc.pressure_solver == solver
    if solver == "direct_extruded":
        magic, _, _, Z, nS2, SP2 = (int(v) for v in sc.direct_header[:6])
        assert magic == p3.FD3E_MAGIC and nS2 >= 1 and SP2 == (nS2 + 31) // 32 * 32
        if cell in ks.CELLS:                    # (the trainer's 16 x 8 x 8 is not a cell of the table)
            assert nS2 * Z == ks.BLOBS[(cell, "cylinder")][0]
    return g, sc


def flow(sc, B, **kw):
    if sc.pressure_solver == "cg":
        kw.setdefault("cg_rtol", CG_RTOL)
        kw.setdefault("cg_max_iter", CG_MAX_ITER)
    sim = k3.Karman3DFlow(sc, B, **kw)
    assert sim.cg == (sc.pressure_solver == "cg")
    return sim


class options:
    """process-wide kernel options for the block, restored to what they were"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: _lib.get_option(k) for k in self.kw}
        for k, v in self.kw.items():
            _lib.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            _lib.set_option(k, v)


def kernels_of(p):
    return {k.strip("()").replace(" ", "") for k in p.kernels}


EXTRUDED_KERNELS = {"k3e_gather_tz", "k3e_modes", "k3e_tz_apply"}


def dev_state(st):
    d, v, re = st
    return [f32(d), f32(v[0]), f32(v[1]), f32(v[2]), f32(re)]


def hip_grad(sim, st, w, wd=None, re_leaf=False):
    """one differentiable Karman3DFlow.step + backward of <v_out, w> (+ <d_out, wd>) -> (outputs, (g_d, g_vy, g_vx, g_vz, g_re), None where
    no gradient arrived)"""
    hs = dev_state(st)
    for t in hs[:4]:
        t.requires_grad_(True)
    hs[4].requires_grad_(re_leaf)
    out = sim.step(*hs)
    loss = sum((a * f32(b)).sum() for a, b in zip(out[1:], w))
    if wd is not None:
        loss = loss + (out[0] * f32(wd)).sum()
    loss.backward()
    torch.cuda.synchronize()
    return tuple(t.detach() for t in out), tuple(h.grad for h in hs)


# ---- (a) the solve alone ----------------------------------------------------------------------------------------------------------------
SOLVE_CELLS = [(16, 9, 9), (22, 10, 12), (128, 8, 8), (48, 24, 8), (24, 12, 72), (18, 10, 84), (32, 32, 32), (64, 64, 32)]


@functools.lru_cache(maxsize=None)
def solve_reference(cell):
    g = ks.geometry(cell, "cylinder")
    rhs = ks.step_like_rhs(2, cell) * torch.as_tensor(g.active)          # what the step's solve sees: no divergence inside the obstacle
    return rhs, ks.oracle_solve(rhs, g)


@pytest.mark.parametrize("cell", SOLVE_CELLS, ids=sid)
def test_extruded_solve_alone_against_the_oracle(cell):
    """sol_karman3d_pressure_solve on the cylinder against the float64 oracle's solve (sparse LU below LU_MAX_CELLS, else its PCG), B = 2,
    TOL_FIELD.  Z = 8, 9, 12, 72 and 84 are no multiple of the wave width and pass 64; 64 x 64 x 32 has the full-size in-plane set (nS2 =
    164, SP2 = 192), and its dense blob is the one that takes 23 s to build.  The three correction launches are asserted by name.
    Measured: 1.7e-7 ... 6.4e-7 (the largest at 32 x 32 x 32; 64 x 64 x 32: 4.5e-7, 4.6e-7)."""
    B = 2
    _, sc = scene(cell)
    rhs, ref = solve_reference(cell)
    sim = flow(sc, B)
    with _lib.profile() as prof:
        p = sim.pressure_solve(f32(rhs))
        torch.cuda.synchronize()
    ran = kernels_of(prof)
    assert EXTRUDED_KERNELS <= ran and not ran & {"k3_capacitance", "k3_cap_apply"}, ran
    assert sim.solve_info == {}
    e = [rel(p[b], ref[b]) for b in range(B)]
    print("extruded solve %s (nS2, SP2) = %s: %s" % (sid(cell), sc.direct_header[4:6].tolist(), ["%.3e" % v for v in e]))
    assert bool(torch.isfinite(p).all())
    assert max(e) < TOL_FIELD, e


def test_zero_right_hand_side_gives_exactly_zero():
    """B = 3 at 22 x 10 x 12, the middle right-hand side all zero: its pressure is exactly zero, the others within TOL_FIELD.
    Measured: step-like 2.1e-7, white 2.1e-7."""
    B, cell = 3, (22, 10, 12)
    g, sc = scene(cell)
    rhs = torch.stack([ks.step_like_rhs(1, cell)[0], torch.zeros(cell, dtype=torch.float64), ks.white_rhs(1, cell)[0]])
    ref = ks.oracle_solve(rhs, g)
    p = flow(sc, B).pressure_solve(f32(rhs))
    torch.cuda.synchronize()
    e = [rel(p[b], ref[b]) for b in (0, 2)]
    print("extruded solve, batch of three: step-like %.3e, white %.3e" % tuple(e))
    assert bool(torch.isfinite(p).all())
    assert not bool(p[1].any()), "the zero right-hand side's pressure is not exactly zero"
    assert max(e) < TOL_FIELD, e


@pytest.mark.parametrize("setting", ks.transform_settings(32, 32, 32), ids=lambda s: "mfma%d_fused%d" % s)
def test_extruded_solve_under_every_transform_setting(setting):
    """32 x 32 x 32: the correction between the matrix-core, the LDS-fed and the batched-GEMM forms of G (the result of G lies in another
    buffer under the GEMMs: the scratch follows it).
    Measured: 6.4e-7 / 3.5e-7 on the matrix-core and the LDS-fed transforms alike, 6.9e-7 / 3.4e-7 on the GEMMs."""
    B, cell = 2, (32, 32, 32)
    _, sc = scene(cell)
    rhs, ref = solve_reference(cell)
    sim = flow(sc, B)
    with options(k3d_mfma_tf=setting[0], k3d_fused_tf=setting[1]), _lib.profile() as prof:
        p = sim.pressure_solve(f32(rhs))
        torch.cuda.synchronize()
    path = "gemm" if not setting[1] else ("mfma" if setting[0] else "lds")
    want = {"mfma": {"k3_tzx_mfma<16,16>", "k3_ty_mfma<16>"}, "lds": {"k3_tzx", "k3_ty"}, "gemm": {"k_l_gemm", "k3_scale"}}[path]
    ran = kernels_of(prof)
    assert {k for k in ran if k.startswith(("k3_t", "k_l_gemm", "k3_scale"))} == want and EXTRUDED_KERNELS <= ran, ran
    e = [rel(p[b], ref[b]) for b in range(B)]
    print("extruded solve 32x32x32, %s transforms: %s" % (path, ["%.3e" % v for v in e]))
    assert max(e) < TOL_FIELD, e


def custom_geometry(cell, active):
    """a fresh oracle geometry of the cell with another mask: obstacle, active, the hard-BC face masks and the diagonal restated from it as
    Karman3DGeometry.__post_init__ does"""
    g = o.Karman3DGeometry(*cell)
    g.active = np.array(active, dtype=np.float64)
    g.obstacle = 1.0 - g.active
    acc = np.pad(g.active, 1, mode="edge")
    ms, nacc = [], np.zeros_like(g.active)
    for ax in range(3):
        lo, hi, dn, up = ([slice(1, -1)] * 3 for _ in range(4))
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        dn[ax], up[ax] = slice(0, -2), slice(2, None)
        ms.append(np.minimum(acc[tuple(lo)], acc[tuple(hi)]))
        nacc += acc[tuple(dn)] + acc[tuple(up)]
    g.masks = tuple(ms)
    g.diag = np.minimum(-nacc, -1.0)
    return g


def test_cylinder_with_a_prism_behind_it():
    """32 x 32 x 32, a second extruded scene built with extrude_mask: the cylinder and a box prism of 3 x 6 cells four cells behind it
    (nS2 = 88, SP2 = 96).  Measured: 5.3e-7, 5.7e-7."""
    B, cell = 2, (32, 32, 32)
    a2 = ks.geometry(cell, "cylinder").active[:, :, 0].copy()
    nS2_cyl = int(scene(cell)[1].direct_header[4])
    a2[24:27, 13:19] = 0.0
    active = k3.extrude_mask(a2, cell[2])
    g = custom_geometry(cell, active)
    sc = k3.Scene3D(*cell, device=DEV, active=active, inflow=g.inflow, pressure_solver="direct_extruded")
    assert sc.pressure_solver == "direct_extruded" and int(sc.direct_header[4]) == nS2_cyl + 3 * 6 + 2 * (3 + 6)
    rhs = ks.step_like_rhs(B, cell) * torch.as_tensor(active)
    ref = ks.oracle_solve(rhs, g)
    p = flow(sc, B).pressure_solve(f32(rhs))
    torch.cuda.synchronize()
    e = [rel(p[b], ref[b]) for b in range(B)]
    print("extruded solve 32x32x32, cylinder and prism (nS2, SP2) = %s: %s" % (sc.direct_header[4:6].tolist(), ["%.3e" % v for v in e]))
    assert max(e) < TOL_FIELD, e


# ---- (b) extruded against dense ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [(22, 10, 12), (48, 24, 8)], ids=sid)
def test_extruded_against_the_dense_direct_solve(cell):
    """the same cylinder through "direct" (the dense capacitance matrix) and "direct_extruded": relative L2 < TOL_FIELD on step-like and
    white right-hand sides.  Not bit-equal: the sums differ.
    Measured: 1.2e-7 / 2.0e-7 (22x10x12), 1.7e-7 / 2.4e-7 (48x24x8)."""
    B = 2
    rhs = torch.cat([ks.step_like_rhs(1, cell) * torch.as_tensor(ks.geometry(cell, "cylinder").active), ks.white_rhs(1, cell)])
    p = []
    for solver in ("direct", "direct_extruded"):
        _, sc = scene(cell, solver)
        p.append(flow(sc, B).pressure_solve(f32(rhs)).clone())
    torch.cuda.synchronize()
    e = [rel(p[1][b], p[0][b].double().cpu()) for b in range(B)]
    print("extruded against dense %s: step-like %.3e, white %.3e" % (sid(cell), *e))
    assert float(p[0].abs().max()) > 0 and max(e) < TOL_FIELD, e


# ---- (c) the step and its adjoints ------------------------------------------------------------------------------------------------------
STEP_CELLS = [c for c in ks.CELLS if OBSTACLE[c] == "cylinder"]


@functools.lru_cache(maxsize=None)
def oracle(cell):
    """test_gpu_karman3d_shapes.oracle on the cell's cylinder: B = 2, state seed 5, cotangent seed 3, the float64 oracle's first step with
    the gradient of <v_out, w>, and its second step"""
    g = ks.geometry(cell, "cylinder")
    st = ks.state(2, cell, SEED, g)
    w, _ = ks.cotangent(2, cell, g=g)
    out1, grad1 = ks.oracle_grad(st, g, w)
    with torch.no_grad():
        d2, v2 = o.karman3d_step(out1[0], out1[1:], st[2], g)
    return st, w, out1, grad1, (d2,) + tuple(v2)


def test_step_cells_are_the_shape_tests_cylinder_cells():
    assert STEP_CELLS == [(128, 8, 8), (48, 24, 8)]


@pytest.mark.parametrize("cell", STEP_CELLS, ids=sid)
def test_two_forward_steps_and_velocity_adjoint_against_the_oracle(cell):
    """the cases test_gpu_karman3d_shapes runs on the cylinder through the dense solve (128 x 8 x 8 and 48 x 24 x 8), on the extruded one:
    d, v_y, v_x, v_z after each of two steps at TOL_FIELD, the velocity adjoint in the trimmed metric at TOL_GRAD (the cap on the entries
    left out is asserted by check_grads).
    Measured: fields 4.7e-8 ... 6.6e-7 (v_z after the second step the largest), gradients 1.8e-7 ... 2.4e-7 trimmed and untrimmed alike."""
    B = 2
    st, w, out1, grad1, out2 = oracle(cell)
    _, sc = scene(cell)
    sim = flow(sc, B)
    h = dev_state(st)
    re = h[4]
    for k, ref in enumerate((out1, out2)):
        with torch.no_grad():
            h = sim.step(*h[:4], re)
            torch.cuda.synchronize()
        ks.check_fields(h, ref, "%s extruded step %d" % (sid(cell), k + 1))
    out, got = hip_grad(sim, st, w)
    assert got[0] is None and got[4] is None and sim.solve_info == {}
    ks.check_fields(out, out1, "%s extruded" % sid(cell))
    ks.check_grads(got[1:4], grad1[1:4], "%s extruded" % sid(cell))


def test_density_and_re_gradients_at_32x32x32():
    """Karman3DFlow(density_grad=True, re_grad=True) on the cylinder at 32 x 32 x 32 (matrix-core transforms), the drift state with the
    energy cotangents: fields at TOL_FIELD, g_d and the velocity gradients by check_grads.  g_re is held to TOL_GRAD as a relative L2 over
    the batch, as test_gpu_karman3d_shapes holds it at the drift state (no departure point near a cell boundary: karman3d_shapes.drift_state).
    Measured: fields 4.5e-8 ... 2.6e-7, g_d 4.7e-8, g_v 8.9e-8 ... 1.3e-7 untrimmed, g_re 6.7e-7."""
    B, cell = 2, (32, 32, 32)
    g, sc = scene(cell)
    st = ks.drift_state(B, cell, SEED, g)
    w, wd = ks.energy_cotangent(st, g)
    ref_out, ref_g = ks.oracle_grad(st, g, w, wd, re_grad=True)
    out, got = hip_grad(flow(sc, B, density_grad=True, re_grad=True), st, w, wd, re_leaf=True)
    ks.check_fields(out, ref_out, "32x32x32 extruded drift")
    ks.check_grads(got[:4], ref_g[:4], "32x32x32 extruded drift", names=("g_d", "g_vy", "g_vx", "g_vz"))
    e = rel(got[4], ref_g[4])
    print("32x32x32 extruded drift g_re: rel L2 over the batch %.3e (%s against %s)" % (e, got[4].tolist(), ref_g[4].tolist()))
    assert bool(torch.isfinite(got[4]).all()) and float(got[4].abs().min()) > 0
    assert e < TOL_GRAD, e


# ---- (d) composition with the opt-ins of the step ---------------------------------------------------------------------------------------
def test_every_opt_in_together_against_the_cg_solve():
    """22 x 10 x 12: buoyancy, diffusion_substeps = 2 and the MacCormack advection together (density_grad and re_grad on), one step and its
    adjoint on "direct_extruded" against the same step on "cg" at CG_RTOL: fields < TOL_FIELD, gradients by check_grads, g_re at TOL_GRAD.
    Measured: d bit-equal (it does not pass the solve), v 4.0e-8 ... 1.2e-7, g_d 4.8e-8, g_v 1.2e-7 ... 4.3e-7, g_re 6.7e-8."""
    B, cell = 2, (22, 10, 12)
    g = ks.geometry(cell, "cylinder")
    st = ks.drift_state(B, cell, SEED, g)
    w, wd = ks.energy_cotangent(st, g)
    kw = dict(density_grad=True, re_grad=True, buoyancy=(0.3, -0.1, 0.2), diffusion_substeps=2, advection="mac_cormack", correction_strength=1.0)
    res = {}
    for solver in ("cg", "direct_extruded"):
        sim = flow(scene(cell, solver)[1], B, **kw)
        assert sim.nsub == 2 and sim.adv == 1.0 and sim.buoyancy == (0.3, -0.1, 0.2)
        res[solver] = hip_grad(sim, st, w, wd, re_leaf=True)
        if solver == "cg":
            assert sim.solve_info["converged"].tolist() == [1] * B and sim.solve_info["converged_bwd"].tolist() == [1] * B
        else:
            assert sim.solve_info == {}
    (out_c, g_c), (out_e, g_e) = res["cg"], res["direct_extruded"]
    ks.check_fields(out_e, [t.double().cpu() for t in out_c], "22x10x12 composed, extruded against CG")
    ks.check_grads(g_e[:4], [t.double().cpu() for t in g_c[:4]], "22x10x12 composed, extruded against CG", names=("g_d", "g_vy", "g_vx", "g_vz"))
    e = rel(g_e[4], g_c[4].double().cpu())
    print("22x10x12 composed g_re: %.3e" % e)
    assert float(g_c[4].abs().min()) > 0 and e < TOL_GRAD, e


def test_torch_ops_take_the_extruded_scene():
    """torch.ops.sol.karman3d_step on a registered "direct_extruded" simulator gives the bits of Karman3DFlow.step, forward and backward"""
    from sol_amd import torch_ops
    B, cell = 2, (22, 10, 12)
    g, sc = scene(cell)
    st = ks.state(B, cell, SEED, g)
    w, _ = ks.cotangent(B, cell, g=g)
    sim = flow(sc, B)
    h = torch_ops.register_scene3d(sim)
    res = []
    for step in (lambda *a: torch.ops.sol.karman3d_step(*a, h), sim.step):
        hs = dev_state(st)
        for t in hs[:4]:
            t.requires_grad_(True)
        out = step(*hs)
        sum((a * f32(b)).sum() for a, b in zip(out[1:], w)).backward()
        torch.cuda.synchronize()
        res.append([t.detach() for t in out] + [t.grad for t in hs[1:4]])
    assert all(torch.equal(a, b) and float(a.abs().max()) > 0 for a, b in zip(*res))


# ---- (e) trainer and roll-out -----------------------------------------------------------------------------------------------------------
TRAINER_SHAPE = (2, 16, 8, 8)
STD_V = (0.2, 0.25, 0.3)


@functools.lru_cache(maxsize=None)
def trainer_problem(ms=2):
    import make_golden as mg
    B, Y, X, Z = TRAINER_SHAPE
    d, v = o.synthetic_state(B, Y, X, Z, 77)
    gts = [tuple(c.float().double() for c in o.synthetic_state(B, Y, X, Z, 500 + i)[1]) for i in range(ms)]
    return {"d": d.float().double(), "v": tuple(c.float().double() for c in v), "re": torch.tensor(o.RE_TRAIN[:B], dtype=torch.float64),
            "gts": gts, "params": [p.clone() for p in mg.k3d_params()]}


def trainer_run(solver, use_graph=False):
    """one fwd_bwd of a fresh SOL-2 Karman3DTrainer on the cylinder at 16 x 8 x 8 (use_graph: a second call, the pure replay) -> (loss,
    per-step losses, gradient, final state)"""
    p = trainer_problem()
    B, Y, X, Z = TRAINER_SHAPE
    net = k3.MarsMoon3D(device=DEV)
    net.set_weights([q.detach().numpy() for q in p["params"]])
    tr = k3.Karman3DTrainer(net, scene((Y, X, Z), solver)[1], B, 2, STD_V, o.STD_RE, use_graph=use_graph)
    assert tr.sim.cg is False and tr.sim.scene.pressure_solver == solver
    for _ in range(2 if use_graph else 1):
        tr._grads.zero_()
        loss = tr.fwd_bwd(p["d"], *p["v"], p["re"], p["gts"])
    torch.cuda.synchronize()
    assert (tr._graph is not None) == use_graph          # _lib.capture_graph ran sol_graph_check: kernel nodes only
    return float(loss), tr.loss_steps.clone(), tr.grads.clone(), [t.clone() for t in tr.final]


def test_trainer_sol2_on_the_cylinder():
    """SOL-2 at 16 x 8 x 8, B = 2: loss and gradient on "direct_extruded" against the same trainer on "direct" (loss relative < 1e-5,
    gradient < TOL_GRAD); the captured replay equals eager bit for bit (and passed sol_graph_check when it was captured); two runs are
    bit-identical.
    Measured: the float32 loss is the dense trainer's to the last bit, gradient 9.1e-8; every bit comparison equal."""
    dense = trainer_run("direct")
    eager = trainer_run("direct_extruded")
    el, eg = abs(eager[0] - dense[0]) / abs(dense[0]), rel(eager[2], dense[2].double().cpu())
    print("trainer on the cylinder, extruded against dense: loss %.9e against %.9e (%.2e), gradient %.2e" % (eager[0], dense[0], el, eg))
    assert float(dense[2].abs().max()) > 0 and np.isfinite(eager[0])
    assert el < 1e-5 and eg < TOL_GRAD
    again = trainer_run("direct_extruded")
    graph = trainer_run("direct_extruded", use_graph=True)
    for what, other in (("a second run", again), ("the captured replay", graph)):
        assert other[0] == eager[0] and torch.equal(other[1], eager[1]) and torch.equal(other[2], eager[2]), what
        assert all(torch.equal(a, b) for a, b in zip(other[3], eager[3])), what


def test_rollout_on_the_cylinder():
    """Karman3DRollout, 3 steps at 16 x 8 x 8 on "direct_extruded" against "direct": three steps, each within the one-step field bound.
    Measured: d 2.0e-8, v_y 4.6e-8, v_x 1.9e-7, v_z 3.6e-7."""
    p = trainer_problem()
    B, Y, X, Z = TRAINER_SHAPE
    out = []
    for solver in ("direct", "direct_extruded"):
        net = k3.MarsMoon3D(device=DEV)
        net.set_weights([q.detach().numpy() for q in p["params"]])
        ro = k3.Karman3DRollout(net, scene((Y, X, Z), solver)[1], B, STD_V, o.STD_RE)
        out.append([t.clone() for t in ro.run(f32(p["d"]), *[f32(t) for t in p["v"]], f32(p["re"]), 3)])
    torch.cuda.synchronize()
    errs = [rel(a, b.double().cpu()) for a, b in zip(out[1], out[0])]
    print("roll-out on the cylinder, 3 steps, extruded against dense: %s" % ["%.2e" % e for e in errs])
    assert max(errs) < 3 * TOL_FIELD, errs


# ---- (f) refusal ------------------------------------------------------------------------------------------------------------------------
def test_the_sphere_is_refused_at_construction():
    cell = (22, 10, 12)
    g = ks.geometry(cell, "sphere")
    with pytest.raises(ValueError, match="direct_extruded.*depends on z"):
        k3.Scene3D(*cell, device=DEV, active=g.active, inflow=g.inflow, pressure_solver="direct_extruded")
    with pytest.raises(ValueError, match="no obstacle"):
        k3.Scene3D(*cell, device=DEV, active=np.ones(cell), inflow=g.inflow, pressure_solver="direct_extruded")
    with pytest.raises(ValueError, match="pressure_solver must be one of"):
        k3.Scene3D(*cell, device=DEV, active=g.active, inflow=g.inflow, pressure_solver="direct_scattered")


# ---- (g) the script ---------------------------------------------------------------------------------------------------------------------
def test_karman3d_script_on_the_cylinder(tmp_path):
    """scripts/karman3d.py --obstacle cylinder --pressure-solver direct_extruded at -r 8: generates data, trains (SOL-2, captured) and rolls
    the model out; the obstacle is recorded with the run and with the model, and a --model roll-out picks it up"""
    import importlib.util
    import pickle
    import sol_amd
    from sol_amd import scene as sc_io
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    sys.path.insert(0, sdir)
    spec = importlib.util.spec_from_file_location("sol_script_karman3d_ext", os.path.join(sdir, "karman3d.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    common = ["-r", "8", "-t", "6"]
    ext = ["--obstacle", "cylinder", "--pressure-solver", "direct_extruded"]
    sphere = mod.main(common + ["-o", str(tmp_path / "sphere")])
    tr = mod.main(common + ext + ["-o", str(tmp_path / "cyl"), "--train-sol", "2", "--train-steps", "1"])
    dense = mod.main(common + ["--obstacle", "cylinder", "--pressure-solver", "direct", "-o", str(tmp_path / "dense")])
    a, b, c = (sc_io.read_zipped_array(p + "/velo_000005.npz") for p in (sphere, tr, dense))
    assert a.shape == b.shape == (1, 17, 9, 9, 3) and np.isfinite(b).all()
    assert np.abs(a - b).max() > 1e-4 * np.abs(b).max()                                  # another scene than the sphere's
    assert np.linalg.norm(b - c) < 5 * TOL_FIELD * np.linalg.norm(c)                     # the dense solve's flow: five steps
    rec = [pickle.load(open(p + "/params.pickle", "rb")) for p in (sphere, tr)]
    assert [(r["obstacle"], r["pressure_solver"]) for r in rec] == [("sphere", "auto"), ("cylinder", "direct_extruded")]
    assert "pressure solver: direct_extruded" in open(tr + "/run.log").read()
    model = tr + "/model3d.pt"
    assert torch.load(model, map_location="cpu")["obstacle"] == "cylinder"
    ro = mod.main(common + ["-o", str(tmp_path / "ro"), "--model", model, "--pressure-solver", "direct_extruded"])
    assert pickle.load(open(ro + "/params.pickle", "rb"))["obstacle"] == "cylinder"
    assert np.isfinite(sc_io.read_zipped_array(ro + "/velo_000005.npz")).all()
    with pytest.raises(SystemExit, match="contradicts"):
        mod.main(common + ["--model", model, "--obstacle", "sphere"])
