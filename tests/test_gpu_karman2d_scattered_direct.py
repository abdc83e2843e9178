"""The scattered direct pressure solve of the large-grid karman-2d path on the GPU (pytest -m gpu):
SceneMasks(pressure_solver="direct_scattered") on the scenes the one-window blob refuses (two cylinders in tandem, a plate across the
channel): the solve alone against a sparse LU, the step and its adjoint against the float64 oracle and against the CG path, bit
reproducibility (eager, captured, a workspace full of NaN), LargeGridTrainer and LargeGridRollout captured, and the refusals.

Tolerances are the suite's (large2d_scenes): TOL_FIELD = 1e-5 relative L2 on fields, TOL_GRAD = 1e-4 on gradients (trimmed on the
two-cylinder scene exactly as test_gpu_karman2d_large_adjoint.py does for the CG form: at most 0.1 % of the entries of a component
left out, the count printed), CG_RTOL = 1e-7 for the CG solves compared against.  One oracle computation per scene is shared."""
import functools
import os
import sys

import numpy as np
import pytest
import scipy.sparse.linalg as spla
import torch

import sol_amd
import sol_oracle as o
from sol_amd import _lib, ops, precond

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from large2d_scenes import CG_RTOL, DEV, PLATE, TOL_FIELD, TOL_GRAD, TWO, active_of, f32, geometry, masks, rel, state
from test_gpu_karman2d_large_adjoint import check_grads, cotangent, hip_grad, oracle_grad

pytestmark = pytest.mark.gpu
Y, X = 256, 128
SC = "direct_scattered"
SCENES = {"two_cylinders": TWO, "plate": PLATE}


@functools.lru_cache(maxsize=None)
def scene(name):
    return geometry(Y, X, active_of(SCENES[name], Y, X))


@functools.lru_cache(maxsize=None)
def oracle(name):
    """B = 2, state seed 11 (the seed of the CG tests of these scenes): the state, the cotangent, the oracle's first step with the
    gradient of <out, w>, and its second step"""
    g = scene(name)
    st = state(2, Y, X, 11, g)
    w = cotangent(2)
    out1, grad1 = oracle_grad(st, g, w)
    with torch.no_grad():
        out2 = o.karman_step(*out1, st[3], g)
    return st, w, out1, grad1, tuple(t.detach() for t in out2)


def two_boxes_144x72():
    a = np.ones((144, 72))
    a[20:27, 11:20] = 0.0              # support rows 19..27 and 49..61 (22), columns 10..20 and 39..53 (26): neither a multiple of 4
    a[50:61, 40:53] = 0.0
    return a


# ---- 1. the option is accepted ------------------------------------------------------------------------------------------------
def test_scene_masks_accept_direct_scattered():
    mk = masks(scene("two_cylinders"), SC)
    assert mk.pressure_solver == SC and mk.large and mk.direct is not None and mk.box is None
    assert int(mk.direct_header[0]) == precond.FDS_MAGIC and tuple(mk.direct_header[3:6]) == (55, 28, 1188)
    # the existing choices choose what they chose
    assert masks(scene("two_cylinders"), "auto").pressure_solver == "cg"
    m_def = masks(o.KarmanGeometry(Y, X), "auto")
    assert m_def.pressure_solver == "direct" and int(m_def.direct_header[0]) == precond.FD_MAGIC


# ---- 2. the solve alone against a sparse LU -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["two_cylinders_256x128", "two_boxes_144x72"])
def test_pressure_solve_alone_against_sparse_lu(case):
    B = 2
    if case == "two_cylinders_256x128":
        Yc, Xc, g = Y, X, scene("two_cylinders")
    else:
        Yc, Xc = 144, 72
        g = geometry(Yc, Xc, two_boxes_144x72())
        # (the one-window path takes this grid for the default sphere: the scattered path is compared on equal ground)
        assert precond.direct_solver_blob(o.KarmanGeometry(Yc, Xc).active, max_window=64) is not None
    mk = masks(g, SC)
    hdr = mk.direct_header
    if case != "two_cylinders_256x128":
        assert (int(hdr[3]), int(hdr[4])) == (22, 26) and (int(hdr[7]), int(hdr[8])) == (24, 28)
    _, vy, vx, _ = state(B, Yc, Xc, 4)                  # the right-hand side the step sees: -div of an unprojected field
    rhs = (-((vy[:, 1:] - vy[:, :-1]) + (vx[:, :, 1:] - vx[:, :, :-1]))).float().double()
    lu = spla.splu((-g.pressure_matrix()).tocsc())
    ref = np.stack([lu.solve(r.numpy().ravel()).reshape(Yc, Xc) for r in rhs])
    info = {}
    p = ops.pressure_solve_large(f32(rhs), ops.karman_cfg(B, Yc, Xc, g.dx, masks=mk), mk, info=info)
    torch.cuda.synchronize()
    e = rel(p, ref)
    print("scattered solve alone, %s: %.3e against sparse LU" % (case, e))
    assert info == {}                                   # no iteration, nothing to report
    assert e < TOL_FIELD, e


# ---- 3. two steps against the oracle and against the CG path -------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_two_steps_against_the_oracle_and_the_cg_path(name):
    B = 2
    g = scene(name)
    active = g.active
    st, _, out1, _, out2 = oracle(name)
    mk, m_cg = masks(g, SC), masks(g, "cg")
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk)
    c_cg = ops.karman_cfg(B, Y, X, g.dx, masks=m_cg, cg_rtol=CG_RTOL)
    hd, hy, hx = f32(st[0]), f32(st[1]), f32(st[2])
    cd, cy, cx = hd, hy, hx
    re = f32(st[3])
    for k, ref in enumerate((out1, out2)):
        info, i_cg = {}, {}
        with torch.no_grad():
            hd, hy, hx = ops.karman_step_large(hd, hy, hx, re, cfg, mk, info=info)
            cd, cy, cx = ops.karman_step_large(cd, cy, cx, re, c_cg, m_cg, info=i_cg)
        assert info == {} and i_cg["converged"].tolist() == [1] * B
        errs = [rel(a, b) for a, b in zip((hd, hy, hx), ref)]
        e_cg = [rel(a, b) for a, b in zip((hd, hy, hx), (cd, cy, cx))]
        print("%s step %d: against the oracle %s, against the CG path %s" % (name, k + 1, errs, e_cg))
        assert max(errs) < TOL_FIELD, errs
        assert max(e_cg) < TOL_FIELD, e_cg
        # interior cells (the box faces keep their boundary values: grad p is zero there with replicate padding)
        div = ((hy[:, 1:] - hy[:, :-1]) + (hx[:, :, 1:] - hx[:, :, :-1])).double().cpu().numpy()[:, 1:-1, 1:-1]
        inner = active[1:-1, 1:-1] != 0
        assert np.abs(div[:, inner]).max() < 1e-4 * float(hy.abs().max()), np.abs(div[:, inner]).max()


# ---- 4. the adjoint against the oracle's autograd ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,trimmed", [("plate", False), ("two_cylinders", True)])
def test_adjoint_against_the_oracle(name, trimmed):
    B = 2
    g = scene(name)
    st, w, out1, grad1, _ = oracle(name)
    mk = masks(g, SC)
    info = {}
    out, got = hip_grad(st, g, mk, w, info)
    assert info == {}
    for a, b in zip(out, out1):
        assert rel(a, b) < TOL_FIELD, rel(a, b)
    check_grads(got, grad1, trimmed, "direct_scattered %s seed 11" % name)


# ---- 5. bit reproducibility ---------------------------------------------------------------------------------------------------
def test_step_and_adjoint_are_bit_reproducible_eager_captured_and_on_a_dirty_workspace():
    B = 2
    g = scene("two_cylinders")
    mk = masks(g, SC)
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk)
    d, vy, vx, re = (f32(t) for t in state(B, Y, X, 7))
    w = [f32(t) for t in cotangent(B)]
    ws = torch.zeros((ops.large_workspace_bytes(cfg, mk) + 3) // 4, dtype=torch.float32, device=DEV)
    wb = torch.zeros((ops.large_bwd_workspace_bytes(cfg, mk) + 3) // 4, dtype=torch.float32, device=DEV)
    with torch.no_grad():
        (_, sy, sx), svy, svx = ops.karman_step_large_saved(d, vy, vx, re, cfg, mk, ws)

    def both():
        with torch.no_grad():
            out = ops.karman_step_large(d, vy, vx, re, cfg, mk, ws)
        return list(out) + list(ops.karman_step_large_bwd(svy, svx, re, w[0], w[1], cfg, mk, workspace=wb))

    first = [t.clone() for t in both()]
    assert all(bool(torch.isfinite(t).all()) for t in first) and float(first[3].abs().max()) > 0
    assert torch.equal(first[1], sy) and torch.equal(first[2], sx)                # the differentiable form: the same launches
    # a second call on the same workspaces, then on workspaces full of NaN: W2 is cleared by every call, nothing else is read before written
    for fill in (None, float("nan")):
        if fill is not None:
            ws.fill_(fill); wb.fill_(fill)
        for a, b in zip(both(), first):
            assert torch.equal(a, b), "second call differs (workspace %s)" % ("reused" if fill is None else "filled with NaN")
    # captured: kernel nodes only, the same bits at every replay
    cap = {}
    torch.cuda.synchronize()
    graph = _lib.capture_graph(lambda: cap.__setitem__("o", both()), "large-grid step + adjoint (direct_scattered)")
    for _ in range(2):
        for t in cap["o"]:
            t.zero_()
        ws.fill_(float("nan")); wb.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(cap["o"], first):
            assert torch.equal(a, b), "replay differs from eager"


# ---- 6. LargeGridTrainer, captured ---------------------------------------------------------------------------------------------
def test_large_grid_trainer_captured_against_the_oracle_and_the_cg_trainer():
    from test_gpu_karman2d_large_trainer import SEED, STD_V, batch, net_of, oracle_loss_grad, problem
    from sol_amd import karman
    g = scene("two_cylinders")
    p = problem(SEED, B=1, ms=2, g=g)
    lref, gref = oracle_loss_grad(p)
    kw = dict(obstacles=karman.parse_obstacles(TWO))
    tr = sol_amd.LargeGridTrainer(net_of(p), 1, Y, X, 2, STD_V, o.STD_RE, pressure_solver=SC, **kw)
    args = batch(p)
    loss = float(tr.fwd_bwd(*args))
    g1 = tr.grads.clone()
    assert tr.pressure_solver_used == SC and tr._graph is not None and tr.solve_info == {}
    assert float(tr.fwd_bwd(*args)) == loss and torch.equal(tr.grads, g1)          # a replay: the same bits
    e_l, e_g = abs(loss - lref) / abs(lref), rel(g1, gref)
    tc = sol_amd.LargeGridTrainer(net_of(p), 1, Y, X, 2, STD_V, o.STD_RE, pressure_solver="cg", cg_rtol=CG_RTOL, cg_max_iter=600,
                                  use_graph=False, **kw)
    lc = float(tc.fwd_bwd(*args))
    assert tc.pressure_solver_used == "cg" and bool(tc.solve_info["converged"].all()) and bool(tc.solve_info["converged_bwd"].all())
    c_l, c_g = abs(loss - lc) / abs(lc), rel(g1, tc.grads)
    print("LargeGridTrainer direct_scattered (captured): vs float64 oracle loss %.3e gradient %.3e; vs the CG trainer loss %.3e gradient %.3e"
          % (e_l, e_g, c_l, c_g))
    assert e_l < 1e-5 and e_g < TOL_GRAD, (e_l, e_g)
    assert c_l < 1e-5 and c_g < TOL_GRAD, (c_l, c_g)
    # the factory takes the option as well
    t2 = sol_amd.make_trainer(net_of(p), None, 1, Y, X, 2, 100.0 / X, STD_V, o.STD_RE, pressure_solver=SC, use_graph=False, **kw)
    assert isinstance(t2, sol_amd.LargeGridTrainer) and t2.sim._pressure_solver == SC


# ---- 7. LargeGridRollout, captured ---------------------------------------------------------------------------------------------
def test_captured_rollout_equals_eager_bit_for_bit_and_agrees_with_the_cg_rollout():
    from test_gpu_karman2d_large_rollout import STD_V, net_of
    g = scene("two_cylinders")
    st = state(1, Y, X, 11, g)
    params = o.init_params(3)
    mk = masks(g, SC)
    mkro = lambda m, **kw: sol_amd.make_rollout(net_of(params), m, 1, Y, X, g.dx, STD_V, o.STD_RE, **kw)
    rg, re_, rc = mkro(mk, use_graph=True), mkro(mk, use_graph=False), mkro(masks(g, "cg"), use_graph=False, cg_rtol=CG_RTOL)
    assert isinstance(rg, sol_amd.LargeGridRollout) and rg.pressure_solver_used == SC
    runs = []
    for ro in (rg, re_, rc):
        h = tuple(f32(t) for t in st)
        its = ro.run(*h, 3)
        runs.append(h[:3])
        assert its.shape == (3, 1) and (bool(its.all()) if ro is rc else not its.any())
    assert rg._graph is not None and re_._graph is None and rg.solve_info == {}
    for a, b, c in zip(*runs):
        assert torch.equal(a, b), "captured differs from eager"
        assert rel(a, c) < TOL_FIELD, rel(a, c)
    # cg_warm_start has nothing to start here: ignored, as with "direct"
    assert mkro(mk, use_graph=False, cg_warm_start=True).p_guess is None


# ---- 8. the one-window path is the parent's ------------------------------------------------------------------------------------
def test_default_sphere_direct_step_is_untouched_by_the_dispatch():
    """"direct" and "auto" on the default sphere run the one-window blob (magic FD02) through the same entry points, bit for bit equal to each
    other and to a workspace sized the old way; the comparison against a build of the parent commit is tools/lib_bitcompare.py's."""
    B = 1
    g = o.KarmanGeometry(Y, X)
    m_dir, m_auto = masks(g, "direct"), masks(g, "auto")
    assert int(m_dir.direct_header[0]) == precond.FD_MAGIC and m_dir.pressure_solver == m_auto.pressure_solver == "direct"
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=m_dir)
    import ctypes as C
    lib = sol_amd.load()
    assert ops.large_workspace_bytes(cfg, m_dir) == lib.sol_karman_step_large_workspace_bytes(C.byref(cfg))
    assert ops.large_bwd_workspace_bytes(cfg, m_dir) == lib.sol_karman_step_bwd_large_workspace_bytes(C.byref(cfg))
    # the spun-up state of test_default_scene_cg_matches_direct_and_direct_is_unchanged, where the CG path is held to the same bound (on
    # raw unprojected noise, whose pressure is ten times a flow's, the two fp32 solves measured 1.03e-5 apart in v_x: not a state a step sees)
    d, vy, vx, re = (f32(t) for t in state(B, Y, X, 5, g))
    with torch.no_grad():
        a = ops.karman_step_large(d, vy, vx, re, cfg, m_dir)
        b = ops.karman_step_large(d, vy, vx, re, ops.karman_cfg(B, Y, X, g.dx, masks=m_auto), m_auto)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # where both blobs build, the scattered solve agrees with the one-window solve to fp32 round-off
    m_sc = masks(g, SC)
    with torch.no_grad():
        c = ops.karman_step_large(d, vy, vx, re, ops.karman_cfg(B, Y, X, g.dx, masks=m_sc), m_sc)
    errs = [rel(x, y) for x, y in zip(c, a)]
    print("default sphere, direct_scattered against direct:", errs)
    assert max(errs) < TOL_FIELD, errs


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------
def test_refused_loudly_where_it_does_not_apply(monkeypatch):
    gs = o.geometry(64, 32)
    with pytest.raises(ValueError, match="large-grid path only"):
        ops.SceneMasks(gs.active, gs.inflow, gs.bc_mask, gs.bc_mask, DEV, pressure_solver=SC)
    g = o.KarmanGeometry(Y, X)
    with pytest.raises(ValueError, match="does not support this scene"):
        ops.SceneMasks(np.ones((Y, X)), g.inflow, g.bc_mask, g.bc_mask, DEV, pressure_solver=SC)          # no obstacle: nothing to correct
    monkeypatch.setenv("SOL_PRESSURE_SOLVER", SC)                                                        # the environment spelling
    assert masks(scene("plate"), "auto").pressure_solver == SC
    monkeypatch.delenv("SOL_PRESSURE_SOLVER")
    mk = masks(scene("plate"), SC)
    with pytest.raises(ValueError, match="p_guess"):
        cfg = ops.karman_cfg(1, Y, X, g.dx, masks=mk)
        z = lambda *s: torch.zeros(*s, device=DEV)
        with torch.no_grad():
            ops.karman_step_large(z(1, Y, X), z(1, Y + 1, X), z(1, Y, X + 1), torch.ones(1, device=DEV), cfg, mk, p_guess=z(1, Y, X))
