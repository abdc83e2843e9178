"""The large-grid karman-2d path at ragged shapes, every direct-solve window, in a batch and across cotangent scales (pytest -m gpu).

The rest of the GPU suite runs this path at 256 x 128 (multiples of 16 and 64, one 32-cell window away from the edges, max |u| dt/dx
of about 1.3, cotangents of magnitude 1).  Here: 130 x 65, 144 x 72 and 160 x 80 on the scene table of large2d_scenes (windows 16 / 32 / 64, windows
clamped to the domain edge, the scattered blob and the CG solve where the one-window blob refuses), partial adjoint tiles with the
extra face row / column, back-traces of six cells (beyond the LDS halo of 4, clamped at the domain edge), one-hot cotangents, a batch
whose middle simulation is all zero, and cotangents scaled by 2^-40 ... 2^40.  test_karman2d_large_shapes_cpu.py pins the table.

Tolerances are the suite's (large2d_scenes): TOL_FIELD = 1e-5 relative L2 on fields and pressures, TOL_GRAD = 1e-4 on gradients in
the trimmed metric (at most floor(1e-3 n) entries of a component left out: the step's gradient is discontinuous where a departure
point crosses a cell boundary, test_gpu_karman2d_large_adjoint.py), CG_RTOL = 1e-7 for the CG solves.  Bit comparisons are torch.equal.

Measured with the float64 oracle ALONE (the same oracle in float32 against float64, B = 2, cotangent seed 3), next to the bound:
  adjoint, trimmed (TOL_GRAD = 1e-4; required <= TOL_GRAD / 5 = 2e-5), state seed 11 (seeds 5 and 7 within 3 % of these):
    130 x 65   default 6.7e-6 / 7.1e-6 (g_vy / g_vx, 17 entries left out of 8515 / 8580), corner 6.5e-6 / 6.8e-6, two 6.7e-6 / 6.9e-6
    144 x 72   default 6.9e-6 / 7.4e-6 (20 / 21 left out), corner 6.6e-6 / 7.3e-6, two 6.9e-6 / 7.5e-6
    untrimmed the same cases reach 9.6e-5 (130 x 65 default) and 3.7e-5 (144 x 72 two): no margin, hence the trimmed metric
  one-hot cotangents at 130 x 65 default (ONE_HOT below; trimmed / untrimmed):
    (a) v_y[0, 0]       the reference gradient is exactly zero (the face and all it samples are prescribed by the inflow condition)
    (b) v_y[Y, X-1]     12 non-zero entries: trimmed 0 (all of them fit into the 17 left out), untrimmed 1.4e-4 / 3.1e-6
    (c) v_x[Y-1, X]     13 non-zero entries: trimmed 0, untrimmed 0 / 1.2e-5
    (d) v_x[32, 25]     beside the obstacle, dense through the pressure solve: trimmed 1.2e-6 / 7.6e-7, untrimmed 2.3e-6 / 1.9e-6
    The trimmed metric cannot see a gradient of a dozen entries, so (a)-(c) ALSO assert the untrimmed metric against
    ONE_HOT_UNTRIMMED = 1.4e-3, ten times the largest oracle-alone value above (a kernel that drops the face loses all of it: 1.0),
    and (a) that the gradient is exactly zero.
  forward step at the scaled state of test 5 (TOL_FIELD = 1e-5; required <= TOL_FIELD / 5 = 2e-6), max |u| dt/dx = 6.000 reached
  at every case, so the scale was not lowered:
    130 x 65   default 1.4e-6 / 2.0e-7 / 1.0e-6 (d / v_y / v_x), two 1.3e-6 / 2.5e-7 / 9.7e-7
    144 x 72   default 1.7e-6 / 2.2e-7 / 1.2e-6, two 1.7e-6 / 2.4e-7 / 1.2e-6
    (the density figure is that of the unscaled state, 1.4e-6 / 1.8e-6: uniform noise, not a smooth field)
The values measured on an MI355X (printed by the tests) stand in the docstrings of the tests.  There the HIP gradients lie closer to
the float64 oracle (3e-7 ... 9e-7) than the float32 oracle does (7e-6): the oracle forms its departure points from physical coordinates."""
import ctypes as C
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
from large2d_scenes import (CG_RTOL, DEV, SHAPES, TOL_FIELD, TOL_GRAD, WINDOWS, cfl_scaled, check_grads, cotangent_at, f32, masks, rel,
                            state, step_like_rhs, table_geometry)

pytestmark = pytest.mark.gpu
SC = "direct_scattered"
SEED = 11                           # state seed (module docstring: oracle-alone values)
CFL_TARGET = 6.0                    # max |u| dt/dx of the scaled state: beyond the adjoint tile's halo of 4 faces
ONE_HOT_UNTRIMMED = 1.4e-3          # module docstring


def sid(Y, X):
    return "%dx%d" % (Y, X)


@functools.lru_cache(maxsize=None)
def scene_masks(name, Y, X, solver="auto"):
    """SceneMasks of a table cell; for the one-window blob the header is checked against the table BEFORE anything is launched: the
    case reaches the window edge (hdr[7]) and the origin (hdr[3], hdr[4]) it is listed for"""
    mk = masks(table_geometry(name, Y, X), solver)
    assert mk.large
    want = WINDOWS[(name, Y)]
    if solver in ("auto", "direct"):
        if want is None:
            assert solver == "auto" and mk.pressure_solver == "cg" and mk.direct is None
        else:
            hdr = mk.direct_header
            assert mk.pressure_solver == "direct" and int(hdr[0]) == precond.FD_MAGIC
            assert (int(hdr[7]), int(hdr[3]), int(hdr[4])) == (want[4], want[0], want[1]), (name, Y, X, hdr[:8].tolist())
    elif solver == SC:
        assert mk.pressure_solver == SC and int(mk.direct_header[0]) == precond.FDS_MAGIC
    else:
        assert mk.pressure_solver == "cg" and mk.direct is None and mk.box is not None
    return mk


def cfg_of(B, name, Y, X, mk, **kw):
    if mk.pressure_solver == "cg":
        kw.setdefault("cg_rtol", CG_RTOL)
    return ops.karman_cfg(B, Y, X, table_geometry(name, Y, X).dx, masks=mk, **kw)


@functools.lru_cache(maxsize=None)
def oracle(name, Y, X, grad_pad="replicate"):
    """B = 2, state seed 11, cotangent seed 3: the state, the cotangent, the float64 oracle's first step with the gradient of <out, w>,
    and its second step (one computation per scene, shape and padding, shared and left unchanged)"""
    g = table_geometry(name, Y, X)
    st = state(2, Y, X, SEED, g)
    w = cotangent_at(2, Y, X)
    out1, grad1 = oracle_grad(st, g, w, grad_pad=grad_pad)
    with torch.no_grad():
        out2 = o.karman_step(*out1, st[3], g, grad_pad=grad_pad)
    return st, w, out1, grad1, tuple(t.detach() for t in out2)


def oracle_grad(st, g, w, **kw):
    d, vy, vx, re = st
    ry, rx = vy.clone().requires_grad_(True), vx.clone().requires_grad_(True)
    out = o.karman_step(d, ry, rx, re, g, **kw)
    ((out[1] * w[0]).sum() + (out[2] * w[1]).sum()).backward()
    return tuple(t.detach() for t in out), (ry.grad, rx.grad)


def hip_grad(st, cfg, mk, w, info=None):
    """one differentiable ops.karman_step_large + backward of sum <out, w> -> (outputs, (g_vy, g_vx), (saved v_y, saved v_x))"""
    d, vy, vx, re = st
    hy, hx = f32(vy).requires_grad_(True), f32(vx).requires_grad_(True)
    out = ops.karman_step_large(f32(d), hy, hx, f32(re), cfg, mk, info=info)
    assert out[1].requires_grad and out[2].requires_grad and not out[0].requires_grad
    saved = out[1].grad_fn.saved_tensors[:2]
    ((out[1] * f32(w[0])).sum() + (out[2] * f32(w[1])).sum()).backward()
    torch.cuda.synchronize()
    return tuple(t.detach() for t in out), (hy.grad, hx.grad), saved


def converged(info, B, keys=("converged", "converged_bwd")):
    for k in keys:
        assert info[k].tolist() == [1] * B, (k, info)


# ---- 1. the pressure solve alone against a sparse LU --------------------------------------------------------------------------
SOLVES = ([(name, Y, X, "direct") for Y, X in SHAPES for name in ("default", "small", "big", "corner", "top_edge", "two")
           if WINDOWS[(name, Y)] is not None]
          + [(name, Y, X, SC) for Y, X in SHAPES for name in ("big", "corner", "two")]
          + [("two", 130, 65, "cg"), ("two", 160, 80, "cg")])


@pytest.mark.parametrize("name,Y,X,solver", SOLVES, ids=["%s_%s_%s" % (c[0], sid(c[1], c[2]), c[3]) for c in SOLVES])
def test_pressure_solve_alone_against_sparse_lu(name, Y, X, solver):
    """sol_karman_pressure_solve_large_direct on the one-window blob (windows 16 / 32 / 64, clamped windows, GEMM extents that are no
    multiples of 64) and on the scattered blob, sol_karman_pressure_solve_large (CG), B = 2 with two right-hand sides, TOL_FIELD.
    Measured: one-window 4.8e-7 ... 3.4e-6, scattered 4.9e-7 ... 4.3e-6, CG 7.0e-7 ... 1.2e-6 in [86, 85] (130 x 65) and [102, 104]
    (160 x 80) iterations."""
    B = 2
    g = table_geometry(name, Y, X)
    mk = scene_masks(name, Y, X, solver)
    cfg = cfg_of(B, name, Y, X, mk)
    rhs = step_like_rhs(B, Y, X)
    assert not torch.equal(rhs[0], rhs[1])
    if not hasattr(g, "_mlu"):
        g._mlu = spla.splu((-g.pressure_matrix()).tocsc())
    ref = np.stack([g._mlu.solve(r.numpy().ravel()).reshape(Y, X) for r in rhs])
    info = {}
    if solver == "cg":
        p = ops.pressure_solve_large(f32(rhs), cfg, mk, info=info)
    else:
        h = f32(rhs)
        ws = torch.empty((ops.large_workspace_bytes(cfg, mk) + 3) // 4, dtype=torch.float32, device=DEV)
        p = torch.full_like(h, float("nan"))
        _lib.check(sol_amd.load().sol_karman_pressure_solve_large_direct(C.byref(cfg), _lib.stream(), _lib.ptr(h), _lib.ptr(p),
                                                                         mk.direct_header.ctypes.data_as(C.c_void_p), _lib.ptr(ws), ws.numel() * 4))
    torch.cuda.synchronize()
    e = [rel(p[b], ref[b]) for b in range(B)]
    print("solve alone, %s %s %s: %s against sparse LU%s" % (name, sid(Y, X), solver, e, "" if solver != "cg" else ", iterations %s" % info["iterations"].tolist()))
    if solver == "cg":
        converged(info, B, ("converged",))
    assert max(e) < TOL_FIELD, e


# ---- 2. two forward steps against the float64 oracle ---------------------------------------------------------------------------
STEPS = ([(name, Y, X, "auto", "replicate") for Y, X in SHAPES for name in ("default", "big", "corner", "two")]
         + [("two", Y, X, s, "replicate") for Y, X in SHAPES for s in ("cg", SC)]
         + [("corner", Y, X, "auto", "dirichlet0") for Y, X in SHAPES])


@pytest.mark.parametrize("name,Y,X,solver,pad", STEPS, ids=["%s_%s_%s_%s" % (c[0], sid(c[1], c[2]), c[3], c[4]) for c in STEPS])
def test_two_forward_steps_against_the_oracle(name, Y, X, solver, pad):
    """B = 2, Reynolds numbers 160000 and 320000, density included; TOL_FIELD on d, v_y, v_x after each of two steps.
    Measured: d 4.2e-8 ... 5.8e-8, v_y 4.8e-8 ... 1.3e-7, v_x 3.2e-7 ... 1.0e-6."""
    B = 2
    st, _, out1, _, out2 = oracle(name, Y, X, pad)
    assert float(st[3][0]) != float(st[3][1])
    mk = scene_masks(name, Y, X, solver)
    cfg = cfg_of(B, name, Y, X, mk, grad_pad=pad)
    h = tuple(f32(t) for t in st[:3])
    re = f32(st[3])
    for k, ref in enumerate((out1, out2)):
        info = {}
        with torch.no_grad():
            h = ops.karman_step_large(*h, re, cfg, mk, info=info)
        torch.cuda.synchronize()
        if mk.pressure_solver == "cg":
            converged(info, B, ("converged",))
        else:
            assert info == {}
        errs = [rel(a, b) for a, b in zip(h, ref)]
        print("%s %s %s %s step %d: %s against the oracle" % (name, sid(Y, X), mk.pressure_solver, pad, k + 1, errs))
        assert max(errs) < TOL_FIELD, errs


# ---- 3. the adjoint against the oracle's autograd ------------------------------------------------------------------------------
ADJ = ([(name, Y, X, "auto") for Y, X in SHAPES[:2] for name in ("default", "corner")] + [("two", 130, 65, "auto")]
       + [("two", Y, X, s) for Y, X in SHAPES[:2] for s in ("cg", SC)])


@pytest.mark.parametrize("name,Y,X,solver", ADJ, ids=["%s_%s_%s" % (c[0], sid(c[1], c[2]), c[3]) for c in ADJ])
def test_adjoint_against_the_oracle(name, Y, X, solver):
    """Partial 16 x 16 tiles with the extra face row Y and face column X (130 x 65: 2 rows and 1 column left over; 144 x 72: full tile rows, 8 columns left over), every solver.  Trimmed
    metric, TOL_GRAD; oracle alone 6.5e-6 ... 7.5e-6 (module docstring).  Measured: 3.3e-7 ... 8.6e-7 trimmed; CG iterations forward / backward [86, 87] / [77, 73] at
    130 x 65 and [96, 96] / [81, 82] at 144 x 72."""
    B = 2
    st, w, out1, grad1, _ = oracle(name, Y, X)
    mk = scene_masks(name, Y, X, solver)
    if (name, Y, solver) == ("two", 130, "auto"):
        assert int(mk.direct_header[7]) == 64                  # the one-window blob takes both cylinders at this size
    info = {}
    out, got, _ = hip_grad(st, cfg_of(B, name, Y, X, mk), mk, w, info)
    if mk.pressure_solver == "cg":
        converged(info, B)
        print("CG iterations forward %s, backward %s" % (info["iterations"].tolist(), info["iterations_bwd"].tolist()))
    for a, b in zip(out, out1):
        assert rel(a, b) < TOL_FIELD, rel(a, b)
    check_grads(got, grad1, True, "%s %s %s" % (name, sid(Y, X), mk.pressure_solver))


# ---- 4. one-hot cotangents -----------------------------------------------------------------------------------------------------
def obstacle_face(g):
    """a v_x face with fluid on both sides whose right-hand cell touches the obstacle, on a row through the sphere"""
    j = g.Y // 4
    i = int(np.argmin(g.active[j])) - 1                        # the last fluid cell in front of the obstacle; face i lies on its left
    assert g.active[j, i + 1] == 0 and g.mx[j, i] == 1 and g.mx[j, i + 1] == 0
    return j, i


ONE_HOT = {"a_vy_0_0": lambda g: (0, 0, 0), "b_vy_Y_Xm1": lambda g: (0, g.Y, g.X - 1), "c_vx_Ym1_X": lambda g: (1, g.Y - 1, g.X),
           "d_vx_beside_the_obstacle": lambda g: (1,) + obstacle_face(g)}


@pytest.mark.parametrize("which", list(ONE_HOT))
def test_one_hot_cotangent_against_the_oracle(which):
    """130 x 65, default sphere, B = 2: the cotangent is 1.0 at one face of each simulation and 0 elsewhere (the g != 0 skips; all but
    a few workgroups publish no maximum).  (b) and (c) are the extra face row / column of the ragged last tiles.  Trimmed metric at
    TOL_GRAD as in test 3, and for (a)-(c) the untrimmed one at ONE_HOT_UNTRIMMED (module docstring: why, and the oracle-alone values).
    Measured: (a) exactly zero, (b) 5.0e-7 / 1.3e-8 untrimmed, (c) 0 / 6.1e-8 untrimmed, (d) 4.5e-7 / 6.1e-7 trimmed."""
    B, Y, X, name = 2, 130, 65, "default"
    g = table_geometry(name, Y, X)
    st = oracle(name, Y, X)[0]
    comp, j, i = ONE_HOT[which](g)
    w = [torch.zeros(B, Y + 1, X, dtype=torch.float64), torch.zeros(B, Y, X + 1, dtype=torch.float64)]
    w[comp][:, j, i] = 1.0
    _, ref = oracle_grad(st, g, w)
    mk = scene_masks(name, Y, X)
    _, got, _ = hip_grad(st, cfg_of(B, name, Y, X, mk), mk, w)
    nz = [int((t != 0).sum()) for t in ref]
    print("one-hot %s at component %d face (%d, %d): the reference gradient has %s non-zero entries" % (which, comp, j, i, nz))
    check_grads(got, ref, True, "one-hot " + which)
    if which[0] == "a":
        assert nz == [0, 0] and not bool(got[0].any()) and not bool(got[1].any())
    elif which[0] in "bc":
        assert 0 < sum(nz) < 40
        full = [rel(a, b) for a, b in zip(got, ref)]
        print("one-hot %s untrimmed: %s" % (which, full))
        assert max(full) < ONE_HOT_UNTRIMMED, full
    else:
        assert min(nz) > 1000


# ---- 5. tile window == global atomics, bit for bit, up to six cells of back-trace -------------------------------------------------
TILE = [(name, Y, X, s, scaled) for Y, X in SHAPES[:2] for name, s in (("default", "auto"), ("two", "cg")) for scaled in (False, True)]


@pytest.mark.parametrize("name,Y,X,solver,scaled", TILE,
                         ids=["%s_%s_%s_%s" % (c[0], sid(c[1], c[2]), c[3], "cfl6" if c[4] else "as_is") for c in TILE])
def test_tile_window_equals_global_atomics_bit_for_bit(name, Y, X, solver, scaled):
    """k2d_adj_tile 1 against 0, g_vy and g_vx under torch.equal, at the spun-up state and with its velocity scaled to
    max |u| dt/dx = 6 (asserted > 5): most contributions then land beyond the LDS window and go to global memory, and the back-traces
    near the edges are clamped.  At the scaled state the forward fields are also held to the float64 oracle at TOL_FIELD (oracle alone
    <= 1.8e-6, module docstring) and the gradient to the trimmed metric (oracle alone 6.0e-6 ... 6.7e-6).
    Measured: max |u| dt/dx 1.19 ... 1.35 as is, 6.0000 scaled; forward at the scaled state d 7.8e-8 ... 9.4e-8, v_y 2.7e-7 ... 3.8e-7,
    v_x 2.0e-6 / 2.1e-6 (two, CG) and 4.2e-6 / 4.5e-6 (default, direct); gradients 4.8e-7 ... 8.5e-7 trimmed; CG iterations forward /
    backward [86, 87] / [77, 73] as is and [89, 88] / [77, 73] scaled at 130 x 65, [96, 96] / [81, 82] and [96, 97] / [81, 82] at 144 x 72."""
    B = 2
    g = table_geometry(name, Y, X)
    st, w = oracle(name, Y, X)[:2]
    if scaled:
        st, cfl64 = cfl_scaled(st, g, CFL_TARGET)
        ref_out, ref_g = oracle_grad(st, g, w)
    mk = scene_masks(name, Y, X, solver)
    cfg = cfg_of(B, name, Y, X, mk)
    info = {}
    out, tile, (svy, svx) = hip_grad(st, cfg, mk, w, info)
    cfl = max(float(svy.abs().max()), float(svx.abs().max())) / g.dx
    print("%s %s %s: max |u| dt/dx = %.4f%s" % (name, sid(Y, X), "scaled" if scaled else "as is", cfl,
                                               "" if mk.pressure_solver != "cg" else ", CG iterations %s / %s" % (info["iterations"].tolist(), info["iterations_bwd"].tolist())))
    hw, re = [f32(w[0]), f32(w[1])], f32(st[3])
    _lib.set_option("k2d_adj_tile", 0)
    try:
        glob = ops.karman_step_large_bwd(svy, svx, re, hw[0], hw[1], cfg, mk)
        torch.cuda.synchronize()
    finally:
        _lib.set_option("k2d_adj_tile", 1)
    again = ops.karman_step_large_bwd(svy, svx, re, hw[0], hw[1], cfg, mk)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tile[0]).all()) and float(tile[0].abs().max()) > 0 and float(tile[1].abs().max()) > 0
    assert torch.equal(again[0], tile[0]) and torch.equal(again[1], tile[1])
    assert torch.equal(glob[0], tile[0]), "g_vy: tile window differs from global atomics"
    assert torch.equal(glob[1], tile[1]), "g_vx: tile window differs from global atomics"
    if scaled:
        assert cfl > 5.0 and abs(cfl - cfl64) < 1e-3, (cfl, cfl64)
        errs = [rel(a, b) for a, b in zip(out, ref_out)]
        print("forward at the scaled state against the oracle: %s" % errs)
        assert max(errs) < TOL_FIELD, errs
        check_grads(tile, ref_g, True, "%s %s scaled" % (name, sid(Y, X)))
    else:
        assert cfl < 4.0                                       # every contribution inside the window's halo


# ---- 6. a simulation does not see its batch neighbours --------------------------------------------------------------------------
@pytest.mark.parametrize("name,solver", [("default", "auto"), ("two", "cg"), ("two", SC)], ids=["default_direct", "two_cg", "two_scattered"])
def test_batch_independence_bit_for_bit(name, solver):
    """B = 3 at 130 x 65, three Reynolds numbers.  Simulation 0 is ordinary; simulation 1 has zero velocity, zero density and a zero
    cotangent; simulation 2 is ordinary with its cotangent scaled by 2^20.  Outputs, input gradients and the CG reports of every
    simulation equal, under torch.equal, those of the same simulation run alone (B = 1): the CG done words, the absmax slots and the
    scale of the fixed-point scatter are per simulation.  Simulation 1's adjoint solve has a zero right-hand side and stops at 0
    iterations (a frozen simulation beside two live ones); its max|g_a| is 0 (the m == 0 branch of fx_scale) and its gradient exactly 0.
    Its FORWARD solve does iterate: the inflow condition prescribes v_y = 1 on the boundary faces of a field that is zero elsewhere.
    Measured CG iterations (forward / backward): [87, 76, 88] / [77, 0, 77]."""
    B, Y, X = 3, 130, 65
    g = table_geometry(name, Y, X)
    d, vy, vx, re = (t.clone() for t in state(B, Y, X, SEED, g))
    assert len(set(re.tolist())) == 3
    d[1], vy[1], vx[1] = 0.0, 0.0, 0.0
    w = [t.clone() for t in cotangent_at(B, Y, X)]
    for t in w:
        t[1] = 0.0
        t[2] *= 2.0 ** 20
    mk = scene_masks(name, Y, X, solver)
    info = {}
    out, grad, _ = hip_grad((d, vy, vx, re), cfg_of(B, name, Y, X, mk), mk, w, info)
    cg = mk.pressure_solver == "cg"
    if cg:
        converged(info, B)
        print("batch of three: CG iterations forward %s, backward %s" % (info["iterations"].tolist(), info["iterations_bwd"].tolist()))
        assert int(info["iterations_bwd"][1]) == 0 and int(info["iterations_bwd"][0]) > 0 and int(info["iterations_bwd"][2]) > 0
    assert not bool(grad[0][1].any()) and not bool(grad[1][1].any())
    assert bool(torch.isfinite(grad[0]).all()) and float(grad[0][0].abs().max()) > 0 and float(grad[0][2].abs().max()) > 2.0 ** 10
    for b in range(B):
        sl = slice(b, b + 1)
        i1 = {}
        o1, g1, _ = hip_grad((d[sl], vy[sl], vx[sl], re[sl]), cfg_of(1, name, Y, X, mk), mk, [t[sl] for t in w], i1)
        for what, a, c in zip(("d", "v_y", "v_x", "g_vy", "g_vx"), out + grad, o1 + g1):
            assert torch.equal(a[sl], c), "simulation %d: %s in the batch differs from the run alone (max |diff| %.3e)" % (
                b, what, float((a[sl] - c).abs().max()))
        if cg:
            for k in ("iterations", "converged", "iterations_bwd", "converged_bwd"):
                assert int(info[k][b]) == int(i1[k][0]), (b, k, info[k].tolist(), i1[k].tolist())


# ---- 7. the adjoint is linear in the cotangent, exactly, over powers of two --------------------------------------------------------
@pytest.mark.parametrize("name,solver", [("default", "auto"), ("two", "cg")], ids=["default_direct", "two_cg"])
def test_adjoint_scales_exactly_with_a_power_of_two_cotangent(name, solver):
    """g(2^k w) == 2^k g(w) under torch.equal at 130 x 65, B = 2, for k in {-40, -13, +13, +40} on both simulations and k = (-40, +40)
    per simulation in one batch: every stage is linear, the fixed-point scale qs / qi is a power of two that follows the exponent of
    max|g_a| per simulation, and the CG's ratios are scale free.  |k| <= 40 keeps every fp32 intermediate normal and the scale's
    exponent clamp [-80, 120] out of reach.  The CG solve runs with cg_atol = 0 and cg_rtol = CG_RTOL: a non-zero absolute tolerance is
    a threshold in the cotangent's units, so it legitimately breaks the invariance (a smaller cotangent stops earlier).  The iteration
    counts are equal too.  Measured backward iterations: [77, 73] at every k."""
    B, Y, X = 2, 130, 65
    st, w = oracle(name, Y, X)[:2]
    mk = scene_masks(name, Y, X, solver)
    cg = mk.pressure_solver == "cg"
    cfg = cfg_of(B, name, Y, X, mk, **({"cg_atol": 0.0} if cg else {}))
    hy, hx = f32(st[1]).requires_grad_(True), f32(st[2]).requires_grad_(True)
    out = ops.karman_step_large(f32(st[0]), hy, hx, f32(st[3]), cfg, mk)
    svy, svx = out[1].grad_fn.saved_tensors[:2]
    re, hw = f32(st[3]), [f32(w[0]), f32(w[1])]

    def bwd(scale):
        s = torch.tensor(scale, dtype=torch.float32, device=DEV).reshape(B, 1, 1)
        info = {}
        gy, gx = ops.karman_step_large_bwd(svy, svx, re, hw[0] * s, hw[1] * s, cfg, mk, info=info)
        torch.cuda.synchronize()
        if cg:
            converged(info, B, ("converged_bwd",))
        return gy, gx, s, (info["iterations_bwd"].tolist() if cg else None)

    by, bx, _, its = bwd([1.0, 1.0])
    assert bool(torch.isfinite(by).all()) and float(by.abs().max()) > 0
    print("power-of-two scaling, %s: backward iterations %s" % (mk.pressure_solver, its))
    for ks in ((-40, -40), (-13, -13), (13, 13), (40, 40), (-40, 40)):
        gy, gx, s, it = bwd([2.0 ** k for k in ks])
        for what, a, b in (("g_vy", gy, by * s), ("g_vx", gx, bx * s)):
            assert bool(torch.isfinite(a).all())
            assert torch.equal(a, b), "k = %s: %s differs from the scaled gradient in %d entries (max relative %.3e)" % (
                ks, what, int((a != b).sum()), float(((a - b).abs() / b.abs().clamp_min(1e-45)).max()))
        assert it == its, (ks, it, its)
