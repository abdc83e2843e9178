"""The karman-3d step at ragged shapes, through every transform kernel, in a batch and across cotangent scales (pytest -m gpu).

The rest of the 3-D suite runs csrc/karman3d.hip, csrc/pcg.hip and csrc/karman3d_density_bwd.hip at 16 x 8 x 8, 20 x 10 x 10, 32 x 16 x 16
and 128 x 64 x 64 only.  Here: the table of karman3d_shapes.CELLS -- every instantiation of the matrix-core sine transforms, the LDS-fed
transforms with X != Z, Y = 48 and Y = 128, the batched-GEMM fallback, Z beyond the adjoint's and beyond the advection's LDS window,
ragged advection and adjoint tiles at a CFL number beyond their halo, half a block of capacitance padding, a sphere cut by a wall, an
odd Y and the refusal of two odd extents -- plus one-hot cotangents on the extra face row / column / layer, a batch whose middle
simulation is all zero, and cotangents scaled by 2^-40 ... 2^40.  test_karman3d_shapes_cpu.py pins the table and holds the
oracle-alone figures (float32 oracle against float64 oracle) next to which the values measured here stand.

Tolerances are the suite's (karman3d_shapes): TOL_FIELD = 1e-5 relative L2 on fields and pressures, TOL_GRAD = 1e-4 on gradients in
the trimmed metric (at most floor(1e-3 n) entries of a component left out: the step's gradient is discontinuous where a departure
point crosses a cell boundary), CG_RTOL = 1e-7 for the CG solves.  Bit comparisons are torch.equal.  The values measured on an MI355X
(printed by the tests) stand in the docstrings of the tests."""
import ctypes as C
import functools
import os
import sys

import pytest
import torch

import sol_oracle3d as o
from sol_amd import _lib
from sol_amd import karman3d as k3
from sol_amd._lib import ptr, stream

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import karman3d_shapes as ks
from karman3d_shapes import ADJ_CELLS, CELLS, CG_RTOL, DEV, ODD, OBSTACLE, RAGGED, SEED, TOL_FIELD, TOL_GRAD, f32, rel, sid

pytestmark = pytest.mark.gpu
ALL = list(CELLS)
CG_MAX_ITER = 200                   # launch budget of the CG solves here (an obstacle that spans the domain, rtol 1e-7); the counts are printed
FS = (1 / 0.2, 1 / 0.25, 1 / 0.3, 1 / o.STD_RE)


@functools.lru_cache(maxsize=None)
def scene(cell, obstacle, solver="auto"):
    """Scene3D of a table cell on the oracle's masks ("empty": all fluid); the direct blob's (nS, SP) is checked against the table BEFORE
    anything is launched: the case reaches the padding and the capacitance size it is listed for"""
    g = ks.empty_geometry(cell) if obstacle == "empty" else ks.geometry(cell, obstacle)
    sc = k3.Scene3D(*cell, device=DEV, active=g.active, inflow=g.inflow, pressure_solver=solver)
    if solver == "cg":
        assert sc.pressure_solver == "cg" and int(sc.direct_header[4]) == 0
    else:
        assert sc.pressure_solver == "direct"
        want = (0, 0) if obstacle == "empty" else ks.BLOBS[(cell, obstacle)]
        assert (int(sc.direct_header[4]), int(sc.direct_header[5])) == want, (cell, obstacle, sc.direct_header[:6].tolist())
    return g, sc


def flow(sc, B, **kw):
    if sc.pressure_solver == "cg":
        kw.setdefault("cg_rtol", CG_RTOL)
        kw.setdefault("cg_max_iter", CG_MAX_ITER)
    return k3.Karman3DFlow(sc, B, **kw)


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
    """the kernel names a _lib.profile() block launched, as SOL_LAUNCH spells them, without blanks and parentheses"""
    return {k.strip("()").replace(" ", "") for k in p.kernels}


def dev_state(st):
    d, v, re = st
    return [f32(d), f32(v[0]), f32(v[1]), f32(v[2]), f32(re)]


@functools.lru_cache(maxsize=None)
def oracle(cell, grad_pad="replicate"):
    """B = 2, state seed 5, cotangent seed 3 on the cell's scene: the state, the cotangents, the float64 oracle's first step with the
    gradient of <v_out, w>, and its second step (one computation per cell and padding, shared and left unchanged)"""
    g = ks.geometry(cell, OBSTACLE[cell])
    st = ks.state(2, cell, SEED, g)
    w, wd = ks.cotangent(2, cell, g=g)
    out1, grad1 = ks.oracle_grad(st, g, w, grad_pad=grad_pad)
    with torch.no_grad():
        d2, v2 = o.karman3d_step(out1[0], out1[1:], st[2], g, grad_pad=grad_pad)
    return st, w, wd, out1, grad1, (d2,) + tuple(v2)


def hip_grad(sim, st, w, wd=None, re_leaf=False):
    """one differentiable Karman3DFlow.step + backward of <v_out, w> (+ <d_out, wd>) -> (outputs, (g_d, g_vy, g_vx, g_vz, g_re) with None
    where no gradient arrived)"""
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


def forward_saved(sim, st):
    """a plain forward step that keeps the post-diffusion velocity -> (device state, outputs, saved)"""
    hs = dev_state(st)
    saved = [torch.empty_like(t) for t in hs[1:4]]
    with torch.no_grad():
        out = sim._fwd(*hs, saved)
    torch.cuda.synchronize()
    return hs, out, saved


def converged(sim, B, keys=("converged", "converged_bwd")):
    for k in keys:
        assert sim.solve_info[k].tolist() == [1] * B, (k, sim.solve_info)


def iters(sim, keys=("iterations", "iterations_bwd")):
    return " / ".join(str(sim.solve_info[k].tolist()) for k in keys if k in sim.solve_info)


# ---- (a) the empty-box solve alone: every transform kernel ----------------------------------------------------------------------------
EMPTY = [(c, s) for c in ALL for s in ks.transform_settings(*c)]


@pytest.mark.parametrize("cell,setting", EMPTY, ids=["%s_mfma%d_fused%d" % (sid(c), s[0], s[1]) for c, s in EMPTY])
def test_empty_box_solve_alone(cell, setting):
    """Karman3DFlow.pressure_solve on the all-fluid scene against float64 o.rect_solve under every setting of (k3d_mfma_tf, k3d_fused_tf)
    that runs other kernels at the cell: the matrix-core kernels, the LDS-fed ones, the batched GEMMs.  B = 3, the middle right-hand side
    all zero: its pressure is exactly zero; the others (step-like, white) within TOL_FIELD (float32 restatement alone: 1.6e-7 ... 4.0e-7).
    Measured: 1.8e-7 ... 3.8e-7 on every path; the matrix-core and the LDS-fed kernels give the same figures to four digits (both add in ascending
    k), the GEMMs differ in the third.  The kernels each setting launched are asserted by name (_lib.profile)."""
    B = 3
    _, sc = scene(cell, "empty")
    rhs = torch.stack([ks.step_like_rhs(1, cell)[0], torch.zeros(cell, dtype=torch.float64), ks.white_rhs(1, cell)[0]])
    ref = ks.rect_solve(rhs, cell)
    sim = flow(sc, B)
    with options(k3d_mfma_tf=setting[0], k3d_fused_tf=setting[1]), _lib.profile() as prof:
        p = sim.pressure_solve(f32(rhs))
        torch.cuda.synchronize()
    # the kernels the case is listed for did run, and no other transform did
    Y, X, Z = cell
    path = ks.transform_path(*cell) if setting[1] else "gemm"
    path = "lds" if path == "mfma" and not setting[0] else path
    want = {"mfma": {"k3_tzx_mfma<%d,%d>" % (X // 2, Z // 2), "k3_ty_mfma<%d>" % (Y // 2)}, "lds": {"k3_tzx", "k3_ty"}, "gemm": {"k_l_gemm", "k3_scale"}}[path]
    ran = {k for k in kernels_of(prof) if k.startswith(("k3_t", "k_l_gemm", "k3_scale"))}
    assert ran == want, (ran, want)
    e = [rel(p[b], ref[b]) for b in (0, 2)]
    print("empty box %s (%s path) mfma %d fused %d: step-like %.3e, white %.3e" % (sid(cell), ks.transform_path(*cell), *setting, *e))
    assert bool(torch.isfinite(p).all())
    assert not bool(p[1].any()), "the zero right-hand side's pressure is not exactly zero"
    assert max(e) < TOL_FIELD, e


# ---- (b) the direct solve with an obstacle, and the CG solve ----------------------------------------------------------------------------
SOLVES = ([(c, ob, "direct") for c in ALL for ob in ("sphere", "cylinder") if ks.BLOBS[(c, ob)][0] and (c, ob) not in ks.SLOW_BLOBS]
          + [(c, "cylinder", "cg") for c in ALL] + [(c, "sphere", "cg") for c in ALL[:3]])


@functools.lru_cache(maxsize=None)
def solve_reference(cell, obstacle):
    g = ks.geometry(cell, obstacle)
    rhs = ks.step_like_rhs(2, cell) * torch.as_tensor(g.active)          # what the step's solve sees: no divergence inside the obstacle
    return rhs, ks.oracle_solve(rhs, g)


@pytest.mark.parametrize("cell,obstacle,solver", SOLVES, ids=["%s_%s_%s" % (sid(c), ob, s) for c, ob, s in SOLVES])
def test_pressure_solve_with_obstacle_against_the_oracle(cell, obstacle, solver):
    """sol_karman3d_pressure_solve on the sphere and the cylinder (which spans the domain along z) of every cell: the capacitance
    correction with SP = 64 ... 1664 (half a block of padding at 22 x 10 x 12, a sphere cut by the z wall at 64 x 64 x 32), and the CG
    solve, against the float64 oracle's solve (sparse LU below LU_MAX_CELLS, else its own PCG).  B = 2, TOL_FIELD.
    Measured: direct 1.7e-7 ... 4.6e-7; CG 1.3e-7 ... 3.5e-7 in 13 ... 58 iterations (cylinder: 16x9x9 [13, 14], 22x10x12 [18, 19], 128x8x8 [16, 16],
    48x24x8 [24, 25], 24x12x72 and 18x10x84 [28, 28], 32x32x32 [43, 42], 64x32x64 [53, 53], 64x64x32 [58, 58]; sphere [27, 27], [28, 28], [34, 35])."""
    B = 2
    _, sc = scene(cell, obstacle, solver)
    rhs, ref = solve_reference(cell, obstacle)
    sim = flow(sc, B)
    p = sim.pressure_solve(f32(rhs))
    torch.cuda.synchronize()
    e = [rel(p[b], ref[b]) for b in range(B)]
    print("solve %s %s %s (nS, SP) = %s: %s%s" % (sid(cell), obstacle, solver, ks.BLOBS[(cell, obstacle)], ["%.3e" % v for v in e],
                                                  "" if solver != "cg" else ", iterations %s" % iters(sim)))
    if solver == "cg":
        converged(sim, B, ("converged",))
    assert max(e) < TOL_FIELD, e


# ---- (c) two forward steps against the oracle ----------------------------------------------------------------------------------------------
STEPS = ([(c, t, "replicate") for c in ALL for t in (0, 1)] + [(c, t, "dirichlet0") for c in ((22, 10, 12), (32, 32, 32)) for t in (0, 1)])


@pytest.mark.parametrize("cell,tile,pad", STEPS, ids=["%s_tile%d_%s" % (sid(c), t, p) for c, t, p in STEPS])
def test_two_forward_steps_against_the_oracle(cell, tile, pad):
    """B = 2, Reynolds numbers 160000 and 320000; d, v_y, v_x, v_z and the four channels of the fused feature output after each of two
    steps, TOL_FIELD (oracle alone <= 1.4e-6).  k3d_tile = 1: the advection from LDS tiles of 8 x 8 columns (ragged at 22 x 10 x 12 and
    21 x 10 x 12, Z = 72 still in LDS, Z = 84 falls back to the global gathers).
    Measured: d 5.0e-8 ... 7.2e-8, v_y 4.4e-8 ... 6.1e-8, v_x 2.7e-7 ... 8.1e-7, v_z 4.0e-7 ... 8.6e-7; features the same, f_re 2.6e-8.  The advection
    kernel each case launched (k3_advect_tile / k3_advect) is asserted by name."""
    B = 2
    st, _, _, out1, _, out2 = oracle(cell, pad)
    _, sc = scene(cell, OBSTACLE[cell])
    sim = flow(sc, B, grad_pad=pad)
    h = dev_state(st)
    re = h[4]
    feat = torch.full((B,) + tuple(cell) + (4,), float("nan"), dtype=torch.float32, device=DEV)
    with options(k3d_tile=tile):
        for k, ref in enumerate((out1, out2)):
            with torch.no_grad(), _lib.profile() as prof:
                h = sim.step(*h[:4], re, feat_out=feat, feat_scale=FS)
                torch.cuda.synchronize()
            ran = {n for n in kernels_of(prof) if n.startswith("k3_advect")}
            assert ran == ({"k3_advect_tile"} if tile and ks.advect_tile_fits(cell[2]) else {"k3_advect"}), ran
            ks.check_fields(h, ref, "%s tile %d %s step %d" % (sid(cell), tile, pad, k + 1))
            fref = o.to_feature(ref[1:], st[2]) * torch.tensor(FS, dtype=torch.float64)
            ks.check_fields([feat[..., c] for c in range(4)], [fref[..., c] for c in range(4)],
                            "%s tile %d %s step %d features" % (sid(cell), tile, pad, k + 1), names=("f_y", "f_x", "f_z", "f_re"))


# ---- (d) the velocity adjoint against the oracle's autograd ---------------------------------------------------------------------------------
ADJ = [(c, s) for c in ADJ_CELLS for s in ("direct", "cg")]


@pytest.mark.parametrize("cell,solver", ADJ, ids=["%s_%s" % (sid(c), s) for c, s in ADJ])
def test_velocity_adjoint_against_the_oracle(cell, solver):
    """Every cell but 16 x 9 x 9, the direct and the CG solve: adjoint tiles of 4 x 4 columns that leave 2 rows and 2 columns plus the
    face row Y, face column X and face layer Z (22 x 10 x 12), an odd Y (21 x 10 x 12), Z beyond the LDS window (72, 84).  Trimmed
    metric, TOL_GRAD (oracle alone 6.9e-7 ... 7.3e-6).
    Measured: direct 1.5e-7 ... 3.0e-7, CG 1.1e-7 ... 1.7e-7, trimmed and untrimmed alike; CG iterations forward / backward [29, 29] / [24, 24]
    (32x32x32), [30, 30] / [25, 24] (64x32x64), [39, 40] / [29, 29] (64x64x32), [17, 17] / [16, 16] (128x8x8), [27, 27] / [23, 24] (48x24x8),
    [11, 11] / [11, 11] (22x10x12, 21x10x12), [11, 11] / [11, 10] (24x12x72), [10, 11] / [10, 11] (18x10x84)."""
    B = 2
    st, w, _, out1, grad1, _ = oracle(cell)
    _, sc = scene(cell, OBSTACLE[cell], "auto" if solver == "direct" else "cg")
    sim = flow(sc, B)
    out, got = hip_grad(sim, st, w)
    if solver == "cg":
        converged(sim, B)
        print("%s CG iterations forward / backward %s" % (sid(cell), iters(sim)))
    assert got[0] is None and got[4] is None
    ks.check_fields(out, out1, "%s %s" % (sid(cell), solver))
    ks.check_grads(got[1:4], grad1[1:4], "%s %s" % (sid(cell), solver))


def test_two_odd_extents_are_refused_before_anything_is_launched():
    """16 x 9 x 9: 3 Y X Z + X Z + Y Z + Y X faces, odd when two extents are odd (the fixed-point accumulators are zeroed in pairs).  The
    forward step runs (test (c)); every adjoint entry point refuses with the face-count message, and the C entry points leave the
    gradient buffers and the workspace as they were."""
    B, cell = 2, ODD
    g, sc = scene(cell, OBSTACLE[cell])
    st, w, wd = oracle(cell)[:3]
    sim = flow(sc, B, density_grad=True, re_grad=True)
    hs, out, saved = forward_saved(sim, st)
    assert all(bool(torch.isfinite(t).all()) for t in out)
    hw, hwd = [f32(t) for t in w], f32(wd)
    hdr = sc.direct_header.ctypes.data_as(C.c_void_p)
    # the C entry points: a sentinel in every output and in the workspace
    sim._ws(max(sim.lib.sol_karman3d_step_bwd_workspace_bytes(C.byref(sim.cfg)), sim.lib.sol_karman3d_density_bwd_workspace_bytes(C.byref(sim.cfg))))
    gi = [torch.full_like(t, 7.0) for t in saved]
    od = torch.full_like(hs[0], 7.0)
    sim.workspace.fill_(3.0)
    torch.cuda.synchronize()
    code = sim.lib.sol_karman3d_step_bwd(C.byref(sim.cfg), stream(), ptr(saved[0]), ptr(saved[1]), ptr(saved[2]), ptr(hs[4]), ptr(sc.active),
                                         ptr(sc.velBCyMask), sc.bc_stride, ptr(hw[0]), ptr(hw[1]), ptr(hw[2]), ptr(gi[0]), ptr(gi[1]), ptr(gi[2]),
                                         hdr, ptr(sim.workspace), sim.workspace_bytes)
    msg = sim.lib.sol_last_error().decode()
    assert code != 0 and "sol_karman3d_step_bwd: odd face count (4257): even X, Z expected" in msg, (code, msg)
    code = sim.lib.sol_karman3d_density_bwd(C.byref(sim.cfg), stream(), ptr(hs[0]), ptr(sc.inflow), ptr(saved[0]), ptr(saved[1]), ptr(saved[2]),
                                            ptr(hs[4]), ptr(sc.velBCyMask), sc.bc_stride, ptr(hwd), ptr(od), ptr(gi[0]), ptr(gi[1]), ptr(gi[2]), 0,
                                            ptr(sim.workspace), sim.workspace_bytes)
    msg = sim.lib.sol_last_error().decode()
    assert code != 0 and "sol_karman3d_density_bwd: odd face count (4257)" in msg, (code, msg)
    torch.cuda.synchronize()
    for t in gi + [od]:
        assert bool((t == 7.0).all())
    assert bool((sim.workspace == 3.0).all())
    # the host surfaces
    refusal = dict(match="odd face count")
    with pytest.raises(_lib.SolError, **refusal):
        sim._bwd(saved, hs[4], *hw)
    with pytest.raises(_lib.SolError, **refusal):
        sim._bwd(saved, hs[4], *hw, vel_in=hs[1:4])
    with pytest.raises(_lib.SolError, **refusal):
        sim._bwd(saved, hs[4], *hw, buoyancy=(1.0, 0.0, 0.0))
    with pytest.raises(_lib.SolError, **refusal):
        sim._bwd(saved, hs[4], *hw, vel_in=hs[1:4], buoyancy=(1.0, 0.0, 0.0))
    with pytest.raises(_lib.SolError, **refusal):
        k3.density_bwd(sim, hs[0], saved, hs[4], hwd)
    with pytest.raises(_lib.SolError, **refusal):
        k3.density_bwd(sim, hs[0], saved, hs[4], hwd, g_v=gi, vel_in=hs[1:4])
    with pytest.raises(_lib.SolError, **refusal):
        hip_grad(sim, st, w, wd, re_leaf=True)
    torch.cuda.synchronize()
    for t in gi:
        assert bool((t == 7.0).all())


# ---- (e) LDS windows == global atomics, bit for bit, at a CFL number beyond the halo ------------------------------------------------------------
TILE = [(c, scaled) for c in RAGGED + [(24, 12, 72)] for scaled in (False, True)]


@pytest.mark.parametrize("cell,scaled", TILE, ids=["%s_%s" % (sid(c), "cfl3" if s else "as_is") for c, s in TILE])
def test_lds_windows_equal_global_atomics_bit_for_bit(cell, scaled):
    """k3d_adj_tile and k3d_dens_adj_tile 1 against 0: the velocity adjoint's and the density adjoint's results under torch.equal, at the
    spun-up state and with its velocity scaled to max |u| dt/dx = 3 (asserted > 2.5): beyond the halo of 2 of the adjoint tiles (4 x 4
    columns, ragged here) and of the advection tiles (8 x 8), so contributions leave the LDS window for global memory and back-traces
    are clamped at the walls.  At the scaled state the forward fields (k3d_tile 0 and 1) and the gradients are also held to the oracle.
    Measured: max |u| dt/dx 0.118 (22x10x12, 21x10x12) and 0.140 (24x12x72) as is, 3.0000 scaled.  Forward at the scaled state (d / v_y / v_x / v_z),
    k3d_tile 0 and 1 within 3 %: 8.0e-8 / 1.1e-7 / 7.0e-7 / 6.1e-7 (22x10x12), 8.3e-8 / 1.4e-7 / 6.9e-7 / 6.7e-7 (21x10x12), 1.0e-7 / 2.7e-7 /
    1.7e-6 / 4.3e-6 (24x12x72; oracle alone 1.1e-6 / 3.5e-7 / 8.4e-7 / 2.2e-6).  Gradients at the scaled state 1.9e-7 ... 3.6e-7 trimmed
    (oracle alone 6.9e-7 ... 3.7e-6); untrimmed g_vy 2.1e-3 (21x10x12) and 1.1e-3 (24x12x72) -- the oracle alone reads the same there
    (2.1e-3, 1.1e-3): a departure point on a cell boundary.  The scatter kernels each setting launched are asserted by name."""
    B = 2
    g = ks.geometry(cell, OBSTACLE[cell])
    st, w, wd = oracle(cell)[:3]
    if scaled:
        st, cfl64 = ks.cfl_scaled(st, g)
        ref_out, ref_g = ks.oracle_grad(st, g, w)
    _, sc = scene(cell, OBSTACLE[cell])
    sim = flow(sc, B, density_grad=True)
    hs, out, saved = forward_saved(sim, st)
    cfl = max(float(t.abs().max()) for t in saved) / g.dx
    print("%s %s: max |u| dt/dx = %.4f" % (sid(cell), "scaled" if scaled else "as is", cfl))
    hw, hwd = [f32(t) for t in w], f32(wd)

    def both(want):
        with _lib.profile() as prof:
            gv = sim._bwd(saved, hs[4], *hw)
            gd = k3.density_bwd(sim, hs[0], saved, hs[4], hwd)
            torch.cuda.synchronize()
        ran = {n for n in kernels_of(prof) if "advect_adj" in n}
        assert ran == want, (ran, want)
        return list(gv) + list(gd)

    windows = {"k3b_advect_adj_tile" if cell[2] <= 64 else "k3b_advect_adj", "k3d_advect_adj_tile"}      # Z = 72: the velocity adjoint has no window
    tile = both(windows)
    with options(k3d_adj_tile=0, k3d_dens_adj_tile=0):
        glob = both({"k3b_advect_adj", "k3d_advect_adj"})
    again = both(windows)
    names = ("g_vy", "g_vx", "g_vz", "density: g_d", "density: g_vy", "density: g_vx", "density: g_vz")
    for n, a, b, c in zip(names, tile, glob, again):
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0, n
        assert torch.equal(a, c), "%s: two runs differ" % n
        assert torch.equal(a, b), "%s: LDS window differs from global atomics in %d entries" % (n, int((a != b).sum()))
    if scaled:
        assert cfl > 2.5 and abs(cfl - cfl64) < 1e-3, (cfl, cfl64)
        ks.check_fields(out, ref_out, "%s scaled, k3d_tile 0" % sid(cell))
        with options(k3d_tile=1):
            out_t = forward_saved(sim, st)[1]
        ks.check_fields(out_t, ref_out, "%s scaled, k3d_tile 1" % sid(cell))
        ks.check_grads(tile[:3], ref_g[1:4], "%s scaled" % sid(cell))
    else:
        assert cfl < 2.0                                        # every contribution inside the window's halo


# ---- (f) one-hot cotangents -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(ks.ONE_HOT))
def test_one_hot_cotangent_against_the_oracle(which):
    """22 x 10 x 12, sphere, B = 2: the cotangent is 1.0 at one face of each simulation and 0 elsewhere: (a) v_y[Y, X-1, Z-1], (b)
    v_x[Y-1, X, 0], (c) v_z[0, 0, Z] -- the extra face row, column and layer of the ragged last tiles -- and (d) a v_x face beside the
    obstacle (dense through the pressure solve).  Trimmed metric at TOL_GRAD, and the untrimmed one at ten times the oracle-alone
    untrimmed value of the case (karman3d_shapes.ONE_HOT_ALONE; a kernel that drops the face loses all of it: 1.0); where the reference
    gradient is exactly zero, so is the kernel's.  (b)-(d) run at the spun-up state, (a) at the drift state: its face lies on the wall
    column, and at the spun-up state the float32 oracle alone misses TOL_GRAD there (karman3d_shapes.ONE_HOT; measured here at that
    state: 3.9e-5 / 5.8e-5 / 6.7e-4 trimmed on a gradient whose largest entry is 5e-6, largest deviation 6.5e-10).
    Measured: (a) 4.6e-8 / 4.5e-7 / 1.3e-6 trimmed, 7.0e-8 / 9.4e-7 / 2.6e-6 untrimmed (bound 3.0e-5); (b) g_vy exactly zero, 3.7e-8 / 2.0e-8
    untrimmed (bound 6.2e-6); (c) g_vy exactly zero, 1.5e-7 / 5.4e-8 untrimmed (bound 8.5e-6); (d) 2.1e-7 / 1.5e-7 / 2.0e-7 trimmed, 2.1e-7 /
    1.2e-7 / 2.2e-7 untrimmed (bound 7.0e-5)."""
    B, cell = 2, (22, 10, 12)
    _, sc = scene(cell, "sphere")
    comp, j, i, k, _ = ks.ONE_HOT[which]
    st, g, w = ks.one_hot_case(which, B)
    _, ref = ks.oracle_grad(st, g, w)
    _, got = hip_grad(flow(sc, B), st, w)
    nz = [int((t != 0).sum()) for t in ref[1:4]]
    print("one-hot %s at component %d face (%d, %d, %d): the reference gradient has %s non-zero entries" % (which, comp, j, i, k, nz))
    ks.check_grads(got[1:4], ref[1:4], "one-hot " + which)
    bound = 10 * ks.ONE_HOT_ALONE[which]
    full = []
    for a, b in zip(got[1:4], ref[1:4]):
        if not bool(b.any()):
            assert not bool(a.any()), "the reference gradient is exactly zero, the kernel's is not"
            full.append(0.0)
        else:
            full.append(rel(a, b))
    print("one-hot %s untrimmed: %s (bound %.1e)" % (which, ["%.3e" % e for e in full], bound))
    assert sum(nz) > 0 and max(full) < bound, (full, bound)
    if which[0] != "d":
        assert sum(nz) < 60
    else:
        assert min(nz) > 1000


# ---- (g) a simulation does not see its batch neighbours --------------------------------------------------------------------------------------------
BATCH = [(c, s) for c in ((22, 10, 12), (48, 24, 8), (32, 32, 32)) for s in ("direct", "cg")]


@pytest.mark.parametrize("cell,solver", BATCH, ids=["%s_%s" % (sid(c), s) for c, s in BATCH])
def test_batch_independence_bit_for_bit(cell, solver):
    """B = 3, three Reynolds numbers, on the GEMM, the LDS-fed and the matrix-core transforms.  Simulation 0 is ordinary; simulation 1 has
    zero velocity, zero density and zero cotangents; simulation 2 is ordinary with its cotangents (velocity and density) scaled by 2^20.
    Outputs, input gradients (density_grad on) and the CG reports of every simulation equal, under torch.equal, those of the same
    simulation run alone (B = 1): the CG done words, the absmax slots and the scale of the fixed-point scatter are per simulation.
    Simulation 1's gradient is exactly zero and its adjoint solve stops at 0 iterations.
    Measured: every comparison bit-equal; CG iterations forward / backward [11, 10, 11] / [11, 0, 10] (22x10x12), [26, 24, 26] / [23, 0, 24]
    (48x24x8), [29, 25, 29] / [25, 0, 25] (32x32x32)."""
    B = 3
    g, sc = scene(cell, OBSTACLE[cell], "auto" if solver == "direct" else "cg")
    d, v, re = ks.state(B, cell, SEED, g)
    assert len(set(re.tolist())) == 3
    d, v = d.clone(), [t.clone() for t in v]
    w, wd = ks.cotangent(B, cell, g=g)
    w, wd = [t.clone() for t in w], wd.clone()
    for t in [d] + v + w + [wd]:
        t[1] = 0.0
    for t in w + [wd]:
        t[2] *= 2.0 ** 20
    sim = flow(sc, B, density_grad=True)
    out, grad = hip_grad(sim, (d, v, re), w, wd)
    cg = solver == "cg"
    if cg:
        converged(sim, B)
        print("batch of three %s: CG iterations forward / backward %s" % (sid(cell), iters(sim)))
        ib = sim.solve_info["iterations_bwd"].tolist()
        assert ib[1] == 0 and ib[0] > 0 and ib[2] > 0
    for c in range(4):
        assert not bool(grad[c][1].any()) and bool(torch.isfinite(grad[c]).all())
        assert float(grad[c][0].abs().max()) > 0 and float(grad[c][2].abs().max()) > 2.0 ** 10
    for b in range(B):
        sl = slice(b, b + 1)
        sim1 = flow(sc, 1, density_grad=True)
        o1, g1 = hip_grad(sim1, (d[sl], [t[sl] for t in v], re[sl]), [t[sl] for t in w], wd[sl])
        for what, a, c in zip(("d", "v_y", "v_x", "v_z", "g_d", "g_vy", "g_vx", "g_vz"), out + grad[:4], o1 + g1[:4]):
            assert torch.equal(a[sl], c), "simulation %d: %s in the batch differs from the run alone (max |diff| %.3e)" % (
                b, what, float((a[sl] - c).abs().max()))
        if cg:
            for k in ("iterations", "converged", "iterations_bwd", "converged_bwd"):
                assert int(sim.solve_info[k][b]) == int(sim1.solve_info[k][0]), (b, k, sim.solve_info, sim1.solve_info)


# ---- (h) the adjoints are linear in the cotangent, exactly, over powers of two --------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["direct", "cg"])
def test_adjoints_scale_exactly_with_a_power_of_two_cotangent(solver):
    """g(2^k w) == 2^k g(w) under torch.equal at 22 x 10 x 12, B = 2, for k in {-40, -13, +13, +40} on both simulations and k = (-40, +40)
    per simulation in one batch, for the velocity adjoint (sol_karman3d_step_bwd) and the density adjoint (sol_karman3d_density_bwd):
    every stage is linear, the fixed-point scale is a power of two that follows the exponent of the cotangent's maximum per simulation,
    and the CG's ratios are scale free.  The CG solve runs with cg_atol = 0: an absolute tolerance is a threshold in the cotangent's units
    and legitimately breaks the invariance.  The iteration counts are equal too.
    Measured: every comparison bit-equal; backward iterations [11, 11] at every k."""
    B, cell = 2, (22, 10, 12)
    st, w, wd = oracle(cell)[:3]
    _, sc = scene(cell, "sphere", "auto" if solver == "direct" else "cg")
    cg = solver == "cg"
    sim = flow(sc, B, density_grad=True, **({"cg_atol": 0.0} if cg else {}))
    hs, _, saved = forward_saved(sim, st)
    hw, hwd = [f32(t) for t in w], f32(wd)

    def bwd(scale):
        s = torch.tensor(scale, dtype=torch.float32, device=DEV).reshape(B, 1, 1, 1)
        gv = sim._bwd(saved, hs[4], *[t * s for t in hw])
        torch.cuda.synchronize()
        it = None
        if cg:
            converged(sim, B, ("converged_bwd",))
            it = sim.solve_info["iterations_bwd"].tolist()
        gd = k3.density_bwd(sim, hs[0], saved, hs[4], hwd * s)
        torch.cuda.synchronize()
        return list(gv) + list(gd), s, it

    base, _, its = bwd([1.0, 1.0])
    assert all(bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0 for t in base)
    print("power-of-two scaling, %s: backward iterations %s" % (solver, its))
    names = ("g_vy", "g_vx", "g_vz", "density: g_d", "density: g_vy", "density: g_vx", "density: g_vz")
    for kk in ((-40, -40), (-13, -13), (13, 13), (40, 40), (-40, 40)):
        got, s, it = bwd([2.0 ** k for k in kk])
        for what, a, b in zip(names, got, base):
            b = b * s
            assert bool(torch.isfinite(a).all())
            assert torch.equal(a, b), "k = %s: %s differs from the scaled gradient in %d entries (max relative %.3e)" % (
                kk, what, int((a != b).sum()), float(((a - b).abs() / b.abs().clamp_min(1e-45)).max()))
        assert it == its, (kk, it, its)


# ---- (i) the density adjoint and the gradient in Re ---------------------------------------------------------------------------------------------------
DENS = [(c, s) for c in ks.DENS_CELLS for s in ("spun_up", "drift")]


@pytest.mark.parametrize("cell,which", DENS, ids=["%s_%s" % (sid(c), s) for c, s in DENS])
def test_density_adjoint_and_re_gradient_against_the_oracle(cell, which):
    """Karman3DFlow(density_grad=True, re_grad=True) against the oracle's autograd: ragged density-adjoint tiles (22 x 10 x 12), Z = 72,
    and the matrix-core transforms (64 x 32 x 64).  spun_up: the loss <d_out, w_d> + <v_out, w> with the seeded-noise cotangents at the
    spun-up state -- g_d and the velocity gradients in the trimmed metric at TOL_GRAD; g_re is printed, not asserted: it moves by 1.8e-4
    ... 5.1e-4 in the oracle alone there (test_karman3d_shapes_cpu.py, karman3d_shapes.drift_state).  drift: the state with a lateral
    drift of 0.3 cells per step and the energy cotangents -- no departure point near a cell boundary, so every field gradient is held
    UNTRIMMED at TOL_GRAD (oracle alone 4.3e-7 ... 2.8e-6), and g_re as a relative L2 over the batch at TOL_GRAD (oracle alone 2.3e-6 ...
    3.2e-5; the density path is 1.4 % of it or more).
    Measured: spun_up: fields 4.6e-8 ... 6.3e-7; g_d 5.9e-8 ... 7.4e-8, g_v 1.6e-7 ... 3.0e-7 trimmed; g_re 1.1e-6 / 7.7e-7 / 6.3e-7 (the kernels form
    their departure points in index space and sit on the float64 side of every boundary here).  drift: fields 4.2e-8 ... 7.5e-8; g_d 4.7e-8 ...
    5.3e-8, g_v 8.5e-8 ... 3.3e-7 untrimmed; g_re 5.0e-6 (22x10x12), 2.2e-5 (24x12x72), 1.9e-6 (64x32x64)."""
    B = 2
    g = ks.geometry(cell, OBSTACLE[cell])
    if which == "spun_up":
        st, w, wd = oracle(cell)[:3]
    else:
        st = ks.drift_state(B, cell, SEED, g)
        w, wd = ks.energy_cotangent(st, g)
    ref_out, ref_g = ks.oracle_grad(st, g, w, wd, re_grad=True)
    _, sc = scene(cell, OBSTACLE[cell])
    out, got = hip_grad(flow(sc, B, density_grad=True, re_grad=True), st, w, wd, re_leaf=True)
    what = "%s %s" % (sid(cell), which)
    ks.check_fields(out, ref_out, what)
    res = ks.check_grads(got[:4], ref_g[:4], what, names=("g_d", "g_vy", "g_vx", "g_vz"))
    e = rel(got[4], ref_g[4])
    print("%s g_re: rel L2 over the batch %.3e (%s against %s)" % (what, e, got[4].tolist(), ref_g[4].tolist()))
    assert bool(torch.isfinite(got[4]).all()) and float(got[4].abs().min()) > 0
    if which == "drift":
        assert max(full for _, full in res) < TOL_GRAD, res
        assert e < TOL_GRAD, e
