"""Poisoned scratch and output buffers on the GPU (pytest -m gpu): every solver, network, trainer and roll-out entry point below
runs with each torch.empty / torch.empty_like of the package pre-filled with 0x00000000, 0xFFFFFFFF (NaN / -1), 0x7F7FFFFF (FLT_MAX) and
0x00000001 (a denormal / a set flag) -- tests/poison.py -- and must return the bits of the zero-pattern run, with no NaN or FLT_MAX
word in an output that run has none in.  include/sol_hip.h: workspaces are scratch, every output element is written.

Default options only; cnn_persistent and k3d_conv_persist stay off (their flag regions have a zero-before-first-use contract).  The
options named by a case (k2d_mc_tile, k2d_adj_tile, k2d_dens_adj_tile) select between two forms of the same launch.

Inputs come from the suite's case tables (large2d_scenes, periodic_cases, karman2d_small_shapes, burgers_small_cases, karman3d_shapes,
periodic3d_cases, karman2d_multi_launch_cases) WITHOUT their float64 spin-up step: nothing here is compared with a reference, so any
finite state serves, and the spin-up is host time.  B = 2.

Objects that keep a scratch buffer across eager calls are also called a second time after that buffer was overwritten in place with
each pattern (refill()).  Never between replays of a captured graph.  Buffers left out, by contract:
  - LargeGridRollout.p_guess (trainer.py:411, `self.p_guess = z(B, Y, X) if self.cg_warm_start`; include/sol_hip.h:209-214,
    sol_karman_step_fwd_large_cg_warm: `p_inout` "is read as the initial guess x0 and overwritten with" the step's pressure): state,
    allocated with zeros, not part of any workspace.  It is reset between runs (reset_guess), never refilled.
  - the absmax slots and weight-gradient partials of the network schedules: allocated with torch.zeros (a stated requirement), so the
    stand-in never touches them.
Every scratch buffer the issue lists is refilled: sim.workspace / _sub_ws (Karman3DFlow), tr.workspace (SolTrainer), ro.workspace
(SolRollout), _ws (LargeGridRollout), _ws_fwd / _ws_bwd / _ws_bwd_d (LargeGridTrainer) and the Burgers _ws dict (BurgersTest._ws).
Not run here: the stand-alone convolution and l2-loss ops (their tests pre-fill outputs with NaN), dist.py's packing buffer (needs a
process group) and KarmanFlow's _large_ws (karman.py:281: the same ops.karman_step_large call with a kept workspace, as
test_2d_large_workspace_refilled_between_eager_calls makes it).
Safety: the workspaces hold data only (carve.hpp: offsets are computed on the host, no pointer or index is read back from scratch);
the one polled region on the default paths, the band exchange of the 128 x 64 forward launch, is zeroed by the library itself in the
step's first launch (csrc/train.hip, `z.zero(w.xchg, ...)`) and its wait is bounded (csrc/karman_step.hip, BD_SPIN_LIMIT)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

import sol_amd
import sol_oracle as o
import sol_oracle3d as o3
from sol_amd import _lib, karman3d as k3, ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import burgers_small_cases as bs
import karman2d_multi_launch_cases as ml
import karman2d_small_shapes as k2s
import karman3d_shapes as ks
import periodic3d_cases as p3c
import periodic_cases as pc
import poison
from large2d_scenes import DEV, TWO, active_of, cotangent_at, f32, geometry, masks, state, step_like_rhs

pytestmark = pytest.mark.gpu
B = 2
SC = "direct_scattered"
RAGGED, SMALL = (130, 65), (40, 24)


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


def sync(x):
    torch.cuda.synchronize()
    return x


def refill(call, buffers, what):
    """call() once, then for each pattern: overwrite every buffer of buffers() in place and call() again -- same bits.  buffers: a
    callable (an object may grow or replace a workspace on its first call)"""
    base = poison.snapshot(sync(call()))
    bufs = [b for b in buffers() if b is not None]
    assert bufs, "%s: no scratch buffer to refill" % what
    for p in poison.PATTERNS:
        for b in bufs:
            poison.fill_(b, p)
        got = poison.snapshot(sync(call()))
        diff = poison.first_difference(got, base, what)
        assert diff is None, "scratch refilled with 0x%08X between two eager calls changes the result -- %s" % (p, diff)
        leak = poison.leaked_pattern(got, base, what)
        assert leak is None, "refill 0x%08X -- %s" % (p, leak)


def test_the_stand_in_reaches_device_allocations_and_stays_out_of_captures(monkeypatch):
    """The mechanism itself on the device: a workspace and an output the package allocates hold the pattern before the kernel runs; an
    output element a launch does not write shows up as a difference (sol_copy_words over all but the last word of a fresh output);
    inside a stream capture the allocation is handed through unfilled and the captured graph stays one of kernel nodes."""
    src = torch.arange(1, 65, dtype=torch.float32, device=DEV)
    for p in poison.PATTERNS:
        with poison.pattern(monkeypatch, p) as proxy:
            ws = ops._workspace(100, None, DEV)
            like = _lib.torch.empty_like(src[:7])
            assert proxy.filled == 2
        for t in (ws, like):
            assert set(t.view(torch.int32).tolist()) == {p - (1 << 32) if p >> 31 else p}

    def short_copy():
        out = ops.torch.empty(64, dtype=torch.float32, device=DEV)
        _lib.check(_lib.load().sol_copy_words(_lib.stream(), _lib.ptr(out), _lib.ptr(src), 63))
        return sync(out)
    with pytest.raises(AssertionError, match="changes the result.*word 63 of 64"):
        poison.check_patterns(monkeypatch, short_copy, "short copy")

    def full_copy():
        return sync(_lib.dcopy_(ops.torch.empty(64, dtype=torch.float32, device=DEV), src))
    poison.check_patterns(monkeypatch, full_copy, "full copy")
    with poison.pattern(monkeypatch, poison.ALL_ONES) as proxy:
        kept = []
        graph = _lib.capture_graph(lambda: kept.append(_lib.dcopy_(ops.torch.empty(64, dtype=torch.float32, device=DEV), src)), "poison probe")
        assert proxy.in_capture == 1 and proxy.filled == 0
    graph.replay()
    assert torch.equal(sync(kept[0]), src)


# =====================================================================================================================================
# 2-D large grids
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def scene2d(Y, X, kind="default", solver="auto", multi_launch=False):
    """(geometry, SceneMasks): no uninitialised allocation in either, so one instance serves every pattern"""
    g = o.geometry(Y, X) if kind == "default" else geometry(Y, X, active_of(TWO, Y, X))
    mk = ops.SceneMasks(g.active, g.inflow, g.bc_mask, g.bc_mask, DEV, pressure_solver=solver, multi_launch=multi_launch)
    return g, mk


@functools.lru_cache(maxsize=None)
def periodic_scene(name, Y, X):
    g = pc.scene_geometry(name, Y, X)
    mk = ops.SceneMasks(g.active, g.inflow, g.bc_mask, g.bc_mask, DEV, pressure_solver=pc.SCENES[name][4],
                        multi_launch=not ops.beyond_one_workgroup(Y, X), boundaries=pc.SCENES[name][0])
    return g, mk


@functools.lru_cache(maxsize=None)
def inputs2d(Y, X, seed=11):
    """device (d, vy, vx, re), cotangents (wy, wx, wd) and a right-hand side: the tables' generators, computed once, never modified"""
    st = tuple(f32(t) for t in state(B, Y, X, seed))
    wy, wx = (f32(t) for t in cotangent_at(B, Y, X))
    gen = torch.Generator().manual_seed(7)
    wd = f32(torch.randn(B, Y, X, generator=gen, dtype=torch.float64))
    return st, (wy, wx, wd), f32(step_like_rhs(B, Y, X))


def cfg2d(Y, X, g, mk):
    return ops.karman_cfg(B, Y, X, g.dx, masks=mk)


FWD_FORMS = {
    # name -> (grid, scene kind, solver, keywords of the step)
    "plain": (RAGGED, "default", "auto", {}),
    "cg_two_cylinders": (RAGGED, "two", "cg", {}),
    "direct_scattered": (RAGGED, "two", SC, {}),
    "buoyancy": (SMALL, "default", "auto", {"buoyancy": (0.3, 0.1)}),
    "mac_cormack": (SMALL, "default", "auto", {"advection": "mac_cormack", "correction_strength": 1.0}),
    "diffusion_substeps_5": (SMALL, "default", "auto", {"diffusion_substeps": 5}),
}


@pytest.mark.parametrize("form", list(FWD_FORMS))
def test_2d_large_forward_step_and_saved_step(monkeypatch, form):
    """karman_step_large and karman_step_saved; "plain" also with feat=, the CG scene also with p_guess (a fresh zero guess per call:
    the guess is state by contract, module docstring), mac_cormack under both k2d_mc_tile values"""
    (Y, X), kind, solver, kw = FWD_FORMS[form]
    g, mk = scene2d(Y, X, kind, solver, multi_launch=not ops.beyond_one_workgroup(Y, X))
    cfg = cfg2d(Y, X, g, mk)
    (d, vy, vx, re), _, _ = inputs2d(Y, X)

    def run():
        res = {}
        with torch.no_grad():
            info = {}
            res["step_large"] = (ops.karman_step_large(d, vy, vx, re, cfg, mk, info=info, **kw), info)
            info = {}
            res["step_saved"] = (ops.karman_step_saved(d, vy, vx, re, cfg, mk, info=info, **kw), info)
            if form == "plain":
                feat = ops.torch.empty(B, Y, X, 4, dtype=torch.float32, device=DEV)       # (the stand-in: an output handed in is poisoned too)
                res["feat"] = (ops.karman_step_large(d, vy, vx, re, cfg, mk, feat=feat, feat_scale=(5.0, 4.0, 1e-5)), feat)
            if solver == "cg":
                guess, info = torch.zeros(B, Y, X, dtype=torch.float32, device=DEV), {}
                res["p_guess"] = (ops.karman_step_large(d, vy, vx, re, cfg, mk, p_guess=guess, info=info), guess, info)
        return sync(res)

    if form == "mac_cormack":
        for tile in (0, 1):
            with options(k2d_mc_tile=tile):
                poison.check_patterns(monkeypatch, run, "%s k2d_mc_tile=%d" % (form, tile))
    else:
        poison.check_patterns(monkeypatch, run, form)


@pytest.mark.parametrize("name", ["A", "D", "E"])
def test_2d_periodic_forward_adjoint_and_seams(monkeypatch, name):
    """periodic-x (A), periodic-y (D, scattered blob across the seam) and both (E) at 40 x 24: the step, its velocity adjoint, and the
    in-place seam sync / fold on copies"""
    Y, X = SMALL
    g, mk = periodic_scene(name, Y, X)
    cfg = cfg2d(Y, X, g, mk)
    (d, vy, vx, re), (wy, wx, _), _ = inputs2d(Y, X)

    def run():
        res = {}
        with torch.no_grad():
            res["step_large"] = ops.karman_step_large(d, vy, vx, re, cfg, mk)
            outs, svy, svx = ops.karman_step_saved(d, vy, vx, re, cfg, mk)
            res["step_saved"] = (outs, svy, svx)
            res["bwd"] = ops.karman_step_large_bwd(svy, svx, re, wy, wx, cfg, mk)
            res["seam_sync"] = ops.karman_seam_sync(wy.clone(), wx.clone(), mk.periodic)
            res["seam_fold"] = ops.karman_seam_fold(wy.clone(), wx.clone(), mk.periodic)
        return sync(res)

    poison.check_patterns(monkeypatch, run, "periodic scene %s" % name)


@pytest.mark.parametrize("kind,solver", [("default", "auto"), ("two", "cg"), ("two", SC)], ids=["direct", "cg", "scattered"])
def test_2d_large_velocity_adjoints(monkeypatch, kind, solver):
    """karman_step_large_bwd, _bwd_re and _bwd_buoy at 130 x 65 under both k2d_adj_tile values"""
    Y, X = RAGGED
    g, mk = scene2d(Y, X, kind, solver)
    cfg = cfg2d(Y, X, g, mk)
    (d, vy, vx, re), (wy, wx, wd), _ = inputs2d(Y, X)
    with torch.no_grad():
        _, svy, svx = ops.karman_step_saved(d, vy, vx, re, cfg, mk)
        _, bvy, bvx = ops.karman_step_saved(d, vy, vx, re, cfg, mk, buoyancy=(0.3, 0.1))
    torch.cuda.synchronize()

    def run():
        res = {}
        with torch.no_grad():
            info = {}
            res["bwd"] = (ops.karman_step_large_bwd(svy, svx, re, wy, wx, cfg, mk, info=info), info)
            info = {}
            res["bwd_re"] = (ops.karman_step_large_bwd_re(svy, svx, re, wy, wx, vy, vx, cfg, mk, info=info), info)
            if kind == "default":
                res["bwd_buoy"] = ops.karman_step_large_bwd_buoy(d, bvy, bvx, re, wy, wx, wd, cfg, mk, (0.3, 0.1), vel_in=(vy, vx))
        return sync(res)

    for tile in (0, 1):
        with options(k2d_adj_tile=tile):
            poison.check_patterns(monkeypatch, run, "%s k2d_adj_tile=%d" % (solver, tile))


def test_2d_density_adjoint_advection_stage_and_substeps(monkeypatch):
    """karman_density_bwd(_re) under both k2d_dens_adj_tile values (semi-Lagrangian at 130 x 65, MacCormack at 40 x 24), karman_advect and
    karman_advect_bwd in both schemes and both scatter forms, karman_diffuse_sub in one launch and chunked, karman_correct"""
    Y, X = RAGGED
    g, mk = scene2d(Y, X)
    cfg = cfg2d(Y, X, g, mk)
    (d, vy, vx, re), (wy, wx, wd), _ = inputs2d(Y, X)
    sY, sX = SMALL
    sg, smk = scene2d(sY, sX, multi_launch=True)
    scfg = cfg2d(sY, sX, sg, smk)
    (sd, svy_, svx_, sre), (swy, swx, swd), _ = inputs2d(sY, sX)
    gen = torch.Generator().manual_seed(2)
    net_out = f32(torch.randn(B, Y, X, 2, generator=gen, dtype=torch.float64))

    def run():
        res = {}
        with torch.no_grad():
            res["density_bwd"] = ops.karman_density_bwd(d, vy, vx, re, wd, cfg, mk)
            res["density_bwd_re"] = ops.karman_density_bwd_re(d, vy, vx, re, wd, vy, vx, cfg, mk)
            res["density_bwd_accumulate"] = ops.karman_density_bwd(d, vy, vx, re, wd, cfg, mk, g_vy=wy.clone(), g_vx=wx.clone())
            res["density_bwd_mac"] = ops.karman_density_bwd(sd, svy_, svx_, sre, swd, scfg, smk, advection="mac_cormack")
            res["density_bwd_re_mac"] = ops.karman_density_bwd_re(sd, svy_, svx_, sre, swd, svy_, svx_, scfg, smk, advection="mac_cormack")
            for adv in ("semi_lagrangian", "mac_cormack"):
                res["advect_" + adv] = ops.karman_advect(d, vy, vx, cfg, mk.active, mk.inflow, advection=adv)
                for tile in (True, False):
                    res["advect_bwd_%s_%d" % (adv, tile)] = ops.karman_advect_bwd(d, vy, vx, cfg, mk.active, mk.inflow, wd, wy, wx, advection=adv, tile=tile)
            res["diffuse_sub"] = ops.karman_diffuse_sub(vy, vx, re, cfg, 5)
            res["diffuse_sub_chunk_2"] = ops.karman_diffuse_sub(vy, vx, re, cfg, 5, chunk=2)
            cy, cx, cor = vy.clone(), vx.clone(), (ops.torch.empty_like(vy), ops.torch.empty_like(vx))      # (cor: an output, through the stand-in)
            ops.karman_correct(net_out, cy, cx, (0.2, 0.25), cor)
            res["correct"] = (cy, cx, cor)
        return sync(res)

    for tile in (0, 1):
        with options(k2d_dens_adj_tile=tile):
            poison.check_patterns(monkeypatch, run, "k2d_dens_adj_tile=%d" % tile)


def test_2d_pressure_solves(monkeypatch):
    """karman_pressure_solve_large on a one-window blob and a CG scene at 130 x 65, the scattered blob, and the one-launch solve
    (multi_launch=True at 64 x 32)"""
    Y, X = RAGGED
    rhs = inputs2d(Y, X)[2]
    cases = {k: scene2d(Y, X, kind, s) for k, (kind, s) in {"direct": ("default", "auto"), "cg": ("two", "cg"), "scattered": ("two", SC)}.items()}
    g1, mk1 = scene2d(64, 32, multi_launch=True)
    assert int(mk1.direct_header[ops.DIRECT_HEADER_FLAGS]) & ops.DIRECT_ONE_WG
    rhs1 = inputs2d(64, 32)[2]

    def run():
        res = {}
        for k, (g, mk) in cases.items():
            info = {}
            res[k] = (ops.karman_pressure_solve_large(rhs, cfg2d(Y, X, g, mk), mk, info=info), info)
        res["one_launch"] = ops.karman_pressure_solve_large(rhs1, cfg2d(64, 32, g1, mk1), mk1)
        return sync(res)

    poison.check_patterns(monkeypatch, run, "pressure solve")


def test_2d_large_workspace_refilled_between_eager_calls(monkeypatch):
    """One caller-owned workspace across calls (what a data-generation loop does): forward direct and CG, both adjoints"""
    Y, X = RAGGED
    (d, vy, vx, re), (wy, wx, wd), _ = inputs2d(Y, X)
    for kind, solver in (("default", "auto"), ("two", "cg")):
        g, mk = scene2d(Y, X, kind, solver)
        cfg = cfg2d(Y, X, g, mk)
        n = max(ops.large_workspace_bytes(cfg, mk, saved=True), ops.large_bwd_workspace_bytes(cfg, mk, re=True), ops.density_bwd_workspace_bytes(cfg, re=True))
        ws = torch.zeros((n + 3) // 4, dtype=torch.float32, device=DEV)

        def call():
            with torch.no_grad():
                info = {}
                outs, svy, svx = ops.karman_step_saved(d, vy, vx, re, cfg, mk, workspace=ws, info=info)
                gv = ops.karman_step_large_bwd_re(svy, svx, re, wy, wx, vy, vx, cfg, mk, workspace=ws, info=info)
                gd = ops.karman_density_bwd(d, svy, svx, re, wd, cfg, mk, workspace=ws)
            return outs, svy, svx, gv, gd, info

        refill(call, lambda: [ws], "2-D large step, %s" % solver)


# =====================================================================================================================================
# one-workgroup 2-D
# =====================================================================================================================================
@pytest.mark.parametrize("Y,X,solver", [(32, 16, "cg"), (32, 16, "direct"), (64, 32, "cg"), (64, 32, "direct")])
def test_one_workgroup_step_forward_and_backward(monkeypatch, Y, X, solver):
    """ops.karman_step with its backward: plain, density_grad and re_grad"""
    g = o.geometry(Y, X)
    mk = ops.SceneMasks(g.active, g.inflow, g.bc_mask, g.bc_mask, DEV, pressure_solver="auto" if solver == "direct" else "cg")
    assert mk.pressure_solver == solver and not mk.large
    cfg = cfg2d(Y, X, g, mk)
    (d, vy, vx, re), (wy, wx, wd), _ = inputs2d(Y, X, k2s.SEEDS.get((Y, X), 77))

    def run():
        res = {}
        for mode, kw in (("plain", {}), ("density_grad", {"density_grad": True}), ("re_grad", {"re_grad": True, "density_grad": True})):
            leaves = [t.clone().requires_grad_(True) for t in (d, vy, vx, re)]
            info = {}
            out = ops.karman_step(*leaves, cfg, mk, info=info, **kw)
            loss = (out[1] * wy).sum() + (out[2] * wx).sum()
            if "density_grad" in kw:
                loss = loss + (out[0] * wd).sum()
            loss.backward()
            res[mode] = (tuple(t.detach() for t in out), tuple(t.grad for t in leaves), info)
        return sync(res)

    poison.check_patterns(monkeypatch, run, "%dx%d %s" % (Y, X, solver))


# =====================================================================================================================================
# Burgers
# =====================================================================================================================================
@pytest.mark.parametrize("Y,X", [(32, 32), (70, 36), (24, 100)])
def test_burgers_step_forward_and_adjoint(monkeypatch, Y, X):
    """32 x 32: the one-workgroup kernels; (70, 36) and (24, 100): sol_burgers_step_fwd_large / _bwd_large; with and without force"""
    dx, dt = 32.0 / Y, 0.1
    c = bs.inputs(Y, X, dx, dt, None)
    vy, vx, fy, fx, wy, wx = (f32(c[k]) for k in ("vy", "vx", "fy", "fx", "wy", "wx"))
    cfg, circ = _lib.BurgersCfg(B, Y, X, dx, dt), ops.burgers_circ(Y, X, dt * bs.NU)
    large = max(Y, X) > ops.BURGERS_LDS_MAX
    step = ops.burgers_step_large if large else ops.burgers_step

    def run():
        res = {}
        for force in (True, False):
            ay, ax = vy.clone().requires_grad_(True), vx.clone().requires_grad_(True)
            oy, ox = step(ay, ax, fy if force else None, fx if force else None, cfg, circ)
            ((oy * wy).sum() + (ox * wx).sum()).backward()
            res["force" if force else "no_force"] = (oy.detach(), ox.detach(), ay.grad, ax.grad)
        if large:
            with torch.no_grad():
                res["bwd_direct"] = ops.burgers_step_large_bwd(vy, vx, wy, wx, cfg, circ)
        return sync(res)

    poison.check_patterns(monkeypatch, run, "burgers %dx%d" % (Y, X))
    if large:
        ws = torch.zeros((ops.burgers_large_workspace_bytes(cfg) + 3) // 4, dtype=torch.float32, device=DEV)

        def call():
            with torch.no_grad():
                return ops.burgers_step_large(vy, vx, fy, fx, cfg, circ, ws), ops.burgers_step_large_bwd(vy, vx, wy, wx, cfg, circ, ws)
        refill(call, lambda: [ws], "burgers %dx%d" % (Y, X))


# =====================================================================================================================================
# 3-D
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def scene3d(cell, obstacle, solver="auto"):
    g = ks.geometry(cell, obstacle)
    return k3.Scene3D(*cell, device=DEV, active=g.active, inflow=g.inflow, pressure_solver=solver)


@functools.lru_cache(maxsize=None)
def periodic_scene3d(cell, obstacle):
    g = p3c.scene_geometry(tuple(cell), obstacle)
    return k3.Scene3D(*cell, device=DEV, active=g.active, inflow=g.inflow, velBCy=g.bc_mask, velBCyMask=g.bc_mask,
                      pressure_solver=p3c.SOLVER[obstacle], boundaries="periodic-z")


@functools.lru_cache(maxsize=None)
def inputs3d(cell):
    d, v, re = ks.state(B, cell)
    w, wd = ks.cotangent(B, cell)
    return [f32(d)] + [f32(t) for t in v] + [f32(re)], [f32(t) for t in w], f32(wd), f32(ks.step_like_rhs(B, cell))


def step3d_with_grads(sim, st, w, wd=None, re_leaf=False):
    leaves = [t.clone().requires_grad_(True) for t in st[:4]] + [st[4].clone().requires_grad_(re_leaf)]
    out = sim.step(*leaves)
    loss = sum((a * b).sum() for a, b in zip(out[1:], w))
    if wd is not None:
        loss = loss + (out[0] * wd).sum()
    loss.backward()
    return tuple(t.detach() for t in out), tuple(t.grad for t in leaves), dict(sim.solve_info)


FLOW3D = {
    # name -> (cell, scene, Karman3DFlow keywords, density cotangent?, re leaf?)
    "sphere_direct": ((22, 10, 12), lambda: scene3d((22, 10, 12), "sphere", "direct"), {}, False, False),
    "cylinder_cg": ((22, 10, 12), lambda: scene3d((22, 10, 12), "cylinder", "cg"), {}, False, False),
    "global_atomics_adjoint": ((24, 12, 72), lambda: scene3d((24, 12, 72), "sphere", "direct"), {}, False, False),
    "density_and_re_grad": ((22, 10, 12), lambda: scene3d((22, 10, 12), "sphere", "direct"), {"density_grad": True, "re_grad": True}, True, True),
    "buoyancy": ((16, 8, 8), lambda: scene3d((16, 8, 8), "cylinder", "auto"), {"buoyancy": (0.3, 0.1, 0.05)}, True, False),
    "mac_cormack": ((16, 8, 8), lambda: scene3d((16, 8, 8), "cylinder", "auto"), {"advection": "mac_cormack"}, False, False),
    "diffusion_substeps_3": ((16, 8, 8), lambda: scene3d((16, 8, 8), "cylinder", "auto"), {"diffusion_substeps": 3}, False, False),
    "direct_extruded": ((22, 10, 12), lambda: scene3d((22, 10, 12), "cylinder", "direct_extruded"), {}, False, False),
    "periodic_z_cylinder": ((22, 10, 12), lambda: periodic_scene3d((22, 10, 12), "cylinder"), {}, False, False),
    "periodic_z_empty": ((22, 10, 12), lambda: periodic_scene3d((22, 10, 12), "empty"), {}, False, False),
}


@pytest.mark.parametrize("form", list(FLOW3D))
def test_3d_step_forward_adjoint_and_solve(monkeypatch, form):
    """Karman3DFlow built under the pattern: the differentiable step with its backward (_fwd / _bwd, density_bwd and the re gradient
    where the form asks), the no-grad step with feat_out, pressure_solve; then the same object called again with its workspaces refilled"""
    cell, make_scene, kw, dens, re_leaf = FLOW3D[form]
    sc = make_scene()
    st, w, wd, rhs = inputs3d(cell)
    periodic = bool(sc.periodic_bits)

    def calls(sim):
        res = {"step_bwd": step3d_with_grads(sim, st, w, wd if dens else None, re_leaf)}
        with torch.no_grad():
            feat = k3.torch.empty(B, *cell, 4, dtype=torch.float32, device=DEV)       # (the stand-in under a pattern; refill(): uninitialised)
            res["step_feat"] = (sim.step(*st, feat_out=feat, feat_scale=(5.0, 4.0, 3.0, 1e-5)), feat)
            res["pressure_solve"] = (sim.pressure_solve(rhs), dict(sim.solve_info))
            if periodic:
                res["seam_sync3d"] = k3.seam_sync3d(sc, w[2].clone())
                res["seam_fold3d"] = k3.seam_fold3d(sc, w[2].clone())
        return sync(res)

    poison.check_patterns(monkeypatch, lambda: calls(k3.Karman3DFlow(sc, B, **kw)), form)
    sim = k3.Karman3DFlow(sc, B, **kw)
    refill(lambda: calls(sim), lambda: [sim.workspace, sim._sub_ws], form)


def test_3d_stages_alone(monkeypatch):
    """advect3d / advect3d_bwd (both schemes, both scatter forms), diffuse_sub (one and two substeps a launch), density_bwd as a direct
    call, at 22 x 10 x 12"""
    cell = (22, 10, 12)
    sc = scene3d(cell, "sphere", "direct")
    st, w, wd, _ = inputs3d(cell)
    d, v, re = st[0], st[1:4], st[4]

    def run():
        sim = k3.Karman3DFlow(sc, B)
        res = {}
        with torch.no_grad():
            for name, adv in (("sl", None), ("mac", 1.0)):
                res["advect3d_" + name] = k3.advect3d(sim, d, *v, adv=adv)
                for tile in (True, False):
                    res["advect3d_bwd_%s_%d" % (name, tile)] = k3.advect3d_bwd(sim, d, *v, wd, *w, adv=adv, tile_window=tile)
            res["diffuse_sub"] = k3.diffuse_sub(sim, *v, re, 3)
            res["diffuse_sub_chunk_2"] = k3.diffuse_sub(sim, *v, re, 3, chunk=2)
            res["density_bwd"] = k3.density_bwd(sim, d, v, re, wd)
            res["density_bwd_re"] = k3.density_bwd(sim, d, v, re, wd, vel_in=v)
        return sync(res)

    poison.check_patterns(monkeypatch, run, "3-D stages")


# =====================================================================================================================================
# networks, trainers, roll-outs
# =====================================================================================================================================
def batch2d(Y, X, ms, seed=31):
    d, vy, vx = (f32(t) for t in o.synthetic_state(B, Y, X, seed, project_it=False))
    re = f32(torch.tensor([o.RE_TRAIN[i % 6] for i in range(B)]))
    gts = [o.synthetic_state(B, Y, X, 600 + i, project_it=False) for i in range(ms)]
    return d, vy, vx, re, f32(torch.stack([s[1] for s in gts])), f32(torch.stack([s[2] for s in gts]))


def small_last_layer(net):
    with torch.no_grad():
        net.tensors()[-2].mul_(0.05)
    return net


def trainer_results(tr, net, batch, captured):
    """two fwd_bwd calls where captured (capture + replay, then a pure replay), one train_step, the weights after it"""
    res = {}
    for k in range(2 if captured else 1):
        tr.grads.zero_()
        loss = tr.fwd_bwd(*batch, want_final=True)
        res["run%d" % k] = poison.snapshot(sync({"loss": loss, "loss_steps": tr.loss_steps, "grads": tr.grads, "final": tuple(tr.final)}))
    tr.grads.zero_()
    res["train_step_loss"] = tr.train_step(*batch, lr=1e-4)
    res["weights"] = net.params.detach()
    return poison.snapshot(sync(res))


TRAINERS2D = {
    # name -> (Y, X, ms, captured)
    "sol_16x8": (16, 8, 2, False),
    "sol_16x8_captured": (16, 8, 2, True),
    "sol_128x64_band_split": (128, 64, 2, False),
    "graph_mercury_32x16": (32, 16, 2, True),
    "large_64x32_eager": (64, 32, 2, False),
    "large_64x32_captured": (64, 32, 2, True),
    "large_any_width_24x100": (24, 100, 2, False),
}


@pytest.mark.parametrize("name", list(TRAINERS2D))
def test_2d_trainers(monkeypatch, name):
    """SolTrainer (16 x 8; 128 x 64: the band-split forward launch), GraphTrainer with mercury, LargeGridTrainer (multi_launch at 64 x 32,
    eager and captured; any_width at 24 x 100), each built under the pattern: loss, per-step losses, flat gradient, final state, and the
    weights after one train_step"""
    Y, X, ms, captured = TRAINERS2D[name]
    batch = batch2d(Y, X, ms)
    g = o.geometry(Y, X)

    def run():
        if name.startswith("sol"):
            mk = ops.SceneMasks(g.active, g.inflow, g.bc_mask, g.bc_mask, DEV)
            net = small_last_layer(sol_amd.model_mars_moon(cin=3, cout=2, seed=0, device=DEV))
            tr = sol_amd.SolTrainer(net, mk, B, Y, X, ms, g.dx, (0.2, 0.25), o.STD_RE, use_graph=captured)
        elif name.startswith("graph"):
            net = small_last_layer(sol_amd.model_mercury(cin=3, cout=2, seed=0, device=DEV))
            tr = sol_amd.GraphTrainer(net, B, Y, X, ms, (0.2, 0.25), o.STD_RE, dx=g.dx)
        else:
            net = small_last_layer(sol_amd.model_mars_moon(cin=3, cout=2, seed=0, device=DEV))
            kw = {"any_width": True} if "any_width" in name else {"multi_launch": True}
            tr = sol_amd.LargeGridTrainer(net, B, Y, X, ms, (0.2, 0.25), o.STD_RE, dx=g.dx, use_graph=captured, **kw)
        return trainer_results(tr, net, batch, captured)

    poison.check_patterns(monkeypatch, run, name)


def test_2d_trainers_workspace_refilled_between_eager_calls(monkeypatch):
    """SolTrainer.workspace (16 x 8 and the band-split 128 x 64: the library zeroes what it needs zero itself) and LargeGridTrainer's
    _ws_fwd / _ws_bwd between two eager steps"""
    for Y, X in ((16, 8), (128, 64)):
        g = o.geometry(Y, X)
        mk = ops.SceneMasks(g.active, g.inflow, g.bc_mask, g.bc_mask, DEV)
        net = small_last_layer(sol_amd.model_mars_moon(cin=3, cout=2, seed=0, device=DEV))
        tr = sol_amd.SolTrainer(net, mk, B, Y, X, 2, g.dx, (0.2, 0.25), o.STD_RE, use_graph=False)
        batch = batch2d(Y, X, 2)

        def call():
            tr.grads.zero_()
            loss = tr.fwd_bwd(*batch, want_final=True)
            return loss, tr.loss_steps, tr.grads, tuple(tr.final)
        refill(call, lambda: [tr.workspace], "SolTrainer %dx%d" % (Y, X))
    Y, X = 64, 32
    g = o.geometry(Y, X)
    net = small_last_layer(sol_amd.model_mars_moon(cin=3, cout=2, seed=0, device=DEV))
    lt = sol_amd.LargeGridTrainer(net, B, Y, X, 2, (0.2, 0.25), o.STD_RE, dx=g.dx, use_graph=False, multi_launch=True, buoyancy=(0.3, 0.0))
    batch = batch2d(Y, X, 2)

    def call_large():
        loss = lt.fwd_bwd(*batch, want_final=True)
        return loss, lt.loss_steps, lt.grads, tuple(lt.final)
    refill(call_large, lambda: [lt._ws_fwd, lt._ws_bwd, getattr(lt, "_ws_bwd_d", None)], "LargeGridTrainer 64x32 buoyant")


ROLLOUTS2D = ["sol_16x8", "large_64x32_captured", "large_64x32_eager", "large_cg_cold", "large_cg_warm_start"]


@pytest.mark.parametrize("name", ROLLOUTS2D)
def test_2d_rollouts(monkeypatch, name):
    """SolRollout and LargeGridRollout (direct scene captured and eager; CG scene cold and with cg_warm_start), three steps; the eager
    ones again with their workspace refilled (a fresh object per refill would hide nothing: the warm-start guess is reset instead)"""
    Y, X = (16, 8) if name.startswith("sol") else (64, 32)
    g = o.geometry(Y, X)
    d, vy, vx, re = batch2d(Y, X, 1)[:4]
    cg = "cg" in name
    mk = ops.SceneMasks(g.active, g.inflow, g.bc_mask, g.bc_mask, DEV, multi_launch=not name.startswith("sol"), pressure_solver="cg" if cg else "auto")

    def build():
        net = small_last_layer(sol_amd.model_mars_moon(cin=3, cout=2, seed=0, device=DEV))
        if name.startswith("sol"):
            return sol_amd.SolRollout(net, mk, B, Y, X, g.dx, (0.2, 0.25), o.STD_RE)
        return sol_amd.LargeGridRollout(net, mk, B, Y, X, g.dx, (0.2, 0.25), o.STD_RE, multi_launch=True, use_graph="captured" in name,
                                        cg_warm_start="warm" in name)

    def roll(ro):
        if getattr(ro, "p_guess", None) is not None:
            ro.reset_guess()
        st = [t.clone() for t in (d, vy, vx)]
        iters = ro.run(*st, re, 3)
        return sync((st, iters, dict(getattr(ro, "solve_info", {}))))

    poison.check_patterns(monkeypatch, lambda: roll(build()), name)
    if "captured" not in name:
        ro = build()
        refill(lambda: roll(ro), lambda: [ro.workspace if name.startswith("sol") else ro._ws], name)


@pytest.mark.parametrize("Y,X,noforce", [(32, 32, False), (32, 32, True), (24, 128, False)])
def test_burgers_trainer_and_rollout(monkeypatch, Y, X, noforce):
    """BurgersTrainer (captured: two replays, then one train_step) and BurgersRollout (three steps, captured and eager) on a
    one-workgroup grid and on the large form.  On the large form also the workspace the simulator keeps per shape (BurgersTest._ws,
    burgers.py:40-47, which BurgersTrainer and BurgersRollout reserve at construction): an eager trainer and an eager roll-out are
    called again after every buffer of that dict was refilled."""
    ms, steps, dt, std_v, std_f = 2, 3, 0.1, (0.21, 0.19), (0.09, 0.11)
    gen = torch.Generator().manual_seed(3)
    sm = lambda *shape: o._smooth(torch.randn(*shape, generator=gen, dtype=torch.float64))
    velo = torch.stack([o.staggered_tensor(0.3 * sm(B, Y + 1, X), 0.3 * sm(B, Y, X + 1)) for _ in range(ms + 1)])
    forc = torch.stack([o.staggered_tensor(0.15 * sm(B, Y + 1, X), 0.15 * sm(B, Y, X + 1)) for _ in range(steps + 1)])
    dom = lambda: sol_amd.Domain([Y, X], box=sol_amd.box([Y, X]), boundaries=sol_amd.PERIODIC)
    new_net = lambda: sol_amd.model_mars_moon(cin=2 if noforce else 4, cout=2, seed=0)

    def roll(ro):
        ro.reset(velo[0])
        for i in range(steps):
            ro.step(forc[i], forc[i + 1])
        return poison.snapshot(sync((ro.vel, ro.corr)))

    def run():
        net = new_net()
        tr = sol_amd.BurgersTrainer(net, dom(), B, ms, dt, std_v, std_f, noforce=noforce)
        res = {}
        for k in range(2):
            loss = tr.fwd_bwd(velo, forc[:ms])
            res["run%d" % k] = poison.snapshot(sync((loss, net.params.grad)))
        res["train_step_loss"] = tr.train_step(velo, forc[:ms], 1e-4)
        res["weights"] = net.params.detach()
        for graph in (True, False):
            ro = sol_amd.BurgersRollout(new_net(), dom(), B, dt, std_v, std_f, noforce=noforce, use_graph=graph)
            res["rollout_%s" % ("captured" if graph else "eager")] = roll(ro)
        return poison.snapshot(sync(res))

    poison.check_patterns(monkeypatch, run, "burgers trainer %dx%d" % (Y, X))
    if max(Y, X) > ops.BURGERS_LDS_MAX:
        net = new_net()
        te = sol_amd.BurgersTrainer(net, dom(), B, ms, dt, std_v, std_f, noforce=noforce, use_graph=False)
        assert te.sim._ws

        def call():
            return te.fwd_bwd(velo, forc[:ms]), net.params.grad
        refill(call, lambda: list(te.sim._ws.values()), "BurgersTrainer %dx%d, eager" % (Y, X))
        ro = sol_amd.BurgersRollout(new_net(), dom(), B, dt, std_v, std_f, noforce=noforce, use_graph=False)
        assert ro.sim._ws
        refill(lambda: roll(ro), lambda: list(ro.sim._ws.values()), "BurgersRollout %dx%d, eager" % (Y, X))


TRAINERS3D = [("manual", False), ("manual", True), ("autograd", False), ("autograd", True)]


def batch3d(cell, ms):
    st = inputs3d(cell)[0]
    gts = [[f32(t) for t in o3.synthetic_state(B, *cell, 600 + i)[1]] for i in range(ms)]
    return st, gts


@pytest.mark.parametrize("schedule,captured", TRAINERS3D, ids=["%s_%s" % (s, "captured" if c else "eager") for s, c in TRAINERS3D])
def test_3d_trainer(monkeypatch, schedule, captured):
    """Karman3DTrainer at 16 x 8 x 8, ms = 2, both schedules, eager and captured (two replays), and one train_step"""
    cell, ms = (16, 8, 8), 2
    sc = scene3d(cell, "cylinder", "auto")
    st, gts = batch3d(cell, ms)

    def run():
        net = k3.MarsMoon3D(device=DEV)
        wts = net.get_weights()
        wts[22] = wts[22] * 0.05
        net.set_weights(wts)
        tr = k3.Karman3DTrainer(net, sc, B, ms, (0.2, 0.25, 0.3), o3.STD_RE, use_graph=captured, schedule=schedule)
        res = {}
        for k in range(2 if captured else 1):
            loss = tr.fwd_bwd(*st, gts)
            res["run%d" % k] = poison.snapshot(sync({"loss": loss, "loss_steps": tr.loss_steps, "grads": tr.grads, "final": tuple(tr.final)}))
        res["train_step_loss"] = tr.train_step(*st, gts, lr=1e-4)
        res["weights"] = net.params.detach()
        return poison.snapshot(sync(res))

    poison.check_patterns(monkeypatch, run, "Karman3DTrainer %s" % schedule)
    if not captured:            # the simulator's workspace between two eager steps
        net = k3.MarsMoon3D(device=DEV)
        tr = k3.Karman3DTrainer(net, sc, B, ms, (0.2, 0.25, 0.3), o3.STD_RE, schedule=schedule)

        def call():
            loss = tr.fwd_bwd(*st, gts)
            return loss, tr.loss_steps, tr.grads, tuple(tr.final)
        refill(call, lambda: [tr.sim.workspace], "Karman3DTrainer %s" % schedule)


def test_3d_network_at_row_width_4_and_rollout(monkeypatch):
    """The (1, 3, 16, 4) row of karman3d_net_shapes (Z = 4: sixteen rows of a plane share a tile; network only, the step needs
    Z >= 8): MarsMoon3D forward and backward, inputs drawn as karman3d_net_shapes.network_case draws them.  Then Karman3DRollout at
    16 x 8 x 8 for three steps, built under the pattern, and once more with the simulator's workspace and the feature buffer refilled
    between runs."""
    import karman3d_net_shapes as kn
    shape = (1, 3, 16, 4)
    assert shape in kn.CELLS
    gen = torch.Generator().manual_seed(21)
    x = torch.randn(*shape, 4, generator=gen, dtype=torch.float32).to(DEV)
    gy = (torch.randn(*shape, 3, generator=gen, dtype=torch.float32) * 1e-3).to(DEV)
    cell = (16, 8, 8)
    st = inputs3d(cell)[0]
    sc = scene3d(cell, "cylinder", "auto")

    def run():
        net = k3.MarsMoon3D(device=DEV)
        net.params.requires_grad_(True)
        xi = x.clone().requires_grad_(True)
        out = net(xi)
        (out * gy).sum().backward()
        res = {"network": poison.snapshot(sync((out.detach(), xi.grad, net.params.grad)))}
        ro = k3.Karman3DRollout(k3.MarsMoon3D(device=DEV), sc, B, (0.2, 0.25, 0.3), o3.STD_RE)
        with torch.no_grad():
            res["rollout"] = ro.run(*st, 3)
        return poison.snapshot(sync(res))

    poison.check_patterns(monkeypatch, run, "3-D network at Z = 4, roll-out")
    ro = k3.Karman3DRollout(k3.MarsMoon3D(device=DEV), sc, B, (0.2, 0.25, 0.3), o3.STD_RE)

    def call():
        with torch.no_grad():
            return ro.run(*st, 3)
    refill(call, lambda: [ro.sim.workspace, ro.feat], "Karman3DRollout 16x8x8")
