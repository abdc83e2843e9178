"""MacCormack advection of the large-grid karman-2d step, CPU side (no GPU needed): the reference of maccormack_cases.py against the oracle
(s = 0 is o.karman_step to float64 rounding), what the scheme is for (a Gaussian blob carried 100 steps keeps more than twice the peak),
the new C entry points' declarations, bindings, workspace sizes and argument checks (rejected before any launch), the refusals that need
no device, and the input condition of the GPU tests (test_gpu_karman2d_maccormack.py): how far the reference in float32 is from the
reference in float64 on every field and gradient those tests compare on the solver step.

Measured (reference float32 against float64, relative L2, worst over the three scenes, one step from seed 11 and two from seed 13):
  fields 2.3e-6 (also at CFL 2.5 / 6, at s = 0.5, with the force (0.3, -0.2) and with 2 diffusion substeps);
  gradients UNTRIMMED up to 4.1e-3 (144 x 72, two steps, g_vx): the limiter and the clamped edges tie exactly in places and fp32 decides a
  few entries the other way; with at most TRIM of the entries left out 1.8e-5 on the six step cases and <= 8.5e-6 on the others -- so every
  MacCormack gradient comparison uses the trimmed metric, the cap a condition;  g_re (2 substeps, 144 x 72) 2.4e-6, with the force 2.2e-6.
  The limiter reverts 4.4 - 10.5 % of the entries (2.3 - 3.9 % at s = 0.5): both branches are exercised; the step differs from the plain
  one by 5 - 8 % in v_x and 7 - 9 % in the density.
Pinned at about 2.5x those figures (maccormack_cases.FIELD_PIN / GRAD_PIN / RE_PIN), inside the GPU tolerances (1e-5 / 1e-4).
The stage-alone GPU tests run on seeded noise and are compared with float64 only: in float32 torch the reference's physical-coordinate
arithmetic ((x - u dt) / dx - 0.5 at |x| ~ 100) alone costs 1e-5 there, which index arithmetic (the kernels') does not pay."""
import ctypes as C
import os
import sys

import pytest
import torch

import sol_amd
import sol_oracle as o
from sol_amd import _lib, ops, trainer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buoyancy_cases as bc
import maccormack_cases as mc
from large2d_scenes import TOL_FIELD, TOL_GRAD, TRIM, rel, trimmed_rel

NEW = ("sol_karman_advect", "sol_karman_advect_bwd", "sol_karman_advect_workspace_bytes", "sol_karman_advect_bwd_workspace_bytes",
       "sol_karman_step_fwd_large_adv", "sol_karman_step_fwd_large_saved_adv", "sol_karman_step_bwd_large_adv",
       "sol_karman_step_bwd_large_adv_re", "sol_karman_density_bwd_adv", "sol_karman_density_bwd_adv_re",
       "sol_karman_step_fwd_large_adv_workspace_bytes_for", "sol_karman_step_fwd_large_saved_adv_workspace_bytes_for",
       "sol_karman_step_bwd_large_adv_workspace_bytes_for", "sol_karman_density_bwd_adv_workspace_bytes")
P = lambda v: C.c_void_p(v)


@pytest.fixture(scope="module")
def lib():
    return sol_amd.load()


# ---- the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(bc.SCENES))
def test_reference_at_zero_strength_is_the_oracle_step(name):
    g, order = bc.geometry_of(name), bc.SCENES[name][3]
    st = mc.start_state(name)
    with torch.no_grad():
        ref = o.karman_step(*st, g, inflow_order=order)
        got = mc.step(*st, g, s=0.0, inflow_order=order)
        sl = mc.step(*st, g, scheme="semi_lagrangian", inflow_order=order)
        moved = mc.step(*st, g, inflow_order=order)
    errs = [rel(a, b) for a, b in zip(got, ref)] + [rel(a, b) for a, b in zip(sl, ref)]
    print("s = 0 against o.karman_step, %s:" % name, errs)
    assert max(errs) < 1e-13
    # a silently ignored keyword cannot pass the GPU tests
    assert rel(moved[0], ref[0]) > 0.05 and rel(moved[2], ref[2]) > 0.03


def test_the_blob_keeps_more_than_twice_the_peak():
    """a Gaussian density blob (sigma = 3 cells) carried 100 steps by a uniform flow of (0.37, 0.21) cells per step, float64"""
    m, s = mc.blob_peak("mac_cormack"), mc.blob_peak("semi_lagrangian")
    print("blob peak after 100 steps: mac_cormack %.3f, semi_lagrangian %.3f" % (m, s))
    assert abs(m - 0.720) < 2e-3 and abs(s - 0.312) < 2e-3
    assert m > 2.0 * s


def test_the_stage_reference_semi_lagrangian_is_the_oracles_advection():
    Y, X = 40, 24
    g = mc.stage_geometry(Y, X)
    d, cy, cx = mc.stage_inputs(Y, X)[:3]
    a = mc.advect(d, cy, cx, 1.0, g.dx, scheme="semi_lagrangian")
    b = o.advect_mac(d, cy, cx, 1.0, g.dx)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- float32 against float64: the input condition of the GPU tests ------------------------------------------------------------------
# (name, s, kind, steps, force, n, re_grad, cfl): every reference the GPU tests of the solver step compare with
CASES = [(n, 1.0, k, 1, None, 1, False, None) for n in sorted(bc.SCENES) for k in ("vel", "dens", "both")]
CASES += [(n, 1.0, "both", 2, None, 1, False, None) for n in sorted(bc.SCENES)]
CASES += [("sphere_130", 0.5, "both", 1, None, 1, False, None), ("sphere_130", 1.0, "both", 1, None, 1, False, 2.5),
          ("sphere_130", 1.0, "both", 1, None, 1, False, 6.0), ("sphere_130", 1.0, "both", 1, mc.FORCE, 1, False, None),
          ("two_144", 1.0, "both", 1, None, mc.NSUB, True, None), ("two_144", 1.0, "both", 1, mc.FORCE, mc.NSUB, True, None)]


@pytest.mark.parametrize("name,s,kind,steps,force,n,re_grad,cfl", CASES)
def test_the_gpu_tests_inputs_in_float32_against_float64(name, s, kind, steps, force, n, re_grad, cfl):
    out64, g64, reverted = mc.reference(name, s, kind, steps, force, n, re_grad, cfl)
    out32, g32, _ = mc.reference(name, s, kind, steps, force, n, re_grad, cfl, dtype=torch.float32)
    ef = [rel(a, b) for a, b in zip(out32, out64)]
    eg = [rel(a, b) for a, b in zip(g32, g64)]
    trims = [trimmed_rel(a, b) for a, b in zip(g32[:3], g64[:3])]
    print("reference float32 vs float64 %s s=%s %s steps=%d F=%s n=%d re=%s cfl=%s: fields %s gradients %s trimmed %s reverted %s" % (
        name, s, kind, steps, force, n, re_grad, cfl, ["%.2e" % e for e in ef], ["%.2e" % e for e in eg], ["%.2e" % t[0] for t in trims],
        ["%.3f" % r for r in reverted]))
    assert mc.FIELD_PIN < TOL_FIELD and mc.GRAD_PIN < TOL_GRAD and mc.RE_PIN < TOL_GRAD
    assert max(ef) < mc.FIELD_PIN, ef
    assert all(t[1] <= int(TRIM * b.numel()) for t, b in zip(trims, g64))
    assert max(t[0] for t in trims) < mc.GRAD_PIN, (eg, trims)
    if re_grad:
        assert eg[3] < mc.RE_PIN, eg
    # both branches of the limiter are exercised
    assert all(0.02 <= r <= 0.2 for r in reverted), reverted


# ---- the Python surface: arguments ------------------------------------------------------------------------------------------------------
def test_advection_arguments():
    assert ops.ADVECTIONS == ("semi_lagrangian", "mac_cormack")
    assert ops.advection_arg() is None and ops.advection_arg("semi_lagrangian", 0.3) is None
    assert ops.advection_arg("mac_cormack") == 1.0 and ops.advection_arg("mac_cormack", 0.5) == 0.5 and ops.advection_arg("mac_cormack", 0) == 0.0
    for bad in ("maccormack", "MacCormack", None, 1):
        with pytest.raises(ValueError, match="must be one of"):
            ops.advection_arg(bad)
    for bad in (-0.01, 1.01, float("nan"), float("inf"), "1", None, True):
        for name in ops.ADVECTIONS:
            with pytest.raises(ValueError, match="correction_strength"):
                ops.advection_arg(name, bad)
    with pytest.raises(ValueError, match="must be one of"):
        sol_amd.KarmanFlow(advection="upwind")
    with pytest.raises(ValueError, match="correction_strength"):
        sol_amd.KarmanFlow(advection="mac_cormack", correction_strength=2.0)
    assert sol_amd.KarmanFlow(advection="mac_cormack", correction_strength=0.5)._adv == 0.5 and sol_amd.KarmanFlow()._adv is None


def test_the_one_workgroup_classes_refuse_mac_cormack_and_say_why():
    kw = dict(advection="mac_cormack")
    with pytest.raises(ValueError, match="SolTrainer: advection='mac_cormack' -- the mac_cormack advection is built on the multi-launch"):
        trainer.SolTrainer(None, None, 2, 64, 32, 2, 100.0 / 32, (1.0, 1.0), 1.0, **kw)
    with pytest.raises(ValueError, match="GraphTrainer: advection='mac_cormack'"):
        trainer.GraphTrainer(None, 2, 64, 32, 2, (1.0, 1.0), 1.0, **kw)
    with pytest.raises(ValueError, match="SolRollout: advection='mac_cormack'"):
        trainer.SolRollout(None, None, 2, 64, 32, 100.0 / 32, (1.0, 1.0), 1.0, **kw)
    with pytest.raises(ValueError, match="make_rollout: the mac_cormack advection is built on the multi-launch"):
        trainer.make_rollout(None, None, 2, 64, 32, 100.0 / 32, (1.0, 1.0), 1.0, **kw)
    # the default keyword passes the check (and fails later, on the missing network, like a call without it)
    assert trainer._refuse_advection("SolTrainer", "semi_lagrangian", 0.5) is None
    with pytest.raises(ValueError, match="correction_strength"):
        trainer._refuse_advection("SolTrainer", "semi_lagrangian", 1.5)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def cfg2d(Y=130, X=65, B=2, **kw):
    c = _lib.KarmanCfg(B, Y, X, 100.0 / X, 1.0, float(X), 1e-6, 1e-9, 2000, 0, 0, 0, None, 0, None)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_new_symbols_are_declared_exported_and_bound(lib):
    assert lib.sol_version() == _lib.ABI_VERSION          # additions only: the ABI number stays
    decl = _lib.declared_symbols()
    for name in NEW:
        assert name in decl and name in _lib._SIGS and hasattr(lib, name), name
    # the _adv forms take the _buoy forms' arguments and two more
    for adv, base in (("sol_karman_step_fwd_large_adv", "sol_karman_step_fwd_large_buoy"),
                      ("sol_karman_step_fwd_large_saved_adv", "sol_karman_step_fwd_large_saved_buoy"),
                      ("sol_karman_step_bwd_large_adv", "sol_karman_step_bwd_large_buoy"),
                      ("sol_karman_step_bwd_large_adv_re", "sol_karman_step_bwd_large_buoy_re"),
                      ("sol_karman_density_bwd_adv", "sol_karman_density_bwd"), ("sol_karman_density_bwd_adv_re", "sol_karman_density_bwd_re")):
        assert _lib._SIGS[adv][1] == _lib._SIGS[base][1] + [C.c_int32, C.c_float], adv
    assert "karman_maccormack.hip" in sol_amd._build.SOURCES and "karman_maccormack.hip" not in sol_amd._build.EXTRA      # the default flags
    assert _lib.get_option("k2d_mc_tile") == 1
    _lib.set_option("k2d_mc_tile", 0)
    try:
        assert _lib.get_option("k2d_mc_tile") == 0
    finally:
        _lib.set_option("k2d_mc_tile", 1)
    with pytest.raises(sol_amd.SolError):
        _lib.set_option("k2d_mc_tile", 2)


@pytest.mark.parametrize("Y,X", [(16, 16), (130, 65), (256, 128)])
def test_workspace_sizes(lib, Y, X):
    """advection = 0 is the plain size, byte for byte; advection = 1 holds at least the plain part and the arrays the kernels carve"""
    c = cfg2d(Y, X, 3)
    r = C.byref(c)
    N, faces, B = Y * X, (Y + 1) * X + Y * (X + 1), 3
    plain_fwd = lib.sol_karman_step_large_cg_workspace_bytes(r)            # cfg.direct NULL: the CG layout
    plain_bwd, plain_bwd_re = lib.sol_karman_step_bwd_large_workspace_bytes_for(r, None), lib.sol_karman_step_bwd_large_re_workspace_bytes_for(r, None)
    plain_d, plain_d_re = lib.sol_karman_density_bwd_workspace_bytes(r), lib.sol_karman_density_bwd_re_workspace_bytes(r)
    assert lib.sol_karman_step_fwd_large_adv_workspace_bytes_for(r, None, 0) == plain_fwd
    assert lib.sol_karman_step_bwd_large_adv_workspace_bytes_for(r, None, 0, 0) == plain_bwd
    assert lib.sol_karman_step_bwd_large_adv_workspace_bytes_for(r, None, 1, 0) == plain_bwd_re
    assert lib.sol_karman_density_bwd_adv_workspace_bytes(r, 0, 0) == plain_d and lib.sol_karman_density_bwd_adv_workspace_bytes(r, 1, 0) == plain_d_re
    h, gh = 4 * B * (faces + N), 8 * B * (faces + N)
    assert lib.sol_karman_advect_workspace_bytes(r, 0) == 0 and h <= lib.sol_karman_advect_workspace_bytes(r, 1) < h + 4 * 256
    assert plain_fwd + h <= lib.sol_karman_step_fwd_large_adv_workspace_bytes_for(r, None, 1) < plain_fwd + h + 4 * 256
    assert 0 < lib.sol_karman_step_fwd_large_saved_adv_workspace_bytes_for(r, None, 0) < lib.sol_karman_step_fwd_large_saved_adv_workspace_bytes_for(r, None, 1)
    for re in (0, 1):
        assert (plain_bwd_re if re else plain_bwd) + h + gh <= lib.sol_karman_step_bwd_large_adv_workspace_bytes_for(r, None, re, 1)
        assert (plain_d_re if re else plain_d) + h + gh <= lib.sol_karman_density_bwd_adv_workspace_bytes(r, re, 1)
    assert lib.sol_karman_advect_bwd_workspace_bytes(r) >= h + gh + 8 * B * (faces + N)
    assert lib.sol_karman_advect_bwd_workspace_bytes(C.byref(cfg2d(8, 8))) == 0 and lib.sol_karman_advect_workspace_bytes(C.byref(cfg2d(8, 8)), 1) == 0


def test_bad_arguments_are_rejected_before_any_launch(lib):
    """fake device pointers: never dereferenced, every case fails validation first"""
    q = [P(4096 * (k + 1)) for k in range(40)]
    c = cfg2d()
    r = C.byref(c)
    big = 1 << 30
    adv = lambda *tail, cfg=r, ptrs=None: lib.sol_karman_advect(cfg, None, *(ptrs or q[:5]), *tail)
    assert adv(2, 1.0, q[5], q[6], q[7], q[8], big) == -1 and b"advection must be 0" in lib.sol_last_error()
    for s in (-0.1, 1.5, float("nan"), float("inf")):
        for a in (0, 1):
            assert adv(a, s, q[5], q[6], q[7], q[8], big) == -1 and b"correction_strength must lie in [0, 1]" in lib.sol_last_error()
    assert adv(1, 1.0, q[5], q[6], q[7], q[8], big, cfg=C.byref(cfg2d(8, 8))) == -1 and b"Y, X >= 16" in lib.sol_last_error()
    assert adv(1, 1.0, q[5], q[6], None, q[8], big) == -1 and b"NULL pointer" in lib.sol_last_error()
    assert adv(1, 1.0, q[0], q[6], q[7], q[8], big) == -1 and b"alias" in lib.sol_last_error()
    assert adv(1, 1.0, q[5], q[6], q[6], q[8], big) == -1 and b"buffers of their own" in lib.sol_last_error()
    assert adv(1, 1.0, q[5], q[6], q[7], None, 0) == -1 and b"needs a workspace" in lib.sol_last_error()
    assert adv(1, 1.0, q[5], q[6], q[7], q[8], 64) == -1 and b"workspace too small" in lib.sol_last_error()
    bwd = lambda a, s, tile, ws, n, outs=(q[8], q[9], q[10]): lib.sol_karman_advect_bwd(r, None, *q[:5], a, s, q[5], q[6], q[7], *outs, tile, ws, n)
    assert bwd(3, 1.0, 1, q[11], big) == -1 and b"advection must be 0" in lib.sol_last_error()
    assert bwd(1, 2.0, 1, q[11], big) == -1 and b"correction_strength" in lib.sol_last_error()
    assert bwd(1, 1.0, 2, q[11], big) == -1 and b"tile_window" in lib.sol_last_error()
    assert bwd(1, 1.0, 1, None, big) == -1 and b"NULL pointer" in lib.sol_last_error()
    assert bwd(1, 1.0, 1, q[11], 64) == -1 and b"workspace too small" in lib.sol_last_error()
    assert bwd(1, 1.0, 1, q[11], big, (q[8], q[8], q[10])) == -1 and b"buffers of their own" in lib.sol_last_error()
    assert bwd(1, 1.0, 1, q[11], big, (q[5], q[9], q[10])) == -1 and b"alias" in lib.sol_last_error()
    # the step's _adv forms check the two new arguments before they touch a solver blob
    head = [r, None] + q[:8] + [0] + q[8:11]
    fwd = lambda a, s: lib.sol_karman_step_fwd_large_adv(*head, None, None, None, q[11], q[12], q[13], None, q[14], big, 0.0, 0.0, a, s)
    assert fwd(7, 1.0) == -1 and b"sol_karman_step_fwd_large_adv: advection must be 0" in lib.sol_last_error()
    assert fwd(1, -1.0) == -1 and b"correction_strength" in lib.sol_last_error()
    sav = lambda a, s: lib.sol_karman_step_fwd_large_saved_adv(*head, q[15], q[16], None, q[11], q[12], q[13], q[14], big, 0.0, 0.0, a, s)
    assert sav(2, 1.0) == -1 and b"advection must be 0" in lib.sol_last_error()
    bh = [r, None] + q[:5] + [0] + q[5:9] + [None, q[11], q[12], q[13], q[14], big]
    assert lib.sol_karman_step_bwd_large_adv(*bh, 0.0, 0.0, None, q[15], 2, 1.0) == -1 and b"advection must be 0" in lib.sol_last_error()
    assert lib.sol_karman_step_bwd_large_adv_re(*bh, q[16], q[17], q[18], 0, 0.0, 0.0, None, q[15], 1, 3.0) == -1 and b"correction_strength" in lib.sol_last_error()
    dh = [r, None] + q[:6] + [0] + q[6:10] + [0, q[10], big]
    assert lib.sol_karman_density_bwd_adv(*dh, 2, 1.0) == -1 and b"advection must be 0" in lib.sol_last_error()
    assert lib.sol_karman_density_bwd_adv_re(*dh, q[16], q[17], q[18], 0, 1, float("nan")) == -1 and b"correction_strength" in lib.sol_last_error()
    assert lib.sol_karman_density_bwd_adv(C.byref(cfg2d(8, 8)), *dh[1:], 1, 1.0) == -1 and b"Y, X >= 16" in lib.sol_last_error()
    assert lib.sol_karman_density_bwd_adv(*dh[:-1], 64, 1, 1.0) == -1 and b"workspace too small" in lib.sol_last_error()
