"""Buoyancy of the large-grid karman-2d step, CPU side (no GPU needed): the reference of buoyancy_cases.py against the oracle (F = 0 is
o.karman_step exactly), the adjoint COMPOSITION the library runs against the reference's autograd, the new C entry points' declarations,
bindings and argument checks (rejected before any launch), the refusals that need no device, and the input condition of the GPU tests
(test_gpu_karman2d_buoyancy.py): how far the reference in float32 is from the reference in float64 on every field and gradient those
tests compare.

Measured (reference float32 against float64, relative L2, worst over the forces (0.981, 0) and (0.3, -0.2) and the three scenes):
  fields 1.8e-6;  one step from seed 11: gradients of a density-only loss 7.5e-6 untrimmed, with a velocity cotangent 9.6e-5 untrimmed
  (g_vx at 130 x 65: a few faces of the velocity's own advection, force or no force) and 7.5e-6 trimmed, g_re 2.7e-5;  two chained steps
  from seed 13: 7.7e-6 untrimmed (seed 11 flips a cell of the second step under the force (0.981, 0): 8e-4, trimmed 3e-4 -- hence the
  other seed, buoyancy_cases.CHAIN_SEED).
Pinned at about 2.5x those figures (buoyancy_cases.FIELD_PIN / GRAD_PIN / RE_PIN), far inside the GPU tolerances (1e-5 / 1e-4): a moved
oracle default fails here first and the GPU tests' inputs are re-examined rather than silently trimmed."""
import ctypes as C
import os
import sys

import pytest
import torch

import sol_amd
import sol_oracle as o
from sol_amd import _lib, karman, ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buoyancy_cases as bc
from large2d_scenes import TOL_FIELD, TOL_GRAD, TRIM, rel, trimmed_rel

NEW = ("sol_karman_step_fwd_large_saved_buoy", "sol_karman_step_fwd_large_buoy", "sol_karman_step_bwd_large_buoy",
       "sol_karman_step_bwd_large_buoy_re", "sol_karman_buoyancy_add", "sol_karman_buoyancy_add_bwd")
P = lambda v: C.c_void_p(v)


@pytest.fixture(scope="module")
def lib():
    return sol_amd.load()


# ---- the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(bc.SCENES))
def test_reference_without_a_force_is_the_oracle_step(name):
    g, order = bc.geometry_of(name), bc.SCENES[name][3]
    d, vy, vx, re = bc.start_state(name)
    with torch.no_grad():
        ref = o.karman_step(d, vy, vx, re, g, inflow_order=order)
        got = bc.buoyant_step(d, vy, vx, re, g, (0.0, 0.0), inflow_order=order)
        moved = bc.buoyant_step(d, vy, vx, re, g, bc.FORCES[0], inflow_order=order)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    # a silently ignored force cannot pass the GPU tests: it moves v_y by tens of per cent on these inputs
    assert torch.equal(moved[0], ref[0]) and rel(moved[1], ref[1]) > 0.1


@pytest.mark.parametrize("Y,X", [(32, 16), (130, 65)])
@pytest.mark.parametrize("force", bc.FORCES)
def test_the_adjoint_composition_equals_the_references_autograd(Y, X, force):
    """g_a -> g_dsum = g_d_out + dt F . transpose -> today's velocity and density adjoints, against autograd through the buoyant step"""
    from density_adjoint_cases import w_dens
    from large2d_scenes import cotangent_at, state
    g = o.KarmanGeometry(Y, X)
    d, vy, vx, re = state(2, Y, X, bc.SEED, g)
    wy, wx = cotangent_at(2, Y, X)
    wd = w_dens(2, Y, X, g)
    leaves = [t.clone().requires_grad_(True) for t in (d, vy, vx)]
    out = bc.buoyant_step(*leaves, re, g, force)
    ((out[0] * wd).sum() + (out[1] * wy).sum() + (out[2] * wx).sum()).backward()
    got = bc.composed_adjoint(d, vy, vx, re, g, force, wd, wy, wx)
    errs = [rel(a, b.grad) for a, b in zip(got, leaves)]
    print("composition against autograd, %dx%d F=%s:" % (Y, X, force), errs)
    assert max(errs) < 1e-12, errs
    assert float(leaves[0].grad.abs().max()) > 0


# ---- float32 against float64: the input condition of the GPU tests ------------------------------------------------------------------
# A gradient that needs the trimmed metric (at most TRIM of its entries left out, as the large-grid adjoint tests apply it) is marked by
# buoyancy_cases.needs_trim, here and in the GPU test alike.
CASES = [(n, f, k, 1, False) for n in sorted(bc.SCENES) for f in bc.FORCES for k in ("vel", "dens", "both")]
CASES += [("sphere_130", f, "both", 1, True) for f in bc.FORCES] + [("sphere_130", f, "both", 2, False) for f in bc.FORCES]
CASES += [("two_144", bc.FORCES[0], "both", 1, True)]


@pytest.mark.parametrize("name,force,kind,steps,re_grad", CASES)
def test_the_gpu_tests_inputs_in_float32_against_float64(name, force, kind, steps, re_grad):
    out64, g64 = bc.reference(name, force, kind, steps, re_grad)
    out32, g32 = bc.reference(name, force, kind, steps, re_grad, dtype=torch.float32)
    ef = [rel(a, b) for a, b in zip(out32, out64)]
    eg = [rel(a, b) for a, b in zip(g32, g64)]
    trims = [trimmed_rel(a, b) for a, b in zip(g32, g64)]
    et = [t[0] for t in trims]
    assert all(t[1] <= int(TRIM * b.numel()) for t, b in zip(trims, g64))
    print("reference float32 vs float64 %s F=%s %s steps=%d re=%s: fields %s gradients %s trimmed %s" % (
        name, force, kind, steps, re_grad, ["%.2e" % e for e in ef], ["%.2e" % e for e in eg], ["%.2e" % e for e in et]))
    assert max(ef) < bc.FIELD_PIN < TOL_FIELD, ef
    assert bc.GRAD_PIN < bc.RE_PIN < TOL_GRAD
    assert max(et[:3]) < bc.GRAD_PIN, (eg, et)
    if not bc.needs_trim(kind, steps):
        assert max(eg[:3]) < bc.GRAD_PIN, eg
    if re_grad:
        assert eg[3] < bc.RE_PIN, eg
    # with a force the density gradient of a velocity-only loss is there and is large
    if kind == "vel":
        assert float(g64[0].abs().max()) > 0


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
    assert "karman_buoyancy.hip" in sol_amd._build.SOURCES and "karman_buoyancy.hip" not in sol_amd._build.EXTRA


def test_bad_arguments_are_rejected_before_any_launch(lib):
    """fake device pointers: never dereferenced, every case fails validation first"""
    one = [P(4096 * (k + 1)) for k in range(32)]
    # the stand-alone pair
    assert lib.sol_karman_buoyancy_add(None, 0, 8, 8, one[0], one[1], 1.0, 0.0, one[2], one[3]) == -1 and b"B in [1, 65535]" in lib.sol_last_error()
    assert lib.sol_karman_buoyancy_add(None, 1, 8, 8, one[0], None, 1.0, 0.0, one[2], one[3]) == -1 and b"NULL pointer" in lib.sol_last_error()
    assert lib.sol_karman_buoyancy_add(None, 1, 8, 8, one[0], one[1], 1.0, 0.0, one[2], one[2]) == -1 and b"alias" in lib.sol_last_error()
    assert lib.sol_karman_buoyancy_add_bwd(None, 1, 8, 8, one[0], one[1], one[2], 1.0, 0.0, None, None) == -1 and b"NULL pointer" in lib.sol_last_error()
    assert lib.sol_karman_buoyancy_add_bwd(None, 1, 8, 8, one[0], one[1], one[2], 1.0, 0.0, one[3], one[3]) == -1 and b"alias" in lib.sol_last_error()
    assert lib.sol_karman_buoyancy_add_bwd(None, 1, 1 << 15, 1 << 15, one[0], one[1], one[2], 1.0, 0.0, None, one[3]) == -1
    assert b"grid too large" in lib.sol_last_error()
    # the forward step: a force needs the density; the force must be finite (checked after the plain call's own checks)
    c = cfg2d(direct_n=1 << 20, direct=4096 * 40)
    hdr = (C.c_int32 * 16)(0x46443032, 130, 65, 25, 25, 177, 192, 16)
    head = [C.byref(c), None] + one[0:8] + [0]
    ws = 1 << 40
    rc = lib.sol_karman_step_fwd_large_saved_buoy(*head, None, one[9], one[10], one[11], one[12], hdr, None, None, None, one[13], ws, 1.0, 0.0)
    assert rc == -1 and b"needs d_in, inflow and d_out" in lib.sol_last_error(), lib.sol_last_error()
    rc = lib.sol_karman_step_fwd_large_saved_buoy(*head, one[8], one[9], one[10], one[11], one[12], hdr, None, None, None, one[13], ws, float("nan"), 0.0)
    assert rc == -1 and b"finite" in lib.sol_last_error(), lib.sol_last_error()
    rc = lib.sol_karman_step_fwd_large_buoy(*head, None, one[9], one[10], None, None, hdr, None, None, None, None, one[13], ws, 0.0, 2.0)
    assert rc == -1 and b"needs d_in, inflow and d_out" in lib.sol_last_error(), lib.sol_last_error()
    rc = lib.sol_karman_step_fwd_large_buoy(*head, one[8], one[9], one[10], None, None, hdr, None, None, None, one[14], one[13], ws, 0.0, 2.0)
    assert rc == -1 and b"p_inout" in lib.sol_last_error(), lib.sol_last_error()
    # the adjoint: g_dsum is required and a buffer of its own
    bhead = [C.byref(c), None] + one[0:5] + [0] + one[5:9] + [hdr, None, None, None, one[13], ws]
    rc = lib.sol_karman_step_bwd_large_buoy(*bhead, 1.0, 0.0, None, None)
    assert rc == -1 and b"g_dsum" in lib.sol_last_error(), lib.sol_last_error()
    rc = lib.sol_karman_step_bwd_large_buoy(*bhead, 1.0, 0.0, None, one[7])             # = g_vy_in
    assert rc == -1 and b"g_dsum must be a buffer of its own" in lib.sol_last_error(), lib.sol_last_error()
    rc = lib.sol_karman_step_bwd_large_buoy(*bhead, 1.0, 0.0, one[20], one[20])          # g_d_out = g_dsum
    assert rc == -1 and b"alias" in lib.sol_last_error(), lib.sol_last_error()
    rc = lib.sol_karman_step_bwd_large_buoy(*bhead, float("inf"), 0.0, None, one[20])
    assert rc == -1 and b"finite" in lib.sol_last_error(), lib.sol_last_error()
    rc = lib.sol_karman_step_bwd_large_buoy_re(*bhead, one[21], one[22], None, 0, 1.0, 0.0, None, one[20])
    assert rc == -1 and b"NULL pointer" in lib.sol_last_error(), lib.sol_last_error()


# ---- Python surface without a device ----------------------------------------------------------------------------------------------
def test_force_spellings_and_defaults():
    assert ops.buoyancy_force() is None
    assert ops.buoyancy_force((0.3, -0.2)) == (0.3, -0.2) and ops.buoyancy_force(0.5) == (0.5, 0.0)
    f = ops.buoyancy_force(buoyancy_factor=0.1)
    assert abs(f[0] - 0.981) < 1e-12 and f[1] == 0.0                      # PhiFlow: -gravity * buoyancy_factor, Gravity() = -9.81 along y
    assert ops.buoyancy_force(buoyancy_factor=2.0, gravity=(0.0, -1.0)) == (0.0, 2.0)
    for bad in (dict(buoyancy=(1.0, 2.0, 3.0)), dict(buoyancy=(float("nan"), 0.0)), dict(buoyancy=1.0, buoyancy_factor=1.0)):
        with pytest.raises(ValueError):
            ops.buoyancy_force(**bad)
    assert karman.KarmanFlow()._buoyancy is None and karman.KarmanFlow(buoyancy=(0.0, 0.0))._buoyancy is None
    assert karman.KarmanFlow(buoyancy_factor=0.1, gravity=(-9.81, 0.0))._buoyancy == ops.buoyancy_force(buoyancy_factor=0.1)
    assert karman.KarmanFlow(buoyancy=(0.3, -0.2))._buoyancy == (0.3, -0.2)


def test_the_one_workgroup_trainers_refuse_a_force_at_construction():
    net = sol_amd.model_mars_moon(cin=3, cout=2, seed=0, device="cpu")
    with pytest.raises(ValueError, match="buoyancy"):
        sol_amd.SolTrainer(net, None, 1, 64, 32, 2, 100.0 / 32, (0.2, 0.2), o.STD_RE, buoyancy=(0.981, 0.0))
    with pytest.raises(ValueError, match="buoyancy"):
        sol_amd.GraphTrainer(net, 1, 64, 32, 2, (0.2, 0.2), o.STD_RE, buoyancy=(0.0, 0.5))
    with pytest.raises(ValueError, match="buoyancy"):
        sol_amd.make_trainer(net, None, 1, 64, 32, 2, 100.0 / 32, (0.2, 0.2), o.STD_RE, buoyancy=(0.981, 0.0))
    with pytest.raises(ValueError, match="buoyancy"):
        sol_amd.make_rollout(net, None, 1, 64, 32, 100.0 / 32, (0.2, 0.2), o.STD_RE, buoyancy=(0.981, 0.0))


def test_the_scripts_buoyancy_flag():
    import argparse
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    sys.path.insert(0, sdir)
    import _common
    p = argparse.ArgumentParser()
    _common.add_buoyancy_arg(p)
    parse = lambda *a: _common.buoyancy_from_args(vars(p.parse_args(list(a))))
    assert parse() is None and parse("--buoyancy", "0.981") == (0.981, 0.0) and parse("--buoyancy", "0.3,-0.2") == (0.3, -0.2)
    for bad in ("a", "1,2,3", "nan"):
        with pytest.raises(SystemExit):
            parse("--buoyancy", bad)
    assert _common.agreed_buoyancy((0.3, -0.2), None, "set") == (0.3, -0.2) and _common.agreed_buoyancy(None, None, "set") is None
    assert _common.agreed_buoyancy(None, (0.0, 0.0), "set") is None                 # an explicit zero agrees with "off"
    with pytest.raises(SystemExit, match="contradicts"):
        _common.agreed_buoyancy(None, (0.3, 0.0), "set")
