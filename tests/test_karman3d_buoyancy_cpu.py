"""Buoyancy of the karman-3d step, CPU side (no GPU needed): the reference of buoyancy3d_cases.py against the oracle (F = 0 is
o.karman3d_step exactly), the transpose identity of the reference's term, the adjoint COMPOSITION the library runs against the reference's
autograd, the new C entry points' declarations, bindings, arity and argument checks (rejected before any launch), the force spellings and
the script flag, and the input condition of the GPU tests (test_gpu_karman3d_buoyancy.py): how far the reference in float32 is from the
reference in float64 on every field and gradient those tests compare.

Measured (reference float32 against float64, max |a - b| / max |b|, untrimmed, worst over the forces (0.981, 0, 0) and (0.3, -0.2, 0.15)):
  fields            1.11e-6 (d_out of 32_x35; the 16 x 8 x 8 cases and 20_comb stay below 8.5e-7)
  g_d, g_v*         3.7e-6  (g_vy of 32_x35, two steps, density-only loss; 16_comb stays below 1.6e-6)
  g_re              1.46e-5 (32_x35, two steps, density-only loss, force (0.981, 0, 0); every other case below 4.3e-6)
over one and two chained steps and the three kinds of loss.  Pinned at about 2.5x those figures (buoyancy3d_cases.FIELD_PIN / GRAD_PIN /
RE_PIN); the GPU tests allow buoyancy3d_cases.MARGIN times the pin.  A moved oracle default fails here first and the GPU tests' inputs
are re-examined rather than silently trimmed."""
import ctypes as C
import os
import re as regex
import sys

import numpy as np
import pytest
import torch

import sol_amd
import sol_oracle3d as o
from sol_amd import _lib
from sol_amd import karman3d as k3

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buoyancy3d_cases as bc
import karman3d_adjoint_cases as kc

# name -> number of parameters: the plain sibling's, then fy, fx, fz (and g_d_out, g_dsum)
NEW = {"sol_karman3d_step_fwd_buoy": 24 + 3, "sol_karman3d_step_bwd_buoy": 18 + 5, "sol_karman3d_step_bwd_buoy_re": 23 + 5,
       "sol_karman3d_buoyancy_add": 13, "sol_karman3d_buoyancy_add_bwd": 14}
PLAIN = {"sol_karman3d_step_fwd_buoy": "sol_karman3d_step_fwd", "sol_karman3d_step_bwd_buoy": "sol_karman3d_step_bwd",
         "sol_karman3d_step_bwd_buoy_re": "sol_karman3d_step_bwd_re"}
P = lambda v: C.c_void_p(v)
FD3_MAGIC = 0x46443333


@pytest.fixture(scope="module")
def lib():
    return sol_amd.load()


# ---- the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.FORWARD_CASES)
def test_reference_without_a_force_is_the_oracle_step(name):
    d, v, re = kc.state(name)
    with torch.no_grad():
        ref = kc.step(d, v, re, name)
        got = bc.step_of(name, (0.0, 0.0, 0.0))(d, v, re)
        moved = bc.step_of(name, bc.FORCES[1])(d, v, re)
    assert torch.equal(got[0], ref[0]) and all(torch.equal(a, b) for a, b in zip(got[1], ref[1]))
    # a silently ignored force, or component, cannot pass the GPU tests: each one moves its component by per cents on these inputs
    assert torch.equal(moved[0], ref[0])
    for c in range(3):
        assert bc.maxrel(moved[1][c], ref[1][c]) > 1e-2, (name, c)


def test_face_masks_helper_is_the_oracles():
    g = o.geometry(16, 8, 8)
    for a, b in zip(bc.face_masks(np.asarray(g.active)), g.masks):
        assert np.array_equal(a, np.asarray(b))


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 3, 5, 7), (2, 16, 8, 8)])
def test_the_term_and_its_transpose(shape):
    """<add(d), w> = <d, add^T(w)> in float64 on a mask with an obstacle touching two walls"""
    B, Y, X, Z = shape
    masks = bc.face_masks(bc.wall_mask(Y, X, Z))
    gen = torch.Generator().manual_seed(5)
    d = torch.randn(B, Y, X, Z, generator=gen, dtype=torch.float64)
    w = tuple(torch.randn(s, generator=gen, dtype=torch.float64) for s in ((B, Y + 1, X, Z), (B, Y, X + 1, Z), (B, Y, X, Z + 1)))
    f = (0.3, -0.2, 0.15)
    lhs = sum(float((a * b).sum()) for a, b in zip(bc.add_term(d, masks, f), w))
    rhs = float((d * bc.add_term_transpose(w, masks, f)).sum())
    assert abs(lhs) > 1e-3 and abs(lhs - rhs) < 1e-13 * max(abs(lhs), 1.0), (lhs, rhs)


@pytest.mark.parametrize("force", bc.FORCES)
def test_the_adjoint_composition_equals_the_references_autograd(force):
    """g_a -> g_dsum = g_d_out + dt F . transpose(g_a) -> today's velocity and density adjoints, against autograd through the buoyant step"""
    name = "16_comb"
    g = kc.geometry(name)
    d, v, re = kc.state(name)
    wd, wv = kc.w_dens(name), kc.w_vel(name)
    _, ref = bc.reference(name, force, "both", 1)
    rd, *rv = (t.clone().requires_grad_(True) for t in (d, *v))
    c = o.diffuse_bc(tuple(rv), re, g.X, 1.0, g)
    d2, a = o.advect_mac(rd, c, 1.0, g.dx)
    d2 = d2 + o._t(g.inflow, d) * 1.0
    with torch.no_grad():
        term = bc.add_term(d2, g.masks, force)
    al = [(ac.detach() + tc).requires_grad_(True) for ac, tc in zip(a, term)]
    out = o.project(tuple(al), g)
    sum((p * w).sum() for p, w in zip(out, wv)).backward()
    ga = [t.grad for t in al]                                            # carries the face mask
    g_dsum = wd + bc.add_term_transpose(ga, g.masks, force)
    (sum((ac * gc).sum() for ac, gc in zip(a, ga)) + (d2 * g_dsum).sum()).backward()
    errs = [bc.maxrel(t.grad, r) for t, r in zip((rd, *rv), ref)]
    print("composition against autograd, F=%s:" % (force,), errs)
    assert max(errs) < 1e-12, errs


# ---- float32 against float64: the input condition of the GPU tests ------------------------------------------------------------------
@pytest.mark.parametrize("force", bc.FORCES)
@pytest.mark.parametrize("name", bc.FORWARD_CASES)
def test_the_forward_cases_in_float32_against_float64(name, force):
    out64, _ = bc.reference(name, force, "dens", 1)
    out32, _ = bc.reference(name, force, "dens", 1, dtype=torch.float32)
    ef = [bc.maxrel(a, b) for a, b in zip(out32, out64)]
    print("reference float32 vs float64 %s F=%s: fields %s" % (name, force, ["%.2e" % e for e in ef]))
    assert max(ef) < bc.FIELD_PIN, ef


@pytest.mark.parametrize("steps", [1, 2])
@pytest.mark.parametrize("kind", bc.KINDS)
@pytest.mark.parametrize("force", bc.FORCES)
@pytest.mark.parametrize("name", bc.ADJOINT_CASES)
def test_the_adjoint_cases_in_float32_against_float64(name, force, kind, steps):
    out64, g64 = bc.reference(name, force, kind, steps)
    out32, g32 = bc.reference(name, force, kind, steps, dtype=torch.float32)
    ef = [bc.maxrel(a, b) for a, b in zip(out32, out64)]
    eg = [bc.maxrel(a, b) for a, b in zip(g32, g64)]
    print("reference float32 vs float64 %s F=%s %s steps=%d: fields %s gradients %s" % (
        name, force, kind, steps, ["%.2e" % e for e in ef], ["%.2e" % e for e in eg]))
    assert bc.FIELD_PIN * bc.MARGIN <= 1.5e-5 and bc.GRAD_PIN * bc.MARGIN <= 5e-5 and bc.RE_PIN * bc.MARGIN <= 2e-4
    assert max(ef) < bc.FIELD_PIN, ef
    assert max(eg[:4]) < bc.GRAD_PIN, eg
    assert eg[4] < bc.RE_PIN, eg
    # with a force every gradient is there: a velocity-only loss reaches the density, a density-only loss of two steps the projection
    assert all(float(t.abs().max()) > 0 for t in g64[1:])
    assert float(g64[0].abs().max()) > 0


def test_a_density_only_loss_reaches_the_velocity_through_the_projection():
    """two chained steps: without the force the first step's velocity gets the density advection's gradient alone; with it the gradient
    differs by far more than any tolerance"""
    _, buoy = bc.reference("16_comb", bc.FORCES[0], "dens", 2)
    _, plain = bc.reference("16_comb", (0.0, 0.0, 0.0), "dens", 2)
    for c in (1, 2, 3):
        assert bc.maxrel(buoy[c], plain[c]) > 1e-2, c


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def declared_arity(name):
    """number of parameters of `name` as include/sol_hip.h declares it"""
    with open(_lib.HEADER) as f:
        text = regex.sub(r"/\*.*?\*/", "", f.read(), flags=regex.S)
    m = regex.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=regex.S)
    assert m, name
    return len([p for p in m.group(1).split(",") if p.strip()])


def test_new_symbols_are_declared_exported_and_bound(lib):
    assert lib.sol_version() == _lib.ABI_VERSION == 216          # additions only: the ABI number stays
    assert lib.sol_abi_size_karman3d() == C.sizeof(_lib.Karman3DCfg)
    decl = _lib.declared_symbols()
    for name, arity in NEW.items():
        assert name in decl and name in _lib._SIGS and hasattr(lib, name), name
        assert declared_arity(name) == arity == len(_lib._SIGS[name][1]), (name, declared_arity(name), len(_lib._SIGS[name][1]))
    for name, plain in PLAIN.items():
        extra = 3 if "fwd" in name else 5
        assert declared_arity(name) == declared_arity(plain) + extra
        assert _lib._SIGS[name][1][:len(_lib._SIGS[plain][1])] == _lib._SIGS[plain][1]
    assert "karman3d_buoyancy.hip" in sol_amd._build.SOURCES and "karman3d_buoyancy.hip" not in sol_amd._build.EXTRA
    # face_mask lives in ONE shared header
    csrc = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "csrc")
    holders = [f for f in sorted(os.listdir(csrc)) if "float face_mask(" in open(os.path.join(csrc, f)).read()]
    assert holders == ["karman3d_mask.hpp"], holders


def cfg3d(Y=16, X=8, Z=8, B=2, **kw):
    """cfg with a fake device blob pointer (never dereferenced) of the size the empty-box blob has"""
    c = _lib.Karman3DCfg(B, Y, X, Z, 100.0 / X, 1.0, float(X), 0, 0, 16 + Y * Y + X * X + Z * Z + Y * X * Z, 1 << 20, 0, 0, 0.0, 0.0, None)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def header(c):
    h = np.zeros(16, dtype=np.int32)
    h[:4] = (FD3_MAGIC, c.Y, c.X, c.Z)
    return h


def test_bad_arguments_are_rejected_before_any_launch(lib):
    """fake device pointers: never dereferenced, every case fails validation first"""
    one = [P(4096 * (k + 1)) for k in range(40)]
    err = lambda: lib.sol_last_error()
    # the stand-alone pair
    add, add_bwd = lib.sol_karman3d_buoyancy_add, lib.sol_karman3d_buoyancy_add_bwd
    assert add(None, 0, 8, 8, 8, one[0], one[1], 1.0, 0.0, 0.0, one[2], one[3], one[4]) == -1 and b"B in [1, 65535]" in err()
    assert add(None, 1, 8, 0, 8, one[0], one[1], 1.0, 0.0, 0.0, one[2], one[3], one[4]) == -1 and b"Y, X, Z >= 1" in err()
    assert add(None, 1, 8, 8, 8, one[0], None, 1.0, 0.0, 0.0, one[2], one[3], one[4]) == -1 and b"NULL pointer" in err()
    assert add(None, 1, 8, 8, 8, one[0], one[1], 1.0, 0.0, 0.0, one[2], one[3], None) == -1 and b"NULL pointer" in err()
    assert add(None, 1, 8, 8, 8, one[0], one[1], 1.0, 0.0, 0.0, one[2], one[3], one[2]) == -1 and b"alias" in err()
    assert add(None, 1, 8, 8, 8, one[0], one[1], 1.0, 0.0, 0.0, one[2], one[1], one[4]) == -1 and b"alias" in err()
    assert add(None, 1, 8, 8, 8, one[0], one[1], float("nan"), 0.0, 0.0, one[2], one[3], one[4]) == -1 and b"finite" in err()
    assert add_bwd(None, 1, 8, 8, 8, one[0], one[1], one[2], one[3], 1.0, 0.0, 0.0, None, None) == -1 and b"NULL pointer" in err()
    assert add_bwd(None, 1, 8, 8, 8, one[0], one[1], one[2], None, 1.0, 0.0, 0.0, None, one[4]) == -1 and b"NULL pointer" in err()
    assert add_bwd(None, 1, 8, 8, 8, one[0], one[1], one[2], one[3], 1.0, 0.0, 0.0, one[4], one[4]) == -1 and b"alias" in err()
    assert add_bwd(None, 1, 8, 8, 8, one[0], one[1], one[2], one[3], 1.0, 0.0, 0.0, None, one[3]) == -1 and b"alias" in err()
    assert add_bwd(None, 1, 1 << 10, 1 << 10, 1 << 10, one[0], one[1], one[2], one[3], 1.0, 0.0, 0.0, None, one[4]) == -1 and b"grid too large" in err()
    # the forward step: a force needs the density; the force must be finite; F = 0 passes these checks as the plain call does
    c = cfg3d()
    hdr = header(c).ctypes.data_as(C.c_void_p)
    ws = 1 << 40
    fwd = lib.sol_karman3d_step_fwd_buoy
    head = [C.byref(c), None] + one[0:9] + [0]                        # d_in, vy, vx, vz, re, active, inflow, velBCy, velBCyMask, stride
    outs = one[10:14]                                                 # d_out, vy_out, vx_out, vz_out
    rest = [None, None, None, None, None, hdr, one[20], ws]
    assert fwd(*head, None, *outs[1:], *rest, 1.0, 0.0, 0.0) == -1 and b"needs d_in, inflow and d_out" in err(), err()
    nod = [C.byref(c), None, None] + one[1:9] + [0]
    assert fwd(*nod, None, *outs[1:], *rest, 0.0, 0.0, 0.5) == -1 and b"needs d_in, inflow and d_out" in err(), err()
    assert fwd(*head, *outs, *rest, float("inf"), 0.0, 0.0) == -1 and b"finite" in err(), err()
    assert fwd(*head, *outs, *rest, 0.0, float("nan"), 0.0) == -1 and b"finite" in err(), err()
    assert fwd(*head, *outs, *rest[:-1], 16, 1.0, 0.0, 0.0) == -1 and b"workspace too small" in err(), err()
    assert fwd(*head, one[0], *outs[1:], *rest, 1.0, 0.0, 0.0) == -1 and b"alias" in err(), err()
    assert fwd(None, None, *head[2:], *outs, *rest, 1.0, 0.0, 0.0) == -1 and b"cfg is NULL" in err()
    # the adjoint: g_dsum is required and a buffer of its own
    bhead = [C.byref(c), None] + one[0:6] + [0] + one[6:12] + [hdr, one[20], ws]      # saved x3, re, active, bcm, stride, g_out x3, g_in x3
    bwd, bwd_re = lib.sol_karman3d_step_bwd_buoy, lib.sol_karman3d_step_bwd_buoy_re
    assert bwd(*bhead, 1.0, 0.0, 0.0, None, None) == -1 and b"g_dsum" in err(), err()
    assert bwd(*bhead, 1.0, 0.0, 0.0, None, one[9]) == -1 and b"g_dsum must be a buffer of its own" in err(), err()      # = g_vy_in
    assert bwd(*bhead, 1.0, 0.0, 0.0, None, one[0]) == -1 and b"g_dsum must be a buffer of its own" in err(), err()      # = saved_vy
    assert bwd(*bhead, 1.0, 0.0, 0.0, one[30], one[30]) == -1 and b"g_dsum must be a buffer of its own" in err(), err()  # = g_d_out
    assert bwd(*bhead, float("inf"), 0.0, 0.0, None, one[30]) == -1 and b"finite" in err(), err()
    assert bwd(*bhead[:2], None, *bhead[3:], 1.0, 0.0, 0.0, None, one[30]) == -1 and b"NULL pointer" in err(), err()
    assert bwd_re(*bhead, one[31], one[32], one[33], None, 0, 1.0, 0.0, 0.0, None, one[30]) == -1 and b"NULL pointer" in err(), err()
    assert bwd_re(*bhead, one[31], one[32], one[33], one[34], 0, 1.0, 0.0, 0.0, None, one[34]) == -1 and b"g_dsum must be a buffer of its own" in err(), err()
    assert bwd_re(*bhead, one[31], one[32], one[33], one[34], 0, 1.0, 0.0, 0.0, None, one[32]) == -1 and b"g_dsum must be a buffer of its own" in err(), err()
    # the workspace is the plain call's
    assert bwd(*bhead[:-1], 16, 1.0, 0.0, 0.0, None, one[30]) == -1 and b"workspace too small" in err(), err()


# ---- Python surface without a device ----------------------------------------------------------------------------------------------
def test_force_spellings_and_defaults():
    f3 = k3.buoyancy_force3d
    assert f3() is None
    assert f3((0.3, -0.2, 0.15)) == (0.3, -0.2, 0.15) and f3(0.5) == (0.5, 0.0, 0.0) and f3((0.3, -0.2)) == (0.3, -0.2, 0.0)
    f = f3(buoyancy_factor=0.1)
    assert abs(f[0] - 0.981) < 1e-12 and f[1] == 0.0 and f[2] == 0.0      # PhiFlow: -gravity * buoyancy_factor, Gravity() = -9.81 along y
    assert f3(buoyancy_factor=2.0, gravity=(0.0, 0.0, -1.0)) == (0.0, 0.0, 2.0)
    assert f3((0.0, 0.0, 0.0)) == (0.0, 0.0, 0.0) and not k3._buoyant3d(f3((0.0, 0.0, 0.0))) and k3._buoyant3d((0.0, 0.0, -1e-3))
    for bad in (dict(buoyancy=(1.0, 2.0, 3.0, 4.0)), dict(buoyancy=(float("nan"), 0.0, 0.0)), dict(buoyancy=1.0, buoyancy_factor=1.0),
                dict(buoyancy_factor=1.0, gravity=(-9.81, 0.0)), dict(buoyancy=())):
        with pytest.raises(ValueError):
            f3(**bad)
    import inspect
    for cls in (k3.Karman3DFlow, k3.Karman3DTrainer, k3.Karman3DRollout):
        assert "buoyancy" in inspect.signature(cls.__init__).parameters, cls
    sig = inspect.signature(k3.Karman3DFlow.__init__).parameters
    assert sig["buoyancy_factor"].default is None and sig["gravity"].default == (-9.81, 0.0, 0.0)


def test_the_scripts_buoyancy_flag():
    import argparse
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    sys.path.insert(0, sdir)
    import _common
    p = argparse.ArgumentParser()
    _common.add_buoyancy_arg(p, ncomp=3)
    parse = lambda *a: _common.buoyancy_from_args(vars(p.parse_args(list(a))), ncomp=3)
    assert parse() is None and parse("--buoyancy", "0.981") == (0.981, 0.0, 0.0) and parse("--buoyancy", "0.3,-0.2") == (0.3, -0.2, 0.0)
    assert parse("--buoyancy", "0.3,-0.2,0.15") == (0.3, -0.2, 0.15)
    for bad in ("a", "1,2,3,4", "nan", ""):
        with pytest.raises(SystemExit):
            parse("--buoyancy", bad)
    assert _common.agreed_buoyancy((0.3, -0.2, 0.15), None, "set") == (0.3, -0.2, 0.15) and _common.agreed_buoyancy(None, None, "set") is None
    assert _common.agreed_buoyancy(None, (0.0, 0.0, 0.0), "set") is None                 # an explicit zero agrees with "off"
    assert _common.agreed_buoyancy((0.3, 0.0, 0.0), (0.3, 0.0, 0.0), "set") == (0.3, 0.0, 0.0)
    with pytest.raises(SystemExit, match="contradicts"):
        _common.agreed_buoyancy(None, (0.0, 0.0, 0.3), "set")
    # the 2-D spelling is what it was
    q = argparse.ArgumentParser()
    _common.add_buoyancy_arg(q)
    assert _common.buoyancy_from_args(vars(q.parse_args(["--buoyancy", "0.3,-0.2"]))) == (0.3, -0.2)
    with pytest.raises(SystemExit):
        _common.buoyancy_from_args(vars(q.parse_args(["--buoyancy", "1,2,3"])))
