"""CPU twin of test_gpu_karman3d_maccormack.py: what the MacCormack advection of the karman-3d step shows without a device.

1. The reference of maccormack3d_cases.py itself: its semi-Lagrangian branch equals o.advect_mac exactly, s = 0 gives the
   semi-Lagrangian values bit for bit (both in float32), and the blob experiment's two peaks are pinned in float64.
2. The usability measurement.  The limiter and the clamps tie exactly in places and float32 decides a few entries the other way, so every
   gradient comparison uses trimmed_rel with TRIM = 1e-3 as a condition (k <= int(TRIM n)).  The reference runs in float32 against float64
   on every case the GPU tests use; a row of STEP_CASES whose fields sit further apart than FIELD_ADMIT = 2e-6 (relative L2, worst array)
   or whose trimmed gradients sit further apart than GRAD_ADMIT = 2e-5 is refused -- a fifth of the GPU bounds TOL_FIELD = 1e-5 /
   TOL_GRAD = 1e-4 -- and g_re is held to RE_ADMIT = 2e-5 relative on the rows that assert it.  Measured (worst array; reverted = the
   largest share of an array's entries the limiter reverted):
     row                        reverted  fields   trimmed  (untrimmed)  g_re
     16_comb-s1-x1               0.285    4.7e-7   4.9e-6   7.3e-6       2.3e-6
     16_comb-s0.5-x1             0.267    4.4e-7   3.9e-6   3.1e-5       9.8e-7
     16_before-s1-x1             0.285    4.7e-7   4.9e-6   7.3e-6       2.5e-6
     16_dirichlet-s1-x1          0.285    5.2e-7   4.0e-6   6.0e-6       1.6e-6
     20_comb-s1-x1               0.227    4.3e-7   3.2e-6   1.8e-4       1.9e-5
     32_x35-s1-x1                0.178    6.8e-7   1.0e-6   1.1e-6       4.2e-6
     32_cfl-s1-x1                0.267    6.4e-7   1.3e-6   1.3e-6       1.4e-5
     16_wall-s1-x1               0.285    3.6e-7   5.0e-6   7.5e-6       3.0e-6
     16_lowre-s1-x1              0.287    4.4e-7   1.1e-5   2.3e-5       1.1e-5
     16_comb-s1-x1-force         0.285    2.3e-7   4.9e-6   7.2e-6       2.4e-6
     32_x35-s1-x1-force          0.178    6.3e-7   1.0e-6   1.1e-6       4.7e-6
     16_lowre-s1-x1-force-n3     0.284    2.4e-7   2.6e-6   2.3e-5       3.4e-6
     16_comb-s1-x2               0.301    6.3e-7   5.1e-6   9.6e-6       3.5e-6
     16_lowre-s1-x2              0.293    5.8e-7   1.0e-5   1.4e-5       5.0e-6
     16_comb-s0.5-x2             0.278    6.0e-7   1.5e-6   2.4e-6       1.1e-6
     16_wall-s1-x2-force         0.305    2.4e-7   2.0e-6   2.9e-6       1.6e-6
   Refused, and therefore in no test (a limiter decision flips in float32): two chained steps of 32_x35 (fields 5.7e-4 apart), two chained
   steps of 16_comb with the force (4.7e-4), two chained steps of 20_comb (trimmed gradient 5e-5), the substep suite's unstable Reynolds
   numbers (2.4e-5 .. 7e-5).  The stage alone on its seeded normal fields (STAGE_CASES), held to the SAME FIELD_ADMIT / GRAD_ADMIT:
   fields <= 1.7e-6, trimmed gradients <= 1.7e-6 (worst: 18x10x70; 17x11x37 1.0e-6, the small shapes 4e-7 .. 6e-7) with the stage's
   dx = 2 -- at dx = 100 / X the float32 reference's own coordinate rounding put the Z = 37 and Z = 70 fields at 2.2e-6 .. 3.1e-6, which
   this bound refuses (maccormack3d_cases.stage_geometry).  The roll-out of the GPU file (three steps): 9.8e-7, held to three times
   FIELD_ADMIT.  The trainer problem (2x32x16x16, SOL-2, s = 1): loss 3.6e-7, per-step losses 5.7e-7, weight gradient
   4.6e-6, worst layer 4.5e-5, final state 1.4e-4 (entries whose limiter decision float32 takes the other way); the pins of
   maccormack3d_cases are these times about 2.5 and the GPU tests allow MARGIN = 5 times each pin (the 3-D convention).
3. Host logic: the validators and their messages, StepPhysics3D unchanged, the _adv names looked up, every new symbol declared, exported
   and bound, sol_version() == 216, the cfg's size, advection = 0 workspace sizes equal to the plain ones, bad arguments refused before any
   launch, the script's flags and the record / agree logic."""
import ctypes as C
import importlib.util
import os
import sys

import pytest
import torch

import sol_amd
import sol_oracle3d as o
from sol_amd import _lib, ops
from sol_amd import karman3d as k3

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buoyancy3d_cases as bc
import karman3d_adjoint_cases as kc
import maccormack3d_cases as mc
from large2d_scenes import rel

NEW = ("sol_karman3d_advect", "sol_karman3d_advect_workspace_bytes", "sol_karman3d_advect_bwd", "sol_karman3d_advect_bwd_workspace_bytes",
       "sol_karman3d_step_fwd_adv", "sol_karman3d_step_fwd_adv_workspace_bytes", "sol_karman3d_step_bwd_adv", "sol_karman3d_step_bwd_adv_re",
       "sol_karman3d_step_bwd_adv_workspace_bytes", "sol_karman3d_density_bwd_adv", "sol_karman3d_density_bwd_adv_re",
       "sol_karman3d_density_bwd_adv_workspace_bytes")
P = lambda v: C.c_void_p(v)


@pytest.fixture(scope="module")
def lib():
    return sol_amd.load()


# ---- the reference itself --------------------------------------------------------------------------------------------------------------
def test_reference_semi_lagrangian_branch_is_the_oracles_and_s0_is_semi_lagrangian():
    name = "16_comb"
    g = kc.geometry(name)
    d, v, re = kc.state(name)
    c = o.diffuse_bc(tuple(t.float() for t in v), re.float(), g.X, 1.0, g)
    want = o.advect_mac(d.float(), c, 1.0, g.dx)
    sl = mc.advect(d.float(), c, 1.0, g.dx, scheme="semi_lagrangian")
    s0 = mc.advect(d.float(), c, 1.0, g.dx, 0.0)
    for a, b, z in zip((want[0], *want[1]), (sl[0], *sl[1]), (s0[0], *s0[1])):
        assert torch.equal(a, b) and torch.equal(a, z)


def test_blob_peaks():
    """the experiment of the README paragraph: MacCormack keeps the peak the semi-Lagrangian step smears"""
    sl, mac = mc.blob_peak("semi_lagrangian"), mc.blob_peak("mac_cormack")
    print("blob peaks after %d steps: semi-Lagrangian %.4f, MacCormack %.4f" % (mc.BLOB["steps"], sl, mac))
    assert abs(sl - mc.BLOB_PEAKS["semi_lagrangian"]) < 5e-4 and abs(mac - mc.BLOB_PEAKS["mac_cormack"]) < 5e-4
    assert mac > sl


# ---- the usability measurement ----------------------------------------------------------------------------------------------------------
def trimmed_worst(got, ref):
    """worst trimmed metric over the components, the cap asserted"""
    worst = 0.0
    for a, b in zip(got, ref):
        if float(b.abs().max()) == 0.0:
            assert float(a.abs().max()) == 0.0
            continue
        t, k, _ = mc.trimmed_rel(a, b)
        assert k <= int(mc.TRIM * b.numel())
        worst = max(worst, t)
    return worst


@pytest.mark.parametrize("row", mc.STEP_CASES, ids=[mc.case_id(r) for r in mc.STEP_CASES])
def test_step_case_is_usable_float32_against_float64(row):
    name, s, steps, force, n, with_re = row
    o64, g64, st = mc.reference(name, s, steps, force, n)
    o32, g32, _ = mc.reference(name, s, steps, force, n, dtype=torch.float32)
    fields = max(rel(a, b) for a, b in zip(o32, o64))
    grads = trimmed_worst(g32[:4], g64[:4])
    gre = float(((g32[4] - g64[4]).abs() / g64[4].abs()).max())
    print("%s: reverted %.3f fields %.1e trimmed gradient %.1e g_re %.1e" % (mc.case_id(row), max(st), fields, grads, gre))
    assert 0.02 < max(st) < 0.6                    # the limiter is at work, and not everywhere
    assert fields <= mc.FIELD_ADMIT and grads <= mc.GRAD_ADMIT
    assert not with_re or gre <= mc.RE_ADMIT


@pytest.mark.parametrize("kind", mc.KINDS)
def test_kinds_of_loss_float32_against_float64(kind):
    name, s, steps, force, n, _ = mc.KIND_CASE
    _, g64, _ = mc.reference(name, s, steps, force, n, kind)
    _, g32, _ = mc.reference(name, s, steps, force, n, kind, dtype=torch.float32)
    assert trimmed_worst(g32[:4], g64[:4]) <= mc.GRAD_ADMIT
    assert float(((g32[4] - g64[4]).abs() / g64[4].abs()).max()) <= mc.RE_ADMIT
    if kind == "dens":                              # without a force a density loss reaches the velocity through the departure points only
        assert float(g64[0].abs().max()) > 0 and float(g64[1].abs().max()) > 0


@pytest.mark.parametrize("c", mc.STAGE_CASES, ids=[mc.stage_id(c) for c in mc.STAGE_CASES])
def test_stage_float32_against_float64(c):
    o64, g64, st = mc.stage_reference(*c)
    o32, g32, _ = mc.stage_reference(*c, dtype=torch.float32)
    fields, grads = max(rel(a, b) for a, b in zip(o32, o64)), trimmed_worst(g32, g64)
    print("%s: reverted %.3f fields %.1e trimmed gradient %.1e" % (mc.stage_id(c), max(st), fields, grads))
    assert fields <= mc.FIELD_ADMIT and grads <= mc.GRAD_ADMIT and max(st) > 0.02


def test_rollout_reference_float32_against_float64():
    """the GPU file's roll-out (three steps of 16_comb at s = 1 with the golden small-weight network): three times the one-step admission"""
    import make_golden as mg
    name, s, steps = "16_comb", 1.0, 3
    d, v, re = mc.state(name)
    g, params = mc.ds.geometry(name), mg.k3d_params()
    std_v, std_re = (0.2, 0.25, 0.3), o.STD_RE
    d64, v64 = mc.rollout_reference(params, d, v, re, g, std_v, std_re, s, steps)
    f = lambda t: t.float()
    d32, v32 = mc.rollout_reference([f(p) for p in params], f(d), tuple(f(t) for t in v), f(re), g, std_v, std_re, s, steps)
    errs = [rel(a, b) for a, b in zip((d32, *v32), (d64, *v64))]
    print("roll-out of %d steps: %s" % (steps, ["%.1e" % e for e in errs]))
    assert max(errs) <= steps * mc.FIELD_ADMIT


def test_stage_s0_and_cfl():
    """s = 0 is the semi-Lagrangian stage in float64 too, and the scaled run has the CFL number it names"""
    shape = (16, 8, 8)
    a = mc.stage_reference(shape, 0.0)[0]
    b = mc.stage_reference(shape, 1.0, scheme="semi_lagrangian")[0]
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    g = mc.stage_geometry(*shape)
    _, cy, cx, cz, *_ = mc.stage_inputs(shape, 2.5)
    assert abs(max(float(t.abs().max()) for t in (cy, cx, cz)) / g.dx - 2.5) < 1e-6
    _, cy, cx, cz, *_ = mc.stage_inputs(shape)
    assert 3.0 < max(float(t.abs().max()) for t in (cy, cx, cz)) / g.dx < 6.0          # about one cell per step, tails of a few


def test_trainer_reference_float32_against_float64():
    l64, ls64, g64, f64 = mc.trainer_reference()
    l32, ls32, g32, f32 = mc.trainer_reference(dtype=torch.float32)
    sl = mc.layer_slices(bc.trainer_problem(2)["params"])
    loss = max([abs(l32 / l64 - 1.0)] + [abs(a / b - 1.0) for a, b in zip(ls32, ls64)])
    grad, layer = rel(g32, g64), max(rel(g32[q], g64[q]) for q in sl)
    final = max(rel(a, b) for a, b in zip(f32, f64))
    print("trainer: loss %.1e gradient %.1e worst layer %.1e final state %.1e" % (loss, grad, layer, final))
    for got, pin in ((loss, mc.TRAINER_LOSS_PIN), (grad, mc.TRAINER_GRAD_PIN), (layer, mc.TRAINER_LAYER_PIN), (final, mc.TRAINER_FINAL_PIN)):
        assert pin / 6.0 <= got <= pin              # the pin is about 2.5 times the worst figure: neither missed nor stale


# ---- host logic --------------------------------------------------------------------------------------------------------------------------
def test_validators_and_messages_before_any_device_call():
    assert ops.advection_arg() is None and ops.advection_arg("mac_cormack") == 1.0 and ops.advection_arg("mac_cormack", 0.25) == 0.25
    assert ops.advection_arg("semi_lagrangian", 0.5) is None
    for who, build in (("Karman3DFlow: advection", lambda **kw: k3.Karman3DFlow(None, 1, **kw)),
                       ("Karman3DTrainer: advection", lambda **kw: k3.Karman3DTrainer(None, None, 1, 2, (1, 1, 1), 1.0, **kw)),
                       ("Karman3DRollout: advection", lambda **kw: k3.Karman3DRollout(None, None, 1, (1, 1, 1), 1.0, **kw))):
        with pytest.raises(ValueError, match="%s must be one of semi_lagrangian, mac_cormack" % who):
            build(advection="maccormack")
        for bad in (-0.1, 1.5, float("nan"), float("inf"), "1", None, True):
            for scheme in ops.ADVECTIONS:          # s is checked for either scheme
                with pytest.raises(ValueError, match="correction_strength must be"):
                    build(advection=scheme, correction_strength=bad)
    assert k3._adv_pair(None) == (0, 1.0) and k3._adv_pair(0.5) == (1, 0.5) and k3._adv_tail(0.25) == (1, 0.25)


def test_step_physics_is_unchanged_and_the_adv_names_are_looked_up():
    assert k3.StepPhysics3D._fields == ("buoyancy", "nsub")

    class Lib:
        def __getattr__(self, name):
            return name
    names = {(half, re): k3._adjoint_entry(Lib(), half, "_adv", re) for half in ("step_bwd", "density_bwd") for re in (False, True)}
    assert names == {("step_bwd", False): "sol_karman3d_step_bwd_adv", ("step_bwd", True): "sol_karman3d_step_bwd_adv_re",
                     ("density_bwd", False): "sol_karman3d_density_bwd_adv", ("density_bwd", True): "sol_karman3d_density_bwd_adv_re"}


def test_the_chain_hands_adv_to_the_halves_only_when_it_is_set():
    """_step_adjoint3d with stand-ins: halves that take today's arguments only serve the default, halves that take adv= receive it"""
    saved = tuple(torch.zeros(1, *s) for s in ((3, 2, 2), (2, 3, 2), (2, 2, 3)))
    gv = tuple(torch.ones_like(t) for t in saved)
    seen = []

    class Plain:
        def _bwd(self, saved, re, gvy, gvx, gvz, vel_in=None, g_d=None, physics=None):
            seen.append("plain")
            return [gvy, gvx, gvz]

    class Adv:
        def _bwd(self, saved, re, gvy, gvx, gvz, vel_in=None, g_d=None, physics=None, adv=None):
            seen.append(adv)
            return [gvy, gvx, gvz]
    k3._step_adjoint3d(Plain(), k3.StepPhysics3D(), False, None, saved, None, None, gv)
    k3._step_adjoint3d(Adv(), k3.StepPhysics3D(), False, None, saved, None, None, gv, adv=0.5)
    k3._step_adjoint3d(Adv(), k3.StepPhysics3D(), False, None, saved, None, None, gv)
    assert seen == ["plain", 0.5, None]
    with pytest.raises(TypeError):
        k3._step_adjoint3d(Plain(), k3.StepPhysics3D(), False, None, saved, None, None, gv, adv=1.0)


def cfg3d(Y=20, X=10, Z=10, B=2):
    return _lib.Karman3DCfg(B, Y, X, Z, 100.0 / X, 1.0, float(X), 0, 0, 0, None, 0, 0, 0.0, 0.0, None)


def test_new_symbols_are_declared_exported_and_bound(lib):
    assert lib.sol_version() == _lib.ABI_VERSION == 216        # additions only: the ABI number stays
    decl = _lib.declared_symbols()
    for name in NEW:
        assert name in decl and name in _lib._SIGS and hasattr(lib, name), name
    assert "karman3d_maccormack.hip" in sol_amd._build.SOURCES and "karman3d_maccormack.hip" not in sol_amd._build.EXTRA
    assert lib.sol_abi_size_karman3d() == C.sizeof(_lib.Karman3DCfg)


def test_workspace_sizes(lib):
    """advection = 0 through an _adv function is the plain size; advection = 1 holds at least what the layout must on top of it: h of the
    arrays (forward), h, the int64 accumulators G_h and stage B's cotangent g_h (adjoints)"""
    for B, Y, X, Z in ((1, 16, 8, 8), (3, 20, 10, 10), (2, 18, 10, 70), (1, 128, 64, 64)):
        c = C.byref(cfg3d(Y, X, Z, B))
        faces = B * ((Y + 1) * X * Z + Y * (X + 1) * Z + Y * X * (Z + 1))
        N = B * Y * X * Z
        fwd, bwd, bwd_re = lib.sol_karman3d_step_workspace_bytes(c), lib.sol_karman3d_step_bwd_workspace_bytes(c), lib.sol_karman3d_step_bwd_re_workspace_bytes(c)
        den, den_re = lib.sol_karman3d_density_bwd_workspace_bytes(c), lib.sol_karman3d_density_bwd_re_workspace_bytes(c)
        assert lib.sol_karman3d_step_fwd_adv_workspace_bytes(c, 0) == fwd
        assert lib.sol_karman3d_step_bwd_adv_workspace_bytes(c, 0, 0) == bwd and lib.sol_karman3d_step_bwd_adv_workspace_bytes(c, 1, 0) == bwd_re
        assert lib.sol_karman3d_density_bwd_adv_workspace_bytes(c, 0, 0) == den and lib.sol_karman3d_density_bwd_adv_workspace_bytes(c, 1, 0) == den_re
        assert lib.sol_karman3d_advect_workspace_bytes(c, 0) == 0 and lib.sol_karman3d_advect_workspace_bytes(c, 1) >= 4 * (faces + N)
        assert lib.sol_karman3d_step_fwd_adv_workspace_bytes(c, 1) >= fwd + 4 * (faces + N)
        for re, plain in ((0, bwd), (1, bwd_re)):
            assert lib.sol_karman3d_step_bwd_adv_workspace_bytes(c, re, 1) >= plain + 16 * faces
        for re, plain in ((0, den), (1, den_re)):
            assert lib.sol_karman3d_density_bwd_adv_workspace_bytes(c, re, 1) >= plain + 16 * N
        assert lib.sol_karman3d_advect_bwd_workspace_bytes(c) >= 28 * faces + 36 * N      # g_c, g_a and the velocity part; g_d_in, gU and the density part
    assert lib.sol_karman3d_step_fwd_adv_workspace_bytes(None, 1) == 0
    assert lib.sol_karman3d_advect_workspace_bytes(C.byref(cfg3d(6, 8, 8)), 1) == 0 and lib.sol_karman3d_advect_bwd_workspace_bytes(C.byref(cfg3d(6, 8, 8))) == 0


def test_bad_arguments_are_rejected_before_any_launch(lib):
    """fake device pointers: never dereferenced, every case fails validation first"""
    p = [P(4096 * (k + 1)) for k in range(20)]
    err = lambda: lib.sol_last_error()
    c = cfg3d()
    adv = lambda cfg, args, a=1, s=1.0, ws=p[18], n=1 << 30: lib.sol_karman3d_advect(C.byref(cfg) if cfg is not None else None, None, *args[:6], a, s, *args[6:10], ws, n)
    good = p[:10]
    assert adv(None, good) == -1 and b"cfg is NULL" in err()
    assert adv(cfg3d(6, 10, 10), good) == -1 and b"Y, X, Z >= 8" in err()
    assert adv(cfg3d(20, 10, 10, 70000), good) == -1 and b"B in [1, 65535]" in err()
    assert adv(cfg3d(2048, 1024, 1024), good) == -1 and b"32-bit face indices" in err()
    assert adv(c, good, a=2) == -1 and b"advection must be 0 (semi-Lagrangian) or 1 (MacCormack), got 2" in err()
    for a in (0, 1):
        for s in (-0.5, 1.25, float("nan")):
            assert adv(c, good, a=a, s=s) == -1 and b"correction_strength must lie in [0, 1]" in err()
    for k in range(10):
        args = list(good)
        args[k] = None
        assert adv(c, args) == -1 and b"NULL pointer" in err(), k
    for out in range(6, 10):
        args = list(good)
        args[out] = good[out - 6]
        assert adv(c, args) == -1 and b"alias" in err()
    args = list(good)
    args[7] = good[6]
    assert adv(c, args) == -1 and b"buffers of their own" in err()
    assert adv(c, good, ws=None, n=0) == -1 and b"needs a workspace" in err()
    assert adv(c, good, n=1024) == -1 and b"workspace too small" in err()
    bwd = lambda args, a=1, s=1.0, tile=1, n=1 << 30: lib.sol_karman3d_advect_bwd(C.byref(c), None, *args[:6], a, s, *args[6:14], tile, p[18], n)
    good = p[:14]
    assert bwd(good, tile=2) == -1 and b"tile_window must be 0 or 1" in err()
    assert bwd(good, a=3) == -1 and b"advection must be 0" in err()
    assert bwd(good, s=2.0) == -1 and b"correction_strength" in err()
    assert bwd(good, n=1024) == -1 and b"workspace too small" in err()
    args = list(good)
    args[10] = good[6]
    assert bwd(args) == -1 and b"alias" in err()
    # the _adv step entries check the two arguments before anything else they dereference
    z = [None] * 20
    fwd = lambda a, s: lib.sol_karman3d_step_fwd_adv(C.byref(c), None, *z[:9], 0, *z[:8], None, None, None, 0, 0.0, 0.0, 0.0, a, s)
    assert fwd(5, 1.0) == -1 and b"sol_karman3d_step_fwd_adv: advection must be 0" in err()
    assert fwd(0, 7.0) == -1 and b"sol_karman3d_step_fwd_adv: correction_strength must lie in [0, 1]" in err()
    assert lib.sol_karman3d_step_bwd_adv(C.byref(c), None, *z[:6], 0, *z[:6], None, None, 0, 0.0, 0.0, 0.0, None, None, 1, -1.0) == -1
    assert b"sol_karman3d_step_bwd_adv: correction_strength" in err()
    assert lib.sol_karman3d_density_bwd_adv(C.byref(c), None, *z[:7], 0, *z[:5], 0, None, 0, 9, 1.0) == -1
    assert b"sol_karman3d_density_bwd_adv: advection must be 0" in err()


def test_the_scripts_flags_parse_record_and_agree():
    """scripts/karman3d.py --advection / --mc-strength: validated, recorded in the parameters (what params.pickle holds) as "advection" and
    "correction_strength", and a model's record wins.  parse_params and apply_model_record touch no device."""
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    sys.path.insert(0, sdir)
    spec = importlib.util.spec_from_file_location("sol_script_karman3d_maccormack", os.path.join(sdir, "karman3d.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    def rec(*a, model_record=None):
        p = mod.apply_model_record(mod.parse_params(list(a)), model_record)
        return p["advection"], p["correction_strength"]
    raw = mod.parse_params([])
    assert raw["advection"] is None and raw["mc_strength"] is None
    assert rec() == ("semi_lagrangian", 1.0)
    assert rec("--advection", "mac_cormack") == ("mac_cormack", 1.0) and rec("--advection", "mac_cormack", "--mc-strength", "0.5") == ("mac_cormack", 0.5)
    assert rec("--advection", "semi_lagrangian", "--mc-strength", "0.25") == ("semi_lagrangian", 0.25)
    for bad in ("-0.1", "1.5", "nan"):
        with pytest.raises(SystemExit, match="--mc-strength"):
            rec("--advection", "mac_cormack", "--mc-strength", bad)
    with pytest.raises(SystemExit):
        mod.parse_params(["--advection", "upwind"])
    model = {"advection": "mac_cormack", "correction_strength": 0.5, "buoyancy": None, "diffusion_substeps": 1}
    assert rec("--model", "m.pt", model_record=model) == ("mac_cormack", 0.5)
    assert rec("--model", "m.pt", "--advection", "mac_cormack", "--mc-strength", "0.5", model_record=model) == ("mac_cormack", 0.5)
    with pytest.raises(SystemExit, match="--advection semi_lagrangian contradicts"):
        rec("--model", "m.pt", "--advection", "semi_lagrangian", model_record=model)
    with pytest.raises(SystemExit, match="--mc-strength 1.0 contradicts"):
        rec("--model", "m.pt", "--mc-strength", "1.0", model_record=model)
    assert rec("--model", "m.pt", "--advection", "mac_cormack", model_record={"buoyancy": None}) == ("mac_cormack", 1.0)      # no record: the flag
    assert rec("--model", "m.pt", model_record={"buoyancy": None}) == ("semi_lagrangian", 1.0)
    p = mod.apply_model_record(mod.parse_params(["--advection", "mac_cormack", "--buoyancy", "0.5", "--diffusion-substeps", "2"]))
    assert (p["advection"], p["buoyancy"], p["diffusion_substeps"]) == ("mac_cormack", (0.5, 0.0, 0.0), 2)


def test_the_torch_op_is_defined():
    from sol_amd import torch_ops      # noqa: F401
    schema = str(torch.ops.sol.karman3d_step_adv.default._schema)
    assert "int advection, float s=1., int nsub=1, bool density=False, bool re_grad=False, float fy=0., float fx=0., float fz=0." in schema
    with pytest.raises(ValueError, match="advection must be 0"):
        torch_ops._adv3d("karman3d_step_adv", 2, 1.0)
    assert torch_ops._adv3d("karman3d_step_adv", 0, 0.5) is None and torch_ops._adv3d("karman3d_step_adv", 1, 0.5) == 0.5
    with pytest.raises(ValueError, match="correction_strength"):
        torch_ops._adv3d("karman3d_step_adv", 0, 2.0)
