"""Diffusion substeps of the karman-2d step, CPU side (no GPU needed): ops.min_diffusion_substeps at its boundaries, the rejection of
bad counts, the scripts' flag, the refusals of the one-workgroup trainers, the new C entry points' declarations, bindings, argument
checks (rejected before any launch) and workspace size function, the identities the design rests on (L is symmetric, the adjoint and
the re gradient compose as the library composes them), and the input condition of the GPU tests
(test_gpu_karman2d_diffusion_substeps.py): how far the reference in float32 is from the reference in float64 on every field and gradient
those tests compare.

Measured (reference float32 against float64, relative L2, worst over the cases of the GPU tests):
  pre-diffusion alone (16x16, 40x24, 130x65; n = 2, 3, 9, 12) 1.4e-7;  |<Mx, y> - <x, My>| in float32 at most 6.5e-9 of |Mx||y|
  (pinned below SYM_PIN = 1e-8; the GPU test allows 4x that for its other summation order);
  one step from seed 11 (sphere_130, two_144, before_160; n = 2, 5): fields 1.8e-6; gradients with a velocity cotangent 8.4e-5 untrimmed
  on the adjoint tests' cases (2.4e-4 at before_160, forward only) and 1.7e-5 trimmed; density-only loss 7.5e-6; g_re 9.8e-6;
  buoyancy + re_grad (n = 5): as the plain case;  two chained steps from seed 13 (n = 2): 1.7e-5 untrimmed;
  one-workgroup grids (64x32, 32x16; n = 3): fields 6.4e-7, gradients 3.1e-6, g_re 2.6e-5.
  The step's output velocity v_y moves against n = 1 by 0.025 .. 0.046 (large grids) and 0.053 / 0.104 (64x32 / 32x16) -- pinned above
  0.02; the GPU tests ask for more than 0.01.
  Trainer problem (144x72, B = 1, two steps, mars_moon, n = 4): loss 8.7e-7, weight gradient 3.6e-7, final state 2.0e-6; with n = 1 the
  loss is 45x off and the gradient differs by 0.41.  Roll-out of four steps: 1.9e-6, 1.02x the error after one step.
  Stability (32x16, alpha = 0.85, 40 steps, float64 and float32 alike): max|v| 1.55 at first; n = 4 ends at 1.008, n = 1 at 3e6.
Pinned at about 2.5x those figures (FIELD_PIN / GRAD_PIN / RE_PIN below), far inside the GPU tolerances (1e-5 / 1e-4)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import sol_amd
import sol_oracle as o
from sol_amd import _lib, karman, ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buoyancy_cases as bc
import diffusion_substeps_cases as dc
from large2d_scenes import TOL_FIELD, TOL_GRAD, TRIM, rel, trimmed_rel

NEW = ("sol_karman_diffuse_sub", "sol_karman_diffuse_sub_workspace_bytes", "sol_karman_diffuse_sub_max")
FIELD_PIN, GRAD_PIN, RE_PIN, PRE_PIN, SYM_PIN, MOVED_PIN, ROLLOUT_GROWTH = 4e-6, 4e-5, 7e-5, 4e-7, 1e-8, 0.02, 1.5
P = lambda v: C.c_void_p(v)


@pytest.fixture(scope="module")
def lib():
    return sol_amd.load()


# ---- the bound -------------------------------------------------------------------------------------------------------------------------
def test_min_diffusion_substeps_at_its_boundaries():
    m = ops.min_diffusion_substeps
    assert m(65536.0, 128) == 1                           # alpha exactly 1/4: the single stencil is still a convex combination
    assert m(65535.0, 128) == 2                           # just above
    assert m(1e6, 32) == 1 and m(5.12e6, 128) == 1
    assert m(4096.0, 64) == 4 and m(4095.0, 64) == 5      # alpha / n exactly 1/4, just above
    assert m(160000.0, 256) == 2                          # the reference's lowest Reynolds number at res = 256: alpha = 0.41
    assert m(8000.0, 80) == 4 and m(2000.0, 64, dt=0.5) == 5
    for re_min, res, dt in ((3000.0, 64, 1.0), (777.0, 48, 0.3), (1e4, 128, 1.0)):
        n = m(re_min, res, dt)
        assert dt * res * res / (n * re_min) <= 0.25 and (n == 1 or dt * res * res / ((n - 1) * re_min) > 0.25)
    for bad in ((0.0, 64), (-1.0, 64), (1e4, 0), (float("nan"), 64)):
        with pytest.raises(ValueError):
            m(*bad)


def test_bad_counts_are_rejected():
    for bad in (0, -3, 2.0, 1.5, "2", None, True):
        with pytest.raises(ValueError, match="integer >= 1"):
            ops.diffusion_substeps_arg(bad)
        with pytest.raises(ValueError, match="integer >= 1"):
            karman.KarmanFlow(diffusion_substeps=bad)
    assert ops.diffusion_substeps_arg(np.int64(3)) == 3 and karman.KarmanFlow()._nsub == 1 and karman.KarmanFlow(diffusion_substeps=4)._nsub == 4
    cfg = ops.karman_cfg(2, 130, 65, 100.0 / 65)
    assert ops.diffusion_sub_cfg(cfg, 1) is cfg
    sc = ops.diffusion_sub_cfg(cfg, 4)
    assert sc is not cfg and sc.res == 32.5 and cfg.res == 65.0 and (sc.B, sc.Y, sc.X, sc.dx, sc.dt) == (cfg.B, cfg.Y, cfg.X, cfg.dx, cfg.dt)
    assert ops.diffusion_sub_cfg(cfg, 3).res == float(np.float32(65.0 / np.sqrt(3.0)))
    # refused before any device call
    z = torch.zeros(1)
    small = ops.karman_cfg(1, 16, 8, 100.0 / 8)
    for call in (lambda: ops.karman_step(z, z, z, z, small, None, diffusion_substeps=2),
                 lambda: ops.karman_step_large(z, z, z, z, small, None, diffusion_substeps=2),
                 lambda: ops.karman_step_saved(z, z, z, z, small, None, diffusion_substeps=2)):
        with pytest.raises(sol_amd.SolError, match="Y, X >= 16"):
            call()
    with pytest.raises(ValueError, match="integer >= 1"):
        ops.karman_step_large(z, z, z, z, cfg, None, diffusion_substeps=0)


def test_the_one_workgroup_trainers_and_rollouts_refuse_substeps_at_construction():
    net = sol_amd.model_mars_moon(cin=3, cout=2, seed=0, device="cpu")
    mercury = sol_amd.model.MODELS["mercury"](3, 2, 0, "cpu")
    a = (100.0 / 32, (0.2, 0.2), o.STD_RE)
    with pytest.raises(ValueError, match="SolTrainer: diffusion_substeps=3"):
        sol_amd.SolTrainer(net, None, 1, 64, 32, 2, *a, diffusion_substeps=3)
    with pytest.raises(ValueError, match="GraphTrainer: diffusion_substeps=2"):
        sol_amd.GraphTrainer(net, 1, 64, 32, 2, (0.2, 0.2), o.STD_RE, diffusion_substeps=2)
    with pytest.raises(ValueError, match="SolRollout: diffusion_substeps=2"):
        sol_amd.SolRollout(net, None, 1, 64, 32, *a, diffusion_substeps=2)
    with pytest.raises(ValueError, match="make_trainer: diffusion_substeps=2"):
        sol_amd.make_trainer(net, None, 1, 64, 32, 2, *a, diffusion_substeps=2)
    with pytest.raises(ValueError, match="GraphTrainer: diffusion_substeps=2"):
        sol_amd.make_trainer(mercury, None, 1, 64, 32, 2, *a, diffusion_substeps=2)
    with pytest.raises(ValueError, match="make_rollout: diffusion_substeps=2"):
        sol_amd.make_rollout(net, None, 1, 64, 32, *a, diffusion_substeps=2)
    for cls_call in (lambda n: sol_amd.SolTrainer(net, None, 1, 64, 32, 2, *a, diffusion_substeps=n),
                     lambda n: sol_amd.LargeGridTrainer(net, 1, 256, 128, 2, (0.2, 0.2), o.STD_RE, diffusion_substeps=n),
                     lambda n: sol_amd.LargeGridRollout(net, None, 1, 256, 128, *a, diffusion_substeps=n)):
        with pytest.raises(ValueError, match="integer >= 1"):
            cls_call(0)
        with pytest.raises(ValueError, match="integer >= 1"):
            cls_call(2.5)


def test_the_scripts_flag_and_auto():
    import argparse
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    sys.path.insert(0, sdir)
    import _common
    p = argparse.ArgumentParser()
    _common.add_substeps_arg(p)
    gen = lambda *a: _common.substeps_from_args(vars(p.parse_args(list(a))), [8000.0, 16000.0], 80)
    assert gen() is None and gen("--diffusion-substeps", "3") == 3 and gen("--diffusion-substeps", "auto") == 4 == ops.min_diffusion_substeps(8000.0, 80)
    assert _common.substeps_from_args({"diffusion_substeps": "AUTO"}, [1e6], 32) == 1
    for bad in ("0", "-2", "1.5", "many"):
        with pytest.raises(SystemExit, match="integer >= 1"):
            gen("--diffusion-substeps", bad)
    read = lambda v: _common.substeps_from_args({"diffusion_substeps": v})
    assert read(None) is None and read("2") == 2
    with pytest.raises(SystemExit, match="data generation"):
        read("auto")
    assert _common.agreed_substeps(None, None, "set") == 1 and _common.agreed_substeps(4, None, "set") == 4 and _common.agreed_substeps(4, 4, "set") == 4
    with pytest.raises(SystemExit, match="contradicts"):
        _common.agreed_substeps(4, 2, "set")
    with pytest.raises(SystemExit, match="contradicts"):
        _common.agreed_substeps(None, 2, "set")


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def cfg2d(Y=130, X=65, B=2):
    return _lib.KarmanCfg(B, Y, X, 100.0 / X, 1.0, float(X), 1e-6, 1e-9, 2000, 0, 0, 0, None, 0, None)


def test_new_symbols_are_declared_exported_and_bound(lib):
    assert lib.sol_version() == _lib.ABI_VERSION          # additions only: the ABI number stays
    decl = _lib.declared_symbols()
    for name in NEW:
        assert name in decl and name in _lib._SIGS and hasattr(lib, name), name
    assert "karman_diffuse_sub.hip" in sol_amd._build.SOURCES and "karman_diffuse_sub.hip" not in sol_amd._build.EXTRA
    assert lib.sol_karman_diffuse_sub_max() == 8 == ops.diffuse_sub_max()


def test_workspace_size_against_the_layout(lib):
    """one launch: nothing; more: ONE ping-pong pair (the last launch writes the outputs), each buffer rounded up to 256 bytes, plus the
    256 bytes of base alignment (csrc/carve.hpp)"""
    up = lambda n: (4 * n + 255) // 256 * 256
    for B, Y, X in ((1, 16, 16), (3, 40, 24), (2, 130, 65), (1, 256, 128)):
        c = cfg2d(Y, X, B)
        pair = up(B * (Y + 1) * X) + up(B * Y * (X + 1)) + 256
        for m, chunk, launches in ((1, 0, 1), (8, 0, 1), (8, 8, 1), (9, 0, 2), (11, 0, 2), (11, 3, 4), (5, 1, 5), (17, 8, 3), (3, 3, 1)):
            got = lib.sol_karman_diffuse_sub_workspace_bytes(C.byref(c), m, chunk)
            assert got == (pair if launches > 1 else 0), (B, Y, X, m, chunk, got)
            assert ops.diffuse_sub_workspace_bytes(c, m + 1, chunk or None) == got
    assert lib.sol_karman_diffuse_sub_workspace_bytes(None, 9, 0) == 0
    assert lib.sol_karman_diffuse_sub_workspace_bytes(C.byref(cfg2d(8, 8)), 9, 0) == 0
    assert ops.diffuse_sub_workspace_bytes(cfg2d(), 1) == 0


def test_bad_arguments_are_rejected_before_any_launch(lib):
    """fake device pointers: never dereferenced, every case fails validation first"""
    one = [P(4096 * (k + 1)) for k in range(8)]
    c = cfg2d()
    call = lambda cfg, *a: lib.sol_karman_diffuse_sub(C.byref(cfg) if cfg is not None else None, None, *a)
    good = one[0:5]
    assert call(None, *good, 3, 0, None, 0) == -1 and b"cfg is NULL" in lib.sol_last_error()
    assert call(cfg2d(8, 65), *good, 3, 0, None, 0) == -1 and b"Y, X >= 16" in lib.sol_last_error()
    assert call(cfg2d(130, 65, 70000), *good, 3, 0, None, 0) == -1 and b"B in [1, 65535]" in lib.sol_last_error()
    assert call(c, *good, 0, 0, None, 0) == -1 and b"substeps m must be in" in lib.sol_last_error()
    assert call(c, *good, 3, 9, None, 0) == -1 and b"chunk" in lib.sol_last_error()
    assert call(c, *good, 3, -1, None, 0) == -1 and b"chunk" in lib.sol_last_error()
    assert call(c, one[0], None, one[2], one[3], one[4], 3, 0, None, 0) == -1 and b"NULL pointer" in lib.sol_last_error()
    assert call(c, one[0], one[1], one[2], one[0], one[4], 3, 0, None, 0) == -1 and b"alias" in lib.sol_last_error()
    assert call(c, one[0], one[1], one[2], one[3], one[3], 3, 0, None, 0) == -1 and b"buffers of their own" in lib.sol_last_error()
    assert call(c, *good, 9, 0, None, 0) == -1 and b"need a workspace" in lib.sol_last_error()
    assert call(c, *good, 9, 0, one[5], 1024) == -1 and b"workspace too small" in lib.sol_last_error()
    assert call(c, *good, 4, 1, one[5], 1024) == -1 and b"workspace too small" in lib.sol_last_error()


# ---- the identities of the design, in float64 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("Y,X", dc.PRE_SHAPES)
def test_the_laplacian_with_replicate_padding_is_symmetric_on_both_face_grids(Y, X):
    xy, xx, re = dc.pre_inputs(Y, X, seed=21)
    yy, yx, _ = dc.pre_inputs(Y, X, seed=22)
    dot = lambda a, b: float((a * b).sum())
    for x, y in ((xy, yy), (xx, yx)):
        lhs, rhs = dot(o.laplace_replicate(x), y), dot(x, o.laplace_replicate(y))
        assert abs(lhs - rhs) < 1e-12 * abs(lhs) and abs(lhs) > 1.0
    for n in dc.PRE_N:                                       # hence M^(n-1) is its own transpose; in float32 within SYM_PIN of |Mx||y|
        for dtype, bound in ((torch.float64, 1e-14), (torch.float32, SYM_PIN)):
            mx = dc.pre_diffuse(xy.to(dtype), xx.to(dtype), re.to(dtype), X, n)
            my = dc.pre_diffuse(yy.to(dtype), yx.to(dtype), re.to(dtype), X, n)
            mx, my = [t.double() for t in mx], [t.double() for t in my]
            lhs, rhs = dot(mx[0], yy) + dot(mx[1], yx), dot(xy, my[0]) + dot(xx, my[1])
            scale = float(np.sqrt((dot(mx[0], mx[0]) + dot(mx[1], mx[1])) * (dot(yy, yy) + dot(yx, yx))))
            print("%dx%d n=%d %s: |<Mx,y> - <x,My>| / (|Mx||y|) = %.2e" % (Y, X, n, dtype, abs(lhs - rhs) / scale))
            assert abs(lhs - rhs) < bound * scale


@pytest.mark.parametrize("n", [2, 5])
def test_the_composition_the_library_runs_equals_the_references_autograd(n):
    """today's step at alpha / n applied to M^(n-1) v; its adjoint (autograd through the plain step) followed by M^(n-1); the plain
    step's re gradient at re * n, fed M^(n-1) v as a constant, times n ... against autograd through the reference"""
    Y, X = 32, 16
    g, (d, vy, vx, re) = dc.small_state(Y, X)
    wy, wx = dc.small_cotangents(Y, X)
    ref_out, ref_g = dc.small_reference(Y, X, n, True)
    with torch.no_grad():
        py, px = dc.pre_diffuse(vy, vx, re, X, n)
    ly, lx = py.clone().requires_grad_(True), px.clone().requires_grad_(True)
    # the "scaled cfg": res / sqrt(n) at the same re  ->  d alpha' / d re carries the 1 / n
    lr = re.clone().requires_grad_(True)
    out = o.karman_step(d, ly, lx, lr, g, res=X / np.sqrt(n))
    ((out[1] * wy).sum() + (out[2] * wx).sum()).backward()
    gy, gx = dc.pre_diffuse(ly.grad, lx.grad, re, X, n)
    errs = [rel(a, b) for a, b in zip(out, ref_out)] + [rel(gy, ref_g[0]), rel(gx, ref_g[1]), rel(lr.grad * n, ref_g[2])]
    print("composition against autograd n=%d:" % n, errs)
    assert max(errs) < 1e-12


# ---- float32 against float64: the input condition of the GPU tests ----------------------------------------------------------------
@pytest.mark.parametrize("n", dc.PRE_N)
@pytest.mark.parametrize("Y,X", dc.PRE_SHAPES)
def test_pre_diffusion_in_float32_against_float64(Y, X, n):
    r64, r32 = dc.pre_reference(Y, X, n), dc.pre_reference(Y, X, n, dtype=torch.float32)
    errs = [rel(a, b) for a, b in zip(r32, r64)]
    print("pre-diffusion float32 vs float64 %dx%d n=%d: %s" % (Y, X, n, errs))
    assert max(errs) < PRE_PIN < TOL_FIELD
    assert rel(r64[0], dc.pre_inputs(Y, X)[0]) > 0.5


CASES = [(nm, n, "vel", 1, False, None) for nm in sorted(bc.SCENES) for n in dc.STEP_N]
CASES += [(nm, 5, k, 1, rg, None) for nm in ("sphere_130", "two_144") for k, rg in (("both", True), ("dens", False))]
CASES += [("sphere_130", 5, "both", 1, True, dc.FORCE), ("sphere_130", 5, "vel", 1, False, dc.FORCE), ("sphere_130", 2, "both", 2, False, None)]
FORWARD_ONLY = ("before_160",)          # its gradient is not compared on the GPU


@pytest.mark.parametrize("name,n,kind,steps,re_grad,force", CASES)
def test_the_gpu_tests_inputs_in_float32_against_float64(name, n, kind, steps, re_grad, force):
    out64, g64 = dc.reference(name, n, kind, steps, re_grad, force)
    out32, g32 = dc.reference(name, n, kind, steps, re_grad, force, dtype=torch.float32)
    plain = dc.reference(name, 1, kind, steps, re_grad, force)[0]
    ef = [rel(a, b) for a, b in zip(out32, out64)]
    eg = [rel(a, b) for a, b in zip(g32, g64)]
    trims = [trimmed_rel(a, b) for a, b in zip(g32, g64)]
    et = [t[0] for t in trims]
    moved = rel(plain[1], out64[1])
    print("reference float32 vs float64 %s n=%d %s steps=%d re=%s F=%s: fields %s gradients %s trimmed %s; v_y against n = 1 %.3f" % (
        name, n, kind, steps, re_grad, force, ["%.2e" % e for e in ef], ["%.2e" % e for e in eg], ["%.2e" % e for e in et], moved))
    assert max(ef) < FIELD_PIN < TOL_FIELD, ef
    assert GRAD_PIN < RE_PIN < TOL_GRAD
    assert moved > MOVED_PIN
    if name in FORWARD_ONLY:
        return
    assert all(t[1] <= int(TRIM * b.numel()) for t, b in zip(trims, g64))
    assert max(et[:3]) < GRAD_PIN, (eg, et)
    if not dc.needs_trim(kind, steps):
        assert max(eg[:3]) < GRAD_PIN, eg
    if re_grad:
        assert eg[3] < RE_PIN and float(g64[3].abs().min()) > 0, eg


@pytest.mark.parametrize("Y,X", dc.SMALL)
def test_the_one_workgroup_cases_in_float32_against_float64(Y, X):
    n = dc.SMALL_N
    out64, g64 = dc.small_reference(Y, X, n, True)
    out32, g32 = dc.small_reference(Y, X, n, True, dtype=torch.float32)
    plain = dc.small_reference(Y, X, 1, True)[0]
    ef, eg = [rel(a, b) for a, b in zip(out32, out64)], [rel(a, b) for a, b in zip(g32, g64)]
    moved = rel(plain[1], out64[1])
    print("reference float32 vs float64 %dx%d n=%d: fields %s gradients %s; v_y against n = 1 %.3f" % (Y, X, n, ef, eg, moved))
    assert max(ef) < FIELD_PIN and max(eg[:2]) < GRAD_PIN and eg[2] < RE_PIN and moved > MOVED_PIN


def test_stability_four_substeps_stay_bounded_where_the_single_stencil_blows_up():
    """32 x 16, alpha = 0.85, 40 steps, float64 and float32: n = 4 ends near the initial max|v| (1.55 -> 1.01), n = 1 at 3e6"""
    for dtype in (torch.float64, torch.float32):
        first, one = dc.stability_run(1, dtype)
        _, four = dc.stability_run(dc.STABILITY["n"], dtype)
        print("stability %s: max|v| %.3f initially; after %d steps n = 1 %.3e, n = %d %.3f" % (dtype, first, dc.STABILITY["steps"], one, dc.STABILITY["n"], four))
        assert one > 1e5 and four < 1.2 * first          # (the GPU test asks for > 1e3 and < 2 x the initial value)
    assert ops.min_diffusion_substeps(dc.STABILITY["X"] ** 2 / dc.STABILITY["alpha"], dc.STABILITY["X"]) == dc.STABILITY["n"]


def test_the_trainer_and_rollout_problem_in_float32_and_against_one_substep():
    """144 x 72, B = 1, two steps, mars_moon, n = 4: the float32 reference against float64, and how far the n = 1 loss and gradient lie
    from the n = 4 ones (an ignored parameter cannot pass the GPU test: it asks for the loss within 1e-5); four roll-out steps in
    float32 against float64 stay within ROLLOUT_GROWTH x TOL_FIELD of the GPU test with margin"""
    n = dc.TRAINER_N
    p = dc.trainer_problem(2)
    l64, s64, g64, f64 = dc.trainer_reference(p, n)
    l1, _, g1, _ = dc.trainer_reference(p, 1)
    p32 = dc.trainer_problem(2, dtype=torch.float32)
    l32, s32, g32, f32_ = dc.trainer_reference(p32, n, torch.float32)
    e_l, e_g, e_f = abs(l32 - l64) / abs(l64), rel(g32, g64), max(rel(a, b) for a, b in zip(f32_, f64))
    d_l, d_g = abs(l1 - l64) / abs(l64), rel(g1, g64)
    print("trainer problem float32 vs float64: loss %.2e gradient %.2e final state %.2e;  n = 1 against n = %d: loss %.3f gradient %.3f"
          % (e_l, e_g, e_f, n, d_l, d_g))
    assert e_l < 4e-6 and e_g < GRAD_PIN and e_f < FIELD_PIN
    assert d_l > 0.1 and d_g > 0.1
    r64, r32 = dc.rollout_reference(p, n, 4), dc.rollout_reference(p, n, 4, torch.float32)
    e_r = [rel(a, b) for a, b in zip(r32, r64)]
    print("roll-out of four steps float32 vs float64: %s" % e_r)
    one = max(rel(a, b) for a, b in zip(dc.rollout_reference(p, n, 1, torch.float32), dc.rollout_reference(p, n, 1)))
    print("growth of the float32 error from one step to four: %.2f" % (max(e_r) / one))
    assert max(e_r) < ROLLOUT_GROWTH * one < ROLLOUT_GROWTH * FIELD_PIN          # the GPU test's bound is ROLLOUT_GROWTH x TOL_FIELD
