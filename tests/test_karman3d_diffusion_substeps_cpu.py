"""Diffusion substeps of the karman-3d step, CPU side (no GPU needed): karman3d.min_diffusion_substeps3d at its boundaries, the rejection
of bad counts, the script's flag, the new C entry points' declarations, bindings, argument checks (rejected before any launch) and
workspace size function, the identities the design rests on (L is symmetric on the three face grids; the adjoint and the re gradient
compose as the library composes them), the stability figures, and the input condition of the GPU tests
(test_gpu_karman3d_diffusion_substeps.py): how far the reference in float32 is from the reference in float64 on every field and gradient
those tests compare, in their metric -- max |a - b| / max |b| (maxrel), untrimmed, no element left out.

Measured (reference float32 against float64, worst over the cases of the GPU tests):
  pre-diffusion alone (16x8x8, 20x10x10, 18x10x70, 17x11x37; B = 3, alpha 0.45 / 0.3 / 0.9; n = 2 .. 10) 5.3e-7 (PRE_PIN 1.3e-6);
  |<Mx, y> - <x, My>| in float32 at most 2.2e-8 of |Mx||y| (far inside PRE_PIN, which the GPU test allows);
  fields of one or two steps (16_comb, 16_before, 16_dirichlet, 20_comb, 32_x35, 16_wall; n = 3, 5) 1.1e-6 (FIELD_PIN 2.7e-6);
  gradients g_d, g_vy, g_vx, g_vz on the (case, n, steps, force) rows of diffusion_substeps3d_cases.GRAD_CASES, GRAD_CASES_NO_RE and
  the CG scene 4.7e-6 (GRAD_PIN 8e-6) -- every row below the flipped-cell condition 1e-4 (16_* and 32_x35 at n = 3 are NOT: g_vx 2e-3,
  g_vz 8e-3, and are not used);  g_re 3.7e-6 (RE_PIN 1e-5) on the rows that carry it.
  Conditioning of g_re (diffusion_substeps3d_cases.re_condition: kappa = sum |terms| / |sum| of the reduction, float64), the criterion
  by which a row is given a g_re comparison: kappa 2^-24 < RE_PIN.  21 .. 117 on every row of GRAD_CASES and the CG scene (at most
  7.0e-6).  One step of 32_x35 fails it at every alpha and n tried (alpha 0.2 .. 1.2, n 4 .. 9: kappa 193 .. 5476; n = 5 at alpha 0.45:
  5476, kappa 2^-24 = 3.3e-4 -- the reference in float32 does not show it, 4.0e-6, because its pressure solve runs in float64, so its
  cotangent is better than any fp32 pipeline's), so that row is in GRAD_CASES_NO_RE (run with re_grad off) and the rows that carry g_re
  at 32 x 16 x 16 are two chained steps: with the force (kappa 46) and, without it, at alpha 0.9, n = 6 (kappa 65).
  Stability (16x8x8, alpha = 0.45, 40 steps, no network): max|v| 1.10 at first; n = 1 ends at 305 in float64 and 235 in float32 (a
  growing mode: the figure depends on round-off, the order of magnitude does not), n = 3 at 1.00001, n = 4 at 1.00001.
  Trainer problem (2x32x16x16, two steps, mars_moon3d, n = 4, re = 256 / (0.45, 0.3)): see TRAINER below.
The GPU tests allow MARGIN = 5 times each pin (the 3-D convention: buoyancy3d_cases)."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import sol_amd
import sol_oracle3d as o
from sol_amd import _lib, ops
from sol_amd import karman3d as k3

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diffusion_substeps3d_cases as dc
from large2d_scenes import rel

NEW = ("sol_karman3d_diffuse_sub", "sol_karman3d_diffuse_sub_workspace_bytes", "sol_karman3d_diffuse_sub_max")
FLIPPED = 1e-4          # a density or velocity gradient component further apart than this between float32 and float64: a flipped cell
P = lambda v: C.c_void_p(v)


@pytest.fixture(scope="module")
def lib():
    return sol_amd.load()


# ---- the bound -------------------------------------------------------------------------------------------------------------------------
def test_min_diffusion_substeps3d_against_the_closed_form():
    m = k3.min_diffusion_substeps3d
    assert m(24576.0, 64) == 1                            # alpha exactly 1/6: the single stencil is still a convex combination
    assert m(24575.0, 64) == 2                            # just above
    assert m(98304.0, 128) == 1 and m(98303.0, 128) == 2
    assert m(1e6, 32) == 1 and m(1.6e5, 64) == 1
    assert m(6144.0, 64) == 4 and m(6143.0, 64) == 5      # alpha / n exactly 1/6, just above
    for re_min, res, dt in ((3000.0, 64, 1.0), (777.0, 48, 0.3), (1e4, 128, 1.0), (142.2, 8, 1.0), (1e4, 64, 0.5)):
        n = m(re_min, res, dt)
        alpha = dt * res * res / re_min
        assert n == max(1, int(np.ceil(6.0 * alpha - 1e-9)))
        assert alpha / n <= 1.0 / 6.0 and (n == 1 or alpha / (n - 1) > 1.0 / 6.0)
    assert m(float(dc.re_of(8, 1)[0]), 8) == 3 == dc.STABILITY["n"]          # the stability case: alpha = 0.45
    for bad in ((0.0, 64), (-1.0, 64), (1e4, 0), (float("nan"), 64), (1e4, 64, 0.0), (1e4, float("inf"))):
        with pytest.raises(ValueError):
            m(*bad)


def test_bad_counts_are_rejected_before_any_device_call():
    for bad in (0, -3, 2.0, 1.5, "2", None, True):
        with pytest.raises(ValueError, match="integer >= 1"):
            k3.Karman3DFlow(None, 1, diffusion_substeps=bad)
        with pytest.raises(ValueError, match="integer >= 1"):
            k3.diffuse_sub(None, None, None, None, None, bad)
    assert k3.diffusion_sub_res(64.0, 1) == 64.0 and k3.diffusion_sub_res(64.0, 4) == 32.0
    assert k3.diffusion_sub_res(16.0, 3) == float(np.float32(16.0 / np.sqrt(3.0)))


def test_the_scripts_flag_parses_and_records():
    """scripts/karman3d.py --diffusion-substeps N|auto: auto is min_diffusion_substeps3d of --re; the count is recorded in the parameters
    (what params.pickle holds) and a model's record wins.  parse_params and apply_model_record touch no device."""
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    sys.path.insert(0, sdir)
    spec = importlib.util.spec_from_file_location("sol_script_karman3d_substeps", os.path.join(sdir, "karman3d.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rec = lambda *a, model_record=None: mod.apply_model_record(mod.parse_params(list(a)), model_record)["diffusion_substeps"]
    assert mod.parse_params([])["diffusion_substeps"] is None and mod.parse_params(["--diffusion-substeps", "2"])["diffusion_substeps"] == 2
    assert rec() == 1 and rec("--diffusion-substeps", "3") == 3
    assert rec("-r", "64", "--re", "24576", "--diffusion-substeps", "auto") == 1
    assert rec("-r", "64", "--re", "24575", "--diffusion-substeps", "auto") == 2
    assert rec("-r", "8", "--re", "142.2", "--diffusion-substeps", "auto") == 3 == k3.min_diffusion_substeps3d(142.2, 8)
    assert rec("-r", "64", "--re", "1e6", "--diffusion-substeps", "AUTO") == 1
    for bad in ("0", "-2", "1.5", "many"):
        with pytest.raises(SystemExit, match="integer >= 1"):
            rec("--diffusion-substeps", bad)
    model = {"diffusion_substeps": 4, "buoyancy": None}
    assert rec("--model", "m.pt", model_record=model) == 4 and rec("--model", "m.pt", "--diffusion-substeps", "4", model_record=model) == 4
    with pytest.raises(SystemExit, match="contradicts"):
        rec("--model", "m.pt", "--diffusion-substeps", "2", model_record=model)
    assert rec("--model", "m.pt", "--diffusion-substeps", "2", model_record={"buoyancy": None}) == 2      # a model without the record takes the flag
    p = mod.apply_model_record(mod.parse_params(["--buoyancy", "0.5", "--diffusion-substeps", "2"]))
    assert p["buoyancy"] == (0.5, 0.0, 0.0) and p["diffusion_substeps"] == 2


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def cfg3d(Y=20, X=10, Z=10, B=2):
    return _lib.Karman3DCfg(B, Y, X, Z, 100.0 / X, 1.0, float(X), 0, 0, 0, None, 0, 0, 0.0, 0.0, None)


def test_new_symbols_are_declared_exported_and_bound(lib):
    assert lib.sol_version() == _lib.ABI_VERSION          # additions only: the ABI number stays
    decl = _lib.declared_symbols()
    for name in NEW:
        assert name in decl and name in _lib._SIGS and hasattr(lib, name), name
    assert "karman3d_diffuse_sub.hip" in sol_amd._build.SOURCES and "karman3d_diffuse_sub.hip" not in sol_amd._build.EXTRA
    smax = lib.sol_karman3d_diffuse_sub_max()
    assert 2 <= smax < ops.diffuse_sub_max() and smax == k3.diffuse_sub_max3d()        # the 3-D halo is dear: fewer than the 2-D kernel's 8
    assert 1 <= k3.DIFFUSE_SUB_CHUNK3D <= smax
    assert lib.sol_abi_size_karman3d() == C.sizeof(_lib.Karman3DCfg)


def test_workspace_size_against_the_layout(lib):
    """one launch: nothing; more: TWO velocity triples (the launches before the last alternate between them, the last writes the outputs),
    each buffer rounded up to 256 bytes, plus the 256 bytes of base alignment (csrc/carve.hpp)"""
    up = lambda n: (4 * n + 255) // 256 * 256
    S = lib.sol_karman3d_diffuse_sub_max()
    for B, Y, X, Z in ((1, 16, 8, 8), (3, 20, 10, 10), (2, 18, 10, 70), (1, 128, 64, 64)):
        c = cfg3d(Y, X, Z, B)
        triple = up(B * (Y + 1) * X * Z) + up(B * Y * (X + 1) * Z) + up(B * Y * X * (Z + 1))
        for m, chunk, launches in ((1, 0, 1), (S, 0, 1), (S, S, 1), (S + 1, 0, 2), (2 * S + 1, 0, 3), (2, 1, 2), (5, 1, 5), (S, 1, S), (4096, 0, -1)):
            got = lib.sol_karman3d_diffuse_sub_workspace_bytes(C.byref(c), m, chunk)
            assert got == (2 * triple + 256 if launches != 1 else 0), (B, Y, X, Z, m, chunk, got)
    assert lib.sol_karman3d_diffuse_sub_workspace_bytes(None, 9, 0) == 0
    assert lib.sol_karman3d_diffuse_sub_workspace_bytes(C.byref(cfg3d(8, 8, 8)), 9, 0) == 0         # a grid the entry point refuses
    assert lib.sol_karman3d_diffuse_sub_workspace_bytes(C.byref(cfg3d()), 0, 0) == 0


def test_bad_arguments_are_rejected_before_any_launch(lib):
    """fake device pointers: never dereferenced, every case fails validation first"""
    one = [P(4096 * (k + 1)) for k in range(9)]
    S = lib.sol_karman3d_diffuse_sub_max()
    c = cfg3d()
    call = lambda cfg, *a: lib.sol_karman3d_diffuse_sub(C.byref(cfg) if cfg is not None else None, None, *a)
    good = one[0:7]
    err = lambda: lib.sol_last_error()
    assert call(None, *good, 2, 0, None, 0) == -1 and b"cfg is NULL" in err()
    assert call(cfg3d(8, 10, 10), *good, 2, 0, None, 0) == -1 and b"Y >= 16, X, Z >= 8" in err()
    assert call(cfg3d(20, 10, 4), *good, 2, 0, None, 0) == -1 and b"Y >= 16, X, Z >= 8" in err()
    assert call(cfg3d(20, 10, 10, 70000), *good, 2, 0, None, 0) == -1 and b"B in [1, 65535]" in err()
    assert call(cfg3d(2048, 1024, 1024), *good, 2, 0, None, 0) == -1 and b"32-bit face indices" in err()
    assert call(c, *good, 0, 0, None, 0) == -1 and b"substeps m must be in" in err()
    assert call(c, *good, 4097, 0, None, 0) == -1 and b"substeps m must be in" in err()
    assert call(c, *good, 2, S + 1, None, 0) == -1 and b"chunk" in err()
    assert call(c, *good, 2, -1, None, 0) == -1 and b"chunk" in err()
    for k in range(7):
        args = list(good)
        args[k] = None
        assert call(c, *args, 2, 0, None, 0) == -1 and b"NULL pointer" in err(), k
    for out in (4, 5, 6):
        for src in (0, 1, 2, 3):
            args = list(good)
            args[out] = good[src]
            assert call(c, *args, 2, 0, None, 0) == -1 and b"alias" in err(), (out, src)
    for a, b in ((4, 5), (4, 6), (5, 6)):
        args = list(good)
        args[b] = good[a]
        assert call(c, *args, 2, 0, None, 0) == -1 and b"buffers of their own" in err()
    assert call(c, *good, S + 1, 0, None, 0) == -1 and b"need a workspace" in err()
    assert call(c, *good, S + 1, 0, one[7], 1024) == -1 and b"workspace too small" in err()
    assert call(c, *good, 2, 1, one[7], 1024) == -1 and b"workspace too small" in err()


# ---- the identities of the design ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", dc.PRE_SHAPES)
def test_the_substep_operator_is_symmetric_on_the_three_face_grids(shape):
    x, re = dc.pre_inputs(shape, seed=21)
    y, _ = dc.pre_inputs(shape, seed=22)
    dot = lambda a, b: float((a.double() * b.double()).sum())
    for a, b in zip(x, y):
        lhs, rhs = dot(o.laplace_replicate(a), b), dot(a, o.laplace_replicate(b))
        assert abs(lhs - rhs) < 1e-12 * abs(lhs) and abs(lhs) > 1.0
    for n in (2, 4, 8):                                      # hence M^(n-1) is its own transpose; in float32 far inside PRE_PIN of |Mx||y|
        for dtype, bound in ((torch.float64, 1e-14), (torch.float32, dc.PRE_PIN)):
            mx = dc.pre_diffuse([t.to(dtype) for t in x], re.to(dtype), shape[1], n)
            my = dc.pre_diffuse([t.to(dtype) for t in y], re.to(dtype), shape[1], n)
            lhs, rhs = sum(dot(a, b) for a, b in zip(mx, y)), sum(dot(a, b) for a, b in zip(x, my))
            scale = float(np.sqrt(sum(dot(a, a) for a in mx) * sum(dot(b, b) for b in y)))
            print("%s n=%d %s: |<Mx,y> - <x,My>| / (|Mx||y|) = %.2e" % (shape, n, dtype, abs(lhs - rhs) / scale))
            assert abs(lhs - rhs) < bound * scale


@pytest.mark.parametrize("n", [3, 5])
def test_the_composition_the_library_runs_equals_the_references_autograd(n):
    """today's step at alpha / n (re * n) applied to M^(n-1) v; its adjoint (autograd through the plain step) followed by M^(n-1); the plain
    step's re gradient at re * n, fed M^(n-1) v as a constant, times n ... against autograd through the reference, float64"""
    name = "20_comb"
    g = dc.geometry(name)
    d, v, re = dc.state(name)
    ref_out, ref_g = dc.reference(name, n)
    pv = [t.detach().clone().requires_grad_(True) for t in dc.pre_diffuse(v, re, g.X, n)]
    d_l = d.clone().requires_grad_(True)
    re_n = (re * n).clone().requires_grad_(True)          # the scaled step's coefficient dt res^2 / (n re): its gradient in (n re) is 1/n of re's ...
    od, ov = o.karman3d_step(d_l, tuple(pv), re_n, g)
    ((od * dc.w_dens(name)).sum() + sum((a * w).sum() for a, w in zip(ov, dc.w_vel(name)))).backward()
    gv = dc.pre_diffuse([t.grad for t in pv], re, g.X, n)                    # the same operator on the cotangent
    # d/d re of step(M^(n-1)(re) v; a(re)), a = dt res^2 / (n re): the n factors commute, so the plain reduction (v held fixed at M^(n-1) v,
    # the derivative of the LAST factor alone) times n.  The library scales res, so its reduction carries da / d re; this emulation scales
    # re instead, and re_n.grad carries da / d(n re) = (1 / n) da / d re: one more factor n here
    g_re = re_n.grad * n * n
    errs = [dc.maxrel(a, b) for a, b in zip((od, *ov), ref_out)] + [dc.maxrel(d_l.grad, ref_g[0])]
    errs += [dc.maxrel(a, b) for a, b in zip(gv, ref_g[1:4])] + [dc.maxrel(g_re, ref_g[4])]
    print("composition against autograd n=%d:" % n, errs)
    assert max(errs) < 1e-12


# ---- the input condition of the GPU tests: the reference in float32 against the reference in float64 -----------------------------------
@pytest.mark.parametrize("shape", dc.PRE_SHAPES)
def test_pre_diffusion_float32_against_float64(shape):
    worst = 0.0
    for n in (2, 3, 4, 5, 8, 10):
        e = max(dc.maxrel(a, b) for a, b in zip(dc.pre_reference(shape, n, dtype=torch.float32), dc.pre_reference(shape, n)))
        worst = max(worst, e)
        ref = dc.pre_reference(shape, n)
        assert all(dc.maxrel(a, b) > 0.05 for a, b in zip(dc.pre_inputs(shape)[0], ref))          # the operator does something
    print("pre-diffusion %s: %.2e (pin %.1e)" % (shape, worst, dc.PRE_PIN))
    assert worst < dc.PRE_PIN


@pytest.mark.parametrize("name,n", dc.FIELD_CASES)
def test_fields_float32_against_float64(name, n):
    ref = dc.reference(name, n)[0]
    errs = [dc.maxrel(a, b) for a, b in zip(dc.reference(name, n, dtype=torch.float32)[0], ref)]
    print("%s n=%d fields: %s (pin %.1e)" % (name, n, ["%.2e" % e for e in errs], dc.FIELD_PIN))
    assert max(errs) < dc.FIELD_PIN
    # ... and the single stencil computes something else entirely
    plain = o.karman3d_step(dc.state(name)[0], dc.state(name)[1], dc.state(name)[2], dc.geometry(name), dt=dc.case(name)["dt"], **dc.case(name)["kw"])
    assert dc.maxrel(plain[1][0], ref[1]) > 0.01


@pytest.mark.parametrize("name,n,steps,force", dc.GRAD_CASES + dc.GRAD_CASES_NO_RE + (dc.CG_CASE,))
def test_gradients_float32_against_float64_and_no_flipped_cell(name, n, steps, force):
    ref_out, ref_g = dc.reference(name, n, steps, force)
    out, g = dc.reference(name, n, steps, force, dtype=torch.float32)
    ef = [dc.maxrel(a, b) for a, b in zip(out, ref_out)]
    eg = [dc.maxrel(a, b) for a, b in zip(g, ref_g)]
    print("%s n=%d steps=%d force=%s: fields %s, gradients %s" % (name, n, steps, force, ["%.2e" % e for e in ef], ["%.2e" % e for e in eg]))
    assert max(eg[:4]) < FLIPPED, "a flipped cell: replace the case's inputs"
    assert max(ef) < dc.FIELD_PIN and max(eg[:4]) < dc.GRAD_PIN
    assert all(float(t.abs().max()) > 0 for t in ref_g)
    # g_re: a row carries the comparison only if one aligned rounding of the reduction's terms stays inside the pin
    kappa = max(dc.re_condition(name, n, steps, force))
    print("    g_re conditioning: kappa = %.0f, kappa 2^-24 = %.1e (pin %.1e)" % (kappa, kappa * 2.0 ** -24, dc.RE_PIN))
    if (name, n, steps, force) in dc.GRAD_CASES_NO_RE:
        assert kappa * 2.0 ** -24 >= dc.RE_PIN, "well conditioned: this row belongs in GRAD_CASES"
    else:
        assert kappa * 2.0 ** -24 < dc.RE_PIN, "ill conditioned: replace the row's inputs"
        assert eg[4] < dc.RE_PIN


def test_stability_figures():
    first, one = dc.stability_run(1)
    assert abs(first - 1.10) < 0.01 and one > 50.0, (first, one)
    for n in (dc.STABILITY["n"], 4):
        for dtype in (torch.float64, torch.float32):
            _, last = dc.stability_run(n, dtype)
            print("stability n=%d %s: max|v| %.6f" % (n, dtype, last))
            assert last <= 1.05 and abs(last - 1.00001) < 1e-5, (n, dtype, last)
    assert dc.stability_run(1, torch.float32)[1] > 50.0


# ---- the trainer problem -----------------------------------------------------------------------------------------------------------------
def test_trainer_reference_float32_against_float64():
    """SOL-2 at 2x32x16x16, n = 4, re = 256 / (0.45, 0.3), the golden network: the reference's unrolled loss in float32 against float64.
    TRAINER: measured loss 3.8e-8, per-step losses 6.3e-8, weight gradient 8.1e-7 relative L2 (worst layer 1.8e-5), final state 1.2e-6
    relative L2; pins in diffusion_substeps3d_cases (TRAINER_*_PIN), about 2.5 times these.  The reference with n = 1 has a loss 13 % larger
    (1372.6 against 1217.0) and a weight gradient 0.030 (relative L2) away."""
    a, b = dc.trainer_reference(), dc.trainer_reference(dtype=torch.float32)
    off = np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in o.mars_moon3d_param_shapes()])])
    el = abs(a[0] - b[0]) / abs(a[0])
    es = max(abs(x - y) / abs(x) for x, y in zip(a[1], b[1]))
    eg = rel(b[2], a[2])
    per = max(rel(b[2][off[k]:off[k + 1]], a[2][off[k]:off[k + 1]]) for k in range(len(off) - 1))
    ef = max(rel(x, y) for x, y in zip(b[3], a[3]))
    print("trainer reference float32 against float64: loss %.2e, per-step %.2e, gradient %.2e (worst layer %.2e), final state %.2e" % (el, es, eg, per, ef))
    assert el < dc.TRAINER_LOSS_PIN and es < dc.TRAINER_LOSS_PIN
    assert eg < dc.TRAINER_GRAD_PIN and per < dc.TRAINER_LAYER_PIN and ef < dc.TRAINER_FINAL_PIN
