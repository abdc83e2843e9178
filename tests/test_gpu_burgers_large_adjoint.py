"""Adjoint of the large-grid Burgers step on the GPU (pytest -m gpu): sol_burgers_step_bwd_large (csrc/burgers_step.hip) behind
ops.burgers_step_large, BurgersTest(large_grid_grad=True) and torch.ops.sol.burgers_step, against the float64 oracle's autograd, against
the one-workgroup adjoint where both apply, bit reproducibility (eager, captured), poisoning, argument checks, and that the forward
path did not move.

Metric.  The step's gradient is discontinuous where a departure point crosses a cell boundary (floorf): fp32 and float64 decide a few
faces differently, and each such face moves a few gradient entries by O(1).  With the oracle alone (fp32 against float64) on the inputs
below the untrimmed relative L2 reaches 1.6e-4 .. 2.7e-3 on some components; after leaving out the 0.1 % of entries with the largest
deviation it is 3e-6 .. 1.2e-5 on every shape, seed and dt tried.  So the TRIMMED metric is asserted below TOL_GRAD = 1e-4 for the
gradients; each component may leave out at most 0.1 % of its entries (asserted).  Fields are checked untrimmed below TOL_FIELD = 1e-5.
Those oracle-only figures are for inputs held in float64.  The inputs here are rounded to fp32 values first, so the kernels and the
float64 oracle trace the same numbers and a face flips only where fp32 ARITHMETIC lands on the other side of a cell boundary: measured
on an MI355X, no face does on any case below, and both metrics read 1.9e-7 .. 2.9e-7 (printed by every test).  The trimmed metric and
its cap stay the assertion: a flip on another device or compiler is the expected event it allows for, not a defect.

Inputs: B = 2, nu = 0.1, dx = 32 / Y, generator seed 3, v = amp * smooth(randn), f = 0.2 * smooth(randn), cotangents randn, drawn in
the order vy, vx, fy, fx, wy, wx and rounded to fp32 values (the oracle and the kernels see the same numbers).  Shapes: (70, 36) tall
with partial 16 x 16 tiles on both axes, (24, 100) wide, (128, 128) the reference's hi-res setting, each at dt = 0.1, amp = 0.8; and
(70, 36) at dt = 0.5, amp = 3.0, where departure points land several cells away and wrap across both seams modulo Y+1 / X+1."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

import sol_amd
import sol_oracle as o
from sol_amd import _lib, ops, torch_ops  # noqa: F401  (torch_ops registers torch.ops.sol.*)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from large2d_scenes import DEV, TOL_FIELD, TOL_GRAD, f32, rel

pytestmark = pytest.mark.gpu
TRIM = 1e-3                                          # a cap, not a tuning knob (module docstring)
B, NU = 2, 0.1
CASES = [(70, 36, 0.1, 0.8), (24, 100, 0.1, 0.8), (128, 128, 0.1, 0.8), (70, 36, 0.5, 3.0)]


def trimmed_rel(a, b, frac=TRIM):
    """relative L2 of a against b after leaving out the floor(frac * n) entries with the largest |a - b| (the norm of b is taken over
    the entries kept) -> (value, entries left out, entries in all)"""
    a = torch.as_tensor(np.asarray(a.detach().cpu()), dtype=torch.float64).reshape(-1)
    b = torch.as_tensor(np.asarray(b.detach().cpu()), dtype=torch.float64).reshape(-1)
    dev = (a - b).abs()
    k = int(frac * dev.numel())
    if k == 0:
        return float(dev.norm() / (b.norm() + 1e-300)), 0, dev.numel()
    keep = torch.argsort(dev)[:-k]
    return float(dev[keep].norm() / (b[keep].norm() + 1e-300)), k, dev.numel()


def check_grad(name, got, ref):
    t, k, n = trimmed_rel(got, ref)
    print("%s: trimmed %.3e (left out %d of %d), untrimmed %.3e" % (name, t, k, n, rel(got, ref)))
    assert k <= TRIM * n
    assert t < TOL_GRAD, (name, t)


@functools.lru_cache(maxsize=None)
def case(Y, X, dt, amp):
    """inputs (float64 tensors holding fp32 values) and the oracle's outputs / gradients, with and without force; computed once"""
    gen = torch.Generator().manual_seed(3)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    r32 = lambda t: t.float().double()
    vy, vx = r32(amp * o._smooth(rn(B, Y + 1, X))), r32(amp * o._smooth(rn(B, Y, X + 1)))
    fy, fx = r32(0.2 * o._smooth(rn(B, Y + 1, X))), r32(0.2 * o._smooth(rn(B, Y, X + 1)))
    wy, wx = r32(rn(B, Y + 1, X)), r32(rn(B, Y, X + 1))
    dx = 32.0 / Y
    ref = {}
    for force in (True, False):
        ay, ax = vy.clone().requires_grad_(True), vx.clone().requires_grad_(True)
        ry, rx = o.burgers_step(ay, ax, dt, NU, fy if force else None, fx if force else None, dx=dx)
        ((ry * wy).sum() + (rx * wx).sum()).backward()
        ref[force] = (ry.detach(), rx.detach(), ay.grad, ax.grad)
    return dict(vy=vy, vx=vx, fy=fy, fx=fx, wy=wy, wx=wx, dx=dx, ref=ref)


def hip_inputs(c, Y, X, dt):
    return (sol_amd._lib.BurgersCfg(B, Y, X, c["dx"], dt), ops.burgers_circ(Y, X, dt * NU),
            f32(c["vy"]), f32(c["vx"]), f32(c["fy"]), f32(c["fx"]), f32(c["wy"]), f32(c["wx"]))


@pytest.mark.parametrize("Y,X,dt,amp", CASES)
def test_ops_burgers_step_large_gradient_against_oracle(Y, X, dt, amp):
    c = case(Y, X, dt, amp)
    cfg, circ, vy, vx, fy, fx, wy, wx = hip_inputs(c, Y, X, dt)
    for force in (True, False):
        ry, rx, gy, gx = c["ref"][force]
        ay, ax = vy.clone().requires_grad_(True), vx.clone().requires_grad_(True)
        af, bf = (fy.clone().requires_grad_(True), fx.clone().requires_grad_(True)) if force else (None, None)
        hy, hx = ops.burgers_step_large(ay, ax, af, bf, cfg, circ)
        ((hy * wy).sum() + (hx * wx).sum()).backward()
        print("fields (force=%s): %.3e %.3e" % (force, rel(hy, ry), rel(hx, rx)))
        assert rel(hy, ry) < TOL_FIELD and rel(hx, rx) < TOL_FIELD
        check_grad("g_vy %dx%d dt=%g force=%s" % (Y, X, dt, force), ay.grad, gy)
        check_grad("g_vx %dx%d dt=%g force=%s" % (Y, X, dt, force), ax.grad, gx)
        if force:
            assert rel(af.grad, dt * c["wy"]) < 1e-6 and rel(bf.grad, dt * c["wx"]) < 1e-6
        # calls without grad: the same forward launches, the same bits, nothing kept
        with torch.no_grad():
            ny, nx = ops.burgers_step_large(vy, vx, af, bf, cfg, circ)
        assert torch.equal(ny, hy) and torch.equal(nx, hx) and ny.grad_fn is None


@pytest.mark.parametrize("Y,X,dt,amp", CASES[:2])
def test_burgers_test_surface_and_dispatcher_op(Y, X, dt, amp):
    """The same gradient through BurgersTest(large_grid_grad=True).step_with_f and through torch.ops.sol.burgers_step; the
    default-constructed BurgersTest still refuses."""
    c = case(Y, X, dt, amp)
    ry, rx, gy, gx = c["ref"][True]
    dom = sol_amd.Domain([Y, X], box=sol_amd.box([32.0, 32.0 * X / Y]), boundaries=sol_amd.PERIODIC)
    stag = f32(o.staggered_tensor(c["vy"], c["vx"])).requires_grad_(True)
    st = sol_amd.BurgersVelocitySMAC(dom, velocity=stag, batch_size=B)
    fr = sol_amd.BurgersVelocitySMAC(dom, velocity=f32(o.staggered_tensor(c["fy"], c["fx"])), batch_size=B)
    out = sol_amd.BurgersTest(large_grid_grad=True).step_with_f(st, fr, dt=dt).velocity.staggered_tensor()
    assert rel(out, o.staggered_tensor(ry, rx)) < TOL_FIELD
    (out * f32(o.staggered_tensor(c["wy"], c["wx"]))).sum().backward()
    check_grad("BurgersTest g_vy", stag.grad[:, :, :X, 0], gy)
    check_grad("BurgersTest g_vx", stag.grad[:, :Y, :, 1], gx)
    with pytest.raises(NotImplementedError, match="large_grid_grad"):
        st2 = sol_amd.BurgersVelocitySMAC(dom, velocity=f32(o.staggered_tensor(c["vy"], c["vx"])).requires_grad_(True), batch_size=B)
        sol_amd.BurgersTest().step(st2, dt=dt)
    ay, ax = f32(c["vy"]).requires_grad_(True), f32(c["vx"]).requires_grad_(True)
    hy, hx = torch.ops.sol.burgers_step(ay, ax, f32(c["fy"]), f32(c["fx"]), c["dx"], dt, NU)
    ((hy * f32(c["wy"])).sum() + (hx * f32(c["wx"])).sum()).backward()
    assert rel(hy, ry) < TOL_FIELD and rel(hx, rx) < TOL_FIELD
    check_grad("torch.ops g_vy", ay.grad, gy)
    check_grad("torch.ops g_vx", ax.grad, gx)


def test_large_adjoint_equals_the_one_workgroup_adjoint_at_64x64():
    """At 64 x 64 both kernels apply.  They share the fp32 floor decisions (same expressions on the same input), so no trimming: the
    LDS kernel scatters in int32 fixed point, the large one in int64."""
    Y = X = 64
    c = case(Y, X, 0.1, 0.8)
    cfg, circ, vy, vx, fy, fx, wy, wx = hip_inputs(c, Y, X, 0.1)
    sy, sx = torch.empty_like(vy), torch.empty_like(vx)
    _lib.check(_lib.load().sol_burgers_step_bwd(C.byref(cfg), _lib.stream(), _lib.ptr(vy), _lib.ptr(vx), *(_lib.ptr(t) for t in circ),
                                                _lib.ptr(wy), _lib.ptr(wx), _lib.ptr(sy), _lib.ptr(sx)))
    ly, lx = ops.burgers_step_large_bwd(vy, vx, wy, wx, cfg, circ)
    print("large vs one-workgroup adjoint at 64x64: %.3e %.3e" % (rel(ly, sy), rel(lx, sx)))
    assert rel(ly, sy) < TOL_GRAD and rel(lx, sx) < TOL_GRAD


def test_bit_reproducibility_eager_and_captured_and_forward_unmoved():
    Y, X, dt = 70, 36, 0.5
    c = case(Y, X, dt, 3.0)
    cfg, circ, vy, vx, fy, fx, wy, wx = hip_inputs(c, Y, X, dt)
    ws = torch.empty((ops.burgers_large_workspace_bytes(cfg) + 3) // 4, dtype=torch.float32, device=DEV)
    with torch.no_grad():
        before = ops.burgers_step_large(vy, vx, fy, fx, cfg, circ, ws)
    g1 = ops.burgers_step_large_bwd(vy, vx, wy, wx, cfg, circ, ws)
    g2 = ops.burgers_step_large_bwd(vy, vx, wy, wx, cfg, circ)                 # a fresh workspace
    assert torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1])
    with torch.no_grad():
        after = ops.burgers_step_large(vy, vx, fy, fx, cfg, circ, ws)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    # the autograd form runs the same launches
    ay, ax = vy.clone().requires_grad_(True), vx.clone().requires_grad_(True)
    hy, hx = ops.burgers_step_large(ay, ax, fy, fx, cfg, circ, ws)
    ((hy * wy).sum() + (hx * wx).sum()).backward()
    assert torch.equal(hy, before[0]) and torch.equal(hx, before[1])
    assert torch.equal(ay.grad, g1[0]) and torch.equal(ax.grad, g1[1])
    # captured and replayed: kernel nodes only (capture_graph refuses anything else), the same bits
    res = {}

    def body():
        with torch.no_grad():
            res["out"] = ops.burgers_step_large(vy, vx, fy, fx, cfg, circ, ws)
            res["g"] = ops.burgers_step_large_bwd(vy, vx, wy, wx, cfg, circ, ws)

    graph = _lib.capture_graph(body, "burgers large forward + adjoint")
    census = _lib.graph_census(graph.raw_cuda_graph())
    assert set(census) <= {"kernel", "empty"} and census["kernel"] == 5 + 7, census
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(res["out"][0], before[0]) and torch.equal(res["out"][1], before[1])
    assert torch.equal(res["g"][0], g1[0]) and torch.equal(res["g"][1], g1[1])


def test_non_finite_cotangent_poisons_its_simulation_only():
    Y, X, dt = 70, 36, 0.1
    c = case(Y, X, dt, 0.8)
    cfg, circ, vy, vx, fy, fx, wy, wx = hip_inputs(c, Y, X, dt)
    clean = ops.burgers_step_large_bwd(vy, vx, wy, wx, cfg, circ)
    bad = wy.clone()
    bad[0, 5, 7] = float("inf")
    gy, gx = ops.burgers_step_large_bwd(vy, vx, bad, wx, cfg, circ)
    assert bool(torch.isnan(gy[0]).all()) and bool(torch.isnan(gx[0]).all())
    assert torch.equal(gy[1], clean[0][1]) and torch.equal(gx[1], clean[1][1])
    assert bool(torch.isfinite(clean[0]).all()) and bool(torch.isfinite(clean[1]).all())


def test_bad_arguments_are_rejected_without_a_launch():
    Y, X, dt = 70, 36, 0.1
    c = case(Y, X, dt, 0.8)
    cfg, circ, vy, vx, fy, fx, wy, wx = hip_inputs(c, Y, X, dt)
    lib = _lib.load()
    p = _lib.ptr
    gy, gx = torch.full_like(vy, 7.0), torch.full_like(vx, 7.0)
    nbytes = lib.sol_burgers_step_bwd_large_workspace_bytes(C.byref(cfg))
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=DEV)
    good = [p(vy), p(vx), *(p(t) for t in circ), p(wy), p(wx), p(gy), p(gx), p(ws)]
    for k in range(len(good)):                               # every pointer argument
        args = list(good)
        args[k] = None
        assert lib.sol_burgers_step_bwd_large(C.byref(cfg), _lib.stream(), *args, nbytes) != 0
        assert b"NULL" in lib.sol_last_error()
    assert lib.sol_burgers_step_bwd_large(C.byref(cfg), _lib.stream(), *good, nbytes - 1) != 0
    assert b"workspace too small" in lib.sol_last_error()
    big = sol_amd._lib.BurgersCfg(B, 1025, X, c["dx"], dt)
    assert lib.sol_burgers_step_bwd_large(C.byref(big), _lib.stream(), *good, nbytes) != 0
    assert b"1024" in lib.sol_last_error()
    torch.cuda.synchronize()
    assert bool((gy == 7.0).all()) and bool((gx == 7.0).all())       # nothing was launched
    with pytest.raises(_lib.SolError, match="workspace too small"):
        _lib.check(lib.sol_burgers_step_bwd_large(C.byref(cfg), _lib.stream(), *good, 16))
