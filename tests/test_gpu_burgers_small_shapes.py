"""The one-workgroup Burgers step and its adjoint at every kind of shape (pytest -m gpu): k_burgers_fwd / k_burgers_bwd
(csrc/burgers_step.hip) behind ops.burgers_step, torch.ops.sol.burgers_step and BurgersTest.step_with_f, against the float64 oracle
(o.burgers_step and autograd through it), with and without force.  The twin of test_gpu_burgers_large_adjoint.py for the small kernels.

Cases (burgers_small_cases.py; B = 2, nu = 0.1, seed 3, inputs rounded to fp32 values):
  * dx = 1, dt = 0.5, velocity scaled to CFL 6 at 2x2, 3x5, 5x3, 2x64, 64x2: departure points go several times round an array of 2..6
    entries (every wrap modulo Y+1 / X+1), Y << X and X << Y, and all cotangents of a component land in a handful of cells;
  * dx = 32 / Y, dt = 0.1, the amplitude as drawn at 33x17, 7x64, 64x7, 63x64, 64x63, 16x48: edges that are a multiple of nothing,
    nVy != nVx with the LDS carve's round-up to 4 floats, the last register row partly filled;
  * 64x64 at dx = 0.5, dt = 0.5, CFL 3: the largest shape that fits the LDS and the MAXTB = 17 register rows, the most arrivals per cell
    of the int32 fixed-point scatter.

Asserted per case: fields untrimmed below TOL_FIELD = 1e-5; input gradients in the trimmed metric of the large-grid test below
TOL_GRAD = 1e-4, at most 0.1 % of a component's entries left out (asserted; none where a component has fewer than 1000 entries, so the
metric is untrimmed on the tiny cases); force gradients equal dt * w to 1e-6; two calls give equal bits; a zero cotangent gives exact
zeros; a NaN cotangent in simulation 0 leaves simulation 1's gradient finite and equal, bit for bit, to its gradient in the clean batch
and to its gradient launched alone.  test_burgers_small_shapes_cpu.py shows that the float32 ORACLE meets the same conditions on the same
inputs (fields <= 1.5e-6, trimmed gradient <= 3.5e-6).

Measured on an MI355X (worst over force / no force and both components; printed by every test):
  case               CFL     fields    gradient (trimmed = untrimmed: no face flips on this device)
  2x2-dt0.5-cfl6      6.000  9.3e-08  1.3e-07
  3x5-dt0.5-cfl6      6.000  1.7e-07  2.1e-07
  5x3-dt0.5-cfl6      6.000  8.7e-08  1.5e-07
  2x64-dt0.5-cfl6     6.000  1.5e-07  2.2e-07
  64x2-dt0.5-cfl6     6.000  1.8e-07  2.6e-07
  33x17-dt0.1-drawn   0.080  1.4e-07  1.5e-07
  7x64-dt0.1-drawn    0.018  1.7e-07  1.8e-07
  64x7-dt0.1-drawn    0.159  1.7e-07  2.0e-07
  63x64-dt0.1-drawn   0.151  2.2e-07  2.2e-07
  64x63-dt0.1-drawn   0.146  2.1e-07  2.1e-07
  16x48-dt0.1-drawn   0.039  1.6e-07  1.7e-07
  64x64-dt0.5-cfl3    3.000  2.0e-07  2.8e-07
The int32 scatter's headroom of 16x one contribution holds at CFL 6 and at 64x64, CFL 3.  Not asserted, printed: under the NaN cotangent
simulation 0's own gradient comes back finite (fmaxf drops the NaN from the scatter's scale, so it quantises to zeros), where the
large-grid adjoint returns NaN for that simulation.
"""
import ctypes as C

import pytest
import torch

import sol_amd
import sol_oracle as o
from sol_amd import _lib, ops, torch_ops  # noqa: F401  (torch_ops registers torch.ops.sol.*)

import burgers_small_cases as bc
from large2d_scenes import DEV, f32

pytestmark = pytest.mark.gpu
B, NU = bc.B, bc.NU


def hip_inputs(c, Y, X, dx, dt):
    return (_lib.BurgersCfg(B, Y, X, dx, dt), ops.burgers_circ(Y, X, dt * NU),
            f32(c["vy"]), f32(c["vx"]), f32(c["fy"]), f32(c["fx"]), f32(c["wy"]), f32(c["wx"]))


def adjoint(cfg, circ, vy, vx, wy, wx):
    """sol_burgers_step_bwd into buffers pre-filled with NaN"""
    gy, gx = torch.full_like(vy, float("nan")), torch.full_like(vx, float("nan"))
    _lib.check(_lib.load().sol_burgers_step_bwd(C.byref(cfg), _lib.stream(), _lib.ptr(vy), _lib.ptr(vx), *(_lib.ptr(t) for t in circ),
                                                _lib.ptr(wy), _lib.ptr(wx), _lib.ptr(gy), _lib.ptr(gx)))
    return gy, gx


@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_step_and_adjoint_against_the_float64_oracle(case):
    Y, X, dx, dt, _ = case
    c = bc.reference(*case)
    cfg, circ, vy, vx, fy, fx, wy, wx = hip_inputs(c, Y, X, dx, dt)
    worst_f = worst_g = 0.0
    for force in (True, False):
        ry, rx, gy, gx = c["ref"][force]
        runs = []
        for _ in range(2):
            ay, ax = vy.clone().requires_grad_(True), vx.clone().requires_grad_(True)
            af, bf = (fy.clone().requires_grad_(True), fx.clone().requires_grad_(True)) if force else (None, None)
            hy, hx = ops.burgers_step(ay, ax, af, bf, cfg, circ)
            ((hy * wy).sum() + (hx * wx).sum()).backward()
            runs.append((hy.detach(), hx.detach(), ay.grad, ax.grad))
        hy, hx = runs[0][:2]
        ef = max(bc.rel(hy, ry), bc.rel(hx, rx))
        print("fields (force=%s): %.3e %.3e" % (force, bc.rel(hy, ry), bc.rel(hx, rx)))
        assert ef < bc.TOL_FIELD
        worst_f = max(worst_f, ef)
        worst_g = max(worst_g, bc.check_grad("g_vy %s force=%s" % (bc.case_id(case), force), ay.grad, gy),
                      bc.check_grad("g_vx %s force=%s" % (bc.case_id(case), force), ax.grad, gx))
        if force:
            assert bc.rel(af.grad, dt * c["wy"]) < 1e-6 and bc.rel(bf.grad, dt * c["wx"]) < 1e-6
        assert all(torch.equal(p, q) for p, q in zip(*runs)), "two calls"
    print("%-18s CFL %6.3f  fields %.1e  gradient %.1e" % (bc.case_id(case), c["cfl"], worst_f, worst_g))

    # the adjoint entry on its own: what autograd returned, exact zeros for a zero cotangent, and a NaN stays in its simulation
    clean = adjoint(cfg, circ, vy, vx, wy, wx)
    assert torch.equal(clean[0], ay.grad) and torch.equal(clean[1], ax.grad)
    zy, zx = adjoint(cfg, circ, vy, vx, torch.zeros_like(wy), torch.zeros_like(wx))
    assert bool((zy == 0.0).all()) and bool((zx == 0.0).all())
    bad = wy.clone()
    bad[0, Y // 2, X // 2] = float("nan")
    py, px = adjoint(cfg, circ, vy, vx, bad, wx)
    print("simulation 0 under a NaN cotangent: %d of %d entries non-finite" % (int((~torch.isfinite(py[0])).sum()) + int((~torch.isfinite(px[0])).sum()),
                                                                               py[0].numel() + px[0].numel()))
    assert bool(torch.isfinite(py[1]).all()) and bool(torch.isfinite(px[1]).all())
    assert torch.equal(py[1], clean[0][1]) and torch.equal(px[1], clean[1][1])
    one = _lib.BurgersCfg(1, Y, X, dx, dt)
    sy, sx = adjoint(one, circ, *(t[1:2].contiguous() for t in (vy, vx, wy, wx)))
    assert torch.equal(sy[0], py[1]) and torch.equal(sx[0], px[1])


@pytest.mark.parametrize("case", [bc.TALL, bc.WIDE], ids=bc.case_id)
def test_dispatcher_op_and_burgers_test_surface(case):
    """one tall and one wide case through torch.ops.sol.burgers_step and BurgersTest.step_with_f"""
    Y, X, dx, dt, _ = case
    c = bc.reference(*case)
    ry, rx, gy, gx = c["ref"][True]
    ay, ax = f32(c["vy"]).requires_grad_(True), f32(c["vx"]).requires_grad_(True)
    hy, hx = torch.ops.sol.burgers_step(ay, ax, f32(c["fy"]), f32(c["fx"]), dx, dt, NU)
    ((hy * f32(c["wy"])).sum() + (hx * f32(c["wx"])).sum()).backward()
    assert bc.rel(hy, ry) < bc.TOL_FIELD and bc.rel(hx, rx) < bc.TOL_FIELD
    bc.check_grad("torch.ops g_vy", ay.grad, gy)
    bc.check_grad("torch.ops g_vx", ax.grad, gx)
    dom = sol_amd.Domain([Y, X], box=sol_amd.box([dx * Y, dx * X]), boundaries=sol_amd.PERIODIC)
    stag = f32(o.staggered_tensor(c["vy"], c["vx"])).requires_grad_(True)
    st = sol_amd.BurgersVelocitySMAC(dom, velocity=stag, batch_size=B)
    fr = sol_amd.BurgersVelocitySMAC(dom, velocity=f32(o.staggered_tensor(c["fy"], c["fx"])), batch_size=B)
    out = sol_amd.BurgersTest().step_with_f(st, fr, dt=dt).velocity.staggered_tensor()
    assert bc.rel(out[:, :, :X, 0], ry) < bc.TOL_FIELD and bc.rel(out[:, :Y, :, 1], rx) < bc.TOL_FIELD
    (out * f32(o.staggered_tensor(c["wy"], c["wx"]))).sum().backward()
    bc.check_grad("BurgersTest g_vy", stag.grad[:, :, :X, 0], gy)
    bc.check_grad("BurgersTest g_vx", stag.grad[:, :Y, :, 1], gx)


@pytest.mark.parametrize("Y,X", [(1, 32), (32, 1), (65, 32), (32, 65)])
def test_edges_of_1_or_65_are_refused_without_a_launch(Y, X):
    lib = _lib.load()
    p = _lib.ptr
    cfg = _lib.BurgersCfg(B, Y, X, 1.0, 0.1)
    circ = ops.burgers_circ(Y, X, 0.1 * NU)
    vy, vx = (torch.zeros(*s, dtype=torch.float32, device=DEV) for s in ((B, Y + 1, X), (B, Y, X + 1)))
    oy, ox = torch.full_like(vy, 7.0), torch.full_like(vx, 7.0)
    with pytest.raises(_lib.SolError, match="2 <= Y,X <= 64"):
        _lib.check(lib.sol_burgers_step_fwd(C.byref(cfg), _lib.stream(), p(vy), p(vx), None, None, *(p(t) for t in circ), p(oy), p(ox)))
    with pytest.raises(_lib.SolError, match="2 <= Y,X <= 64"):
        _lib.check(lib.sol_burgers_step_bwd(C.byref(cfg), _lib.stream(), p(vy), p(vx), *(p(t) for t in circ), p(vy), p(vx), p(oy), p(ox)))
    torch.cuda.synchronize()
    assert bool((oy == 7.0).all()) and bool((ox == 7.0).all())       # nothing was launched
