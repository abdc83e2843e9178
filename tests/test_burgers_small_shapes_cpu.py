"""CPU twin of test_gpu_burgers_small_shapes.py (no GPU): on every case of burgers_small_cases.py the float32 oracle is held against
the float64 oracle under the conditions the GPU test puts on the kernels -- fields untrimmed below TOL_FIELD, input gradients in the
trimmed metric below TOL_GRAD with at most 0.1 % of a component's entries left out (none below 1000 entries) -- so that the inputs
themselves cannot hide a failure: where plain float32 arithmetic meets the bounds, a kernel that misses them is wrong.  Also: the scaled
cases reach their target CFL, and the one-workgroup entry points refuse an edge of 1 or 65 before any launch.

Measured (seed 3, torch CPU), worst over force / no force and both components, printed by every test:
  case               CFL     fields    gradient trimmed (left out)   untrimmed
  2x2-dt0.5-cfl6      6.000  7.3e-08  1.7e-07 (0)                   1.7e-07
  3x5-dt0.5-cfl6      6.000  9.7e-08  2.1e-07 (0)                   2.1e-07
  5x3-dt0.5-cfl6      6.000  1.1e-07  2.3e-07 (0)                   2.3e-07
  2x64-dt0.5-cfl6     6.000  5.7e-07  7.5e-07 (0)                   7.5e-07
  64x2-dt0.5-cfl6     6.000  1.1e-06  1.1e-06 (0)                   1.1e-06
  33x17-dt0.1-drawn   0.080  6.2e-07  1.6e-06 (1 of 1156 / 1188)    1.6e-06
  7x64-dt0.1-drawn    0.018  1.0e-06  3.0e-06 (1 of 1024, 0 of 910) 3.0e-06
  64x7-dt0.1-drawn    0.159  5.9e-07  1.3e-06 (0 of 910, 1 of 1024) 1.3e-06
  63x64-dt0.1-drawn   0.151  1.5e-06  3.5e-06 (8 of 8192 / 8190)    1.9e-05
  64x63-dt0.1-drawn   0.146  6.9e-07  1.7e-06 (8 of 8190 / 8192)    1.7e-06
  16x48-dt0.1-drawn   0.039  4.9e-07  1.1e-06 (1 of 1632 / 1568)    1.1e-06
  64x64-dt0.5-cfl3    3.000  7.4e-07  1.8e-06 (8 of 8320)           3.1e-03  (one face flips in g_vx: why the metric is trimmed)
No face flips on a tiny case (CFL 6, nothing left out) with seed 3, so every case keeps the seed of the large-grid test.
"""
import ctypes as C

import pytest
import torch

import sol_amd
from sol_amd import _lib

import burgers_small_cases as bc


@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_float32_oracle_meets_the_gpu_conditions(case):
    Y, X, dx, dt, cfl = case
    c = bc.reference(*case)
    print("%s: CFL reached %.4f" % (bc.case_id(case), c["cfl"]))
    if cfl is not None:
        assert abs(c["cfl"] - cfl) < 1e-5 * cfl                  # one fp32 factor, values rounded to fp32
    else:
        assert 0.0 < c["cfl"] < 1.0                             # the amplitude as drawn: departure points stay within one cell
    worst_f = worst_g = worst_u = 0.0
    for force in (True, False):
        ry, rx, gy, gx = c["ref"][force]
        sy, sx, hy, hx = bc.oracle(c, dx, dt, force, torch.float32)
        ef = max(bc.rel(sy, ry), bc.rel(sx, rx))
        print("fields (force=%s): %.3e %.3e" % (force, bc.rel(sy, ry), bc.rel(sx, rx)))
        assert ef < bc.TOL_FIELD
        worst_f = max(worst_f, ef)
        worst_g = max(worst_g, bc.check_grad("g_vy force=%s" % force, hy, gy), bc.check_grad("g_vx force=%s" % force, hx, gx))
        worst_u = max(worst_u, bc.rel(hy, gy), bc.rel(hx, gx))
    print("%-18s %6.3f  %.1e  %.1e  %.1e" % (bc.case_id(case), c["cfl"], worst_f, worst_g, worst_u))


def test_the_cap_is_zero_entries_below_1000():
    a, b = torch.arange(999.0), torch.arange(999.0) + 1e-3
    assert bc.trimmed_rel(a, b)[1:] == (0, 999) and bc.trimmed_rel(a, b)[0] == pytest.approx(bc.rel(a, b))
    a, b = torch.zeros(4160), torch.ones(4160)
    assert bc.trimmed_rel(a, b)[1:] == (4, 4160)
    for Y, X, *_ in bc.TINY[:3]:
        assert (Y + 1) * X < 1000 and Y * (X + 1) < 1000          # the tiny cases are untrimmed


def test_simulations_of_a_case_are_independent():
    """what the GPU test's poisoning check rests on: the oracle's gradient of simulation 1 alone is its row of the batch's gradient"""
    case = bc.TINY[1]
    c = bc.reference(*case)
    alone = bc.oracle(c, case[2], case[3], True, sims=slice(1, 2))
    for a, r in zip(alone, c["ref"][True]):
        assert torch.equal(a[0], r[1])


@pytest.mark.parametrize("Y,X", [(1, 32), (32, 1), (65, 32), (32, 65), (1, 1), (65, 65)])
def test_edges_of_1_or_65_are_refused_before_any_launch(Y, X):
    lib = sol_amd.load()
    one = C.c_void_p(256)
    cfg = _lib.BurgersCfg(2, Y, X, 1.0, 0.1)
    assert lib.sol_burgers_step_fwd(C.byref(cfg), None, *([one] * 10)) == -1 and b"2 <= Y,X <= 64" in lib.sol_last_error()
    assert lib.sol_burgers_step_bwd(C.byref(cfg), None, *([one] * 10)) == -1 and b"2 <= Y,X <= 64" in lib.sol_last_error()
    with pytest.raises(_lib.SolError, match="2 <= Y,X <= 64"):
        _lib.check(lib.sol_burgers_step_fwd(C.byref(cfg), None, *([one] * 10)))
