"""The one-launch direct pressure solve of the multi-launch path (csrc/karman_solve_small.hip, option k2d_solve_one_wg) against the float64
restatement of the algorithm and against the chain of GEMM launches it replaces (pytest -m gpu).

Through ops.karman_pressure_solve_large on masks built with multi_launch=True, right-hand sides large2d_scenes.step_like_rhs, B = 1 and
B = 3, on the shape table of karman2d_multi_launch_cases.SOLVE_CASES.  Reference: precond.direct_solve_reference(blob, b) in float64.
Tolerance: the same input also runs the GEMM chain (k2d_solve_one_wg = 0); the one-launch error against float64 may be at most twice the
chain's -- both are fp32 sums of the same products in another order, so a factor of two is ordering noise and more is a bug.

Measured on an MI355X, relative L2 against float64, the worst of B = 1 and the three simulations of B = 3 (one launch / chain; the
largest single ratio was 1.67 at 48x32, simulation 0 of B = 3: 5.59e-07 against 3.35e-07):
    16x16              4.55e-07 / 3.96e-07
    48x32              5.59e-07 / 3.53e-07
    32x64              4.88e-07 / 5.93e-07
    40x24              4.82e-07 / 3.30e-07
    96x48              1.08e-06 / 1.09e-06
    128x64             7.32e-07 / 6.57e-07
    128x64_two_boxes   9.89e-07 / 9.68e-07
    512x16             7.06e-07 / 7.06e-07
    49x31              8.48e-07 / 8.89e-07      (beyond the issue's table: the instantiation with guarded loads)
    130x63             1.12e-06 / 1.24e-06      (likewise; largest single ratio 1.61)
"""
import contextlib
import functools
import os
import sys

import numpy as np
import pytest
import torch

import sol_oracle as o
from sol_amd import _lib, ops, precond

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import karman2d_multi_launch_cases as mlc
from large2d_scenes import DEV, f32, rel, state, step_like_rhs

pytestmark = pytest.mark.gpu
CASES = list(mlc.SOLVE_CASES)


@contextlib.contextmanager
def option(name, value):
    old = _lib.get_option(name)
    _lib.set_option(name, value)
    try:
        yield
    finally:
        _lib.set_option(name, old)


@functools.lru_cache(maxsize=None)
def scene(case):
    """(geometry, multi_launch masks, host blob) of a case; the header is held to the table before anything is launched"""
    Y, X = mlc.SOLVE_CASES[case][:2]
    g = mlc.solve_geometry(case)
    mk = ops.SceneMasks(g.active, g.inflow, g.bc_mask, g.bc_mask, DEV, multi_launch=True)
    blob = precond.direct_solver_blob(np.asarray(g.active), 64)
    hdr = mk.direct_header
    assert mk.large and mk.multi_launch and mk.pressure_solver == "direct"
    assert tuple(int(v) for v in hdr[3:8]) == mlc.SOLVE_WINDOWS[case]
    assert int(hdr[ops.DIRECT_HEADER_FLAGS]) & ops.DIRECT_ONE_WG
    assert ops.solve_one_wg_supported(Y, X, int(hdr[7]))
    return g, mk, blob


@functools.lru_cache(maxsize=None)
def problem(case, B):
    """(rhs float64 [B,Y,X], float64 reference): computed once, shared, never modified"""
    Y, X = mlc.SOLVE_CASES[case][:2]
    blob = scene(case)[2]
    rhs = step_like_rhs(B, Y, X)
    return rhs, np.stack([precond.direct_solve_reference(blob, r.numpy()) for r in rhs])


def solve(case, rhs, one_wg):
    g, mk, _ = scene(case)
    Y, X = mlc.SOLVE_CASES[case][:2]
    cfg = ops.karman_cfg(rhs.shape[0], Y, X, g.dx, masks=mk)
    with option("k2d_solve_one_wg", one_wg):
        p = ops.karman_pressure_solve_large(f32(rhs), cfg, mk)
    torch.cuda.synchronize()
    return p


@pytest.mark.parametrize("case", CASES)
def test_one_launch_against_float64_within_twice_the_chain(case):
    worst = [0.0, 0.0]
    for B in (1, 3):
        rhs, ref = problem(case, B)
        one, chain = solve(case, rhs, 1), solve(case, rhs, 0)
        assert bool(torch.isfinite(one).all())
        for b in range(B):
            e1, e0 = rel(one[b], ref[b]), rel(chain[b], ref[b])
            worst = [max(worst[0], e1), max(worst[1], e0)]
            print("solve %s B=%d sim %d: one launch %.3e, chain %.3e against float64" % (case, B, b, e1, e0))
            assert e1 <= 2.0 * e0, (case, B, b, e1, e0)
        # two calls give equal bits
        assert torch.equal(one, solve(case, rhs, 1))
    print("solve %s: worst one launch %.3e, chain %.3e" % (case, worst[0], worst[1]))
    # simulation 2 of B = 3 equals the same right-hand side alone at B = 1, bit for bit
    rhs3 = problem(case, 3)[0]
    assert torch.equal(solve(case, rhs3, 1)[2], solve(case, rhs3[2:3], 1)[0])


def test_the_launches_are_one_against_the_chain():
    """the profiler's launch list: k_solve_one_wg alone under the option, the GEMM chain without it"""
    case = "48x32"
    g, mk, _ = scene(case)
    rhs = f32(problem(case, 1)[0])
    cfg = ops.karman_cfg(1, 48, 32, g.dx, masks=mk)
    names = {}
    for v in (0, 1):
        with option("k2d_solve_one_wg", v):
            with _lib.profile() as prof:
                ops.karman_pressure_solve_large(rhs, cfg, mk)
            names[v] = {n: c for n, (c, _) in prof.kernels.items()}
    count = lambda d, prefix: sum(c for n, c in d.items() if n.startswith(prefix))
    assert count(names[1], "k_solve_one_wg") == 1 and count(names[1], "k_l_gemm") == 0 and count(names[1], "k_l_capacitance") == 0, names[1]
    assert count(names[0], "k_l_gemm") == 8 and count(names[0], "k_l_scale") == 2 and count(names[0], "k_l_capacitance") == 1, names[0]
    assert count(names[0], "k_solve_one_wg") == 0, names[0]


def test_default_masks_keep_the_chain_under_re_grad():
    """masks built without multi_launch at 64 x 32: the staged adjoint of re_grad (and its direct solve) gives the same bits with the
    option at 0 and at 1 -- the flag in the host header is what admits the one-launch solve, not the option alone"""
    Y, X, B = 64, 32, 2
    g = o.geometry(Y, X)
    mk = ops.SceneMasks(g.active, g.inflow, g.bc_mask, g.bc_mask, DEV)
    assert not mk.large and not mk.multi_launch and mk.pressure_solver == "direct" and int(mk.direct_header[ops.DIRECT_HEADER_FLAGS]) == 0
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk)
    d, vy, vx, re = state(B, Y, X, 77, g)
    wy, wx = mlc.cotangent_at(B, Y, X)
    got = []
    for v in (0, 1):
        with option("k2d_solve_one_wg", v):
            leaves = [f32(t).requires_grad_(True) for t in (vy, vx, re)]
            out = ops.karman_step(f32(d), leaves[0], leaves[1], leaves[2], cfg, mk, re_grad=True)
            ((out[1] * f32(wy)).sum() + (out[2] * f32(wx)).sum()).backward()
            torch.cuda.synchronize()
            got.append([t.detach() for t in out] + [t.grad for t in leaves])
    for a, b in zip(*got):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
