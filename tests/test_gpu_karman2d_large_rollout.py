"""LargeGridRollout (pytest -m gpu): the correction launch bit for bit, the roll-out at 256 x 128 against the float64 oracle loop of
test_rollout_against_oracle (o.karman_step, then o.correction), captured against eager, the handed-out correction, the warm-started CG
solve (cold equality on a zero guess, fewer iterations afterwards, the non-finite-guess fallback), the factory's routing and the
scripts generate -> train -> apply end to end.

Tolerances are the suite's (large2d_scenes): TOL_FIELD = 1e-5 relative L2 on fields, CG_RTOL = 1e-7 for solves compared with the
oracle.  One oracle roll-out per scene / network is computed once and shared (the simulations of a batch are independent: the B = 1
cases read simulation 0 of the B = 2 run)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import sol_amd
import sol_oracle as o
from sol_amd import ops, scene

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from large2d_scenes import CG_RTOL, DEV, TOL_FIELD, TWO, active_of, f32, geometry, masks, rel, state

pytestmark = pytest.mark.gpu
Y, X = 256, 128
STD_V = (0.2, 0.2)
SEED = 11


# ---- 1. the correction launch -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Yc,Xc", [(2, 5, 7), (1, 16, 130)])
def test_correct_is_fl_v_plus_fl_s_o_on_every_element(B, Yc, Xc):
    gen = torch.Generator().manual_seed(7)                   # (dtypes spelled out: other test modules set the default dtype to float64)
    out = torch.randn(B, Yc, Xc, 2, generator=gen, dtype=torch.float32)
    vy, vx = torch.randn(B, Yc + 1, Xc, generator=gen, dtype=torch.float32), torch.randn(B, Yc, Xc + 1, generator=gen, dtype=torch.float32)
    s = (0.2137, 1.731)
    s32 = [float(np.float32(v)) for v in s]                  # the scale as the fp32 kernel argument holds it
    # fl(s * o) and fl(v + fl(s * o)): the float64 product of two fp32 values is exact, the sum of two fp32 values is exact in float64
    # unless the exponents are more than 29 apart (randn values: not the case); one rounding each
    cy = (out[..., 0].double() * s32[0]).float()
    cx = (out[..., 1].double() * s32[1]).float()
    ry, rx = vy.clone(), vx.clone()
    ry[:, :Yc] = (vy[:, :Yc].double() + cy.double()).float()
    rx[:, :, :Xc] = (vx[:, :, :Xc].double() + cx.double()).float()
    for with_cor in (False, True):
        hy, hx = f32(vy), f32(vx)
        cor = (torch.full_like(hy, 9.0), torch.full_like(hx, 9.0)) if with_cor else None
        ops.karman_correct(f32(out), hy, hx, s, cor)
        assert torch.equal(hy.cpu(), ry) and torch.equal(hx.cpu(), rx)
        assert torch.equal(hy[:, Yc].cpu(), vy[:, Yc]) and torch.equal(hx[:, :, Xc].cpu(), vx[:, :, Xc])     # bit-unchanged
        if with_cor:
            assert torch.equal(cor[0][:, :Yc].cpu(), cy) and torch.equal(cor[1][:, :, :Xc].cpu(), cx)
            assert not cor[0][:, Yc].any() and not cor[1][:, :, Xc].any()


# ---- shared problems and oracle roll-outs ------------------------------------------------------------------------------------
def geom_of(specs):
    return o.KarmanGeometry(Y, X) if specs is None else geometry(Y, X, active_of(specs, Y, X))


@functools.lru_cache(maxsize=None)
def oracle_rollout(specs, mercury, B, n):
    """start state, parameters and, per step, (d, vy, vx after the corrected step, correction y, correction x) in float64"""
    g = geom_of(None if specs is None else list(specs))
    d, vy, vx, re = state(B, Y, X, SEED, g)
    params = o.init_params_mercury(1) if mercury else o.init_params(3)
    steps = []
    rd, ry, rx = d, vy, vx
    with torch.no_grad():
        for _ in range(n):
            rd, ry, rx = o.karman_step(rd, ry, rx, re, g)
            cy, cx = o.correction(params, ry, rx, re, STD_V, o.STD_RE)
            ry, rx = ry + cy, rx + cx
            steps.append((rd, ry, rx, cy, cx))
    return g, (d, vy, vx, re), params, steps


def net_of(params, mercury=False):
    net = (sol_amd.model_mercury if mercury else sol_amd.model_mars_moon)(cin=3, cout=2, seed=0)
    net.set_weights([q.detach().numpy() for q in params])
    return net


def rollout_of(g, params, B, mercury=False, solver="auto", **kw):
    mk = masks(g, solver)
    return sol_amd.LargeGridRollout(net_of(params, mercury), mk, B, Y, X, g.dx, STD_V, o.STD_RE, **kw), mk


def start(st, B):
    return tuple(f32(t[:B]) for t in st)


def assert_fields(h, ref, B, what):
    errs = [rel(a, b[:B]) for a, b in zip(h, ref)]
    print("%s: d %.3e vy %.3e vx %.3e" % ((what,) + tuple(errs)))
    assert max(errs) < TOL_FIELD, (what, errs)


# ---- 2. against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n", [(1, 1), (1, 2), (2, 3)])
def test_rollout_against_the_float64_oracle(B, n):
    g, st, params, steps = oracle_rollout(None, False, 2, 3)
    ro, mk = rollout_of(g, params, B)
    assert mk.pressure_solver == "direct"
    d, vy, vx, re = start(st, B)
    its = ro.run(d, vy, vx, re, n)
    assert its.shape == (n, B) and its.dtype == torch.int32 and not its.any()
    assert_fields((d, vy, vx), steps[n - 1][:3], B, "mars_moon roll-out B=%d n=%d" % (B, n))


def test_mercury_rollout_against_the_float64_oracle():
    g, st, params, steps = oracle_rollout(None, True, 1, 2)
    ro, _ = rollout_of(g, params, 1, mercury=True)
    d, vy, vx, re = start(st, 1)
    its = ro.run(d, vy, vx, re, 2)
    assert its.shape == (2, 1) and not its.any()
    assert_fields((d, vy, vx), steps[1][:3], 1, "mercury roll-out B=1 n=2")


# ---- 3. captured equals eager ------------------------------------------------------------------------------------------------
def test_captured_rollout_equals_the_eager_rollout_bit_for_bit():
    g, st, params, _ = oracle_rollout(None, False, 2, 3)
    rg, _ = rollout_of(g, params, 2)
    re_, _ = rollout_of(g, params, 2, use_graph=False)
    runs = []
    for ro in (rg, re_, rg):
        h = start(st, 2)
        ro.run(*h, 3)
        runs.append(h[:3])
    assert rg._graph is not None and re_._graph is None
    for a, b, c in zip(*runs):
        assert torch.equal(a, b), "captured differs from eager"
        assert torch.equal(a, c), "two captured runs differ"


# ---- 4. the handed-out correction --------------------------------------------------------------------------------------------
def test_corr_holds_the_last_steps_correction():
    g, st, params, steps = oracle_rollout(None, False, 2, 3)
    ro, mk = rollout_of(g, params, 1)
    d, vy, vx, re = start(st, 1)
    with torch.no_grad():                                    # the same launches as the roll-out's solver step: the uncorrected velocity
        _, by, bx = ops.karman_step_large(d, vy, vx, re, ro.cfg, mk)
    cor = (torch.full_like(vy, 9.0), torch.full_like(vx, 9.0))
    ro.run(d, vy, vx, re, 1, corr=cor)
    for after, before, c, name in ((vy, by, cor[0], "y"), (vx, bx, cor[1], "x")):
        diff = after.double() - before.double()              # exact in float64
        ulp = torch.nextafter(after.abs(), torch.full_like(after, float("inf"))) - after.abs()
        worst = float(((diff - c.double()).abs() / ulp.double()).max())
        print("corr %s: after - before reproduces the field within %.3f ulp of the velocity" % (name, worst))
        assert worst <= 1.0
    assert not cor[0][:, Y].any() and not cor[1][:, :, X].any()
    e_y, e_x = rel(cor[0], steps[0][3][:1]), rel(cor[1], steps[0][4][:1])
    print("corr vs oracle correction: y %.3e x %.3e" % (e_y, e_x))
    assert e_y < TOL_FIELD and e_x < TOL_FIELD


# ---- 5. / 6. CG scene: cold, warm, a non-finite guess ---------------------------------------------------------------------------
def test_two_cylinders_cold_and_warm_started():
    g, st, params, steps = oracle_rollout(tuple(TWO), False, 1, 3)
    res = {}
    for warm in (False, True):
        ro, mk = rollout_of(g, params, 1, use_graph=False, cg_warm_start=warm, cg_rtol=CG_RTOL)
        assert mk.pressure_solver == "cg"
        h = start(st, 1)
        its = ro.run(*h, 3)
        assert its.shape == (3, 1) and bool(ro.solve_info["converged"].all()), ro.solve_info
        assert_fields(h[:3], steps[2][:3], 1, "two cylinders, %s" % ("warm" if warm else "cold"))
        res[warm] = its[:, 0].tolist()
    print("CG iterations per step: cold %s warm %s" % (res[False], res[True]))
    assert res[True][0] == res[False][0]                     # a zero guess is no guess
    assert sum(res[True][1:]) < sum(res[False][1:])


def test_zero_guess_equals_no_guess_bit_for_bit():
    g, st, _, _ = oracle_rollout(tuple(TWO), False, 1, 3)
    mk = masks(g, "cg")
    cfg = ops.karman_cfg(1, Y, X, g.dx, masks=mk, cg_rtol=CG_RTOL)
    d, vy, vx, re = start(st, 1)
    with torch.no_grad():
        i0, i1 = {}, {}
        cold = ops.karman_step_large(d, vy, vx, re, cfg, mk, info=i0)
        pg = torch.zeros(1, Y, X, dtype=torch.float32, device=DEV)
        warm = ops.karman_step_large(d, vy, vx, re, cfg, mk, info=i1, p_guess=pg)
        assert all(torch.equal(a, b) for a, b in zip(cold, warm)) and torch.equal(i0["iterations"], i1["iterations"])
        assert float(pg.abs().max()) > 0                     # the step's pressure came back
        # a guess that already meets the test: the 1e-7 solve's pressure leaves a true fp32 residual of the order eps x condition number
        # (about 1e-6 |b|, which is why it cannot meet 1e-7 again), far below a tolerance of 1e-3 -- 0 iterations, converged, x = the guess
        loose = ops.karman_cfg(1, Y, X, g.dx, masks=mk, cg_rtol=1e-3)
        i2 = {}
        again = ops.karman_step_large(d, vy, vx, re, loose, mk, info=i2, p_guess=pg)
        print("iterations: cold %s, from the solution at rtol 1e-3 %s" % (i0["iterations"].tolist(), i2["iterations"].tolist()))
        assert int(i2["iterations"][0]) == 0 and int(i2["converged"][0]) == 1
        assert max(rel(a, b) for a, b in zip(again, cold)) < TOL_FIELD


def test_a_non_finite_guess_falls_back_to_zero_for_that_simulation():
    g, st, params, _ = oracle_rollout(tuple(TWO), False, 2, 1)
    runs = {}
    for warm in (False, True):
        ro, _ = rollout_of(g, params, 2, use_graph=False, cg_warm_start=warm, cg_rtol=CG_RTOL)
        if warm:
            ro.p_guess[1] = float("nan")
        h = start(st, 2)
        ro.run(*h, 1)
        assert bool(ro.solve_info["converged"].all()), ro.solve_info
        runs[warm] = (h[:3], ro.solve_info["iterations"])
    assert all(bool(torch.isfinite(t).all()) for t in runs[True][0])
    assert_fields(runs[True][0], runs[False][0], 2, "NaN guess for simulation 1 against the cold run")
    assert torch.equal(runs[True][1], runs[False][1])        # both simulations started from zero


# ---- 7. routing -----------------------------------------------------------------------------------------------------------------
def test_make_rollout_routes_by_grid():
    gs = o.geometry(64, 32)
    net = sol_amd.model_mars_moon(cin=3, cout=2, seed=3)
    small = sol_amd.make_rollout(net, ops.SceneMasks(gs.active, gs.inflow, gs.bc_mask, gs.bc_mask), 1, 64, 32, gs.dx, STD_V, o.STD_RE)
    assert type(small) is sol_amd.SolRollout
    g = o.KarmanGeometry(Y, X)
    large = sol_amd.make_rollout(net, masks(g), 1, Y, X, g.dx, STD_V, o.STD_RE)
    assert type(large) is sol_amd.LargeGridRollout


# ---- 8. scripts ----------------------------------------------------------------------------------------------------------------
def test_scripts_generate_train_apply_at_resolution_128(tmp_path):
    """karman.py -r 128 -t 7 -s 1 twice (two cylinders) -> karman_train.py for a few steps -> karman_apply.py -r 128 -t 4 -s 1 with the
    written model.pt and dataStats.pickle (the pattern of test_scripts_end_to_end_at_resolution_128): frames 0..3 of denTf / velTf /
    corTf exist and are finite, and the corrector did something in frame 1"""
    import importlib.util
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    sys.path.insert(0, sdir)

    def load(name):
        spec = importlib.util.spec_from_file_location("sol_script_rollout_" + name, os.path.join(sdir, name + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m

    obst = sum([["--obstacle", s] for s in TWO], [])
    for re_nr in (1.6e5, 3.2e5):
        load("karman").main(["-o", str(tmp_path / "hi"), "-r", "128", "-t", "7", "-s", "1", "--re", str(re_nr)] + obst)
    tf = str(tmp_path / "tf")
    loss = load("karman_train").main(["--train", str(tmp_path / "hi"), "-s", "1", "-n", "2", "-b", "1", "-t", "5", "-m", "2", "-e", "1",
                                      "--lr", "1e-4", "--tf", tf, "--seed", "0"])
    assert loss is not None and np.isfinite(loss)
    run = load("karman_apply").main(["-o", str(tmp_path / "run"), "-r", "128", "-t", "4", "-s", "1", "--stats", tf + "/dataStats.pickle",
                                     "--model", tf + "/model.pt", "--cg-warm-start"])
    for i in range(4):
        for name, shape in (("denTf", (Y, X, 1)), ("velTf", (Y + 1, X + 1, 2)), ("corTf", (Y + 1, X + 1, 2))):
            a = scene.read_zipped_array(os.path.join(run, "%s_%06d.npz" % (name, i)))
            assert a.shape[-3:] == shape and np.isfinite(a).all(), (name, i)
    assert np.abs(scene.read_zipped_array(os.path.join(run, "corTf_000001.npz"))).max() > 0
