"""LargeGridTrainer (pytest -m gpu): the training step at 256 x 128 against the float64 oracle, captured against eager, the hand-written
schedule against the autograd composition on a CG scene, Adam, the factory's routing and the scripts end to end.

Tolerances are the suite's: 1e-5 on the loss, TOL_GRAD = 1e-4 relative L2 on the full weight gradient (untrimmed), 1e-6 captured
against eager, 1e-5 schedule against autograd."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import sol_amd
import sol_oracle as o
from sol_amd import _lib, karman, ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from large2d_scenes import CG_RTOL, DEV, TOL_GRAD, TWO, active_of, f32, geometry, rel, state

pytestmark = pytest.mark.gpu
Y, X = 256, 128
STD_V = (0.2, 0.2)
SEED = 11
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def problem(seed, B=1, ms=2, g=None, mercury=False, dtype=torch.float64):
    """spun-up state (large2d_scenes.state), ground truth = the oracle's roll-out of the state perturbed by 0.05 x a second noise
    field, weights with a small last layer -- o.bench_workload's recipe on the given scene; everything rounded to fp32 values"""
    r32 = lambda t: t.detach().float().double()
    g = o.KarmanGeometry(Y, X) if g is None else g
    d, vy, vx, re = state(B, Y, X, seed, g)
    with torch.no_grad():
        _, py, px = o.synthetic_state(B, Y, X, 4321 + seed, project_it=False)
        gd, gy, gx = d, r32(vy + 0.05 * (py - 1.0)), r32(vx + 0.05 * px)
        gts_y, gts_x = [], []
        for _ in range(ms):
            gd, gy, gx = (r32(t) for t in o.karman_step(gd, gy, gx, re, g))
            gts_y.append(gy)
            gts_x.append(gx)
    params = [r32(p) for p in (o.init_params_mercury(1) if mercury else o.init_params(0))]
    params[-2] = r32(params[-2] * 0.01)
    cast = lambda t: t.to(dtype)
    return {"g": g, "d": cast(d), "vy": cast(vy), "vx": cast(vx), "re": cast(re), "gt_vy": [cast(t) for t in gts_y],
            "gt_vx": [cast(t) for t in gts_x], "params": [cast(p).requires_grad_(True) for p in params]}


def oracle_loss_grad(p, dtype=torch.float64):
    """(loss, flat gradient) of o.unrolled_loss in `dtype` (the geometry's arrays are float64 numpy: the oracle casts them)"""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        loss = o.unrolled_loss(p["params"], p["d"], p["vy"], p["vx"], p["re"], p["gt_vy"], p["gt_vx"], p["g"], STD_V, o.STD_RE)
        loss.backward()
    finally:
        torch.set_default_dtype(prev)
    return float(loss.detach()), torch.cat([q.grad.reshape(-1) for q in p["params"]])


def batch(p):
    return (f32(p["d"]), f32(p["vy"]), f32(p["vx"]), f32(p["re"]), f32(torch.stack(p["gt_vy"])), f32(torch.stack(p["gt_vx"])))


def net_of(p, mercury=False):
    net = (sol_amd.model_mercury if mercury else sol_amd.model_mars_moon)(cin=3, cout=2, seed=0)
    net.set_weights([q.detach().numpy() for q in p["params"]])
    return net


def test_large_grid_trainer_against_the_float64_oracle():
    """mars_moon, 256 x 128, B = 1, SOL-2, default sphere, direct solve: loss 1e-5, full weight gradient 1e-4 (untrimmed).
    The advection's floorf makes the gradient discontinuous, so the state seed is conditioned on the ORACLE alone: seed 11 (the
    seed of the large-grid adjoint tests) was kept after running o.unrolled_loss on the CPU in float32 and in float64.
    Measured with the oracle alone, float32 against float64: loss 6.1e-8, weight gradient 4.0e-7 relative L2 (seeds 12 and 13: 5.0e-7,
    4.6e-7) -- 250x inside the tolerance: with the small last layer no departure point decides the comparison."""
    p = problem(SEED)
    lref, gref = oracle_loss_grad(p)
    tr = sol_amd.LargeGridTrainer(net_of(p), 1, Y, X, 2, STD_V, o.STD_RE, use_graph=False)
    loss = float(tr.fwd_bwd(*batch(p)))
    assert tr.pressure_solver_used == "direct"
    e_l, e_g = abs(loss - lref) / abs(lref), rel(tr.grads, gref)
    print("LargeGridTrainer vs float64 oracle: loss %.3e, gradient %.3e" % (e_l, e_g))
    assert e_l < 1e-5 and e_g < TOL_GRAD, (e_l, e_g)


@pytest.mark.parametrize("mercury", [True, False])
def test_captured_step_equals_the_eager_step(mercury):
    ps = [problem(SEED + it, mercury=mercury) for it in range(2)]
    tg = sol_amd.LargeGridTrainer(net_of(ps[0], mercury), 1, Y, X, 2, STD_V, o.STD_RE)
    te = sol_amd.LargeGridTrainer(net_of(ps[0], mercury), 1, Y, X, 2, STD_V, o.STD_RE, use_graph=False)
    for p in ps:
        lg, le = float(tg.fwd_bwd(*batch(p))), float(te.fwd_bwd(*batch(p)))
        e_g = rel(tg.grads, te.grads)
        print("captured vs eager (%s): loss %.3e gradient %.3e" % ("mercury" if mercury else "mars_moon", abs(lg - le) / abs(le), e_g))
        assert tg._graph is not None and te._graph is None
        assert abs(lg - le) <= 1e-6 * abs(le) and e_g < 1e-6


def test_two_cylinders_cg_schedule_equals_the_autograd_composition():
    g = geometry(Y, X, active_of(TWO, Y, X))
    p = problem(SEED, g=g)
    kw = dict(obstacles=karman.parse_obstacles(TWO), cg_rtol=CG_RTOL, cg_max_iter=600, use_graph=False)
    net = net_of(p)
    tr = sol_amd.LargeGridTrainer(net, 1, Y, X, 2, STD_V, o.STD_RE, **kw)
    args = batch(p)
    loss = float(tr.fwd_bwd(*args))
    g1 = tr.grads.clone()
    assert tr.pressure_solver_used == "cg"
    info = tr.solve_info
    assert info["iterations_bwd"].shape == (1, 1) and int(info["iterations_bwd"].min()) > 0
    assert bool(info["converged_bwd"].all()) and bool(info["converged"].all())
    assert float(tr.fwd_bwd(*args)) == loss and torch.equal(tr.grads, g1)          # bit-identical run to run
    # the same kernels composed by autograd: ops.karman_step_large + the network's __call__
    mk, cfg = tr._mk, tr._kcfg
    net2 = net_of(p)
    net2.params.requires_grad_(True)
    d, vy, vx, re, gt_vy, gt_vx = args
    si = torch.tensor([STD_V[0], STD_V[1], o.STD_RE], device=DEV)
    so = torch.tensor(STD_V, device=DEV)
    losses = []
    with sol_amd.trainer._conv_precision_scope(tr.conv_precision):
        for i in range(2):
            d, vy, vx = ops.karman_step_large(d, vy, vx, re, cfg, mk)
            feat = torch.stack([vy[:, :Y], vx[:, :, :X], re.reshape(1, 1, 1).expand(1, Y, X)], dim=-1) / si
            out = net2(feat) * so
            vy = vy + _lib.pad_high(out[..., 0], 1)
            vx = vx + _lib.pad_high(out[..., 1], 2)
            losses.append(ops.l2_loss((vy, vx), (gt_vy[i], gt_vx[i]), STD_V))
        la = torch.stack(losses).sum() / 2
        la.backward()
    la = float(la.detach())
    e_l, e_g = abs(loss - la) / abs(la), rel(g1, net2.params.grad)
    print("schedule vs autograd (two cylinders, CG): loss %.3e gradient %.3e, iterations_bwd %s" % (e_l, e_g, info["iterations_bwd"].tolist()))
    assert e_l < 1e-5 and e_g < 1e-5, (e_l, e_g)


def test_captured_cg_step_equals_the_eager_step():
    """use_graph=True on a CG scene (two cylinders): the captured step issues the whole cg_max_iter budget per solve (300 here, the
    solves need fewer than 200 at the default tolerance) and must reproduce the eager step, which stops at convergence: 1e-6 on loss
    and gradient as in the direct-solve case; solve_info is refilled by the replay."""
    g = geometry(Y, X, active_of(TWO, Y, X))
    p = problem(SEED, g=g)
    kw = dict(obstacles=karman.parse_obstacles(TWO), cg_max_iter=300)
    tg = sol_amd.LargeGridTrainer(net_of(p), 1, Y, X, 2, STD_V, o.STD_RE, **kw)
    te = sol_amd.LargeGridTrainer(net_of(p), 1, Y, X, 2, STD_V, o.STD_RE, use_graph=False, **kw)
    args = batch(p)
    for _ in range(2):
        lg, le = float(tg.fwd_bwd(*args)), float(te.fwd_bwd(*args))
        e_g = rel(tg.grads, te.grads)
        print("captured vs eager (two cylinders, CG): loss %.3e gradient %.3e, iterations %s / %s" % (
            abs(lg - le) / abs(le), e_g, tg.solve_info["iterations"].tolist(), tg.solve_info["iterations_bwd"].tolist()))
        assert tg._graph is not None and tg.pressure_solver_used == "cg"
        assert abs(lg - le) <= 1e-6 * abs(le) and e_g < 1e-6
        for k in ("converged", "converged_bwd"):
            assert bool(tg.solve_info[k].all()), (k, tg.solve_info)
        assert torch.equal(tg.solve_info["iterations"], te.solve_info["iterations"])
        assert int(tg.solve_info["iterations"].max()) < 300


def test_adam_step_and_routing():
    p = problem(SEED)
    for mercury in (False, True):
        net = net_of(problem(SEED, mercury=True), True) if mercury else net_of(p)
        tr = sol_amd.make_trainer(net, None, 1, Y, X, 2, 100.0 / X, STD_V, o.STD_RE, use_graph=False)
        assert isinstance(tr, sol_amd.LargeGridTrainer)
    before = net_of(p).params.detach().clone()
    net = net_of(p)
    tr = sol_amd.make_trainer(net, None, 1, Y, X, 2, 100.0 / X, STD_V, o.STD_RE, use_graph=False)
    tr.train_step(*batch(p), 1e-4)
    assert tr.t == 1 and float((net.params.detach() - before).abs().max()) > 0


def test_scripts_end_to_end_at_resolution_128(tmp_path):
    """scripts/karman.py -r 128 -t 7 -s 1 (256 x 128 frames, two cylinders) -> scripts/karman_train.py -s 1 --msteps 2 for a few steps
    (the pattern of test_scripts_end_to_end_with_obstacles): runs through on the set's scene and writes a model"""
    import importlib.util
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    sys.path.insert(0, sdir)

    def load(name):
        spec = importlib.util.spec_from_file_location("sol_script_large_" + name, os.path.join(sdir, name + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m

    obst = sum([["--obstacle", s] for s in TWO], [])
    for re_nr in (1.6e5, 3.2e5):                    # two simulations: one Reynolds number alone has no spread to normalise by
        hi = load("karman").main(["-o", str(tmp_path / "hi"), "-r", "128", "-t", "7", "-s", "1", "--re", str(re_nr)] + obst)
    with open(hi + "/params.pickle", "rb") as f:
        rec = pickle.load(f)["scene"]
    tf = str(tmp_path / "tf")
    loss = load("karman_train").main(["--train", str(tmp_path / "hi"), "-s", "1", "-n", "2", "-b", "1", "-t", "5", "-m", "2", "-e", "1",
                                      "--lr", "1e-4", "--tf", tf, "--seed", "0"])
    assert loss is not None and np.isfinite(loss)
    with open(tf + "/dataStats.pickle", "rb") as f:
        assert pickle.load(f)["scene"] == rec
    assert os.path.exists(tf + "/model.pt")
