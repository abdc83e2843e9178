"""Training and roll-out on row widths the convolutions refuse (pytest -m gpu): NetSchedule2D(any_width=True) against torch float64
autograd, LargeGridTrainer / LargeGridRollout(any_width=True) at 144 x 72 and BurgersTrainer / BurgersRollout(any_width=True) at
24 x 100 and 48 x 48 against the float64 oracle, captured against eager, and scripts/karman_train.py --any-width end to end.

Tolerances are the suite's: the network against torch float64 as test_gpu_parity.test_mars_moon_network_full_size_against_torch_
float64_autograd (output 5e-6, input gradient 1e-5, kernels 3e-5, biases 1e-4); 1e-5 on a loss, TOL_GRAD = 1e-4 relative L2 on the
full weight gradient (untrimmed), TOL_FIELD = 1e-5 on fields, 1e-6 captured against eager, CG_RTOL for solves compared with the oracle."""
import functools
import os
import pickle
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sol_amd
import sol_oracle as o
from sol_amd import _lib, karman
from sol_amd.schedule2d import NetSchedule2D, row_pitch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from large2d_scenes import CG_RTOL, DEV, TOL_FIELD, TOL_GRAD, TWO, active_of, f32, geometry, masks, rel, state

pytestmark = pytest.mark.gpu
Y, X = 144, 72                        # the karman-2d grid of this file: scripts/karman.py -r 72 (pitch 128)
STD_V = (0.2, 0.2)
# State seeds, conditioned on the ORACLE alone (o.unrolled_loss / o.burgers_unrolled_loss on the CPU in float32 against float64; relative
# deviation of the loss, relative L2 of the flat weight gradient).  The advection's floorf and the LeakyReLU kinks make the gradient
# discontinuous: a seed is kept when no such point decides the comparison.
#   karman 144 x 72, default sphere (kept when >= 50x inside 1e-5 / 1e-4):  seed 16: loss 6.7e-8, gradient 6.8e-7 (150x, 147x)
#       (seeds 11 .. 15, 17 .. 23: loss 8.4e-8 .. 1.1e-6 -- fp32 rounding of the oracle's own sum --, gradient 3.3e-7 .. 1.0e-6)
#   karman 144 x 72, two cylinders:  seed 18: loss 5.8e-8, gradient 1.7e-6 (170x, 59x)   (seeds 11 .. 21: loss up to 1.9e-6, gradient 6.6e-7 .. 1.7e-6)
#   Burgers (kept when < 1e-5, the rule of test_gpu_burgers_large_trainer.py):
#       24 x 100: seed 3: loss 8.5e-8, gradient 4.8e-6   (seed 1: 2.4e-5, seed 5: 2.7e-6, seed 7: 4.2e-5)
#       48 x 48:  seed 5: loss 6.3e-8, gradient 1.9e-7   (seed 3: 1.6e-5, seed 1: 3.0e-6, seed 7: 4.3e-6)
SEED, SEED_TWO = 16, 18


# ---- 1. the schedule against torch float64 autograd --------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(16, 72), (12, 100)])
@pytest.mark.parametrize("model", ["mars_moon", "mercury"])
def test_schedule_on_pitched_rows_against_torch_float64_autograd(model, H, W):
    """forward, input gradient and flat weight gradient of NetSchedule2D(any_width=True) at B = 1 against plain PyTorch float64
    F.conv2d + autograd on the dense tensors (shares nothing with oracle/ or the product); the reference applies the activation
    with the HIP forward's sign masks, as the test this one is modelled on (one pre-activation that rounds across zero would decide
    the comparison otherwise).  Biases are non-zero: an unmasked pad column would carry them into the next layer's halo."""
    mk = sol_amd.model_mercury if model == "mercury" else sol_amd.model_mars_moon
    net = mk(cin=3, cout=2, seed=5, device=DEV)
    gen = torch.Generator().manual_seed(31 + W)
    with torch.no_grad():
        for k in range(1, len(net.shapes), 2):
            net.params[net.offsets[k]:net.offsets[k + 1]] = (0.1 * torch.randn(net.shapes[k], generator=gen)).to(DEV)
    x = torch.randn(1, H, W, 3, generator=gen, dtype=torch.float32).to(DEV)
    gy = (torch.randn(1, H, W, 2, generator=gen, dtype=torch.float32) * 1e-3).to(DEV)
    sch = NetSchedule2D(net, 1, H, W, any_width=True)
    assert sch.pitched and sch.P == row_pitch(H, W) == 128
    with torch.no_grad():
        sch.begin_step()
        out, st = sch.forward(x)
        dx = sch.backward(st, gy)
        grad = sch.end_step().clone()
    torch.cuda.synchronize()
    assert out.shape == (1, H, W, 2) and dx.shape == (1, H, W, 3)
    acts = st[2]
    for t in [st[0]] + list(acts):
        assert t.shape[2] == 128 and not t[:, :, W:].any()                   # pitched, pad columns zero
    m = [(t[:, :, :W] > 0).permute(0, 3, 1, 2) for t in acts]
    p, sl = [t.detach() for t in net.tensors()], net.slope
    tp = [t.double().clone().requires_grad_(True) for t in p]
    conv = lambda t, k: F.conv2d(t, tp[2 * k].permute(3, 2, 0, 1), tp[2 * k + 1], padding=2)
    lrelu = lambda z, mm: z * torch.where(mm, 1.0, sl).to(z.dtype)
    xt = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    if model == "mars_moon":
        h = lrelu(conv(xt, 0), m[0])
        for k in range(5):
            a = lrelu(conv(h, 1 + 2 * k), m[1 + 2 * k])
            h = lrelu(conv(a, 2 + 2 * k) + h, m[2 + 2 * k])
        ref = conv(h, 11)
    else:
        h = lrelu(conv(xt, 0), m[0])
        ref = conv(lrelu(conv(h, 1), torch.cat([m[1], m[2]], dim=1)), 2)
    (ref * gy.double().permute(0, 3, 1, 2)).sum().backward()
    off = net.offsets
    per = [rel(grad[off[k]:off[k + 1]], tp[k].grad.reshape(-1)) for k in range(len(tp))]
    e_out, e_x = rel(out, ref.detach().permute(0, 2, 3, 1)), rel(dx, xt.grad.permute(0, 2, 3, 1))
    print("%s [1,%d,%d] pitched vs torch float64: out %.2e, dx %.2e, kernels %.2e, biases %.2e" % (model, H, W, e_out, e_x, max(per[0::2]), max(per[1::2])))
    assert e_out < 5e-6 and e_x < 1e-5 and max(per[0::2]) < 3e-5 and max(per[1::2]) < 1e-4, (e_out, e_x, per)


# ---- 2. karman-2d: LargeGridTrainer(any_width=True) at 144 x 72 ------------------------------------------------------------------
def problem(seed, g=None, ms=2, dtype=torch.float64):
    """test_gpu_karman2d_large_trainer.problem restated for 144 x 72, B = 1: spun-up state, ground truth = the oracle's roll-out of the
    state perturbed by 0.05 x a second noise field, mars_moon weights with a small last layer; everything rounded to fp32 values"""
    r32 = lambda t: t.detach().float().double()
    g = o.KarmanGeometry(Y, X) if g is None else g
    d, vy, vx, re = state(1, Y, X, seed, g)
    with torch.no_grad():
        _, py, px = o.synthetic_state(1, Y, X, 4321 + seed, project_it=False)
        gd, gy, gx = d, r32(vy + 0.05 * (py - 1.0)), r32(vx + 0.05 * px)
        gts_y, gts_x = [], []
        for _ in range(ms):
            gd, gy, gx = (r32(t) for t in o.karman_step(gd, gy, gx, re, g))
            gts_y.append(gy)
            gts_x.append(gx)
    params = [r32(p) for p in o.init_params(0)]
    params[-2] = r32(params[-2] * 0.01)
    cast = lambda t: t.to(dtype)
    return {"g": g, "d": cast(d), "vy": cast(vy), "vx": cast(vx), "re": cast(re), "gt_vy": [cast(t) for t in gts_y],
            "gt_vx": [cast(t) for t in gts_x], "params": [cast(p).requires_grad_(True) for p in params]}


def oracle_loss_grad(p, dtype=torch.float64):
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        loss = o.unrolled_loss(p["params"], p["d"], p["vy"], p["vx"], p["re"], p["gt_vy"], p["gt_vx"], p["g"], STD_V, o.STD_RE)
        loss.backward()
    finally:
        torch.set_default_dtype(prev)
    return float(loss.detach()), torch.cat([q.grad.reshape(-1) for q in p["params"]])


@functools.lru_cache(maxsize=None)
def oracle_case(two):
    """(problem, oracle loss, oracle gradient) on the default sphere or the two cylinders -- computed once, never modified"""
    p = problem(SEED_TWO, g=geometry(Y, X, active_of(TWO, Y, X))) if two else problem(SEED)
    return (p,) + oracle_loss_grad(p)


def batch(p):
    return (f32(p["d"]), f32(p["vy"]), f32(p["vx"]), f32(p["re"]), f32(torch.stack(p["gt_vy"])), f32(torch.stack(p["gt_vx"])))


def net_of(params):
    net = sol_amd.model_mars_moon(cin=3, cout=2, seed=0)
    net.set_weights([q.detach().numpy() for q in params])
    return net


def test_large_grid_trainer_any_width_against_the_float64_oracle():
    """mars_moon, 144 x 72, B = 1, SOL-2, default sphere, direct solve: loss 1e-5, full weight gradient 1e-4 (untrimmed) -- the
    recipe of test_large_grid_trainer_against_the_float64_oracle.  The advection's floorf makes the gradient discontinuous, so the state
    seed is conditioned on the ORACLE alone (o.unrolled_loss on the CPU in float32 and in float64): seed 16 agrees to 6.7e-8 on the
    loss and 6.8e-7 on the weight gradient, 150x and 147x inside the tolerances (the table at SEED above)."""
    p, lref, gref = oracle_case(False)
    tr = sol_amd.LargeGridTrainer(net_of(p["params"]), 1, Y, X, 2, STD_V, o.STD_RE, use_graph=False, any_width=True)
    loss = float(tr.fwd_bwd(*batch(p)))
    assert tr.pressure_solver_used == "direct" and tr._sched.pitched and tr._sched.P == 128
    e_l, e_g = abs(loss - lref) / abs(lref), rel(tr.grads, gref)
    print("LargeGridTrainer(any_width) 144x72 vs float64 oracle: loss %.3e, gradient %.3e" % (e_l, e_g))
    assert e_l < 1e-5 and e_g < TOL_GRAD, (e_l, e_g)


def test_large_grid_trainer_any_width_captured_step_equals_the_eager_step():
    ps = [oracle_case(False)[0], problem(SEED + 1)]
    tg = sol_amd.LargeGridTrainer(net_of(ps[0]["params"]), 1, Y, X, 2, STD_V, o.STD_RE, any_width=True)
    te = sol_amd.LargeGridTrainer(net_of(ps[0]["params"]), 1, Y, X, 2, STD_V, o.STD_RE, use_graph=False, any_width=True)
    for p in ps:
        lg, le = float(tg.fwd_bwd(*batch(p))), float(te.fwd_bwd(*batch(p)))
        e_g = rel(tg.grads, te.grads)
        print("any_width captured vs eager: loss %.3e gradient %.3e" % (abs(lg - le) / abs(le), e_g))
        assert tg._graph is not None and te._graph is None
        assert abs(lg - le) <= 1e-6 * abs(le) and e_g < 1e-6


def test_large_grid_trainer_any_width_two_cylinders_cg_against_the_float64_oracle():
    """one eager step on the two-cylinder scene with the CG solve at CG_RTOL, against o.unrolled_loss on that scene (seed 18: the oracle
    alone agrees to 5.8e-8 / 1.7e-6, float32 against float64)"""
    p, lref, gref = oracle_case(True)
    tr = sol_amd.LargeGridTrainer(net_of(p["params"]), 1, Y, X, 2, STD_V, o.STD_RE, use_graph=False, any_width=True,
                                  obstacles=karman.parse_obstacles(TWO), pressure_solver="cg", cg_rtol=CG_RTOL, cg_max_iter=600)
    loss = float(tr.fwd_bwd(*batch(p)))
    assert tr.pressure_solver_used == "cg" and bool(tr.solve_info["converged"].all()) and bool(tr.solve_info["converged_bwd"].all())
    e_l, e_g = abs(loss - lref) / abs(lref), rel(tr.grads, gref)
    print("LargeGridTrainer(any_width) 144x72 two cylinders, CG vs float64 oracle: loss %.3e, gradient %.3e" % (e_l, e_g))
    assert e_l < 1e-5 and e_g < TOL_GRAD, (e_l, e_g)


def test_default_still_refuses_the_width():
    with pytest.raises(ValueError, match="64"):
        sol_amd.LargeGridTrainer(net_of(o.init_params(0)), 1, Y, X, 2, STD_V, o.STD_RE)
    g = o.KarmanGeometry(Y, X)
    with pytest.raises(ValueError, match="64"):
        sol_amd.LargeGridRollout(net_of(o.init_params(0)), masks(g), 1, Y, X, g.dx, STD_V, o.STD_RE)


# ---- 3. karman-2d: LargeGridRollout(any_width=True) ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_rollout(n):
    g = o.KarmanGeometry(Y, X)
    d, vy, vx, re = state(1, Y, X, SEED, g)
    params = o.init_params(3)
    rd, ry, rx = d, vy, vx
    with torch.no_grad():
        for _ in range(n):
            rd, ry, rx = o.karman_step(rd, ry, rx, re, g)
            cy, cx = o.correction(params, ry, rx, re, STD_V, o.STD_RE)
            ry, rx = ry + cy, rx + cx
    return g, (d, vy, vx, re), params, (rd, ry, rx)


@pytest.mark.parametrize("use_graph", [True, False])
def test_rollout_any_width_against_the_float64_oracle(use_graph):
    g, st, params, ref = oracle_rollout(3)
    ro = sol_amd.make_rollout(net_of(params), masks(g), 1, Y, X, g.dx, STD_V, o.STD_RE, use_graph=use_graph, any_width=True)
    assert type(ro) is sol_amd.LargeGridRollout and ro._sched.pitched
    d, vy, vx, re = (f32(t) for t in st)
    ro.run(d, vy, vx, re, 3)
    assert (ro._graph is not None) == use_graph
    errs = [rel(a, b) for a, b in zip((d, vy, vx), ref)]
    print("LargeGridRollout(any_width) 144x72, 3 steps, %s: d %.3e vy %.3e vx %.3e" % (("captured" if use_graph else "eager",) + tuple(errs)))
    assert max(errs) < TOL_FIELD, errs


# ---- 4. Burgers ---------------------------------------------------------------------------------------------------------------------
BB, MS, DT = 2, 2, 0.1
BSTD_V, BSTD_F = (0.21, 0.19), (0.09, 0.11)
BURGERS_SEED = {(24, 100): 3, (48, 48): 5}


def bdomain(by, bx):
    return sol_amd.Domain([by, bx], box=sol_amd.box([by, bx]), boundaries=sol_amd.PERIODIC)


def burgers_inputs(by, bx, seed, dtype=torch.float64):
    """test_gpu_burgers_large_trainer.batch's inputs for a [by, bx] domain (with force)"""
    gen = torch.Generator().manual_seed(seed)
    sm = lambda *shape: o._smooth(torch.randn(*shape, generator=gen, dtype=torch.float64)).to(dtype)
    vy, vx = 0.3 * sm(BB, by + 1, bx), 0.3 * sm(BB, by, bx + 1)
    fy = [0.15 * sm(BB, by + 1, bx) for _ in range(MS)]
    fx = [0.15 * sm(BB, by, bx + 1) for _ in range(MS)]
    gy = [0.3 * sm(BB, by + 1, bx) for _ in range(MS)]
    gx = [0.3 * sm(BB, by, bx + 1) for _ in range(MS)]
    params = [q.to(dtype).clone().requires_grad_(True) for q in o.init_params(0, cin=4)]
    return vy, vx, fy, fx, gy, gx, params


def burgers_oracle(by, bx, seed, dtype=torch.float64):
    vy, vx, fy, fx, gy, gx, params = burgers_inputs(by, bx, seed, dtype)
    loss = o.burgers_unrolled_loss(params, vy, vx, fy, fx, gy, gx, BSTD_V, BSTD_F, DT)
    loss.backward()
    return float(loss.detach()), torch.cat([q.grad.reshape(-1) for q in params])


@functools.lru_cache(maxsize=None)
def burgers_batch(by, bx):
    vy, vx, fy, fx, gy, gx, params = burgers_inputs(by, bx, BURGERS_SEED[(by, bx)])
    loss, gref = burgers_oracle(by, bx, BURGERS_SEED[(by, bx)])
    velo = torch.stack([o.staggered_tensor(a, b) for a, b in zip([vy] + gy, [vx] + gx)])
    forc = torch.stack([o.staggered_tensor(a, b) for a, b in zip(fy, fx)])
    return dict(params=[q.detach() for q in params], loss=loss, gref=gref, velo=velo, forc=forc, vy=vy, vx=vx)


@pytest.mark.parametrize("by,bx", [(24, 100), (48, 48)])
def test_burgers_trainer_any_width_replay_against_oracle_and_eager(by, bx):
    """loss 1e-5, full weight gradient TOL_GRAD against o.burgers_unrolled_loss, replay == eager bit for bit: the tolerances of
    test_large_burgers_trainer_replay_against_oracle_and_eager.  The generator seed per shape is one whose oracle-alone deviation
    (float32 against float64 on the CPU) is below 1e-5, as that file requires (the table at SEED above)."""
    b = burgers_batch(by, bx)
    net = sol_amd.model_mars_moon(cin=4, cout=2, seed=0)
    net.set_weights([q.numpy() for q in b["params"]])
    tr = sol_amd.BurgersTrainer(net, bdomain(by, bx), BB, MS, DT, BSTD_V, BSTD_F, any_width=True)
    assert tr.use_graph and tr.schedule == "manual" and tr.large == (max(by, bx) > 64)
    tr.fwd_bwd(b["velo"], b["forc"])
    assert tr._graph is not None and tr._sched.pitched
    loss = float(tr.fwd_bwd(b["velo"], b["forc"]))            # a pure replay
    grad = net.params.grad.detach().clone()
    e_l, e_g = abs(loss - b["loss"]) / abs(b["loss"]), rel(grad, b["gref"])
    print("BurgersTrainer(any_width) %dx%d: loss rel %.3e, weight gradient rel %.3e" % (by, bx, e_l, e_g))
    assert e_l < 1e-5 and e_g < TOL_GRAD, (e_l, e_g)
    le = tr.fwd_bwd(b["velo"], b["forc"], eager=True).clone()
    assert float(le) == loss and torch.equal(net.params.grad, grad)


@pytest.mark.parametrize("by,bx", [(24, 100), (48, 48)])
@pytest.mark.parametrize("use_graph", [True, False])
def test_burgers_rollout_any_width_against_oracle(use_graph, by, bx):
    """three steps at TOL_FIELD: the loop of test_large_burgers_rollout_against_oracle"""
    b = burgers_batch(by, bx)
    nsteps = 3
    gen = torch.Generator().manual_seed(21)
    sm = lambda *shape: o._smooth(torch.randn(*shape, generator=gen, dtype=torch.float64))
    fy = [0.15 * sm(BB, by + 1, bx) for _ in range(nsteps + 1)]
    fx = [0.15 * sm(BB, by, bx + 1) for _ in range(nsteps + 1)]
    params = [q.clone() for q in b["params"]]
    params[22] = params[22] * 0.1
    net = sol_amd.model_mars_moon(cin=4, cout=2, seed=0)
    net.set_weights([q.numpy() for q in params])
    ro = sol_amd.BurgersRollout(net, bdomain(by, bx), BB, DT, BSTD_V, BSTD_F, use_graph=use_graph, any_width=True)
    ro.reset(o.staggered_tensor(b["vy"], b["vx"]))
    sv = torch.tensor(BSTD_V)
    ry, rx = b["vy"], b["vx"]
    for i in range(1, nsteps + 1):
        ro.step(o.staggered_tensor(fy[i - 1], fx[i - 1]), o.staggered_tensor(fy[i], fx[i]))
        with torch.no_grad():
            ry, rx = o.burgers_step(ry, rx, DT, 0.1, fy[i - 1], fx[i - 1])
            feat = torch.cat([o.staggered_tensor(ry, rx)[:, :-1, :-1, :] / sv, o.staggered_tensor(fy[i], fx[i])[:, :-1, :-1, :] / torch.tensor(BSTD_F)], dim=-1)
            cy, cx = o.to_staggered(o.mars_moon(params, feat) * sv)
            ry, rx = ry + cy, rx + cx
    torch.cuda.synchronize()
    assert (ro._graph is not None) == use_graph
    e = rel(ro.vel, o.staggered_tensor(ry, rx))
    print("BurgersRollout(any_width) %dx%d %s: %.3e" % (by, bx, "captured" if use_graph else "eager", e))
    assert e < TOL_FIELD
    assert float(ro.corr.abs().max()) > 0


# ---- 5. scripts -------------------------------------------------------------------------------------------------------------------
def test_scripts_train_end_to_end_at_resolution_72(tmp_path):
    """scripts/karman.py -r 72 -t 7 -s 1 twice (144 x 72 frames) -> scripts/karman_train.py -s 1 --msteps 2 --any-width for a few steps
    (the pattern of test_scripts_end_to_end_at_resolution_128): runs through and writes a model; without the flag the width is refused"""
    import importlib.util
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    sys.path.insert(0, sdir)

    def load(name):
        spec = importlib.util.spec_from_file_location("sol_script_anyw_" + name, os.path.join(sdir, name + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m

    for re_nr in (1.6e5, 3.2e5):                    # two simulations: one Reynolds number alone has no spread to normalise by
        load("karman").main(["-o", str(tmp_path / "hi"), "-r", "72", "-t", "7", "-s", "1", "--re", str(re_nr)])
    tf = str(tmp_path / "tf")
    args = ["--train", str(tmp_path / "hi"), "-s", "1", "-n", "2", "-b", "1", "-t", "5", "-m", "2", "-e", "1", "--lr", "1e-4", "--tf", tf, "--seed", "0"]
    with pytest.raises(ValueError, match="64"):
        load("karman_train").main(args)
    loss = load("karman_train").main(args + ["--any-width"])
    assert loss is not None and np.isfinite(loss)
    assert os.path.exists(tf + "/model.pt") and os.path.exists(tf + "/dataStats.pickle")
