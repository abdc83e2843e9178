"""Training and roll-out of the Burgers corrector beyond 64 x 64 on the GPU (pytest -m gpu): BurgersTrainer over
sol_burgers_step_fwd_large / sol_burgers_step_bwd_large, BurgersRollout, and scripts/burgers.py -> burgers_train.py at 128 x 128.

Shape and inputs: B = 2, Y, X = 24, 128 (rows of two 64-pixel tiles), msteps = 2, dt = 0.1, box equal to the resolution (dx = 1, what
the oracle's burgers_unrolled_loss assumes), inputs as in test_gpu_parity.test_burgers_unrolled_loss_and_gradient_against_oracle but
with generator seed 3, std_v = (0.21, 0.19), std_f = (0.09, 0.11), model_mars_moon from o.init_params(0, cin), both noforce settings.
Why seed 3: the weight gradient crosses LeakyReLU and floor kinks; with the oracle alone (fp32 against float64) seeds 1, 5 and 7 leave
up to 1.5e-4, seed 3 leaves 3.9e-7 (force) and 1.2e-6 (noforce).  The tolerance is the suite's TOL_GRAD; a different seed, if ever
needed, must be one whose oracle-alone deviation is below 1e-5."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import sol_amd
import sol_oracle as o
from sol_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from large2d_scenes import DEV, TOL_FIELD, TOL_GRAD, f32, rel

pytestmark = pytest.mark.gpu
B, Y, X, MS, DT = 2, 24, 128, 2, 0.1
STD_V, STD_F = (0.21, 0.19), (0.09, 0.11)


def domain():
    return sol_amd.Domain([Y, X], box=sol_amd.box([Y, X]), boundaries=sol_amd.PERIODIC)


@functools.lru_cache(maxsize=None)
def batch(noforce):
    """inputs, the oracle's loss and flat weight gradient (computed once per noforce setting)"""
    gen = torch.Generator().manual_seed(3)
    sm = lambda *shape: o._smooth(torch.randn(*shape, generator=gen, dtype=torch.float64))
    vy, vx = 0.3 * sm(B, Y + 1, X), 0.3 * sm(B, Y, X + 1)
    fy = [0.15 * sm(B, Y + 1, X) for _ in range(MS)]
    fx = [0.15 * sm(B, Y, X + 1) for _ in range(MS)]
    gy = [0.3 * sm(B, Y + 1, X) for _ in range(MS)]
    gx = [0.3 * sm(B, Y, X + 1) for _ in range(MS)]
    cin = 2 if noforce else 4
    params = [p.clone().requires_grad_(True) for p in o.init_params(0, cin=cin)]
    loss = o.burgers_unrolled_loss(params, vy, vx, fy, fx, gy, gx, STD_V, STD_F, DT, noforce=noforce)
    loss.backward()
    velo = torch.stack([o.staggered_tensor(a, b) for a, b in zip([vy] + gy, [vx] + gx)])
    forc = torch.stack([o.staggered_tensor(a, b) for a, b in zip(fy, fx)])
    return dict(params=[p.detach() for p in params], loss=float(loss), gref=torch.cat([p.grad.reshape(-1) for p in params]),
                velo=velo, forc=forc, vy=vy, vx=vx, fy=fy, fx=fx)


def trainer(noforce, **kw):
    b = batch(noforce)
    net = sol_amd.model_mars_moon(cin=2 if noforce else 4, cout=2, seed=0)
    net.set_weights([p.numpy() for p in b["params"]])
    return net, sol_amd.BurgersTrainer(net, domain(), B, MS, DT, STD_V, STD_F, noforce=noforce, **kw)


@pytest.mark.parametrize("noforce", [False, True])
def test_large_burgers_trainer_replay_against_oracle_and_eager(noforce):
    b = batch(noforce)
    net, tr = trainer(noforce)
    assert tr.use_graph and tr.schedule == "manual" and tr.large
    loss = float(tr.fwd_bwd(b["velo"], b["forc"]))
    assert tr._graph is not None
    loss = float(tr.fwd_bwd(b["velo"], b["forc"]))            # a pure replay
    grad = net.params.grad.detach().clone()
    print("loss rel %.3e, weight gradient rel %.3e" % (abs(loss - b["loss"]) / abs(b["loss"]), rel(grad, b["gref"])))
    assert abs(loss - b["loss"]) < 1e-5 * abs(b["loss"])
    assert rel(grad, b["gref"]) < TOL_GRAD
    le = tr.fwd_bwd(b["velo"], b["forc"], eager=True).clone()
    assert float(le) == loss and torch.equal(net.params.grad, grad)


@pytest.mark.parametrize("noforce", [False, True])
def test_large_burgers_trainer_manual_schedule_equals_autograd_composition(noforce):
    """tolerances of test_gpu_parity.test_burgers_trainer_manual_schedule_equals_autograd_composition: the forward passes are the
    same launches; what differs is the summation order of the weight gradients"""
    b = batch(noforce)
    out = {}
    for key, kw in (("manual", dict(schedule="manual")), ("autograd", dict(schedule="autograd")), ("autograd_eager", dict(schedule="autograd", use_graph=False))):
        net, tr = trainer(noforce, **kw)
        for _ in range(2):
            loss = float(tr.fwd_bwd(b["velo"], b["forc"]))
        out[key] = (loss, net.params.grad.detach().clone())
    ref = out["autograd_eager"]
    for key, got in out.items():
        assert abs(got[0] - ref[0]) < 2e-6 * abs(ref[0]), (key, got[0], ref[0])
        assert rel(got[1], ref[1]) < 1e-5, (key, rel(got[1], ref[1]))
    assert rel(ref[1], b["gref"]) < TOL_GRAD


@pytest.mark.parametrize("model", ["mars_moon", "mercury"])
def test_network_call_scaled_is_the_schedules_forward_bit_for_bit(model):
    """net(x, scaled=True), what the autograd schedule calls: on 128-pixel rows the launches of NetSchedule2D's forward (equal bits;
    the plain form ops.conv5x5 runs another arithmetic form there), on 32-pixel rows ops.conv5x5 itself."""
    from sol_amd.schedule2d import NetSchedule2D
    mk = sol_amd.model_mercury if model == "mercury" else sol_amd.model_mars_moon
    net = mk(cin=4, cout=2, seed=2)
    gen = torch.Generator().manual_seed(5)
    for H, W in ((Y, X), (8, 32)):
        x = torch.randn(B, H, W, 4, generator=gen).to(DEV)
        sch = NetSchedule2D(net, B, H, W)
        with torch.no_grad():
            sch.begin_step()
            want = sch.forward(x)[0]
            got, plain = net(x, scaled=True), net(x)
        assert torch.equal(got, want), (H, W)
        assert torch.equal(got, plain) == (W % 64 != 0) and rel(plain, want) < TOL_FIELD, (H, W, rel(plain, want))


def test_large_burgers_train_steps_first_update_is_the_tf_adam_step():
    """Three train_step calls.  The first update is TF-Adam's: d = lr g / (|g| + eh), eh = eps / sqrt(1 - beta2) -- to fp32 rounding of the
    parameters (1e-6) from the gradient the trainer holds, and below 1e-4 (relative L2 of the parameters) from the ORACLE's gradient: the
    update is lr sign(g) wherever |g| >> eh = 3e-7, so only gradient elements at rounding level, whose sign the fp32 sum may flip, move --
    by 2 lr each; 1e-4 is the figure test_gpu_parity.test_burgers_trainer_manual_schedule_equals_autograd_composition allows two
    gradient forms for the same reason."""
    b = batch(False)
    net, tr = trainer(False)
    lr, eh = 1e-4, 1e-8 / (1 - 0.999) ** 0.5
    p0 = net.params.detach().double().cpu()
    adam = lambda g: p0 - lr * g / (g.abs() + eh)
    loss = tr.train_step(b["velo"], b["forc"], lr)
    torch.cuda.synchronize()
    g, p1 = net.params.grad.detach().double().cpu(), net.params.detach().double().cpu()
    assert rel(p1, adam(g)) < 1e-6
    print("first update against the oracle's: %.3e" % rel(p1, adam(b["gref"])))
    assert rel(p1, adam(b["gref"])) < 1e-4 and float((p1 - p0).abs().max()) > 0
    for _ in range(2):
        loss = tr.train_step(b["velo"], b["forc"], lr)
    assert tr.opt.t == 3 and np.isfinite(float(loss))


@pytest.mark.parametrize("use_graph", [True, False])
def test_large_burgers_rollout_against_oracle(use_graph):
    b = batch(False)
    nsteps = 3
    gen = torch.Generator().manual_seed(21)
    sm = lambda *shape: o._smooth(torch.randn(*shape, generator=gen, dtype=torch.float64))
    fy = [0.15 * sm(B, Y + 1, X) for _ in range(nsteps + 1)]
    fx = [0.15 * sm(B, Y, X + 1) for _ in range(nsteps + 1)]
    params = [p.clone() for p in b["params"]]
    params[22] = params[22] * 0.1
    net = sol_amd.model_mars_moon(cin=4, cout=2, seed=0)
    net.set_weights([p.numpy() for p in params])
    ro = sol_amd.BurgersRollout(net, domain(), B, DT, STD_V, STD_F, use_graph=use_graph)
    ro.reset(o.staggered_tensor(b["vy"], b["vx"]))
    sv = torch.tensor(STD_V)
    ry, rx = b["vy"], b["vx"]
    for i in range(1, nsteps + 1):
        ro.step(o.staggered_tensor(fy[i - 1], fx[i - 1]), o.staggered_tensor(fy[i], fx[i]))
        with torch.no_grad():
            ry, rx = o.burgers_step(ry, rx, DT, 0.1, fy[i - 1], fx[i - 1])
            feat = torch.cat([o.staggered_tensor(ry, rx)[:, :-1, :-1, :] / sv, o.staggered_tensor(fy[i], fx[i])[:, :-1, :-1, :] / torch.tensor(STD_F)], dim=-1)
            cy, cx = o.to_staggered(o.mars_moon(params, feat) * sv)
            ry, rx = ry + cy, rx + cx
    torch.cuda.synchronize()
    assert (ro._graph is not None) == use_graph
    print("roll-out: %.3e" % rel(ro.vel, o.staggered_tensor(ry, rx)))
    assert rel(ro.vel, o.staggered_tensor(ry, rx)) < TOL_FIELD
    assert float(ro.corr.abs().max()) > 0


def test_large_burgers_trainer_refuses_a_row_width_at_construction():
    net = sol_amd.model_mars_moon(cin=4, cout=2, seed=0)
    dom = sol_amd.Domain([24, 100], box=sol_amd.box([24, 100]), boundaries=sol_amd.PERIODIC)
    with pytest.raises(_lib.SolError, match="multiple of 64"):
        sol_amd.BurgersTrainer(net, dom, B, MS, DT, STD_V, STD_F)


def test_burgers_scripts_generate_and_train_at_128(tmp_path):
    """scripts/burgers.py -r 128 (two simulations, a handful of frames), then burgers_train.py -s 1 on them: trains at 128 x 128."""
    import importlib.util
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    sys.path.insert(0, sdir)

    def load(name):
        spec = importlib.util.spec_from_file_location("sol_script_" + name, os.path.join(sdir, name + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m

    data = str(tmp_path / "hires128")
    for s in (0, 1):
        load("burgers").main(["-o", data, "-r", "128", "-l", "32", "--dt", "0.1", "--skipsteps", "2", "-t", "6", "--seed", str(s)])
    loss = load("burgers_train").main(["--train", data, "-s", "1", "-n", "2", "-b", "2", "-t", "5", "-m", "2", "-e", "1", "--dt", "0.1",
                                       "--lr", "1e-4", "--tf", str(tmp_path / "tf"), "--seed", "0"])
    assert loss is not None and np.isfinite(loss)
    assert os.path.isfile(str(tmp_path / "tf" / "model.pt"))
