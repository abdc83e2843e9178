"""Circular padding of the karman-2d correction network on the device (pytest -m gpu): sol_conv_halo alone, one layer through
ops.conv5x5_circular, the whole network through NetSchedule2D(padding="circular") and through the autograd composition
(model(..., padding="circular")), translation equivariance, LargeGridTrainer / LargeGridRollout(conv_padding="circular") on periodic
scenes, the poison patterns, the defaults and the scripts.

References: float64 torch with circular index arithmetic (circular_net_cases: a modulo gather + conv2d; the physics is
periodic_cases.periodic_step), independent of oracle/'s networks.  Tolerances are the project's (large2d_scenes): TOL_FIELD = 1e-5 on
fields and losses, TOL_GRAD = 1e-4 on gradients, relative L2; the CPU twin test_circular_net_cpu.py holds the float32 reference alone to
them at every network case and trainer problem used here, and checks that each of them tells circular from zero padding by more than
100 x tolerance.  Every test that passes padding= / conv_padding= or calls sol_conv_halo fails on a library without them (TypeError,
missing symbol).
Measured on an MI355X (printed by the tests): sol_conv_halo bit-exact; one layer out 1.6e-7 ... 4.3e-7, dx 1.1e-7 ... 4.3e-7, dw 8.8e-8
... 2.2e-7, db 4.3e-8 ... 1.7e-7; the schedule against float64 out 3.1e-7 ... 3.6e-7, input gradient 2.6e-7 ... 4.1e-7, weight gradient
2.3e-7 ... 5.0e-7, the autograd composition 5.2e-7 ... 5.9e-7 / 4.5e-7 ... 8.6e-7 / 3.1e-7 ... 1.8e-6, one against the other up to
1.8e-6; a roll commutes with the circular network bit for bit (0.0) and moves the zero-padded one by 0.17 ... 0.53; trainer scene A loss
5.4e-7, per-step 7.3e-7 / 4.0e-7, gradient 2.5e-7, final state up to 6.7e-7, against the autograd composition 1.1e-7 / 6.7e-7; scene E
2.6e-7, 1.0e-6 / 9.7e-8, 1.9e-7, 7.8e-7 and 1.2e-6 / 5.9e-7; roll-out after three steps d 6.3e-8, v_y 6.0e-8, v_x 8.1e-7, captured =
eager bit for bit."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import sol_amd
import sol_oracle as o
from sol_amd import _lib, fluid, karman, ops
from sol_amd.schedule2d import NetSchedule2D

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import circular_net_cases as cc
import periodic_cases as pc
import poison
from large2d_scenes import DEV, TOL_FIELD, TOL_GRAD, f32, rel

pytestmark = pytest.mark.gpu
B = pc.B
AXES = [(False, True), (True, False), (True, True)]
aid = lambda per: {(False, True): "x", (True, False): "y", (True, True): "yx"}[per]
sid = lambda s: "x".join(str(v) for v in s)


# ---- sol_conv_halo alone ------------------------------------------------------------------------------------------------------------
def halo_ref(buf, H, W, bits, mode):
    """numpy: the halo of buf [B, H + 4 py, P, C] := the valid cell at the index modulo H / W (mode 0) or 0 (mode 1)"""
    r0, c0 = 2 * bool(bits & 2), 2 * bool(bits & 4)
    HB, WV = H + 2 * r0, W + 2 * c0
    rows = (np.arange(HB) - r0) % H + r0
    cols = (np.arange(WV) - c0) % W + c0
    out = buf.copy()
    if mode == 0:
        out[:, :, :WV] = buf[:, rows][:, :, cols]
    else:
        z = np.zeros_like(buf[:, :, :WV])
        z[:, r0:r0 + H, c0:c0 + W] = buf[:, r0:r0 + H, c0:c0 + W]
        out[:, :, :WV] = z
    return out


@pytest.mark.parametrize("bits", [2, 4, 6])
@pytest.mark.parametrize("shape", [(2, 5, 6, 4), (1, 1, 3, 32), (2, 7, 60, 32), (1, 3, 62, 32)], ids=sid)
def test_conv_halo_against_a_numpy_modulo_gather(shape, bits):
    Bn, H, W, c = shape
    r0, c0 = 2 * bool(bits & 2), 2 * bool(bits & 4)
    P = 64 * ((W + 2 * c0 + 63) // 64)
    host = (np.arange(Bn * (H + 2 * r0) * P * c, dtype=np.float32) + 1.0).reshape(Bn, H + 2 * r0, P, c)   # every cell its own sentinel
    for mode, word in ((0, "wrap"), (1, "zero")):
        buf = torch.from_numpy(host).to(DEV)
        assert ops.conv_halo(buf, H, W, bits, word) is buf
        torch.cuda.synchronize()
        got, want = buf.cpu().numpy(), halo_ref(host, H, W, bits, mode)
        assert np.array_equal(got, want), (shape, bits, word)
        assert np.array_equal(got[:, r0:r0 + H, c0:c0 + W], host[:, r0:r0 + H, c0:c0 + W])       # valid cells keep their sentinel
        assert np.array_equal(got[:, :, W + 2 * c0:], host[:, :, W + 2 * c0:])                   # and so do the pad columns
        assert not np.array_equal(got, host)
    same = torch.from_numpy(host[:, r0:r0 + H]).contiguous().to(DEV)                             # bits 0: nothing is launched
    for word in ("wrap", "zero"):
        ops.conv_halo(same, H, W, 0, word)
    torch.cuda.synchronize()
    assert np.array_equal(same.cpu().numpy(), host[:, r0:r0 + H])


def test_conv_halo_refuses_bad_arguments():
    lib = _lib.load()
    buf = torch.zeros(1, 8, 64, 4, dtype=torch.float32, device=DEV)
    call = lambda *a: _lib.check(lib.sol_conv_halo(_lib.stream(), *a))
    for args, what in (((None, 1, 4, 4, 64, 4, 4, 0), "NULL buffer"),
                       ((_lib.ptr(buf), 1, 4, 62, 64, 4, 4, 0), "is below W"),
                       ((_lib.ptr(buf), 1, 4, 4, 96, 4, 4, 0), "multiple of 64"),
                       ((_lib.ptr(buf), 1, 4, 4, 64, 4, 1, 0), "periodic_bits must be a combination"),
                       ((_lib.ptr(buf), 1, 4, 4, 64, 4, 8, 0), "periodic_bits must be a combination"),
                       ((_lib.ptr(buf), 1, 4, 4, 64, 4, 6, 2), "mode must be 0"),
                       ((_lib.ptr(buf), 1, 4, 4, 64, 6, 6, 0), "multiple of 4 up to 32")):
        with pytest.raises(sol_amd.SolError, match=what):
            call(*args)
    with pytest.raises(KeyError):
        ops.conv_halo(buf, 4, 4, 6, "reflect")
    torch.cuda.synchronize()
    assert not buf.any()


# ---- one layer through ops.conv5x5_circular ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", AXES, ids=aid)
@pytest.mark.parametrize("chan", [(4, 32), (32, 32), (32, 2)], ids=sid)
@pytest.mark.parametrize("shape", [(2, 6, 12), (2, 5, 60), (1, 7, 62), (2, 9, 124)], ids=sid)
def test_one_circular_layer_against_float64(shape, chan, per):
    """(2, 6, 12): one tile; (2, 5, 60): W + 4 = 64, the unmasked instantiation; (1, 7, 62): the halo across a tile edge; (2, 9, 124):
    the largest width free of the extra tile used here"""
    Bn, H, W = shape
    cin, cout = chan
    g = torch.Generator().manual_seed(11 + W + cin)
    x = torch.randn(Bn, H, W, cin, generator=g, dtype=torch.float64).float().double()
    w = (torch.randn(5, 5, cin, cout, generator=g, dtype=torch.float64) / (5.0 * cin ** 0.5)).float().double()
    b = (0.1 * torch.randn(cout, generator=g, dtype=torch.float64)).float().double()
    gy = torch.randn(Bn, H, W, cout, generator=g, dtype=torch.float64).float().double()
    ref = [t.clone().requires_grad_(True) for t in (x, w, b)]
    yr = cc.conv(*ref, per)
    yr.backward(gy)
    dev = [f32(t).requires_grad_(True) for t in (x, w, b)]
    y = ops.conv5x5_circular(*dev, per)
    y.backward(f32(gy))
    torch.cuda.synchronize()
    assert y.shape == (Bn, H, W, cout) and dev[0].grad.shape == x.shape
    errs = [rel(y, yr)] + [rel(a.grad, r.grad) for a, r in zip(dev, ref)]
    print("conv5x5_circular %s %s periodic %s vs float64: out %.3e, dx %.3e, dw %.3e, db %.3e" % ((sid(shape), sid(chan), aid(per)) + tuple(errs)))
    assert errs[0] < TOL_FIELD and max(errs[1:]) < TOL_GRAD, errs


# ---- the whole network ----------------------------------------------------------------------------------------------------------------------
def device_net(name, params):
    net = (sol_amd.model_mercury if name == "mercury" else sol_amd.model_mars_moon)(cin=3, cout=2, seed=0, device=DEV)
    net.set_weights([q.detach().numpy() for q in params])
    return net


def schedule_run(net, x, gy, **kw):
    """-> out, dx, flat weight gradient of one forward / backward of the schedule"""
    Bn, H, W, _ = x.shape
    sch = NetSchedule2D(net, Bn, H, W, **kw)
    with torch.no_grad():
        sch.begin_step()
        out, st = sch.forward(x)
        dx = sch.backward(st, gy)
        grad = sch.end_step().clone()
    torch.cuda.synchronize()
    return out, dx[..., :x.shape[-1]], grad, sch


@pytest.mark.parametrize("name", ["mars_moon", "mercury"])
@pytest.mark.parametrize("shape,per", cc.NET_CASES, ids=lambda v: aid(v) if isinstance(v[0], bool) else sid(v))
def test_the_circular_schedule_against_float64_and_the_autograd_composition(name, shape, per):
    Bn, H, W = shape
    ps, x, w_out = cc.net_case(name, shape, per)
    ref_out, ref_dx, ref_gw = cc.net_reference(ps, x, w_out, per)
    net = device_net(name, ps)
    out, dx, grad, sch = schedule_run(net, f32(x), f32(w_out), padding="circular", periodic=per)
    assert sch.circular and sch.P == 64 and sch.HB == H + 4 * per[0] and sch.WV == W + 4 * per[1]
    assert out.shape == (Bn, H, W, 2) and dx.shape == (Bn, H, W, 3)
    errs = rel(out, ref_out), rel(dx, ref_dx), rel(grad, ref_gw)
    print("%s %s periodic %s, circular schedule vs float64: out %.3e, input gradient %.3e, weight gradient %.3e" % ((name, sid(shape), aid(per)) + errs))
    assert errs[0] < TOL_FIELD and errs[1] < TOL_GRAD and errs[2] < TOL_GRAD, errs
    # the autograd composition: ops.conv5x5_circular with the skip and the activation in torch
    xa = f32(x).requires_grad_(True)
    net.params.grad = None
    ya = net(xa, padding="circular", periodic=per)
    (ya * f32(w_out)).sum().backward()
    torch.cuda.synchronize()
    comp = rel(ya, ref_out), rel(xa.grad, ref_dx), rel(net.params.grad, ref_gw)
    both = rel(out, ya), rel(dx, xa.grad), rel(grad, net.params.grad)
    print("    autograd composition vs float64: %.3e, %.3e, %.3e; schedule vs composition: %.3e, %.3e, %.3e" % (comp + both))
    assert comp[0] < TOL_FIELD and comp[1] < TOL_GRAD and comp[2] < TOL_GRAD, comp
    assert both[0] < TOL_FIELD and both[1] < TOL_GRAD and both[2] < TOL_GRAD, both


@pytest.mark.parametrize("shape,per", cc.NET_CASES, ids=lambda v: aid(v) if isinstance(v[0], bool) else sid(v))
def test_the_circular_network_commutes_with_a_roll_and_the_zero_padded_one_does_not(shape, per):
    Bn, H, W = shape
    ps, x, _ = cc.net_case("mars_moon", shape, per)
    net = device_net("mars_moon", ps)
    circ = NetSchedule2D(net, Bn, H, W, train=False, padding="circular", periodic=per)
    zero = NetSchedule2D(net, Bn, H, W, train=False, any_width=True)
    dims = [d for d, p in ((1, per[0]), (2, per[1])) if p]
    with torch.no_grad():
        circ.begin_step()
        zero.begin_step()
        base_c, base_z = circ.forward(f32(x))[0].clone(), zero.forward(f32(x))[0].clone()
        for dim in dims:
            n = x.shape[dim]
            for s in (1, 5, n - 1):
                xs = f32(torch.roll(x, s, dim))
                ec = rel(circ.forward(xs)[0], torch.roll(base_c, s, dim))
                ez = rel(zero.forward(xs)[0], torch.roll(base_z, s, dim))
                print("%s periodic %s, roll by %d along dim %d: circular %.3e, zero padded %.3e" % (sid(shape), aid(per), s, dim, ec, ez))
                assert ec < TOL_FIELD, (dim, s, ec)
                assert ez > 100 * TOL_FIELD, (dim, s, ez)          # the zero-padded network sees a wall at the seam: not vacuous
    torch.cuda.synchronize()


# ---- LargeGridTrainer / LargeGridRollout --------------------------------------------------------------------------------------------------
def net_of(p):
    return device_net("mars_moon", p["params"])


def masks_of(p):
    g = p["g"]
    return ops.SceneMasks(g.active, g.inflow, g.bc_mask, g.bc_mask, DEV, multi_launch=True, boundaries=ops.boundaries_name(p["periodic"]))


def batch(p):
    return (f32(p["d"]), f32(p["vy"]), f32(p["vx"]), f32(p["re"]), f32(torch.stack(p["gt_vy"])), f32(torch.stack(p["gt_vx"])))


def dup_planes(vy, vx, per):
    return ([(vy[:, -1], vy[:, 0])] if per[0] else []) + ([(vx[:, :, -1], vx[:, :, 0])] if per[1] else [])


@pytest.mark.parametrize("name", sorted(cc.PROBLEMS))
def test_large_grid_trainer_with_circular_padding(name):
    """scene A (x periodic, 32 x 16) and scene E (doubly periodic, 16 x 16; circular_net_cases.scene says how it differs from
    periodic_cases' E), msteps 2: loss, per-step losses, gradient and final state against float64; the duplicate planes; captured
    replay = the eager bits, twice; the unrolled loss composed by autograd over the model's padding="circular" agrees"""
    (Y, X), _ = cc.PROBLEMS[name]
    ms = pc.TRAINER_MS
    p = cc.trainer_problem(name)
    per = p["periodic"]
    lref, steps_ref, gref, fin_ref = cc.trainer_reference(p)
    args = batch(p)
    kw = dict(multi_launch=True, obstacles=[], conv_padding="circular")
    te = sol_amd.make_trainer(net_of(p), masks_of(p), B, Y, X, ms, 100.0 / X, pc.TRAINER_STD_V, o.STD_RE, use_graph=False, **kw)
    assert isinstance(te, sol_amd.LargeGridTrainer) and te.conv_padding == "circular"
    loss = float(te.fwd_bwd(*args, want_final=True))
    assert te._sched.circular and te._mk.periodic == per and te.pressure_solver_used == "direct"
    e_l, e_g = abs(loss - lref) / abs(lref), rel(te.grads, gref)
    e_s = [abs(a - b) / abs(b) for a, b in zip(te.loss_steps.tolist(), steps_ref)]
    e_f = [rel(a, b) for a, b in zip(te.final, fin_ref)]
    print("LargeGridTrainer(conv_padding='circular'), scene %s %dx%d vs float64: loss %.3e, per-step %s, gradient %.3e, final state %s"
          % (name, Y, X, e_l, e_s, e_g, e_f))
    assert e_l < TOL_FIELD and max(e_s) < TOL_FIELD and e_g < TOL_GRAD and max(e_f) < TOL_FIELD, (e_l, e_s, e_g, e_f)
    for dup, first in dup_planes(te.final[1], te.final[2], per):
        assert torch.equal(dup, first)
    g_eager, l_eager = te.grads.clone(), te.loss_steps.clone()
    # captured replay (kernel nodes only) gives the eager bits, twice
    tg = sol_amd.LargeGridTrainer(net_of(p), B, Y, X, ms, pc.TRAINER_STD_V, o.STD_RE, masks=masks_of(p), **kw)
    lg = float(tg.fwd_bwd(*args))
    assert tg._graph is not None
    assert lg == loss and torch.equal(tg.grads, g_eager) and torch.equal(tg.loss_steps, l_eager)
    assert float(tg.fwd_bwd(*args)) == lg and torch.equal(tg.grads, g_eager)
    # the same unrolled loss composed by autograd: KarmanFlow.step, the model with padding="circular", to_staggered, the seam sync
    net = net_of(p)
    g = p["g"]
    dom = fluid.Domain([Y, X], box=fluid.box[0:Y * g.dx, 0:X * g.dx], boundaries=ops.boundaries_name(per))
    sim = karman.KarmanFlow(multi_launch=True, obstacles=[])
    bc = g.bc_mask.reshape(1, Y + 1, X, 1)
    stag = lambda vy, vx: torch.stack([_lib.pad_high(vy, 2), _lib.pad_high(vx, 1)], dim=-1)
    si = torch.tensor(list(pc.TRAINER_STD_V) + [o.STD_RE], dtype=torch.float32, device=DEV)
    so = torch.tensor(pc.TRAINER_STD_V, dtype=torch.float32, device=DEV)
    st = fluid.Fluid(dom, density=args[0].reshape(B, Y, X, 1), velocity=stag(args[1], args[2]), batch_size=B)
    losses = []
    for i in range(ms):
        st = sim.step(st, re=args[3], res=X, velBCy=bc, velBCyMask=bc)
        corr = karman.to_staggered(net(karman.to_feature(st, args[3]) / si, padding="circular", periodic=per) * so, dom.box)
        v = st.velocity + corr
        vy, vx = ops.SeamSyncFn.apply(v.data[0].data.reshape(B, Y + 1, X), v.data[1].data.reshape(B, Y, X + 1), te._mk.periodic_bits)
        st = st.copied_with(velocity=fluid.StaggeredGrid([vy.reshape(B, Y + 1, X, 1), vx.reshape(B, Y, X + 1, 1)], dom.box))
        losses.append(ops.l2_loss((vy, vx), (args[4][i], args[5][i]), tuple(float(s) for s in pc.TRAINER_STD_V)))
    total = torch.stack([l.reshape(()) for l in losses]).sum() / ms
    net.params.grad = None
    total.backward()
    torch.cuda.synchronize()
    e_al, e_ag = abs(float(total) - loss) / abs(loss), rel(net.params.grad, g_eager)
    print("    manual schedule against the autograd composition: loss %.3e, gradient %.3e" % (e_al, e_ag))
    assert e_al < TOL_FIELD and e_ag < TOL_GRAD


def test_large_grid_rollout_with_circular_padding():
    (Y, X), _ = cc.PROBLEMS["A"]
    steps = 3
    p = cc.trainer_problem("A")
    ref = cc.rollout_reference(p, steps)
    mk = masks_of(p)
    runs = []
    for use_graph in (True, False):
        ro = sol_amd.make_rollout(net_of(p), mk, B, Y, X, p["g"].dx, pc.TRAINER_STD_V, o.STD_RE, multi_launch=True, use_graph=use_graph,
                                  conv_padding="circular")
        assert isinstance(ro, sol_amd.LargeGridRollout) and ro._sched.circular
        h = tuple(f32(p[k]) for k in ("d", "vy", "vx", "re"))
        ro.run(*h, steps)
        torch.cuda.synchronize()
        assert (ro._graph is not None) == use_graph
        errs = [rel(a, b) for a, b in zip(h[:3], ref)]
        print("LargeGridRollout(conv_padding='circular') (use_graph=%s) after %d steps: d %.3e vy %.3e vx %.3e" % ((use_graph, steps) + tuple(errs)))
        assert max(errs) < TOL_FIELD, errs
        assert torch.equal(h[2][:, :, -1], h[2][:, :, 0])
        runs.append(h[:3])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ---- poison: the new entry points under every fill of the uninitialised allocations ------------------------------------------------------
def sync(x):
    torch.cuda.synchronize()
    return x


def test_the_circular_entry_points_under_every_poison_pattern(monkeypatch):
    p = cc.trainer_problem("A")
    (Y, X), _ = cc.PROBLEMS["A"]
    args, mk = batch(p), masks_of(p)
    ps, x, w_out = cc.net_case("mercury", (2, 16, 16), (True, True))
    g = torch.Generator().manual_seed(3)
    lx, lw, lb, lg = (f32(torch.randn(s, generator=g)) for s in ((1, 7, 62, 32), (5, 5, 32, 2), (2,), (1, 7, 62, 2)))

    def run():
        res = {}
        for captured in (False, True):
            tr = sol_amd.LargeGridTrainer(net_of(p), B, Y, X, pc.TRAINER_MS, pc.TRAINER_STD_V, o.STD_RE, masks=mk, multi_launch=True,
                                          obstacles=[], conv_padding="circular", use_graph=captured)
            for k in range(2 if captured else 1):
                tr.grads.zero_()
                loss = tr.fwd_bwd(*args, want_final=True)
                res["trainer captured=%s run %d" % (captured, k)] = poison.snapshot(sync((loss, tr.loss_steps, tr.grads, tuple(tr.final))))
            ro = sol_amd.LargeGridRollout(net_of(p), mk, B, Y, X, p["g"].dx, pc.TRAINER_STD_V, o.STD_RE, multi_launch=True,
                                          use_graph=captured, conv_padding="circular")
            st = [t.clone() for t in args[:3]]
            ro.run(*st, args[3], 3)
            res["rollout captured=%s" % captured] = poison.snapshot(sync(st))
        res["schedule mercury"] = poison.snapshot(schedule_run(device_net("mercury", ps), f32(x), f32(w_out), padding="circular", periodic=(True, True))[:3])
        a = [t.clone().requires_grad_(True) for t in (lx, lw, lb)]
        y = ops.conv5x5_circular(*a, (True, True))
        y.backward(lg)
        res["conv5x5_circular"] = poison.snapshot(sync((y, a[0].grad, a[1].grad, a[2].grad)))
        return res

    poison.check_patterns(monkeypatch, run, "circular padding")


# ---- defaults: conv_padding="zeros" spelled out is the keyword left out ----------------------------------------------------------------------
def test_zeros_spelled_out_gives_the_default_bits():
    (Y, X), _ = cc.PROBLEMS["A"]
    p = cc.trainer_problem("A")
    args, mk = batch(p), masks_of(p)
    res, rolls = [], []
    for kw in ({}, {"conv_padding": "zeros"}):
        tr = sol_amd.LargeGridTrainer(net_of(p), B, Y, X, pc.TRAINER_MS, pc.TRAINER_STD_V, o.STD_RE, masks=mk, multi_launch=True, obstacles=[],
                                      use_graph=False, **kw)
        loss = tr.fwd_bwd(*args, want_final=True)
        assert not tr._sched.circular and tr.conv_padding == "zeros"
        res.append(poison.snapshot(sync((loss, tr.loss_steps, tr.grads, tuple(tr.final)))))
        ro = sol_amd.LargeGridRollout(net_of(p), mk, B, Y, X, p["g"].dx, pc.TRAINER_STD_V, o.STD_RE, multi_launch=True, **kw)
        st = [t.clone() for t in args[:3]]
        ro.run(*st, args[3], 3)
        rolls.append(poison.snapshot(sync(st)))
    assert poison.first_difference(res[0], res[1]) is None and poison.first_difference(rolls[0], rolls[1]) is None
    # and it is the zero-padded reference these bits belong to, not the circular one
    lz = cc.trainer_reference(p, cc.ZEROS)[0]
    assert abs(float(res[0][0]) - lz) / abs(lz) < TOL_FIELD


# ---- the scripts -----------------------------------------------------------------------------------------------------------------------------
def _script(name):
    import importlib.util
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    if sdir not in sys.path:
        sys.path.insert(0, sdir)
    spec = importlib.util.spec_from_file_location("sol_script_circular_" + name, os.path.join(sdir, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_scripts_record_the_padding_and_pick_it_up(tmp_path, caplog):
    """karman.py --boundaries periodic-x generates a tiny periodic set; karman_train.py --conv-padding circular records the word in
    dataStats.pickle and with the model; karman_apply.py runs circular from the record, an explicit flag overrides it with a logged
    line; karman_train.py --conv-padding circular on an open set is refused"""
    import logging
    from sol_amd import scene
    gen = ["-r", "32", "-t", "7", "-s", "0", "--multi-launch"]
    run = [_script("karman").main(["-o", str(tmp_path / "set")] + gen + ["--boundaries", "periodic-x", "--re", str(r)]) for r in (8.0e5, 1.6e6)][0]
    tf = str(tmp_path / "tf")
    train = ["-s", "1", "-n", "2", "-b", "1", "-t", "5", "-m", "2", "-e", "1", "--lr", "1e-4", "--seed", "0"]
    loss = _script("karman_train").main(["--train", str(tmp_path / "set"), "--tf", tf, "--conv-padding", "circular"] + train)
    assert loss is not None and np.isfinite(loss)
    with open(tf + "/dataStats.pickle", "rb") as f:
        stats = pickle.load(f)
    assert stats["conv_padding"] == "circular" and stats["boundaries"] == "periodic-x"
    assert sol_amd.ConvNet.load(tf + "/model.pt").conv_padding == "circular"
    apply = ["--stats", tf + "/dataStats.pickle", "--model", tf + "/model.pt", "-r", "32", "-s", "1", "-t", "4", "--re", "8e5",
             "--initdH", run + "/dens_000005.npz", "--initvH", run + "/velo_000005.npz"]
    frames = {}
    with caplog.at_level(logging.INFO):
        for name, extra in (("record", []), ("circular", ["--conv-padding", "circular"]), ("zeros", ["--conv-padding", "zeros"])):
            caplog.clear()
            out = _script("karman_apply").main(["-o", str(tmp_path / ("apply_" + name))] + apply + extra)
            frames[name] = scene.read_zipped_array(os.path.join(out, "velTf_%06d.npz" % 3))
            text = caplog.text
            assert ("convolution padding: %s" % ("zeros" if name == "zeros" else "circular")) in text
            assert ("--conv-padding zeros overrides the record" in text) == (name == "zeros")
    assert np.isfinite(frames["record"]).all() and np.array_equal(frames["record"], frames["circular"])
    assert not np.array_equal(frames["record"], frames["zeros"])
    assert np.array_equal(frames["record"][:, :-1, -1, 1], frames["record"][:, :-1, 0, 1])           # the roll-out's seam sync
    # refused on an open scene (the roll-out's own refusal: test_circular_net_cpu.py)
    _script("karman").main(["-o", str(tmp_path / "open")] + gen + ["--re", "8e5"])
    with pytest.raises(ValueError, match="--conv-padding circular needs a periodic axis"):
        _script("karman_train").main(["--train", str(tmp_path / "open"), "--tf", str(tmp_path / "to"), "--conv-padding", "circular"] + train)
