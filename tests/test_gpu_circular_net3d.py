"""Circular z padding of the karman-3d correction network on the device (pytest -m gpu): sol_conv3d_circ_pack / _unpack / sol_conv3d_halo
alone, one layer through karman3d.conv3d_circular, the whole network through NetSchedule3D(padding="circular") and through the per-layer
composition (net(x, padding="circular")), the kernels each pass launches, the accumulated reverse sweep, equivariance under a roll along
z, Karman3DTrainer / Karman3DRollout(conv_padding="circular") on the periodic cylinder, the default bits, the poison patterns, the script.

References: float64 torch (circular_net3d_cases: two planes concatenated on either side of z, zeros along y and x, F.conv3d; the physics
is periodic3d_cases.periodic3d_step).  Bounds: karman3d_net_shapes.BOUNDS, relative L2; the CPU twin test_circular_net3d_cpu.py holds the
float32 reference alone to a quarter of each.  Cells are (B, Y, X, Z); the kernels run at the buffer shape (B, Y, HB, X).  Every test
here fails on a library without the feature: TypeError (unknown keyword padding= / conv_padding=), AttributeError (conv3d_circular,
the sol_conv3d_circ_* symbols).
Measured on an MI355X (printed by the tests): the three entries bit-exact; one layer out 1.6e-7 ... 4.9e-7, dx 1.6e-7 ... 4.6e-7, dw 8.1e-8
... 2.2e-7, db 3.9e-8 ... 1.4e-7; the schedule against float64 out 4.6e-7 ... 8.6e-7, dx 4.4e-7 ... 8.5e-7, worst parameter tensor 5.3e-7 ...
1.1e-6 (one activation sign differed, at 2x5x8x12), X = 128 forward 4.3e-7; against the per-layer composition out 0 (X = 64) ... 7.1e-7, dx up
to 8.1e-7, flat up to 5.3e-7; the kernel census equals the restated dispatch at (B, Y, HB, X) at every cell; accumulated sweep 1.1e-7; a
roll along z commutes with the circular roll-out schedule BIT FOR BIT at both cells and all three shifts (recorded, not required) and moves
the zero-padded one by 0.34 ... 0.77; trainer 16x8x8 / 16x8x12 manual against float64 loss 8.3e-8 / 1.5e-7, gradient 1.7e-6 / 1.9e-7, worst
tensor 1.7e-4 / 2.8e-7, final state 7.3e-7 / 7.6e-7; autograd schedule 2.0e-7 / 1.8e-8, 2.1e-7 / 2.7e-7, 3.5e-7 / 2.3e-5; manual against
autograd loss 1.2e-7 / 1.7e-7, gradient 1.7e-6 / 1.8e-7; captured = eager bit for bit; roll-out after three steps up to 8.7e-7 / 9.2e-7."""
import collections
import functools
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import sol_amd
import sol_oracle3d as o
from sol_amd import _lib
from sol_amd import karman3d as k3
from sol_amd.schedule3d import NetSchedule3D

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import circular_net3d_cases as cc
import karman3d_net_shapes as kn
import periodic3d_cases as pc
import poison
from circular_net3d_cases import BOUNDS, sid
from large2d_scenes import DEV, TOL_FIELD, f32, rel

pytestmark = pytest.mark.gpu
PZ = "periodic-z"
B = pc.B


def sync(x=None):
    torch.cuda.synchronize()
    return x


# ---- the three entries against a numpy index gather -------------------------------------------------------------------------------------
def sentinel(*shape):
    return (np.arange(int(np.prod(shape)), dtype=np.float32) + 1.0).reshape(shape)


def pack_ref(src, HB, mode):
    Bn, Y, X, Z, c = src.shape
    out = np.zeros((Bn, Y, HB, X, c), dtype=np.float32)
    for r in range(Z + 4):
        if 2 <= r < Z + 2 or mode == 0:
            out[:, :, r] = src[:, :, :, (r - 2) % Z]
    return out


def halo_ref(buf, Z, mode):
    out = buf.copy()
    out[:, Z + 4:] = 0.0
    for r in (0, 1, Z + 2, Z + 3):
        out[:, r] = buf[:, (r - 2) % Z + 2] if mode == 0 else 0.0
    return out


def nan_dev(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("cell", cc.ENTRY_CELLS, ids=sid)
def test_pack_unpack_and_halo_against_a_numpy_gather(cell):
    Bn, Y, X, Z = cell
    HB = cc.rows(X, Z)
    assert HB == k3.circular_rows3d(X, Z) and HB >= Z + 4 and (X >= 64 or HB % (64 // X) == 0)
    lib = _lib.load()
    call = lambda fn, *a: _lib.check(fn(_lib.stream(), *a))
    # pack, C = 4, both modes; the destination starts as NaN: an unwritten element shows
    host = sentinel(Bn, Y, X, Z, 4)
    for mode in (0, 1):
        dst = nan_dev(Bn, Y, HB, X, 4)
        call(lib.sol_conv3d_circ_pack, _lib.ptr(torch.from_numpy(host).to(DEV)), _lib.ptr(dst), Bn, Y, X, Z, HB, 4, mode)
        sync()
        assert np.array_equal(dst.cpu().numpy(), pack_ref(host, HB, mode)), (cell, "pack", mode)
    # unpack, C = 3 and 4: the inverse of the pack on rows [2, Z + 2)
    for c in (3, 4):
        buf = sentinel(Bn, Y, HB, X, c)
        dst = nan_dev(Bn, Y, X, Z, c)
        call(lib.sol_conv3d_circ_unpack, _lib.ptr(torch.from_numpy(buf).to(DEV)), _lib.ptr(dst), Bn, Y, X, Z, HB, c)
        sync()
        assert np.array_equal(dst.cpu().numpy(), buf[:, :, 2:Z + 2].transpose(0, 1, 3, 2, 4)), (cell, "unpack", c)
    # halo, C = 4 and 32, both modes, in place: halo and pad rows start as NaN, valid rows keep their sentinel
    for c in (4, 32):
        buf = sentinel(Bn * Y, HB, X, c)
        buf[:, :2] = buf[:, Z + 2:] = np.nan
        for mode in (0, 1):
            t = torch.from_numpy(buf).to(DEV)
            call(lib.sol_conv3d_halo, _lib.ptr(t), Bn * Y, Z, HB, X, c, mode)
            sync()
            got = t.cpu().numpy()
            assert np.array_equal(got, halo_ref(buf, Z, mode)), (cell, "halo", c, mode)
            assert np.array_equal(got[:, 2:Z + 2], buf[:, 2:Z + 2]) and not np.isnan(got).any()


def test_the_entries_refuse_bad_arguments_by_message():
    lib = _lib.load()
    a, b = torch.zeros(4096, dtype=torch.float32, device=DEV), torch.zeros(4096, dtype=torch.float32, device=DEV)
    pa, pb = _lib.ptr(a), _lib.ptr(b)
    call = lambda fn, *args: _lib.check(fn(_lib.stream(), *args))
    for fn, args, what in ((lib.sol_conv3d_circ_pack, (None, pb, 1, 3, 4, 6, 16, 4, 0), "sol_conv3d_circ_pack: NULL buffer"),
                           (lib.sol_conv3d_circ_pack, (pa, pb, 1, 3, 4, 6, 9, 4, 0), "HB = 9 is below Z \\+ 4 = 10"),
                           (lib.sol_conv3d_circ_pack, (pa, pb, 1, 3, 4, 1, 16, 4, 0), "Z >= 2"),
                           (lib.sol_conv3d_circ_pack, (pa, pb, 1, 3, 4, 6, 16, 32, 0), "C must be 4"),
                           (lib.sol_conv3d_circ_pack, (pa, pb, 1, 3, 4, 6, 16, 4, 2), "mode must be 0 \\(wrap\\) or 1 \\(zero\\)"),
                           (lib.sol_conv3d_circ_pack, (pa, pb, 0, 3, 4, 6, 16, 4, 0), "B, Y >= 1"),
                           (lib.sol_conv3d_circ_unpack, (pa, None, 1, 3, 4, 6, 16, 3), "sol_conv3d_circ_unpack: NULL buffer"),
                           (lib.sol_conv3d_circ_unpack, (pa, pb, 1, 3, 4, 6, 16, 2), "C must be 3 or 4"),
                           (lib.sol_conv3d_circ_unpack, (pa, pb, 1, 3, 4, 6, 8, 3), "is below Z \\+ 4"),
                           (lib.sol_conv3d_halo, (None, 3, 6, 16, 4, 4, 0), "sol_conv3d_halo: NULL buffer"),
                           (lib.sol_conv3d_halo, (pa, 3, 6, 16, 4, 8, 0), "C must be 4 or 32"),
                           (lib.sol_conv3d_halo, (pa, 3, 6, 16, 4, 4, 3), "mode must be 0"),
                           (lib.sol_conv3d_halo, (pa, 0, 6, 16, 4, 4, 0), "X >= 1"),
                           (lib.sol_conv3d_halo, (pa, 3, 6, 9, 4, 4, 0), "is below Z \\+ 4")):
        with pytest.raises(sol_amd.SolError, match=what):
            call(fn, *args)
    sync()
    assert not a.any() and not b.any()


# ---- one layer ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chan", cc.LAYER_CHANNELS, ids=sid)
@pytest.mark.parametrize("cell", cc.LAYER_CELLS, ids=sid)
def test_one_circular_layer_against_float64(cell, chan):
    x, w, b, gy = cc.layer_case(cell, chan)
    ref = cc.layer_reference(x, w, b, gy)
    dev = [f32(t).requires_grad_(True) for t in (x, w, b)]
    y = k3.conv3d_circular(*dev)
    y.backward(f32(gy))
    sync()
    assert y.shape == gy.shape and dev[0].grad.shape == x.shape and dev[1].grad.shape == w.shape
    errs = [rel(y, ref[0])] + [rel(a.grad, r) for a, r in zip(dev, ref[1:])]
    print("conv3d_circular %s %s vs float64: out %.3e, dx %.3e, dw %.3e, db %.3e" % ((sid(cell), sid(chan)) + tuple(errs)))
    assert errs[0] < BOUNDS["conv_forward"] and max(errs[1:]) < BOUNDS["conv_gradient"], errs
    # and it is the circular reference these numbers belong to
    assert rel(y, cc.layer_reference(x, w, b, gy, padding=cc.ZEROS)[0]) > 100 * BOUNDS["conv_forward"]


# ---- the whole network -----------------------------------------------------------------------------------------------------------------------
def device_net(params):
    net = k3.MarsMoon3D(device=DEV)
    net.set_weights([q.detach().numpy() for q in params])
    return net


def own_kernels(p):
    c = kn.conv_kernels(p)
    return collections.Counter({k: n for k, n in c.items() if k.startswith(("k_conv3d_circ", "k_conv3d_halo"))})


def net_kernels(p):
    c = kn.conv_kernels(p)
    return collections.Counter({k: n for k, n in c.items() if not k.startswith(("k_conv3d_circ", "k_conv3d_halo"))})


FORWARD_OWN = collections.Counter({"k_conv3d_circ_pack<wrap>": 1, "k_conv3d_halo<wrap>": 11, "k_conv3d_circ_unpack3": 1})
# reverse sweep: g_out packed with a zero halo; every one of the eleven dz zeroed before its weight gradient; g_out and every dz wrapped
# before its backward-data convolution; dx unpacked
BACKWARD_OWN = collections.Counter({"k_conv3d_circ_pack<zero>": 1, "k_conv3d_halo<zero>": 11, "k_conv3d_halo<wrap>": 12, "k_conv3d_circ_unpack4": 1})


def valid(t, Z):
    """the valid rows of a buffer-layout tensor [B,Y,HB,X,C] as [B,Y,X,Z,C]"""
    return t[:, :, 2:Z + 2].permute(0, 1, 3, 2, 4)


@pytest.mark.parametrize("cell", list(cc.NET_CELLS), ids=sid)
def test_the_circular_schedule_against_float64_autograd_and_the_per_layer_composition(cell):
    Bn, Y, X, Z = cell
    HB = cc.rows(X, Z)
    kshape = (Bn, Y, HB, X)
    x, gy, params = cc.network_case(cell)
    net = device_net(params)
    net.params.requires_grad_(True)
    sch = net.schedule(*cell, padding="circular")
    assert sch is net.schedule(*cell, padding="circular") and cell + ("circular",) in net._schedules and cell not in net._schedules
    assert sch.circ and sch.kshape == kshape and sch.shape == cell
    xd, gd = x.to(DEV), gy.to(DEV)
    with torch.no_grad():
        sch.begin_step()
        with _lib.profile() as p:
            out, state = sch.forward(xd)
            sync()
        with _lib.profile() as q:
            dx, flat = sch.backward(state, gd)
            sync()
    assert out.shape == (Bn, Y, X, Z, 3) and dx.shape == (Bn, Y, X, Z, 4) and flat.shape == (net.n_params,)
    masks = [valid(a, Z) > 0 for a in state[2]]
    ref, rdx, rg, _, flips = cc.torch_network(x, gy, params, masks=masks, device=DEV)
    off = net.offsets
    per = [rel(flat[off[k]:off[k + 1]], rg[k].reshape(-1)) for k in range(24)]
    errs = rel(out, ref), rel(dx, rdx), max(per)
    print("circular schedule at %s (buffer %s) vs float64: out %.3e, dx %.3e, worst parameter tensor %.3e; sign flips %d"
          % ((sid(cell), sid(kshape)) + errs + (flips,)))
    print("    forward %s %s; reverse %s %s %s" % (dict(net_kernels(p)), dict(own_kernels(p)), dict(net_kernels(q)), dict(kn.bww_kernels(q)), dict(own_kernels(q))))
    assert errs[0] < BOUNDS["net_out"] and errs[1] < BOUNDS["net_dx"] and errs[2] < BOUNDS["net_param"], (errs, per)
    # the kernels: the existing dispatch evaluated at the buffer shape, plus the feature's own launches
    conv, bww = kn.net_backward_launches(*kshape)
    assert net_kernels(p) == kn.net_forward_launches(*kshape) and not kn.bww_kernels(p), sorted(p.kernels)
    assert net_kernels(q) == conv and kn.bww_kernels(q) == bww, sorted(q.kernels)
    assert own_kernels(p) == FORWARD_OWN and own_kernels(q) == BACKWARD_OWN, (sorted(p.kernels), sorted(q.kernels))
    # the autograd node over the same schedule: the same bits
    xi = xd.clone().requires_grad_(True)
    net.params.grad = None
    yi = net(xi, padding="circular")
    (yi * gd).sum().backward()
    sync()
    assert torch.equal(yi, out) and torch.equal(xi.grad, dx[..., :4]) and torch.equal(net.params.grad, flat)
    # the per-layer composition: conv3d_circular with the skip and the activation in torch
    net.fused_backward = False
    xa = xd.clone().requires_grad_(True)
    net.params.grad = None
    ya = net(xa, padding="circular")
    (ya * gd).sum().backward()
    sync()
    pera = [rel(flat[off[k]:off[k + 1]], net.params.grad[off[k]:off[k + 1]]) for k in range(24)]
    both = rel(out, ya), rel(dx, xa.grad), rel(flat, net.params.grad), max(pera)
    print("    schedule vs per-layer composition: out %.3e, dx %.3e, flat %.3e, worst tensor %.3e" % both)
    assert both[0] < BOUNDS["net_out"] and both[1] < BOUNDS["fused_dx"] and both[2] < BOUNDS["fused_flat"] and both[3] < BOUNDS["fused_param"], both


def test_the_forward_schedule_at_x_128():
    Bn, Y, X, Z = cell = cc.WIDE_CELL
    kshape = (Bn, Y, cc.rows(X, Z), X)
    x, _, params = cc.network_case(cell)
    net = device_net(params)
    with pytest.raises(sol_amd.SolError, match="X = 128.*X <= 64.*roll-out"):
        NetSchedule3D(net, *cell, padding="circular")
    sch = NetSchedule3D(net, *cell, train=False, padding="circular")
    with torch.no_grad():
        sch.begin_step()
        with _lib.profile() as p:
            out = sch.forward(x.to(DEV))[0]
            sync()
    ref = cc.torch_network(x, None, params, device=DEV)[0]
    e = rel(out, ref)
    print("circular forward schedule at %s against float64: %.3e; kernels %s" % (sid(cell), e, dict(net_kernels(p))))
    assert out is sch.out and e < BOUNDS["net_out"], e
    assert net_kernels(p) == kn.net_forward_launches(*kshape) and own_kernels(p) == FORWARD_OWN, sorted(p.kernels)
    with pytest.raises(sol_amd.SolError, match="forward pass only"):
        sch.backward(None, out)


def test_the_accumulated_reverse_sweep_is_the_sum_of_its_calls():
    cell = cc.ACC_CELL
    x, gy, params = cc.network_case(cell)
    net = device_net(params)
    sch = net.schedule(*cell, padding="circular")
    xs, gs = [x.to(DEV), (0.7 * x.flip(3)).contiguous().to(DEV)], [gy.to(DEV), (1.3 * gy.flip(2)).contiguous().to(DEV)]
    with torch.no_grad():
        sch.begin_step()
        states = [sch.forward(t)[1] for t in xs]
        single = [sch.backward(s, g)[1].clone() for s, g in zip(states, gs)]
        assert sch.backward(states[0], gs[0], True, False)[1] is None
        acc = sch.backward(states[1], gs[1], False, True)[1]
        sync()
    e = rel(acc, single[0] + single[1])
    print("accumulated reverse sweep at %s against the sum of two single calls: %.3e" % (sid(cell), e))
    assert e < BOUNDS["fused_flat"], e


@pytest.mark.parametrize("cell", cc.EQUIV_CELLS, ids=sid)
def test_the_circular_rollout_schedule_commutes_with_a_roll_along_z(cell):
    Bn, Y, X, Z = cell
    ps, x = cc.equivariance_case(cell)
    net = device_net(ps)
    circ = NetSchedule3D(net, *cell, train=False, padding="circular")
    zero = NetSchedule3D(net, *cell, train=False)
    with torch.no_grad():
        base_c, base_z = circ.forward(f32(x))[0].clone(), zero.forward(f32(x))[0].clone()
        for s in cc.ROLLS(Z):
            xs = f32(torch.roll(x, s, 3))
            oc, oz = circ.forward(xs)[0], zero.forward(xs)[0]
            ec, ez = rel(oc, torch.roll(base_c, s, 3)), rel(oz, torch.roll(base_z, s, 3))
            print("%s roll by %d along z: circular %.3e (bit-identical: %s), zero padded %.3e" % (sid(cell), s, ec, torch.equal(oc, torch.roll(base_c, s, 3)), ez))
            assert ec < BOUNDS["net_out"], (s, ec)
            assert ez > 100 * BOUNDS["net_out"], (s, ez)
    sync()


# ---- Karman3DTrainer / Karman3DRollout ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(cell):
    g = pc.scene_geometry(tuple(cell), "cylinder")
    sc = k3.Scene3D(*cell, device=DEV, active=g.active, inflow=g.inflow, velBCy=g.bc_mask, velBCyMask=g.bc_mask, pressure_solver="direct_extruded",
                    boundaries=PZ)
    assert sc.periodic_bits == 8
    return sc


@functools.lru_cache(maxsize=None)
def trainer_case(cell):
    p = cc.trainer_problem(cell)
    return p, cc.trainer_reference(p)


def run_trainer(cell, p, schedule, use_graph, **kw):
    tr = k3.Karman3DTrainer(device_net(p["params"]), scene(cell), B, pc.TRAINER_MS, pc.TRAINER_STD_V, o.STD_RE, use_graph=use_graph, schedule=schedule, **kw)
    for _ in range(2 if use_graph else 1):                      # (graph: the second call is a pure replay)
        tr._grads.zero_()
        loss = tr.fwd_bwd(p["d"], *p["v"], p["re"], p["gts"])
    sync()
    return tr, float(loss)


@pytest.mark.parametrize("cell", cc.TRAIN_CELLS, ids=sid)
def test_trainer_sol2_with_circular_padding(cell):
    """manual and autograd schedules, eager and captured, against the float64 reference (oracle_* bounds) and each other (manual_*);
    captured = eager bit for bit; the duplicate v_z plane equals plane 0"""
    p, (loss, losses, gref, final) = trainer_case(cell)
    res = {}
    for schedule in ("manual", "autograd"):
        for use_graph in (False, True):
            tr, hl = run_trainer(cell, p, schedule, use_graph, conv_padding="circular")
            assert tr.conv_padding == "circular" and tr.sch.circ and (tr._graph is not None) == use_graph
            off, at, per = tr.net.offsets, 0, []
            for k, q in enumerate(p["params"]):
                per.append(rel(tr.grads[off[k]:off[k + 1]], gref[at:at + q.numel()]))
                at += q.numel()
            e = abs(hl - loss) / abs(loss), rel(tr.grads, gref), max(per), max(rel(a, b) for a, b in zip(tr.final, final))
            print("circular trainer %s %s %s vs float64: loss %.3e, gradient %.3e, worst tensor %.3e, final state %.3e"
                  % ((sid(cell), schedule, "graph" if use_graph else "eager") + e))
            assert e[0] < BOUNDS["oracle_loss"] and e[1] < BOUNDS["oracle_grad"] and e[2] < BOUNDS["oracle_param"] and e[3] < TOL_FIELD, e
            assert torch.equal(tr.final[3][..., -1], tr.final[3][..., 0])
            res[schedule, use_graph] = (hl, tr.loss_steps.clone(), tr.grads.clone(), [t.clone() for t in tr.final])
            del tr
        assert poison.first_difference(res[schedule, True], res[schedule, False]) is None          # captured against eager: the same bits
    lm, la = res["manual", False], res["autograd", False]
    e = abs(lm[0] - la[0]) / abs(la[0]), rel(lm[1], la[1]), rel(lm[2], la[2]), max(rel(a, b) for a, b in zip(lm[3], la[3]))
    print("    manual against autograd schedule: loss %.3e, per-step %.3e, gradient %.3e, final %.3e" % e)
    assert e[0] < BOUNDS["manual_loss"] and e[1] < BOUNDS["manual_steps"] and e[2] < BOUNDS["manual_grad"] and e[3] < BOUNDS["manual_final"], e


@pytest.mark.parametrize("cell", cc.TRAIN_CELLS, ids=sid)
def test_rollout_three_steps_with_circular_padding(cell):
    p, _ = trainer_case(cell)
    ro = k3.Karman3DRollout(device_net(p["params"]), scene(cell), B, pc.TRAINER_STD_V, o.STD_RE, conv_padding="circular")
    assert ro.conv_padding == "circular" and ro.sch.circ
    st = (f32(p["d"]),) + tuple(f32(t) for t in p["v"])
    re = f32(p["re"])
    for _ in range(3):
        st = ro.step(*st, re)
        assert torch.equal(st[3][..., -1], st[3][..., 0])       # after every step
    sync()
    ref = cc.rollout_reference(p, 3)
    errs = [rel(a, b) for a, b in zip(st, ref)]
    print("circular roll-out %s, 3 steps:" % sid(cell), ["%.3e" % e for e in errs])
    assert max(errs) < 3 * TOL_FIELD, errs                      # (three steps: three times one step's bound, as the periodic roll-out test)


def test_refusals_on_the_device_scene():
    cell = cc.TRAIN_CELLS[1]
    p, _ = trainer_case(cell)
    net = device_net(p["params"])
    with pytest.raises(sol_amd.SolError, match="Z = 12.*multiple of 64"):          # what the zero-padded network says of this grid
        k3.Karman3DTrainer(net, scene(cell), B, 2, pc.TRAINER_STD_V, o.STD_RE)
    for ctor in (lambda **kw: k3.Karman3DTrainer(net, scene(cell), B, 2, pc.TRAINER_STD_V, o.STD_RE, **kw),
                 lambda **kw: k3.Karman3DRollout(net, scene(cell), B, pc.TRAINER_STD_V, o.STD_RE, **kw)):
        with pytest.raises(sol_amd.SolError, match="conv_padding must be 'zeros' or 'circular'"):
            ctor(conv_padding="reflect")
    g = pc.scene_geometry((16, 8, 8), "cylinder", False)
    open_scene = k3.Scene3D(16, 8, 8, device=DEV, active=g.active, inflow=g.inflow)
    with pytest.raises(sol_amd.SolError, match="conv_padding='circular' needs a z-periodic scene"):
        k3.Karman3DTrainer(net, open_scene, B, 2, pc.TRAINER_STD_V, o.STD_RE, conv_padding="circular")


# ---- defaults: conv_padding="zeros" spelled out is the keyword left out ------------------------------------------------------------------------
def test_zeros_spelled_out_gives_the_default_bits():
    cell = cc.TRAIN_CELLS[0]
    p, _ = trainer_case(cell)
    res, rolls = [], []
    for kw in ({}, {"conv_padding": "zeros"}):
        tr, loss = run_trainer(cell, p, "manual", False, **kw)
        assert tr.conv_padding == "zeros" and not tr.sch.circ
        res.append(poison.snapshot((loss, tr.loss_steps, tr.grads, tuple(tr.final))))
        ro = k3.Karman3DRollout(device_net(p["params"]), scene(cell), B, pc.TRAINER_STD_V, o.STD_RE, **kw)
        rolls.append(poison.snapshot(sync(ro.run(f32(p["d"]), *(f32(t) for t in p["v"]), f32(p["re"]), 3))))
    assert poison.first_difference(res[0], res[1]) is None and poison.first_difference(rolls[0], rolls[1]) is None
    # and it is the zero-padded reference these bits belong to, not the circular one
    lz = cc.trainer_reference(p, cc.ZEROS)[0]
    assert abs(res[0][0] - lz) / abs(lz) < BOUNDS["oracle_loss"]


# ---- poison ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_circular_entry_points_under_every_poison_pattern(monkeypatch):
    cell = (2, 5, 64, 10)
    x, gy, params = cc.network_case(cell)
    lx, lw, lb, lg = (f32(t) for t in cc.layer_case((1, 3, 4, 6), (32, 3)))
    small = (1, 3, 4, 6)
    sx, sg, _ = cc.network_case(small)

    def run():
        res = {}
        for c, xs, gs in ((cell, x, gy), (small, sx, sg)):
            net = device_net(params)
            sch = NetSchedule3D(net, *c, padding="circular")
            with torch.no_grad():
                out, state = sch.forward(xs.to(DEV))
                dx, flat = sch.backward(state, gs.to(DEV))
            res["schedule " + sid(c)] = poison.snapshot(sync((out, dx, flat)))
            ro = NetSchedule3D(net, *c, train=False, padding="circular")
            with torch.no_grad():
                res["forward schedule " + sid(c)] = poison.snapshot(sync(ro.forward(xs.to(DEV))[0]))
        a = [t.clone().requires_grad_(True) for t in (lx, lw, lb)]
        y = k3.conv3d_circular(*a)
        y.backward(lg)
        res["conv3d_circular"] = poison.snapshot(sync((y, a[0].grad, a[1].grad, a[2].grad)))
        return res

    poison.check_patterns(monkeypatch, run, "circular z padding")


# ---- the script --------------------------------------------------------------------------------------------------------------------------------------
def test_the_script_records_the_padding_and_picks_it_up(tmp_path):
    import importlib.util
    from sol_amd import scene as scn
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    if sdir not in sys.path:
        sys.path.insert(0, sdir)
    spec = importlib.util.spec_from_file_location("sol_script_karman3d_circular", os.path.join(sdir, "karman3d.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    common = ["-r", "8", "--re", "1.6e5", "--obstacle", "cylinder"]
    out = mod.main(common + ["-t", "6", "-o", str(tmp_path / "run"), "--boundaries", PZ, "--conv-padding", "circular", "--train-sol", "2", "--train-steps", "2"])
    with open(out + "/params.pickle", "rb") as f:
        assert pickle.load(f)["conv_padding"] == "circular"
    blob = torch.load(out + "/model3d.pt", weights_only=False)
    assert blob["conv_padding"] == "circular" and blob["boundaries"] == PZ
    out2 = mod.main(common + ["-t", "4", "-o", str(tmp_path / "run2"), "--model", out + "/model3d.pt"])
    with open(out2 + "/params.pickle", "rb") as f:
        rec = pickle.load(f)
    assert rec["conv_padding"] == "circular" and rec["boundaries"] == PZ            # picked up from the model
    v = scn.read_zipped_array(out2 + "/velo_000003.npz")
    assert np.isfinite(v).all() and np.array_equal(v[0, :16, :8, 8, 2], v[0, :16, :8, 0, 2])
    # the same weights rolled out with zero padding give other frames
    blob["conv_padding"] = "zeros"
    torch.save(blob, str(tmp_path / "zeros.pt"))
    out3 = mod.main(common + ["-t", "4", "-o", str(tmp_path / "run3"), "--model", str(tmp_path / "zeros.pt")])
    assert np.abs(scn.read_zipped_array(out3 + "/velo_000003.npz") - v).max() > 0
    with pytest.raises(SystemExit, match="--conv-padding zeros contradicts the padding recorded"):
        mod.main(common + ["-t", "4", "--model", out + "/model3d.pt", "--conv-padding", "zeros"])
