"""Circular padding of the karman-2d correction network, the part that needs no device: the float64 reference of the GPU tests
(circular_net_cases) in float32 against float64 at the trainer problems, the three identities NetSchedule2D(padding="circular") rests
on, the condition that the trainer problem tells the two paddings apart, argument handling and the refusals.

Figures measured here (printed by the tests; float32 reference against float64 reference): scene A 32 x 16 loss / final state 7.0e-7,
weight gradient 4.1e-7, roll-out after three steps 8.6e-7; scene E 16 x 16 8.1e-7 / 4.5e-7 / 1.0e-6; the six whole-network cases output
7.2e-7 ... 8.5e-7, input gradient 2.8e-7 ... 4.7e-7, weight gradient 3.1e-7 ... 8.7e-7 (seed 7 throughout: no case needs another).
Circular against zero-padded reference: the network cases 0.20 ... 0.80 in output and gradients; the trainer problems at the last-layer
scale 0.01: scene A loss 0.28, weight gradient 0.18; scene E loss 1.2, weight gradient 0.52 (the condition asks for more than 100 x
tolerance: 1e-3 in the loss or 1e-2 in the gradient, so the scale stays periodic_cases' 0.01)."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from sol_amd import _lib, model, ops, trainer
from sol_amd.schedule2d import NetSchedule2D

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import circular_net_cases as cc
import periodic_cases as pc
from large2d_scenes import TOL_FIELD, TOL_GRAD, rel

AXES = [(False, True), (True, False), (True, True)]
aid = lambda per: {(False, True): "x", (True, False): "y", (True, True): "yx"}[per]


# ---- the float32 reference alone holds the tolerances ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cc.PROBLEMS))
def test_the_circular_references_in_float32_hold_the_tolerances(name):
    assert TOL_FIELD == 1e-5 and TOL_GRAD == 1e-4
    p = cc.trainer_problem(name)
    l64, s64, g64, f64 = cc.trainer_reference(p)
    l32, s32, g32, f32 = cc.trainer_reference(p, dtype=torch.float32)
    ef = max([abs(l32 - l64) / abs(l64)] + [abs(a - b) / abs(b) for a, b in zip(s32, s64)] + [rel(a, b) for a, b in zip(f32, f64)])
    eg = rel(g32, g64)
    er = max(rel(a, b) for a, b in zip(cc.rollout_reference(p, 3, dtype=torch.float32), cc.rollout_reference(p, 3)))
    print("scene %s circular reference float32 against float64: loss / final state %.3e, weight gradient %.3e; roll-out after three steps %.3e"
          % (name, ef, eg, er))
    assert ef < TOL_FIELD and eg < TOL_GRAD and er < TOL_FIELD
    for dup, first in pc_dups(f64, p["periodic"]):
        assert torch.equal(dup, first)


@pytest.mark.parametrize("name", ["mars_moon", "mercury"])
@pytest.mark.parametrize("shape,per", cc.NET_CASES, ids=lambda v: aid(v) if isinstance(v[0], bool) else "%dx%dx%d" % v)
def test_the_network_cases_in_float32_hold_the_tolerances(name, shape, per):
    ps, x, w = cc.net_case(name, shape, per)
    o64, gx64, gw64 = cc.net_reference(ps, x, w, per)
    o32, gx32, gw32 = cc.net_reference(ps, x, w, per, torch.float32)
    errs = rel(o32, o64), rel(gx32, gx64), rel(gw32, gw64)
    zo, zx, zw = cc.net_reference(ps, x, w, (False, False))
    apart = rel(zo, o64), rel(zx, gx64), rel(zw, gw64)
    print("%s %s periodic %s, float32 against float64: out %.3e, input gradient %.3e, weight gradient %.3e; zero padded against circular: "
          "%.3e, %.3e, %.3e" % ((name, shape, aid(per)) + errs + apart))
    assert errs[0] < TOL_FIELD and errs[1] < TOL_GRAD and errs[2] < TOL_GRAD
    assert apart[0] > 100 * TOL_FIELD and min(apart[1:]) > 100 * TOL_GRAD         # the case tells the two paddings apart


def pc_dups(fin, per):
    return ([(fin[1][:, -1], fin[1][:, 0])] if per[0] else []) + ([(fin[2][:, :, -1], fin[2][:, :, 0])] if per[1] else [])


@pytest.mark.parametrize("name", sorted(cc.PROBLEMS))
def test_the_trainer_problem_tells_the_two_paddings_apart(name):
    """the condition on the problem: circular and zero-padded references differ by more than 100 x tolerance in the loss or the gradient"""
    p = cc.trainer_problem(name)
    lc, _, gc, _ = cc.trainer_reference(p, cc.CIRCULAR)
    lz, _, gz, _ = cc.trainer_reference(p, cc.ZEROS)
    dl, dg = abs(lc - lz) / abs(lc), rel(gz, gc)
    print("scene %s, last-layer scale %g: circular against zero-padded reference: loss %.3e, weight gradient %.3e" % (name, cc.LAST_SCALE, dl, dg))
    assert dl > 100 * TOL_FIELD or dg > 100 * TOL_GRAD
    if name == "A":                     # the zero-padded recipe here is periodic_cases' own
        assert lz == pytest.approx(pc.trainer_reference(pc.trainer_problem())[0], rel=1e-12)


# ---- the identities the schedule rests on, in float64 -----------------------------------------------------------------------------------
def halo_buffer(x, per, P=None):
    """x [B,H,W,c] in the valid region of a zero [B, H + 4 py, P, c] buffer"""
    B, H, W, c = x.shape
    r0, c0 = 2 * per[0], 2 * per[1]
    buf = torch.zeros(B, H + 2 * r0, P or 64 * ((W + 2 * c0 + 63) // 64), c, dtype=x.dtype)
    buf[:, r0:r0 + H, c0:c0 + W] = x
    return buf


def wrap(buf, H, W, per):
    """the halo of buf := the valid cell at the index modulo H / W (what sol_conv_halo mode 0 does)"""
    r0, c0 = 2 * per[0], 2 * per[1]
    rows = (torch.arange(H + 2 * r0) - r0) % H + r0 if per[0] else torch.arange(H)
    cols = (torch.arange(W + 2 * c0) - c0) % W + c0 if per[1] else torch.arange(W)
    out = buf.clone()
    out[:, :, :W + 2 * c0] = buf.index_select(1, rows).index_select(2, cols)
    return out


def crop(buf, H, W, per):
    r0, c0 = 2 * per[0], 2 * per[1]
    return buf[:, r0:r0 + H, c0:c0 + W]


def zero_conv(x, w, b=None):
    """the convolution the kernels compute: zero padding beyond the buffer edge"""
    return F.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), b, padding=2).permute(0, 2, 3, 1)


def zero_conv_transposed(dz, w):
    """the backward-data form: dz convolved with the kernel flipped in space and transposed in the channels"""
    return zero_conv(dz, w.flip(0, 1).permute(0, 1, 3, 2))


@pytest.mark.parametrize("per", AXES, ids=aid)
@pytest.mark.parametrize("shape", [(2, 6, 12), (1, 1, 3), (2, 7, 62)], ids=lambda s: "%dx%dx%d" % s)
def test_the_identities_of_the_halo_layout(per, shape):
    B, H, W = shape
    cin, cout = 3, 4
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, H, W, cin, generator=g, dtype=torch.float64).requires_grad_(True)
    w = torch.randn(5, 5, cin, cout, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(cout, generator=g, dtype=torch.float64).requires_grad_(True)
    gy = torch.randn(B, H, W, cout, generator=g, dtype=torch.float64)
    y = cc.conv(x, w, b, per)
    y.backward(gy)
    with torch.no_grad():
        # 1. the valid region of a zero-padded convolution of a wrapped buffer is the circular convolution
        xb = wrap(halo_buffer(x, per), H, W, per)
        assert rel(crop(zero_conv(xb, w, b), H, W, per), y) < 1e-13
        if W >= 5 and H >= 5:           # (below the padding F.pad refuses; the modulo gather of the reference is the definition there)
            xp = x.permute(0, 3, 1, 2)
            xp = F.pad(xp, (2, 2, 0, 0), mode="circular") if per[1] else F.pad(xp, (2, 2, 0, 0))
            xp = F.pad(xp, (0, 0, 2, 2), mode="circular") if per[0] else F.pad(xp, (0, 0, 2, 2))
            assert rel(F.conv2d(xp, w.permute(3, 2, 0, 1), b).permute(0, 2, 3, 1), y) < 1e-13
        # 2. the weight gradient with x wrapped and dz zero in the halo (and the pad) is autograd's: dw[k] = sum_valid x[p + k] dz[p]
        dzb = halo_buffer(gy, per, xb.shape[2])
        xpad = F.pad(xb, (0, 0, 2, 2, 2, 2))
        dw = torch.stack([torch.stack([torch.einsum("bhwi,bhwo->io", xpad[:, i:i + xb.shape[1], j:j + xb.shape[2]], dzb) for j in range(5)])
                          for i in range(5)])
        assert rel(dw, w.grad) < 1e-13 and rel(dzb.sum((0, 1, 2)), b.grad) < 1e-13
        # 3. the backward-data form on the WRAPPED dz is autograd's input gradient (the adjoint of a circular convolution is the
        #    circular correlation)
        dx = crop(zero_conv_transposed(wrap(dzb, H, W, per), w), H, W, per)
        assert rel(dx, x.grad) < 1e-13


def test_the_float64_networks_with_open_axes_are_the_oracle_networks():
    import sol_oracle as o
    x = cc.smooth_input(2, 6, 12, 3, 3)
    for name, net in (("mars_moon", o.mars_moon), ("mercury", o.mercury)):
        ps = cc.net_params(name)
        assert float((cc.network(ps, x, (False, False)) - net(ps, x)).abs().max()) < 1e-12


def test_the_circular_network_commutes_with_a_roll_and_the_zero_padded_one_does_not():
    x = cc.smooth_input(1, 8, 16, 3, 9)
    ps = cc.net_params("mars_moon")
    for s in (1, 5, 15):
        circ = rel(cc.network(ps, torch.roll(x, s, 2), (False, True)), torch.roll(cc.network(ps, x, (False, True)), s, 2))
        zero = rel(cc.network(ps, torch.roll(x, s, 2), (False, False)), torch.roll(cc.network(ps, x, (False, False)), s, 2))
        assert circ < 1e-13 and zero > 100 * TOL_FIELD, (s, circ, zero)


# ---- argument handling ---------------------------------------------------------------------------------------------------------------------
def masks_of(g, **kw):
    return ops.SceneMasks(g.active, g.inflow, g.bc_mask, g.bc_mask, "cpu", **kw)


def test_refusals_that_need_no_device():
    import sol_oracle as o
    Y, X = 40, 24
    g = pc.scene_geometry("A", Y, X)
    per_mk = masks_of(g, multi_launch=True, boundaries=("open", "periodic"))
    open_mk = masks_of(o.geometry(Y, X), multi_launch=True)
    small_mk = masks_of(o.geometry(Y, X))
    std = (1.0, 1.0)
    net = types.SimpleNamespace(name="mars_moon")
    # "circular" with open masks
    with pytest.raises(ValueError, match="LargeGridTrainer: conv_padding='circular' needs a periodic axis"):
        trainer.LargeGridTrainer(net, 2, Y, X, 2, std, 1.0, multi_launch=True, masks=open_mk, conv_padding="circular")
    with pytest.raises(ValueError, match="LargeGridTrainer: conv_padding='circular' needs a periodic axis"):
        trainer.make_trainer(net, open_mk, 2, Y, X, 2, g.dx, std, 1.0, multi_launch=True, conv_padding="circular")
    with pytest.raises(ValueError, match="LargeGridRollout: conv_padding='circular' needs a periodic axis"):
        trainer.LargeGridRollout(net, open_mk, 2, Y, X, g.dx, std, 1.0, multi_launch=True, conv_padding="circular")
    with pytest.raises(ValueError, match="LargeGridRollout: conv_padding='circular' needs a periodic axis"):
        trainer.make_rollout(net, open_mk, 2, Y, X, g.dx, std, 1.0, multi_launch=True, conv_padding="circular")
    # the classes of the one-workgroup kernels: "circular" refused by name; periodic masks keep their message
    for who, make in (("SolTrainer", lambda mk, **kw: trainer.SolTrainer(None, mk, 2, Y, X, 2, g.dx, std, 1.0, **kw)),
                      ("SolRollout", lambda mk, **kw: trainer.SolRollout(None, mk, 2, Y, X, g.dx, std, 1.0, **kw)),
                      ("GraphTrainer", lambda mk, **kw: trainer.GraphTrainer(None, 2, Y, X, 2, std, 1.0, masks=mk, **kw))):
        with pytest.raises(ValueError, match="%s: conv_padding='circular' pads the network's convolutions circularly" % who):
            make(small_mk, conv_padding="circular")
        with pytest.raises(ValueError, match="%s: the masks were built with periodic boundaries" % who):
            make(per_mk, conv_padding="circular")
        with pytest.raises(ValueError, match="%s: conv_padding must be 'zeros' or 'circular'" % who):
            make(small_mk, conv_padding="reflect")
    with pytest.raises(ValueError, match="SolTrainer: conv_padding='circular'"):
        trainer.make_trainer(net, small_mk, 2, Y, X, 2, g.dx, std, 1.0, conv_padding="circular")
    with pytest.raises(ValueError, match="SolRollout: conv_padding='circular'"):
        trainer.make_rollout(net, small_mk, 2, Y, X, g.dx, std, 1.0, conv_padding="circular")
    # any other word
    with pytest.raises(ValueError, match="LargeGridTrainer: conv_padding must be 'zeros' or 'circular'"):
        trainer.LargeGridTrainer(net, 2, Y, X, 2, std, 1.0, multi_launch=True, any_width=True, masks=per_mk, conv_padding="same")
    with pytest.raises(ValueError, match="LargeGridRollout: conv_padding must be 'zeros' or 'circular'"):
        trainer.LargeGridRollout(net, per_mk, 2, Y, X, g.dx, std, 1.0, multi_launch=True, any_width=True, conv_padding=None)
    # a width the zero-padded network refuses without any_width is served under "circular": the refusal that remains is the missing
    # device, not the width
    with pytest.raises(ValueError, match="take rows of X % 64 == 0 cells"):
        trainer.LargeGridRollout(net, per_mk, 2, Y, X, g.dx, std, 1.0, multi_launch=True)
    assert trainer._width_served(Y, X, False, True) is False
    if not torch.cuda.is_available():
        with pytest.raises(_lib.SolError, match="no ROCm device visible"):
            trainer.LargeGridRollout(net, per_mk, 2, Y, X, g.dx, std, 1.0, multi_launch=True, conv_padding="circular")
    # the schedule and the models
    with pytest.raises(_lib.SolError, match="padding must be 'zeros' or 'circular'"):
        NetSchedule2D(net, 2, Y, X, padding="same")
    with pytest.raises(_lib.SolError, match="padding='circular' needs a periodic axis"):
        NetSchedule2D(net, 2, Y, X, padding="circular")
    with pytest.raises(_lib.SolError, match="padding='circular' needs a periodic axis"):
        NetSchedule2D(net, 2, Y, X, padding="circular", periodic=(False, False))
    with pytest.raises(ValueError, match="padding must be 'zeros' or 'circular'"):
        model._circular_form("same", (False, True), False)
    with pytest.raises(ValueError, match="padding='circular' needs a periodic axis"):
        model._circular_form("circular", None, False)
    with pytest.raises(ValueError, match="scaled=True"):
        model._circular_form("circular", (False, True), True)
    assert model._circular_form("zeros", None, True) is None
    with pytest.raises(_lib.SolError, match="names no periodic axis"):
        ops.conv5x5_circular(None, None, None, (False, False))


def test_the_model_file_carries_the_padding(tmp_path):
    net = model.MarsMoon(3, 2, 0, "cpu")
    assert net.conv_padding == "zeros"
    net.save(str(tmp_path / "zeros.pt"))
    net.conv_padding = "circular"
    net.save(str(tmp_path / "circular.pt"))
    assert model.ConvNet.load(str(tmp_path / "zeros.pt"), device="cpu").conv_padding == "zeros"
    back = model.ConvNet.load(str(tmp_path / "circular.pt"), device="cpu")
    assert back.conv_padding == "circular" and back.clone().conv_padding == "circular" and torch.equal(back.params, net.params)
    blob = torch.load(str(tmp_path / "zeros.pt"))
    del blob["conv_padding"]            # a file written before the record existed
    torch.save(blob, str(tmp_path / "old.pt"))
    assert model.ConvNet.load(str(tmp_path / "old.pt"), device="cpu").conv_padding == "zeros"


def test_the_library_exports_the_halo_entry_and_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    assert lib.sol_version() == _lib.ABI_VERSION == 216          # additions only: the ABI number stays
    assert "sol_conv_halo" in _lib.declared_symbols() and hasattr(lib, "sol_conv_halo")
    host = np.zeros(16, dtype=np.float32)                       # never dereferenced: every call below returns before a launch
    buf = C.c_void_p(host.ctypes.data)
    call = lambda *a: lib.sol_conv_halo(None, *a)
    for args, what in (((None, 1, 4, 4, 64, 4, 4, 0), "NULL buffer"),
                       ((buf, 1, 4, 62, 64, 4, 4, 0), "is below W"),
                       ((buf, 1, 4, 4, 96, 4, 4, 0), "multiple of 64"),
                       ((buf, 1, 4, 4, 0, 4, 4, 0), "multiple of 64"),
                       ((buf, 1, 4, 4, 64, 4, 1, 0), "periodic_bits must be a combination"),
                       ((buf, 1, 4, 4, 64, 4, 8, 0), "periodic_bits must be a combination"),
                       ((buf, 1, 4, 4, 64, 4, 4, 2), "mode must be 0"),
                       ((buf, 1, 4, 4, 64, 4, 4, -1), "mode must be 0"),
                       ((buf, 1, 4, 4, 64, 6, 4, 0), "multiple of 4 up to 32"),
                       ((buf, 1, 4, 4, 64, 36, 4, 0), "multiple of 4 up to 32"),
                       ((buf, 0, 4, 4, 64, 4, 4, 0), "B, H, W >= 1")):
        assert call(*args) == -1, args                           # SOL_ERR_ARG
        assert what in lib.sol_last_error().decode(), (args, lib.sol_last_error())
    assert call(buf, 1, 4, 4, 64, 4, 0, 0) == 0 and call(buf, 1, 4, 4, 64, 4, 0, 1) == 0      # bits 0: nothing is launched
    assert not host.any()
