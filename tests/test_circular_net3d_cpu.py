"""Host twin of test_gpu_circular_net3d.py (no device): the float32 run of the float64 references at every GPU case, the transposed-halo
identity the feature rests on restated in torch, the condition that keeps the trainer test from being vacuous, the shape rule, the
refusals that need no device and the script's argument handling.

Measured here (float32 torch against float64 torch, no project code), next to a quarter of the bound the GPU test uses:
  one layer, worst of the nine cases            out 2.6e-7 (5e-7), gradients 6.8e-7 (1.25e-6)
  network, worst of the five cells              out 5.1e-7 (1.25e-6), dx 2.8e-7 (2.5e-6), parameter tensor 7.0e-7 (2.5e-6)
  trainer 16x8x8 / 16x8x12                      loss 8.4e-8 / 1.0e-7 (2.5e-6), per-step 3.6e-7 / 1.8e-7, gradient 4.3e-7 / 2.9e-7 (2.5e-5),
                                                final state 7.5e-7 / 7.7e-7 (2.5e-6)
  roll-out, three steps                         8.7e-7 / 8.9e-7 (7.5e-6)
  circular against zero-padded trainer          loss 0.28 / 0.17, gradient 0.54 / 0.40 at LAST_SCALE = 0.01 (needed: > 1e-3 or > 1e-2)
  a roll along z                                circular 0 ... 2e-15, zero padded 0.34 ... 0.77
Layers and networks accumulate in blocks in float32 (circular_net3d_cases.conv, blocked); with torch's one sequential run per output the
32-input layers read 7.5e-7 ... 9.9e-7 and the networks 8.9e-7 ... 2.0e-6 (see the two tests).  Figures are printed by the tests (-s)."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sol_oracle3d as o
from sol_amd import _lib
from sol_amd import karman3d as k3

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import circular_net3d_cases as cc
import periodic3d_cases as pc
from circular_net3d_cases import BOUNDS, rel, sid
from large2d_scenes import TOL_FIELD


# ---- 1. the references in float32 against float64, at every GPU case ---------------------------------------------------------------------
@pytest.mark.parametrize("chan", cc.LAYER_CHANNELS, ids=sid)
@pytest.mark.parametrize("cell", cc.LAYER_CELLS, ids=sid)
def test_one_layer_reference_in_float32(cell, chan):
    """float32 with the 25 (k_y, k_x) taps accumulated as partial convolutions (circular_net3d_cases.conv, blocked).  RECORDED: torch's
    single float32 conv3d call on the CPU runs each output's 125 cin terms in one sequence and alone reads 7.5e-7 ... 9.9e-7 on the
    32-input layers at these cells, beyond a quarter of the bound (5e-7) whatever the seed (it is the length of the sum, not the data);
    blocked, float32 reads 2.4e-7.  The bound stays conv_forward = 2e-6 / conv_gradient = 5e-6; the one-run figure is printed beside it."""
    case = cc.layer_case(cell, chan)
    r64, r32 = cc.layer_reference(*case), cc.layer_reference(*case, dtype=torch.float32, blocked=True)
    assert float((cc.layer_reference(*case, blocked=True)[0] - r64[0]).abs().max()) < 1e-12          # the same value in float64
    errs = [rel(a, b) for a, b in zip(r32, r64)]
    print("layer %s %s fp32 alone: out %.2e dx %.2e dw %.2e db %.2e (one sequential run: out %.2e)"
          % ((sid(cell), sid(chan)) + tuple(errs) + (rel(cc.layer_reference(*case, dtype=torch.float32)[0], r64[0]),)))
    assert errs[0] < BOUNDS["conv_forward"] / 4 and max(errs[1:]) < BOUNDS["conv_gradient"] / 4, errs


@pytest.mark.parametrize("cell", list(cc.NET_CELLS) + [cc.WIDE_CELL], ids=sid)
def test_network_reference_in_float32(cell):
    """float32 with blocked accumulation and the float64 run's masks, as in test_one_layer_reference_in_float32.  RECORDED: with torch's
    one sequential run per output the float32 network alone reads out 8.9e-7 ... 2.0e-6 at these cells, beyond a quarter of net_out
    (1.25e-6) at four of the five; the figure is printed beside the blocked one."""
    x, gy, params = cc.network_case(cell)
    gy = None if cell == cc.WIDE_CELL else gy
    o64, dx64, g64, m64, _ = cc.torch_network(x, gy, params)
    o32, dx32, g32, _, _ = cc.torch_network(x, gy, params, masks=m64, dtype=torch.float32, blocked=True)
    e = [rel(o32, o64)] + ([] if gy is None else [rel(dx32, dx64), max(rel(a, b) for a, b in zip(g32, g64))])
    print("network %s fp32 alone:" % sid(cell), ["%.2e" % v for v in e],
          "(one sequential run: out %.2e)" % rel(cc.torch_network(x, None, params, masks=m64, dtype=torch.float32)[0], o64))
    assert e[0] < BOUNDS["net_out"] / 4, e
    if gy is not None:
        assert e[1] < BOUNDS["net_dx"] / 4 and e[2] < BOUNDS["net_param"] / 4, e


@pytest.mark.parametrize("cell", cc.TRAIN_CELLS, ids=sid)
def test_trainer_and_rollout_references_in_float32(cell):
    p = cc.trainer_problem(cell)
    l64, s64, g64, f64 = cc.trainer_reference(p)
    l32, s32, g32, f32_ = cc.trainer_reference(p, dtype=torch.float32)
    e = abs(l32 - l64) / abs(l64), max(abs(a - b) / abs(b) for a, b in zip(s32, s64)), rel(g32, g64), max(rel(a, b) for a, b in zip(f32_, f64))
    print("trainer %s fp32 alone: loss %.2e, per-step %.2e, gradient %.2e, final %.2e" % ((sid(cell),) + e))
    assert e[0] < BOUNDS["oracle_loss"] / 4 and e[1] < BOUNDS["oracle_loss"] / 4 and e[2] < BOUNDS["oracle_grad"] / 4 and e[3] < TOL_FIELD / 4, e
    off, per = 0, []
    for q in p["params"]:
        per.append(rel(g32[off:off + q.numel()], g64[off:off + q.numel()]))
        off += q.numel()
    assert max(per) < BOUNDS["oracle_param"] / 4, per
    r64, r32 = cc.rollout_reference(p, 3), cc.rollout_reference(p, 3, dtype=torch.float32)
    er = max(rel(a, b) for a, b in zip(r32, r64))
    print("    roll-out, three steps, fp32 alone: %.2e" % er)
    assert er < 3 * TOL_FIELD / 4, er
    assert torch.equal(r64[3][..., -1], r64[3][..., 0])


def test_the_float64_network_with_zero_padding_is_the_oracle_network():
    ps, x = cc.equivariance_case((1, 6, 8, 8))
    assert float((cc.mars_moon3d(ps, x, cc.ZEROS) - o.mars_moon3d(ps, x)).abs().max()) < 1e-12
    # (torch_network applies the slope as the device holds it, float32(0.3) = 0.3 (1 + 4e-8), like karman3d_net_shapes.torch_network)
    assert float((cc.torch_network(x, None, ps, padding=cc.ZEROS)[0] - o.mars_moon3d(ps, x)).abs().max()) < 1e-7


# ---- 2. the transposed-halo identity ---------------------------------------------------------------------------------------------------------
def to_buffer(t, HB, halo, garbage=None):
    """t [B,Y,X,Z,C] -> [B,Y,HB,X,C]: planes transposed into rows [2, Z + 2), halo rows wrapped ("wrap") or zero, pad rows garbage or zero"""
    Bn, Y, X, Z, c = t.shape
    buf = torch.zeros(Bn, Y, HB, X, c, dtype=t.dtype)
    if garbage is not None:
        buf[:, :, Z + 4:] = garbage
    tt = t.permute(0, 1, 3, 2, 4)
    buf[:, :, 2:Z + 2] = tt
    if halo == "wrap":
        for r in (0, 1, Z + 2, Z + 3):
            buf[:, :, r] = tt[:, :, (r - 2) % Z]
    return buf


def from_buffer(buf, Z):
    return buf[:, :, 2:Z + 2].permute(0, 1, 3, 2, 4)


def zero_conv(x, w):
    """the convolution the kernels run: zero padding on every side of the volume handed to them"""
    return cc.conv(x, w, None, cc.ZEROS)


@pytest.mark.parametrize("cell", [(1, 3, 4, 6), (2, 5, 16, 12), (1, 3, 64, 5)], ids=sid)
def test_the_transposed_halo_identity(cell):
    """forward: valid rows of zero_conv(wrapped transposed buffer, w with axes 1 and 2 swapped) = the circular convolution, pad rows
    holding garbage; backward-data: the same with the flipped, transposed kernel on the wrapped dz; weight gradient: autograd of the
    zero-padded convolution on the buffer with a zero-halo dz, axes swapped back = autograd of the circular convolution"""
    Bn, Y, X, Z = cell
    HB = cc.rows(X, Z)
    assert HB == k3.circular_rows3d(X, Z)
    if X == 4:
        assert HB > Z + 4
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, w, dz = r(Bn, Y, X, Z, 4), r(5, 5, 5, 4, 6), r(Bn, Y, X, Z, 6)
    xl, wl = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = cc.conv(xl, wl)
    y.backward(dz)
    ws = w.permute(0, 2, 1, 3, 4)
    # forward
    yb = zero_conv(to_buffer(x, HB, "wrap", garbage=1e30), ws)
    assert float((from_buffer(yb, Z) - y.detach()).abs().max()) < 1e-13
    # backward-data on the wrapped dz: the flipped kernel with the channel axes exchanged
    wb = ws.flip(0, 1, 2).permute(0, 1, 2, 4, 3)
    dxb = zero_conv(to_buffer(dz, HB, "wrap", garbage=1e30), wb)
    assert float((from_buffer(dxb, Z) - xl.grad).abs().max()) < 1e-12
    # weight gradient with a zero-halo dz (garbage in the pad rows of x only: dz is zero there)
    wsl = ws.clone().requires_grad_(True)
    zero_conv(to_buffer(x, HB, "wrap", garbage=7.0), wsl).backward(to_buffer(dz, HB, "zero"))
    assert float((wsl.grad.permute(0, 2, 1, 3, 4) - wl.grad).abs().max()) < 1e-11
    assert float((to_buffer(dz, HB, "zero").sum((0, 1, 2, 3)) - dz.sum((0, 1, 2, 3))).abs().max()) < 1e-12      # the bias gradient
    # a wrapped halo on dz would NOT do for the weight gradient
    wsl.grad = None
    zero_conv(to_buffer(x, HB, "wrap"), wsl).backward(to_buffer(dz, HB, "wrap"))
    assert rel(wsl.grad.permute(0, 2, 1, 3, 4), wl.grad) > 1e-2


@pytest.mark.parametrize("cell", cc.EQUIV_CELLS, ids=sid)
def test_the_circular_network_commutes_with_a_roll_and_the_zero_padded_one_does_not(cell):
    ps, x = cc.equivariance_case(cell)
    base_c, base_z = cc.mars_moon3d(ps, x), cc.mars_moon3d(ps, x, cc.ZEROS)
    for s in cc.ROLLS(cell[3]):
        circ = rel(cc.mars_moon3d(ps, torch.roll(x, s, 3)), torch.roll(base_c, s, 3))
        zero = rel(cc.mars_moon3d(ps, torch.roll(x, s, 3), cc.ZEROS), torch.roll(base_z, s, 3))
        print("%s roll %d: circular %.2e, zero padded %.2e" % (sid(cell), s, circ, zero))
        assert circ < 1e-13 and zero > 100 * BOUNDS["net_out"], (s, circ, zero)


# ---- 3. the trainer problem is not vacuous ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", cc.TRAIN_CELLS[:1], ids=sid)
def test_the_trainer_problem_tells_circular_from_zero_padding(cell):
    """the zero-padded network runs at 16 x 8 x 8 only (the other grid it refuses: there the zero-padded float64 reference still exists)"""
    for c in cc.TRAIN_CELLS:
        p = cc.trainer_problem(c)
        lc, _, gc, _ = cc.trainer_reference(p)
        lz, _, gz, _ = cc.trainer_reference(p, cc.ZEROS)
        dl, dg = abs(lc - lz) / abs(lc), rel(gz, gc)
        print("trainer %s, LAST_SCALE %g: circular against zero padded loss %.3e, gradient %.3e" % (sid(c), cc.LAST_SCALE, dl, dg))
        assert dl > 100 * BOUNDS["oracle_loss"] or dg > 100 * BOUNDS["oracle_grad"], (dl, dg)
        assert dg > 100 * BOUNDS["manual_grad"]


# ---- 4. the shape rule and the refusals ------------------------------------------------------------------------------------------------------
def test_the_shape_rule_against_the_table():
    for (Y, X, Z, train), words in cc.SHAPE_TABLE.items():
        why = k3.net3d_circular_shape_reason(Y, X, Z, train)
        assert (why is not None) == cc.circular_shape_refused(Y, X, Z, train) == (words is not None), (Y, X, Z, train, why)
        for wd in words or ():
            assert wd in why, (wd, why)
    # every grid: the function against the restated conditions; Z = 12, 24, 72, which the zero-padded network refuses, are served
    for Y in (2, 3, 16):
        for X in range(1, 200):
            for Z in (1, 2, 5, 12, 24, 64, 72):
                for train in (True, False):
                    assert (k3.net3d_circular_shape_reason(Y, X, Z, train) is not None) == cc.circular_shape_refused(Y, X, Z, train), (Y, X, Z, train)
    for Z in (12, 24, 72):
        assert k3.net3d_shape_reason(16, 8, Z) is not None and k3.net3d_circular_shape_reason(16, 8, Z) is None
    for X in (4, 8, 16, 32, 64, 128):
        for Z in (2, 5, 6, 10, 12, 64):
            HB = k3.circular_rows3d(X, Z)
            assert HB == cc.rows(X, Z) and Z + 4 <= HB < Z + 4 + max(1, 64 // X) and (X >= 64 or HB % (64 // X) == 0)
            assert k3.net3d_shape_reason(16, HB, X, train=X <= 64) is None          # the buffer is a volume the kernels take
    assert k3.circular_rows3d(64, 64) == 68 and k3.circular_rows3d(4, 6) == 16 and k3.circular_rows3d(64, 4) == 8


def test_refusals_that_need_no_device():
    from sol_amd.schedule3d import NetSchedule3D
    net = types.SimpleNamespace(cin=4, cout=3)
    with pytest.raises(_lib.SolError, match="padding must be 'zeros' or 'circular'"):
        NetSchedule3D(net, 2, 16, 8, 8, padding="same")
    with pytest.raises(_lib.SolError, match=r"NetSchedule3D\(train=True, padding='circular'\) at 16 x 12 x 8: X = 12"):
        NetSchedule3D(net, 2, 16, 12, 8, padding="circular")
    with pytest.raises(_lib.SolError, match="X = 128.*X <= 64.*roll-out"):
        NetSchedule3D(net, 2, 16, 128, 8, padding="circular")
    with pytest.raises(_lib.SolError, match=r"NetSchedule3D\(train=True\) at 16 x 8 x 12: Z = 12"):          # the default's message as it was
        NetSchedule3D(net, 2, 16, 8, 12)
    per = types.SimpleNamespace(periodic_bits=8, Y=16, X=8, Z=12)
    wide = types.SimpleNamespace(periodic_bits=8, Y=16, X=128, Z=12)
    bad = types.SimpleNamespace(periodic_bits=8, Y=16, X=10, Z=12)
    opn = types.SimpleNamespace(periodic_bits=0, Y=16, X=8, Z=8)
    std = (1.0, 1.0, 1.0)
    for who, make in (("Karman3DTrainer", lambda sc, **kw: k3.Karman3DTrainer(net, sc, 2, 2, std, 1.0, **kw)),
                      ("Karman3DRollout", lambda sc, **kw: k3.Karman3DRollout(net, sc, 2, std, 1.0, **kw))):
        with pytest.raises(_lib.SolError, match="%s: conv_padding='circular' needs a z-periodic scene" % who):
            make(opn, conv_padding="circular")
        for word in ("same", None, "Circular"):
            with pytest.raises(_lib.SolError, match="%s: conv_padding must be 'zeros' or 'circular'" % who):
                make(per, conv_padding=word)
        with pytest.raises(_lib.SolError, match="%s: conv_padding='circular' at 16 x 10 x 12: X = 10" % who):
            make(bad, conv_padding="circular")
        if not torch.cuda.is_available():              # a served grid: the refusal that remains is the missing device
            with pytest.raises(_lib.SolError, match="no ROCm device visible"):
                make(per, conv_padding="circular")
    with pytest.raises(_lib.SolError, match="Karman3DTrainer: conv_padding='circular' at 16 x 128 x 12: X = 128.*X <= 64"):
        k3.Karman3DTrainer(net, wide, 2, 2, std, 1.0, conv_padding="circular")
    with pytest.raises(_lib.SolError, match="conv3d_circular at 3 x 12 x 6: X = 12"):
        k3.conv3d_circular(torch.zeros(1, 3, 12, 6, 4), torch.zeros(5, 5, 5, 4, 32), torch.zeros(32))
    with pytest.raises(_lib.SolError, match="MarsMoon3D: padding must be 'zeros' or 'circular'"):
        m = k3.MarsMoon3D(device="cpu")
        m.fused_backward = False
        m(torch.zeros(1, 3, 8, 6, 4), padding="same")


def test_the_library_exports_the_entries_and_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    names = ("sol_conv3d_circ_pack", "sol_conv3d_circ_unpack", "sol_conv3d_halo")
    assert all(n in _lib.declared_symbols() and hasattr(lib, n) for n in names)
    host = np.zeros(16, dtype=np.float32)                       # never dereferenced: every call below returns before a launch
    a = C.c_void_p(host.ctypes.data)
    for fn, args, what in ((lib.sol_conv3d_circ_pack, (None, a, 1, 3, 4, 6, 16, 4, 0), "NULL buffer"),
                           (lib.sol_conv3d_circ_pack, (a, a, 1, 0, 4, 6, 16, 4, 0), "B, Y >= 1"),
                           (lib.sol_conv3d_circ_pack, (a, a, 1, 3, 0, 6, 16, 4, 0), "X >= 1"),
                           (lib.sol_conv3d_circ_pack, (a, a, 1, 3, 4, 1, 16, 4, 0), "Z >= 2"),
                           (lib.sol_conv3d_circ_pack, (a, a, 1, 3, 4, 6, 9, 4, 0), "HB = 9 is below Z + 4 = 10"),
                           (lib.sol_conv3d_circ_pack, (a, a, 1, 3, 4, 6, 16, 3, 0), "C must be 4"),
                           (lib.sol_conv3d_circ_pack, (a, a, 1, 3, 4, 6, 16, 4, -1), "mode must be 0 (wrap) or 1 (zero)"),
                           (lib.sol_conv3d_circ_pack, (a, a, 1 << 15, 1 << 15, 4, 6, 16, 4, 0), "32-bit pixel index"),
                           (lib.sol_conv3d_circ_unpack, (a, None, 1, 3, 4, 6, 16, 3), "NULL buffer"),
                           (lib.sol_conv3d_circ_unpack, (a, a, 1, 3, 4, 6, 16, 32), "C must be 3 or 4"),
                           (lib.sol_conv3d_circ_unpack, (a, a, 1, 3, 4, 6, 9, 4), "is below Z + 4"),
                           (lib.sol_conv3d_halo, (None, 3, 6, 16, 4, 4, 0), "NULL buffer"),
                           (lib.sol_conv3d_halo, (a, 0, 6, 16, 4, 4, 0), "X >= 1"),
                           (lib.sol_conv3d_halo, (a, 3, 6, 16, 4, 16, 0), "C must be 4 or 32"),
                           (lib.sol_conv3d_halo, (a, 3, 6, 16, 4, 4, 2), "mode must be 0"),
                           (lib.sol_conv3d_halo, (a, 3, 1, 16, 4, 4, 0), "Z >= 2")):
        assert fn(None, *args) == -1, args                           # SOL_ERR_ARG
        assert what in lib.sol_last_error().decode(), (args, lib.sol_last_error())
    assert not host.any()


# ---- 5. the script's argument handling and its record ------------------------------------------------------------------------------------------
def _script():
    import importlib.util
    import sol_amd
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    if sdir not in sys.path:
        sys.path.insert(0, sdir)
    spec = importlib.util.spec_from_file_location("sol_script_karman3d_circular_cpu", os.path.join(sdir, "karman3d.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_the_script_handles_conv_padding():
    mod = _script()
    base = ["-r", "8", "--re", "1.6e5", "--obstacle", "cylinder"]
    rec = lambda argv, record=None: mod.apply_model_record(dict(mod.parse_params(base + argv), model="m.pt" if record is not None else None), record)
    assert rec([])["conv_padding"] == "zeros"
    assert rec(["--boundaries", "periodic-z", "--conv-padding", "circular"])["conv_padding"] == "circular"
    assert rec(["--boundaries", "periodic-z", "--conv-padding", "zeros"])["conv_padding"] == "zeros"
    # picked up from the model's record, with its boundaries
    got = rec([], {"boundaries": "periodic-z", "conv_padding": "circular"})
    assert got["conv_padding"] == "circular" and got["boundaries"] == "periodic-z"
    assert rec([], {"boundaries": "periodic-z"})["conv_padding"] == "zeros"            # a file written before the record existed
    assert rec(["--conv-padding", "circular"], {"boundaries": "periodic-z"})["conv_padding"] == "circular"
    with pytest.raises(SystemExit, match="--conv-padding zeros contradicts the padding recorded in m.pt \\(circular\\)"):
        rec(["--conv-padding", "zeros"], {"boundaries": "periodic-z", "conv_padding": "circular"})
    # circular on open boundaries exits with a sentence
    for argv in (["--conv-padding", "circular"], ["--conv-padding", "circular", "--boundaries", "open"]):
        with pytest.raises(SystemExit, match="--conv-padding circular pads the correction network circularly along z and needs --boundaries periodic-z"):
            rec(argv)
    with pytest.raises(SystemExit):
        mod.parse_params(base + ["--conv-padding", "reflect"])
    # a grid the circular network refuses exits before a device is asked for; r = 12 (Z = 12) is served under circular only
    with pytest.raises(SystemExit, match="the correction network does not run at 20 x 10 x 10 -- X = 10"):
        mod.main(["-r", "10", "--obstacle", "cylinder", "--boundaries", "periodic-z", "--conv-padding", "circular", "--train-sol", "2"])
    with pytest.raises(SystemExit, match="the correction network does not run at 24 x 12 x 12 -- Z = 12"):
        mod.main(["-r", "12", "--obstacle", "cylinder", "--boundaries", "periodic-z", "--train-sol", "2"])
