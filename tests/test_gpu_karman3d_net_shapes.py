"""The karman-3d correction network, its trainer and its roll-out at every row width (pytest -m gpu).

The rest of the 3-D suite runs MarsMoon3D, schedule3d.NetSchedule3D, Karman3DTrainer and Karman3DRollout on (2r, r, r) grids with Z in
{8, 16, 64} and X = Z.  Here: the table of karman3d_net_shapes -- Z = 32, 16 with X != Z, 8, 4, the one-launch kernels on a ragged row
count, Z = 128 (forward only), the persistent one-launch form with 2 and 3 tiles per workgroup -- through
  (a) every layer entry point against torch float64 conv3d of the same operation, with per-plane and per-depth-slice errors in the message,
  (b) the network against torch float64 autograd and against its own per-layer composition,
  (c) the trainer (hand-written schedule against the autograd composition, captured replay against eager, the float64 oracle at
      16 x 8 x 32) and the roll-out schedule against the training forward,
  (d) a roll-out at Z = 128,
  (e) all-zero operands and the dynamic range of the one-launch kernel's own fp16 x 3 split,
and the refusals of NetSchedule3D / Karman3DTrainer / Karman3DRollout at construction, without a launch.  Every case asserts through the
launch profiler that the kernels the table predicts are the ones that ran.  Bounds are the suite's own (karman3d_net_shapes.BOUNDS); the
figures measured on an MI355X stand in the docstring of karman3d_net_shapes."""
import collections
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sol_oracle3d as o
from sol_amd import _lib
from sol_amd import karman3d as k3
from sol_amd import ops
from sol_amd.schedule3d import NetSchedule3D

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import karman3d_net_shapes as kn
from karman3d_net_shapes import BOUNDS, DEV, GRAD_CELLS, LAYER_CELLS, NET_CELLS, PERSIST_CELLS, SLOPE, STD_V, TRAIN_CELLS, WIDE_CELL, f32, rel, sid
from test_gpu_karman3d_shapes import options

pytestmark = pytest.mark.gpu


def randn(gen, *s, scale=1.0):
    return (torch.randn(*s, generator=gen, dtype=torch.float32) * scale).to(DEV)


def nan_like(*s):
    return torch.full(s, float("nan"), dtype=torch.float32, device=DEV)


def slots():
    return torch.zeros(256, dtype=torch.int32, device=DEV)


def published(ymax):
    return float(ymax.max().view(torch.float32))


def check_absmax(ymax, y, what):
    pub = published(ymax)
    assert np.isfinite(pub) and abs(pub - float(y.abs().max())) <= BOUNDS["absmax"] * pub, (what, pub, float(y.abs().max()))


def grad_ref(x, dz):
    """float64 dW [5,5,5,ci,co], db [co] of y = conv3d(x, W) + b for the output gradient dz, by torch autograd on the device"""
    ci, co = x.shape[-1], dz.shape[-1]
    w = torch.zeros(co, ci, 5, 5, 5, dtype=torch.float64, device=DEV, requires_grad=True)
    (F.conv3d(kn.ncdhw(x.double()), w, padding=2) * kn.ncdhw(dz.double())).sum().backward()
    return w.grad.permute(2, 3, 4, 1, 0), dz.double().sum(dim=(0, 1, 2, 3))


# ---- (a) layers against float64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", LAYER_CELLS, ids=sid)
def test_conv3d_32_to_32_against_float64(cell):
    """k3.conv3d 32 -> 32 with the absmax slots of its input: bias + residual + LeakyReLU, and the reverse sweep's form (residual, times
    LeakyReLU'(act_ref), SOL_EPI_DLRELU), against float64 conv3d; the published y_absmax is max|y|; the kernels are the table's."""
    B, D, H, W = cell
    gen = torch.Generator().manual_seed(1000 * B + 100 * D + W)
    x, r, act = randn(gen, B, D, H, W, 32), randn(gen, B, D, H, W, 32), randn(gen, B, D, H, W, 32)
    w, b = randn(gen, 5, 5, 5, 32, 32, scale=1 / np.sqrt(125 * 32)), randn(gen, 32)
    packed = k3._pack3d(w, 32, 32, 0)
    z = kn.conv3d_ref(x.double(), w.double(), b.double()) + r.double()
    zd = kn.conv3d_ref(x.double(), w.double()) + r.double()
    refs = {"lrelu": torch.where(z > 0, z, SLOPE * z), "dlrelu": zd * torch.where(act > 0, 1.0, SLOPE).double()}
    amax = ops.absmax_slots(x)
    for mode, ref in refs.items():
        ymax, y = slots(), nan_like(B, D, H, W, 32)
        with _lib.profile() as p:
            k3.conv3d(x, packed, b if mode == "lrelu" else None, r, 32, mode == "lrelu", SLOPE, amax, ymax, out=y,
                      act_ref=act if mode == "dlrelu" else None)
            torch.cuda.synchronize()
        assert kn.conv_kernels(p) == kn.conv3d_launches(B, D, H, W), (mode, sorted(p.kernels))
        e = rel(y, ref)
        print("conv3d 32->32 %s at %s: %.2e; kernels %s" % (mode, sid(cell), e, dict(kn.conv_kernels(p))))
        assert not bool(torch.isnan(y).any()) and e < BOUNDS["conv_forward"], (mode, e, kn.per_plane(y, ref))
        check_absmax(ymax, y, mode)


@pytest.mark.parametrize("cell", LAYER_CELLS, ids=sid)
def test_thin_layers_against_float64(cell):
    """conv3d_thin (4 -> 32, bias + LeakyReLU) and conv3d_thin_out (32 -> 3, bias) against float64 conv3d: one 2-D 32 -> 32 launch each"""
    B, D, H, W = cell
    gen = torch.Generator().manual_seed(2000 * B + 100 * D + W)
    x4, x32 = randn(gen, B, D, H, W, 4), randn(gen, B, D, H, W, 32)
    w0, b0 = randn(gen, 5, 5, 5, 4, 32, scale=1 / np.sqrt(125 * 4)), randn(gen, 32)
    w1, b1 = randn(gen, 5, 5, 5, 32, 3, scale=1 / np.sqrt(125 * 32)), randn(gen, 3)
    z = kn.conv3d_ref(x4.double(), w0.double(), b0.double())
    ref0, ref1 = torch.where(z > 0, z, SLOPE * z), kn.conv3d_ref(x32.double(), w1.double(), b1.double())
    ymax, y0, y1 = slots(), nan_like(B, D, H, W, 32), nan_like(B, D, H, W, 3)
    with _lib.profile() as p:
        k3.conv3d_thin(x4, k3._pack3d_thin(w0, 4, 0), b0, True, SLOPE, ymax, out=y0)
        torch.cuda.synchronize()
    assert kn.conv_kernels(p) == kn.thin_launches(B, D, H, W), sorted(p.kernels)
    with _lib.profile() as q:
        k3.conv3d_thin_out(x32, k3._pack3d_thin_out(w1, 3, 0), b1, 3, ops.absmax_slots(x32), out=y1)
        torch.cuda.synchronize()
    assert kn.conv_kernels(q) == kn.thin_launches(B, D, H, W), sorted(q.kernels)
    e0, e1 = rel(y0, ref0), rel(y1, ref1)
    print("thin layers at %s: 4->32 %.2e, 32->3 %.2e; kernels %s" % (sid(cell), e0, e1, dict(kn.conv_kernels(p))))
    assert not bool(torch.isnan(y0).any()) and e0 < BOUNDS["conv_forward"], (e0, kn.per_plane(y0, ref0))
    assert not bool(torch.isnan(y1).any()) and e1 < BOUNDS["conv_forward"], (e1, kn.per_plane(y1, ref1))
    check_absmax(ymax, y0, "thin")


WG_FORMS = [(32, 32), (4, 32), (32, 3)]


def weight_gradient_forms(cell):
    """(name, run(x, dz, acc) -> (dW, db), channels, kernels predicted) of every weight-gradient form of a cell; x / dz as the layer has them"""
    B, D, H, W = cell
    forms = []
    for ci, co in WG_FORMS:
        run = lambda x, dz, acc=None, ci=ci, co=co: k3.conv3d_bwd_weight(k3._pad_ch(x, 4 if ci <= 4 else 32), dz, ci, co, acc=acc)
        forms.append(("five-slice %d->%d" % (ci, co), run, ci, co, kn.bww_launches(B, D, H, W, 4 if ci <= 4 else 32, 32)))
    if W == 64:
        thin = collections.Counter({kn.thin_bww_kernel(B, D, H): 1})
        forms.append(("depth-packed 4->32", lambda x, dz, acc=None: k3.conv3d_thin_bwd_weight(k3._pad_ch(x, 4), dz, 4, acc=acc), 4, 32, thin))
        forms.append(("depth-packed 32->3", lambda x, dz, acc=None: k3.conv3d_thin_bwd_weight(k3._pad_ch(dz, 4), x, 3, acc=acc, thin_out=True), 32, 3, thin))
    return forms


@pytest.mark.parametrize("cell", GRAD_CELLS, ids=sid)
def test_weight_gradients_against_float64(cell):
    """conv3d_bwd_weight (32 -> 32, 4 -> 32, 32 -> 3) and at W = 64 conv3d_thin_bwd_weight in both orientations against float64 autograd of
    conv3d, the output gradient on another scale (x 1e-3): a single call, and a two-call acc= sequence that must equal the sum of two single
    calls; an all-zero dz gives an exactly zero dW and db."""
    B, D, H, W = cell
    gen = torch.Generator().manual_seed(3000 * B + 100 * D + W)
    for name, run, ci, co, want in weight_gradient_forms(cell):
        xs = [randn(gen, B, D, H, W, ci) for _ in range(2)]
        dzs = [randn(gen, B, D, H, W, co, scale=1e-3) for _ in range(2)]
        refs = [grad_ref(x, dz) for x, dz in zip(xs, dzs)]
        with _lib.profile() as p:
            dW, db = (t.clone() for t in run(xs[0], dzs[0]))
            torch.cuda.synchronize()
        assert kn.bww_kernels(p) == want, (name, sorted(p.kernels), want)
        eW, eb = rel(dW, refs[0][0]), rel(db, refs[0][1])
        print("weight gradient %s at %s: dW %.2e, db %.2e; kernels %s" % (name, sid(cell), eW, eb, dict(kn.bww_kernels(p))))
        assert dW.shape == (5, 5, 5, ci, co) and db.shape == (co,)
        assert eW < BOUNDS["conv_gradient"] and eb < BOUNDS["conv_gradient"], (name, eW, eb, kn.per_slice(dW, refs[0][0]))
        single1 = [t.clone() for t in run(xs[1], dzs[1])]
        st = {}
        assert run(xs[0], dzs[0], (st, True, False)) == (None, None)
        dW2, db2 = run(xs[1], dzs[1], (st, False, True))
        torch.cuda.synchronize()
        e2 = (rel(dW2, dW.double() + single1[0].double()), rel(db2, db.double() + single1[1].double()))
        e2r = (rel(dW2, refs[0][0] + refs[1][0]), rel(db2, refs[0][1] + refs[1][1]))
        print("  two calls accumulated: against the sum of two single calls %.2e / %.2e, against float64 %.2e / %.2e" % (e2 + e2r))
        assert max(e2) < 2e-6 and max(e2r) < BOUNDS["conv_gradient"], (name, e2, e2r, kn.per_slice(dW2, refs[0][0] + refs[1][0]))
        zW, zb = run(xs[0], torch.zeros_like(dzs[0]))
        torch.cuda.synchronize()
        assert float(zW.abs().max()) == 0.0 and float(zb.abs().max()) == 0.0 and not bool(torch.isnan(zW).any()), (name, "zero dz")


@pytest.mark.parametrize("cell", PERSIST_CELLS, ids=sid)
def test_persistent_one_launch_form(cell):
    """Option k3d_conv_persist at 512 and 768 eight-row tiles (2 and 3 consecutive tiles per workgroup; the suite has 4 at 128 x 64 x 64): the
    one-launch result against the five-pass form and against one tile per workgroup, both modes of the epilogue."""
    B, D, H, W = cell
    gen = torch.Generator().manual_seed(D)
    x, r, act = randn(gen, B, D, H, W, 32), randn(gen, B, D, H, W, 32), randn(gen, B, D, H, W, 32)
    w, b = randn(gen, 5, 5, 5, 32, 32, scale=1 / np.sqrt(125 * 32)), randn(gen, 32)
    packed, amax = k3._pack3d(w, 32, 32, 0), ops.absmax_slots(x)
    want = kn.one_launch(B, D, H, persist=1)
    assert want["persistent"] and want["tiles_per_wg"] == D // 32
    for mode in ("lrelu", "dlrelu"):
        run = lambda: k3.conv3d(x, packed, b if mode == "lrelu" else None, r, 32, mode == "lrelu", SLOPE, amax, None,
                                act_ref=act if mode == "dlrelu" else None)
        res = {}
        for name, opts in (("one", {}), ("persist", dict(k3d_conv_persist=1)), ("five", dict(k3d_conv_fused=0))):
            with options(**opts), _lib.profile() as p:
                res[name] = run()
                torch.cuda.synchronize()
            assert kn.conv_kernels(p) == kn.conv3d_launches(B, D, H, W, fused=opts.get("k3d_conv_fused", 1), persist=opts.get("k3d_conv_persist", 0)), (name, sorted(p.kernels))
        e5, ep, e1 = rel(res["persist"], res["five"]), rel(res["persist"], res["one"]), rel(res["one"], res["five"])
        print("persistent form %s at %s: against five passes %.2e, against one tile per workgroup %.2e (bit-equal: %s); one tile against five passes %.2e"
              % (mode, sid(cell), e5, ep, torch.equal(res["persist"], res["one"]), e1))
        assert bool(torch.isfinite(res["persist"]).all())
        assert max(e5, ep, e1) < BOUNDS["one_launch_vs_five_pass"], (mode, e5, ep, e1, kn.per_plane(res["persist"][:, ::16], res["five"][:, ::16]))


# ---- (b) the network -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", NET_CELLS, ids=sid)
def test_network_against_torch_float64_autograd(cell):
    """the body of test_network_w64_against_torch_float64_autograd (karman3d_net_shapes.hip_network_against_float64) at every network cell:
    output, input gradient and the 24 parameter gradients, per tensor"""
    e_out, e_x, per, flips = kn.hip_network_against_float64(cell)
    print("network at %s against torch float64: out %.2e, dx %.2e, params max %.2e (tensor %d), %d activation signs differ; fp32 alone %s"
          % (sid(cell), e_out, e_x, max(per), int(np.argmax(per)), flips, kn.FP32_ALONE[cell]))
    b_out, b_x, b_p = kn.NET_BOUNDS[cell]
    assert e_out < b_out and e_x < b_x and max(per) < b_p, (e_out, e_x, per)


NET_SHAPES = NET_CELLS + [(kn.TRAIN_B,) + c for c in TRAIN_CELLS]


@pytest.mark.parametrize("shape", NET_SHAPES, ids=sid)
def test_network_launches_the_kernels_of_the_table(shape):
    """forward and reverse sweep of MarsMoon3D at every network cell and at the shapes of the trainer cells: the launch profiler against
    karman3d_net_shapes.net_forward_launches / net_backward_launches, names and counts"""
    x, gy, params = kn.network_case(shape)
    net = k3.MarsMoon3D(device=DEV)
    net.set_weights([p.numpy() for p in params])
    net.params.requires_grad_(True)
    xi = x.to(DEV).requires_grad_(True)
    net.schedule(*shape).begin_step()
    with _lib.profile() as p:
        out = net(xi)
        torch.cuda.synchronize()
    with _lib.profile() as q:
        (out * gy.to(DEV)).sum().backward()
        torch.cuda.synchronize()
    conv, bww = kn.net_backward_launches(*shape)
    print("network at %s: forward %s; reverse sweep %s, %s" % (sid(shape), dict(kn.conv_kernels(p)), dict(kn.conv_kernels(q)), dict(kn.bww_kernels(q))))
    assert kn.conv_kernels(p) == kn.net_forward_launches(*shape) and not kn.bww_kernels(p), sorted(p.kernels)
    assert kn.conv_kernels(q) == conv and kn.bww_kernels(q) == bww, sorted(q.kernels)


@pytest.mark.parametrize("cell", NET_CELLS, ids=sid)
def test_network_fused_reverse_sweep_equals_per_layer_autograd(cell):
    """test_network_fused_reverse_sweep_equals_per_layer_autograd's comparison at every network cell: outputs bit-equal, gradients to round-off"""
    x, gy, params = kn.network_case(cell, seed=11)
    res = {}
    for fused in (True, False):
        net = k3.MarsMoon3D(device=DEV)
        net.set_weights([p.numpy() for p in params])
        net.fused_backward = fused
        net.params.requires_grad_(True)
        xi = x.to(DEV).requires_grad_(True)
        out = net(xi)
        (out * gy.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        res[fused] = (out.detach(), xi.grad, net.params.grad, net.offsets)
    (oa, xa, pa, off), (ob, xb, pb, _) = res[True], res[False]
    per = [rel(pa[off[k]:off[k + 1]], pb[off[k]:off[k + 1]]) for k in range(24)]
    print("fused against per-layer at %s: dx %.2e, flat gradient %.2e, per tensor max %.2e" % (sid(cell), rel(xa, xb), rel(pa, pb), max(per)))
    assert torch.equal(oa, ob), rel(oa, ob)
    assert rel(xa, xb) < BOUNDS["fused_dx"] and rel(pa, pb) < BOUNDS["fused_flat"] and max(per) < BOUNDS["fused_param"], (rel(xa, xb), rel(pa, pb), per)


# ---- (c) trainer and roll-out --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(cell):
    g = kn.geometry(cell)
    sc = k3.Scene3D(*cell, device=DEV, active=g.active, inflow=g.inflow)
    assert sc.pressure_solver == "direct"
    return g, sc


def golden_net():
    net = k3.MarsMoon3D(device=DEV)
    net.set_weights([p.numpy() for p in kn.golden_params()])
    return net


@functools.lru_cache(maxsize=None)
def trainer_run(cell, schedule="manual", use_graph=False):
    """one SOL-2 fwd_bwd of a trainer cell (captured: the second replay) -> (loss, per-step losses, flat gradient, final state, offsets)"""
    d, v, re, gts = kn.train_case(cell)
    net = golden_net()
    tr = k3.Karman3DTrainer(net, scene(cell)[1], kn.TRAIN_B, kn.TRAIN_MS, STD_V, o.STD_RE, use_graph=use_graph, schedule=schedule)
    for _ in range(2 if use_graph else 1):              # (captured: warm-up, capture and first replay, then the second replay)
        tr._grads.zero_()
        loss = tr.fwd_bwd(d, v[0], v[1], v[2], re, gts)
    torch.cuda.synchronize()
    assert not use_graph or tr._graph is not None
    return float(loss), tr.loss_steps.clone(), tr.grads.clone(), [t.clone() for t in tr.final], net.offsets


@pytest.mark.parametrize("cell", list(TRAIN_CELLS), ids=sid)
def test_trainer_manual_schedule_equals_autograd_composition(cell):
    lm, la = trainer_run(cell, "manual"), trainer_run(cell, "autograd")
    e = (abs(lm[0] - la[0]) / abs(la[0]), rel(lm[1], la[1]), rel(lm[2], la[2]), max(rel(a, b) for a, b in zip(lm[3], la[3])))
    print("trainer at %s, manual against autograd: loss %.2e, per-step losses %.2e, gradient %.2e, final state %.2e" % ((sid(cell),) + e))
    assert np.isfinite(lm[0]) and float(lm[2].abs().max()) > 0
    assert e[0] < BOUNDS["manual_loss"] and e[1] < BOUNDS["manual_steps"] and e[2] < BOUNDS["manual_grad"] and e[3] < BOUNDS["manual_final"], e


@pytest.mark.parametrize("cell", list(TRAIN_CELLS), ids=sid)
def test_trainer_captured_replay_equals_eager_bit_for_bit(cell):
    eager, graph = trainer_run(cell, "manual"), trainer_run(cell, "manual", True)
    assert graph[0] == eager[0] and torch.equal(graph[1], eager[1]), (graph[0], eager[0])
    assert torch.equal(graph[2], eager[2]), rel(graph[2], eager[2])
    assert all(torch.equal(a, b) for a, b in zip(graph[3], eager[3]))


def test_trainer_against_the_float64_oracle_at_16x8x32():
    """loss and the 1.3 M-element gradient of the SOL-2 step at 16 x 8 x 32 (cylinder, B = 2) against autograd through the float64 oracle"""
    cell = kn.ORACLE_CELL
    d, v, re, gts = kn.train_case(cell)
    params = [p.clone().requires_grad_(True) for p in kn.golden_params()]
    loss = o.unrolled_loss(params, d, v, re, gts, scene(cell)[0], STD_V, o.STD_RE)
    loss.backward()
    gref = torch.cat([p.grad.reshape(-1) for p in params])
    hl, _, grads, _, off = trainer_run(cell, "manual")
    per = [rel(grads[off[k]:off[k + 1]], params[k].grad.reshape(-1)) for k in range(24)]
    e = (abs(hl - float(loss.detach())) / abs(float(loss.detach())), rel(grads, gref), max(per))
    print("trainer at %s against the float64 oracle: loss %.2e, gradient %.2e, per tensor max %.2e" % ((sid(cell),) + e))
    assert e[0] < BOUNDS["oracle_loss"] and e[1] < BOUNDS["oracle_grad"] and e[2] < BOUNDS["oracle_param"], (e, per)


@pytest.mark.parametrize("cell", list(TRAIN_CELLS), ids=sid)
def test_rollout_equals_the_training_forward_bit_for_bit(cell):
    """Karman3DRollout (the train=False schedule, three rotating buffers) over two steps: after each, its network output equals the training
    form's (net(x) on the features the step wrote) bit for bit -- a buffer rotated one step too early would show in the second --, and
    the state after two steps is the state the trainer's forward unroll ends in."""
    d, v, re, _ = kn.train_case(cell)
    net = golden_net()
    ro = k3.Karman3DRollout(net, scene(cell)[1], kn.TRAIN_B, STD_V, o.STD_RE)
    st = (f32(d), f32(v[0]), f32(v[1]), f32(v[2]))
    outs = []
    for i in range(2):
        st = ro.step(*st, f32(re))
        with torch.no_grad():
            ref = net(ro.feat.clone())
        assert float(ro.out.abs().max()) > 0 and torch.equal(ro.out, ref), (i, rel(ro.out, ref))
        assert torch.equal(ro.sch.forward(ro.feat)[1][2][-1], net.activations(ro.feat.clone())[-1]), i
        outs.append(ro.out.clone())
    assert not torch.equal(outs[0], outs[1])
    final = trainer_run(cell, "manual")[3]
    e = [rel(a, b) for a, b in zip(st, final)]
    print("roll-out at %s: two steps against the trainer's forward unroll %s (bit-equal: %s)" % (sid(cell), e, [torch.equal(a, b) for a, b in zip(st, final)]))
    assert max(e) < BOUNDS["manual_final"], e


# ---- (d) Z = 128: forward only ------------------------------------------------------------------------------------------------------------------
def test_wide_rows_forward_schedule_against_float64():
    """NetSchedule3D(train=False).forward at (1, 4, 6, 128) and at the roll-out shape (2, 16, 8, 128) against torch float64 (its own LeakyReLU
    masks: the forward is continuous in the pre-activations), and the kernels of the wide-row forms"""
    for shape in (WIDE_CELL, (kn.TRAIN_B,) + kn.Z128_CELL):
        x, _, params = kn.network_case(shape)
        net = k3.MarsMoon3D(device=DEV)
        net.set_weights([p.numpy() for p in params])
        sch = NetSchedule3D(net, *shape, train=False)
        sch.begin_step()
        with _lib.profile() as p:
            out = sch.forward(x.to(DEV))[0]
            torch.cuda.synchronize()
        assert kn.conv_kernels(p) == kn.net_forward_launches(*shape), sorted(p.kernels)
        ref = kn.torch_network(x, None, params, device=DEV)[0]
        e = rel(out, ref)
        print("forward schedule at %s against torch float64: %.2e; kernels %s" % (sid(shape), e, dict(kn.conv_kernels(p))))
        assert e < kn.NET_BOUNDS[WIDE_CELL][0], (e, kn.per_plane(out, ref))


def test_wide_rows_rollout_step_against_the_hand_composition():
    """one Karman3DRollout step at 16 x 8 x 128 (B = 2, cylinder) against the composition by hand: the solver step of a Karman3DFlow, its
    features / std through the float64 torch network, velocity += std * to_staggered(correction).  The network output within the bound of
    the forward (5e-6), the corrected velocities within the field tolerance of the suite (1e-5: they are fields)."""
    cell = kn.Z128_CELL
    B = kn.TRAIN_B
    d, v, re, _ = kn.train_case(cell)
    params = [p.float() for p in kn.golden_params()]
    sc = scene(cell)[1]
    ro = k3.Karman3DRollout(golden_net(), sc, B, STD_V, o.STD_RE)
    got = ro.step(f32(d), f32(v[0]), f32(v[1]), f32(v[2]), f32(re))
    torch.cuda.synchronize()
    with torch.no_grad():
        hd, *hv = k3.Karman3DFlow(sc, B).step(f32(d), f32(v[0]), f32(v[1]), f32(v[2]), f32(re))
        feat = k3.to_feature3d(hv[0], hv[1], hv[2], f32(re)) / torch.tensor(STD_V + (o.STD_RE,), dtype=torch.float32, device=DEV)
        assert rel(ro.feat, feat) < 1e-6, rel(ro.feat, feat)
        out = kn.torch_network(feat.cpu(), None, params, device=DEV)[0]
        corr = k3.to_staggered3d((out * torch.tensor(STD_V, dtype=torch.float64, device=DEV)).float())
        want = [hd] + [a.double() + c.double() for a, c in zip(hv, corr)]
    e_out, e = rel(ro.out, out), [rel(a, b) for a, b in zip(got, want)]
    print("roll-out step at %s: network output %.2e, d / v_y / v_x / v_z %s" % (sid(cell), e_out, e))
    assert float(ro.out.abs().max()) > 0 and e_out < kn.NET_BOUNDS[WIDE_CELL][0] and max(e) < kn.TOL_FIELD, (e_out, e)


# ---- (e) edges of the split arithmetic in the 3-D kernels ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [(2, 5, 10, 64), (2, 5, 6, 32)], ids=sid)
def test_all_zero_input_gives_the_epilogue_of_bias_and_residual_exactly(cell):
    """an all-zero x (absmax slots all zero: the operand scale of the fp16 x 3 split has nothing to scale by) through conv3d gives exactly
    epi(bias + residual) and a finite y_absmax -- both epilogues; a masked or converged simulation sends such tensors"""
    B, D, H, W = cell
    gen = torch.Generator().manual_seed(9)
    r, act, b = randn(gen, B, D, H, W, 32), randn(gen, B, D, H, W, 32), randn(gen, 32)
    packed = k3._pack3d(randn(gen, 5, 5, 5, 32, 32, scale=1 / np.sqrt(125 * 32)), 32, 32, 0)
    x = torch.zeros(B, D, H, W, 32, dtype=torch.float32, device=DEV)
    z, slope = r + b, torch.tensor(SLOPE, dtype=torch.float32, device=DEV)       # (fp32 products, as the epilogues form them)
    for mode, want in (("lrelu", torch.where(z > 0, z, z * slope)), ("dlrelu", torch.where(act > 0, r, r * slope))):
        assert want.dtype == torch.float32
        ymax, y = slots(), nan_like(B, D, H, W, 32)
        with _lib.profile() as p:
            k3.conv3d(x, packed, b if mode == "lrelu" else None, r, 32, mode == "lrelu", SLOPE, slots(), ymax, out=y, act_ref=act if mode == "dlrelu" else None)
            torch.cuda.synchronize()
        assert kn.conv_kernels(p) == kn.conv3d_launches(B, D, H, W), sorted(p.kernels)
        assert not bool(torch.isnan(y).any()), (mode, int(torch.isnan(y).sum()))
        assert torch.equal(y, want), (mode, float((y - want).abs().max()))
        check_absmax(ymax, y, mode)


def test_one_launch_kernel_dynamic_range_not_worse_than_strict_fp32():
    """The claim of test_split_conv_relative_l2_not_worse_than_fp32_mfma for k_conv3d_sb8 and k_pack3_sh, their own implementation of the fp16 x 3
    split, which sums 125 taps: in relative L2 against float64 conv3d, on the whole tensor and on the small half alone (the pixels that see
    only the scaled-down left half of the rows), the one-launch kernel is no worse than the strict-fp32 form of the same call
    (conv_precision = 2: five passes of the fp32-MFMA kernel).  Bound per case: karman3d_net_shapes.SPLIT3D_BOUND (1.0, no allowance)."""
    cases, w = kn.split3d_cases()
    B, D, H, W = kn.SPLIT3D_SHAPE
    w = w.to(DEV)
    packed = k3._pack3d(w, 32, 32, 0)
    bad = []
    for name, x in cases.items():
        x = x.to(DEV)
        ref = kn.conv3d_ref(x.double(), w.double())
        amax = ops.absmax_slots(x)
        with _lib.profile() as p:
            y = k3.conv3d(x, packed, None, None, 32, False, SLOPE, amax, None)
            torch.cuda.synchronize()
        with options(conv_precision=2), _lib.profile() as q:
            yf = k3.conv3d(x, packed, None, None, 32, False, SLOPE, amax, None)
            torch.cuda.synchronize()
        assert kn.conv_kernels(p) == kn.conv3d_launches(B, D, H, W) and kn.conv_kernels(q) == kn.conv3d_launches(B, D, H, W, precision=2), (sorted(p.kernels), sorted(q.kernels))
        ratios = []
        for sl in ((Ellipsis,), (Ellipsis, slice(2, 30), slice(None))):
            ratios.append(rel(y[sl], ref[sl]) / rel(yf[sl], ref[sl]))
        print("one-launch kernel / strict fp32 at %s: whole tensor %.3f, small half %.3f (strict fp32 alone: %.2e / %.2e)"
              % (name, ratios[0], ratios[1], rel(yf, ref), rel(yf[..., 2:30, :], ref[..., 2:30, :])))
        if max(ratios) > kn.SPLIT3D_BOUND[name]:
            bad.append((name, ratios))
    assert not bad, bad


# ---- refusals at construction --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", list(kn.REFUSED), ids=sid)
def test_unsupported_widths_are_refused_at_construction_without_a_launch(grid):
    """NetSchedule3D, Karman3DTrainer and Karman3DRollout at a grid the network does not take raise SolError at construction, naming the
    extent and the rule, before any launch; Z = 128 is refused for training only -- the message says that a roll-out runs there."""
    Y, X, Z, train_only = grid
    words = kn.REFUSED[grid]
    g = kn.geometry((Y, X, Z))
    sc = k3.Scene3D(Y, X, Z, device=DEV, active=g.active, inflow=g.inflow, pressure_solver="cg")
    net = k3.MarsMoon3D(device=DEV)
    torch.cuda.synchronize()
    made = [lambda: NetSchedule3D(net, 2, Y, X, Z, train=True), lambda: k3.Karman3DTrainer(net, sc, 2, 2, STD_V, o.STD_RE),
            lambda: k3.Karman3DTrainer(net, sc, 2, 2, STD_V, o.STD_RE, use_graph=True), lambda: net.schedule(2, Y, X, Z)]
    if not train_only:
        made += [lambda: NetSchedule3D(net, 2, Y, X, Z, train=False), lambda: k3.Karman3DRollout(net, sc, 2, STD_V, o.STD_RE)]
    with _lib.profile() as p:
        for make in made:
            with pytest.raises(_lib.SolError) as e:
                make()
            assert all(w in str(e.value) for w in words), (str(e.value), words)
        torch.cuda.synchronize()
    assert not p.kernels, p.kernels
