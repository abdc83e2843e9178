"""Float64 reference of the 3-D correction network with CIRCULAR z padding and of the corrected z-periodic step built on it, and the case
tables of test_circular_net3d_cpu.py and test_gpu_circular_net3d.py.  A plain module: importing it touches no device.

The convolution pads z by concatenating the two planes of the other end on either side (F.pad(mode="circular") does not take a single axis
of a 5-D tensor), pads y and x with zeros and runs F.conv3d.  The physics and the trainer problem are periodic3d_cases' (periodic3d_step,
seam_sync, scene_geometry, state); the bounds are karman3d_net_shapes.BOUNDS.  Cells are (B, Y, X, Z)."""
import functools
import os
import sys

import torch
import torch.nn.functional as F

import sol_oracle3d as o

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))       # (karman3d_net_shapes.golden_params imports make_golden)
import periodic3d_cases as pc
from karman3d_net_shapes import BOUNDS, SLOPE, golden_params, lrelu_masked, ncdhw, ndhwc, sid  # noqa: F401
from large2d_scenes import rel  # noqa: F401

ZEROS, CIRCULAR = "zeros", "circular"


# ---- the buffer geometry, restated ------------------------------------------------------------------------------------------------------
def rows(X, Z):
    """HB: Z + 4 rows rounded up to a multiple of the 64 / X image rows that share a tile when X < 64 (check_shape: H % (64 / W) == 0)"""
    q = 64 // X if X < 64 else 1
    return (Z + 4 + q - 1) // q * q


def circular_shape_refused(Y, X, Z, train):
    """the rules of the issue, written as conditions: X takes the pixel rule, Y >= 3, Z >= 2, training X <= 64"""
    ok = Y >= 3 and Z >= 2 and X >= 4 and ((X <= 64 and 64 % X == 0) or X % 64 == 0)
    return not (ok and (X <= 64 or not train))


# (Y, X, Z, train) -> accepted?; refused ones with the words the message must hold
SHAPE_TABLE = {
    (16, 8, 8, True): None, (16, 8, 12, True): None, (24, 16, 24, True): None, (24, 32, 72, True): None, (3, 4, 2, True): None,
    (128, 64, 64, True): None, (4, 128, 6, False): None, (16, 192, 5, False): None,
    (2, 8, 8, True): ("Y = 2", "Y >= 3"), (16, 8, 1, True): ("Z = 1", "Z >= 2"),
    (24, 12, 12, True): ("X = 12", "pixel axis"), (24, 10, 16, False): ("X = 10", "multiple of 64"), (16, 2, 8, True): ("X = 2", "4, 8, 16, 32 or 64"),
    (16, 96, 8, False): ("X = 96", "multiple of 64"), (4, 128, 6, True): ("X = 128", "X <= 64", "roll-out"),
}

# ---- case tables -----------------------------------------------------------------------------------------------------------------------------
ENTRY_CELLS = [(1, 3, 4, 6), (2, 5, 16, 12), (2, 5, 64, 10), (1, 4, 128, 6)]        # pack / unpack / halo: HB = 16 with six pad rows first
LAYER_CELLS = [(1, 3, 4, 6), (2, 5, 16, 12), (2, 5, 64, 10)]                        # X = 4, 16, 64
LAYER_CHANNELS = [(4, 32), (32, 32), (32, 3)]
NET_CELLS = {
    (1, 3, 4, 6): "16 rows per tile, D = 3, HB = 16 > Z + 4",
    (2, 5, 8, 12): "a Z the zero-padded network refuses",
    (2, 5, 64, 10): "the one-launch k_conv3d_sb8; 70 rows per sample are ragged: thin weight gradients on k_conv5x5_bww_sb<0>",
    (1, 3, 64, 4): "HB = 8, 24 rows: thin weight gradients on k_conv5x5_bww_sb<2>",
}
WIDE_CELL = (1, 4, 128, 6)          # forward only (train=False) at X = 128
ACC_CELL = (2, 5, 64, 10)
EQUIV_CELLS = [(1, 6, 8, 8), (2, 5, 16, 16)]
ROLLS = lambda Z: (1, 3, Z - 1)
TRAIN_CELLS = [(16, 8, 8), (16, 8, 12)]         # (Y, X, Z); the second is a grid the zero-padded network refuses
# seed per case: a case whose float32 reference alone does not stay within a quarter of the bound gets another seed here, with the reason
NET_SEEDS = {}
NET_DEFAULT_SEED = 21


# ---- one layer ----------------------------------------------------------------------------------------------------------------------------------
def wrap_z(x_ncdhw):
    return torch.cat([x_ncdhw[..., -2:], x_ncdhw, x_ncdhw[..., :2]], dim=-1)


def conv(x, w, b=None, padding=CIRCULAR, blocked=False):
    """x [B,Y,X,Z,ci], w [5,5,5,ci,co] (Keras k_y, k_x, k_z, in, out) -> [B,Y,X,Z,co]: circular along z, zeros along y and x.
    blocked: the same sum taken as 25 partial convolutions, one per (k_y, k_x) tap, added up -- 5 ci terms per partial sum instead of
    125 ci in one run.  The value is the same; in float32 the rounding is that of a blocked accumulation (as the device's MFMA tiles and
    five-pass forms accumulate) instead of torch's one sequential run over 4000 terms."""
    xt, wt = ncdhw(x), w.permute(4, 3, 0, 1, 2)
    xt = wrap_z(xt) if padding == CIRCULAR else F.pad(xt, (2, 2))
    if not blocked:
        return ndhwc(F.conv3d(xt, wt, b, padding=(2, 2, 0)))
    Y, X = xt.shape[2], xt.shape[3]
    xp = F.pad(xt, (0, 0, 2, 2, 2, 2))
    out = 0.0
    for ky in range(5):
        for kx in range(5):
            out = out + F.conv3d(xp[:, :, ky:ky + Y, kx:kx + X], wt[:, :, ky:ky + 1, kx:kx + 1])
    return ndhwc(out if b is None else out + b.view(1, -1, 1, 1, 1))


def layer_case(cell, chan, seed=11):
    """(x, w, b, gy) of a one-layer test, float32 values in float64"""
    B, Y, X, Z = cell
    cin, cout = chan
    g = torch.Generator().manual_seed(seed + X + cin)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return tuple(t.float().double() for t in (r(B, Y, X, Z, cin), r(5, 5, 5, cin, cout) / (11.2 * cin ** 0.5), 0.1 * r(cout), r(B, Y, X, Z, cout)))


def layer_reference(x, w, b, gy, dtype=torch.float64, padding=CIRCULAR, blocked=False):
    leaves = [t.detach().to(dtype).requires_grad_(True) for t in (x, w, b)]
    y = conv(*leaves, padding=padding, blocked=blocked)
    y.backward(gy.to(dtype))
    return [y.detach().double()] + [t.grad.double() for t in leaves]


# ---- the network --------------------------------------------------------------------------------------------------------------------------------
def network_case(cell):
    """(x, gy, params): fp32 values; the golden network's parameters (small non-zero biases: a halo row that is not refreshed would carry
    them into the next layer's stencil), the upstream gradient on another scale"""
    B, Y, X, Z = cell
    gen = torch.Generator().manual_seed(NET_SEEDS.get(tuple(cell), NET_DEFAULT_SEED))
    x = torch.randn(B, Y, X, Z, 4, generator=gen, dtype=torch.float32)
    gy = torch.randn(B, Y, X, Z, 3, generator=gen, dtype=torch.float32) * 1e-3
    return x, gy, [p.float() for p in golden_params()]


def torch_network(x, gy, params, masks=None, dtype=torch.float64, device="cpu", padding=CIRCULAR, blocked=False):
    """karman3d_net_shapes.torch_network with the padding chosen: -> (out, dx, the 24 parameter gradients, its own sign masks, how many
    signs differ from the masks applied); gy = None: forward only"""
    tp = [p.to(device=device, dtype=dtype).requires_grad_(gy is not None) for p in params]
    cv = lambda t, k: conv(t, tp[2 * k], tp[2 * k + 1], padding, blocked)
    xt = x.to(device=device, dtype=dtype).clone().requires_grad_(gy is not None)
    own, flips = [], 0

    def act(z):
        nonlocal flips
        m = (z > 0) if masks is None else masks[len(own)].to(device)
        flips += int(((z > 0) != m).sum())
        own.append((z > 0).detach())
        return lrelu_masked(z, m)

    with torch.set_grad_enabled(gy is not None):
        h = act(cv(xt, 0))
        for k in range(5):
            a = act(cv(h, 1 + 2 * k))
            h = act(cv(a, 2 + 2 * k) + h)
        out = cv(h, 11)
        if gy is None:
            return out, None, None, own, flips
        (out * gy.to(device=device, dtype=dtype)).sum().backward()
    return out.detach(), xt.grad, [p.grad for p in tp], own, flips


def mars_moon3d(params, x, padding=CIRCULAR):
    """sol_oracle3d.mars_moon3d over the convolution above (differentiable, no masks)"""
    act = lambda t: F.leaky_relu(t, SLOPE)
    h = act(conv(x, params[0], params[1], padding))
    for k in range(5):
        a = act(conv(h, params[2 + 4 * k], params[3 + 4 * k], padding))
        h = act(h + conv(a, params[4 + 4 * k], params[5 + 4 * k], padding))
    return conv(h, params[22], params[23], padding)


def equivariance_case(cell):
    """(params, x) of the roll test: the measurement of the issue -- sol_oracle3d.init_params(0) plus small biases, a random input"""
    B, Y, X, Z = cell
    g = torch.Generator().manual_seed(3)
    ps = [p.float().double() for p in o.init_params(0)]
    for k in range(1, 24, 2):
        ps[k] = (0.05 * torch.randn(ps[k].shape, generator=g, dtype=torch.float64)).float().double()
    return ps, torch.randn(B, Y, X, Z, 4, generator=g, dtype=torch.float64).float().double()


# ---- the corrected step and the trainer problem -------------------------------------------------------------------------------------------
def correction(params, v, re, padding, std_v=pc.TRAINER_STD_V):
    """sol_oracle3d.correction with the network's padding chosen"""
    feat = o.to_feature(v, re) / torch.tensor(list(std_v) + [o.STD_RE], dtype=v[0].dtype)
    return o.to_staggered(mars_moon3d(params, feat, padding) * torch.tensor(list(std_v), dtype=v[0].dtype))


def corrected_step(params, d, v, re, g, padding):
    d, v = pc.periodic3d_step(d, v, re, g, True)
    return d, pc.seam_sync(tuple(a + c for a, c in zip(v, correction(params, v, re, padding))), True)


# The last layer of the trainer problem is scaled by this factor (periodic3d_cases.trainer_problem: 0.01).  A condition, checked by the CPU
# test: at this scale the circular and the zero-padded float64 references differ by more than 100 x the loss or the gradient bound.
LAST_SCALE = 0.01
TRAINER_SEEDS = {}


@functools.lru_cache(maxsize=None)
def trainer_problem(cell):
    """periodic3d_cases.trainer_problem at `cell` (the periodic cylinder, B = 2, SOL-2) with the last kernel x LAST_SCALE"""
    p = pc.trainer_problem(tuple(cell), pc.TRAINER_MS, TRAINER_SEEDS.get(tuple(cell), pc.SEED))
    ps = [q.float().double() for q in o.init_params(0)]
    ps[-2] = (ps[-2] * LAST_SCALE).float().double()
    p["params"] = ps
    return p


def trainer_reference(p, padding=CIRCULAR, dtype=torch.float64):
    """(loss, per-step losses, flat weight gradient, final state): periodic3d_cases.trainer_reference's recipe, the correction replaced"""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        params = [q.detach().to(dtype).requires_grad_(True) for q in p["params"]]
        d, re = p["d"].to(dtype), p["re"].to(dtype)
        v = tuple(t.to(dtype) for t in p["v"])
        sv = torch.tensor(pc.TRAINER_STD_V, dtype=dtype)
        losses = []
        for gt in p["gts"]:
            d, v = corrected_step(params, d, v, re, p["g"], padding)
            losses.append(sum(0.5 * (((gt[c].to(dtype) - v[c]) / sv[c]) ** 2).sum() for c in range(3)))
        loss = torch.stack(losses).sum() / len(losses)
        loss.backward()
    finally:
        torch.set_default_dtype(prev)
    return (float(loss.detach()), [float(l.detach()) for l in losses], torch.cat([q.grad.reshape(-1) for q in params]).double(),
            (d.detach().double(),) + tuple(t.detach().double() for t in v))


def rollout_reference(p, steps, padding=CIRCULAR, dtype=torch.float64):
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        with torch.no_grad():
            params = [q.detach().to(dtype) for q in p["params"]]
            d, re = p["d"].to(dtype), p["re"].to(dtype)
            v = tuple(t.to(dtype) for t in p["v"])
            for _ in range(steps):
                d, v = corrected_step(params, d, v, re, p["g"], padding)
    finally:
        torch.set_default_dtype(prev)
    return (d.double(),) + tuple(t.double() for t in v)
