"""Float64 reference of the correction network with CIRCULAR padding and of the corrected periodic step built on it (the circular-padding
tests: test_circular_net_cpu.py and test_gpu_circular_net.py).  A plain module: importing it touches no device.

The 5x5 convolution pads by a modulo gather along a periodic axis (any size >= 1, also below the padding) and with zeros along an open
one; model_mars_moon / model_mercury are the oracle's compositions (sol_oracle.mars_moon / mercury) over that convolution.  The physics
and the trainer problem are periodic_cases' (periodic_step, seam_sync, trainer_problem); tolerances are large2d_scenes'."""
import functools
import os
import sys

import torch
import torch.nn.functional as F

import sol_oracle as o

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import periodic_cases as pc
from large2d_scenes import TOL_FIELD, TOL_GRAD, rel  # noqa: F401

ZEROS, CIRCULAR = "zeros", "circular"


def pad2(x, dim, periodic):
    """two cells on either side of `dim`: wrapped copies (index modulo n) when periodic, zeros when open"""
    n = x.shape[dim]
    if periodic:
        return x.index_select(dim, torch.arange(-2, n + 2) % n)
    shape = list(x.shape)
    shape[dim] = 2
    z = x.new_zeros(shape)
    return torch.cat([z, x, z], dim)


def conv(x_nhwc, w_hwio, b, periodic=(False, False)):
    """5x5 convolution of x [B,H,W,cin] with w [5,5,cin,cout] (Keras HWIO: cross-correlation) + b, circular along the periodic axes"""
    xp = pad2(pad2(x_nhwc, 1, periodic[0]), 2, periodic[1]).permute(0, 3, 1, 2)
    return F.conv2d(xp, w_hwio.permute(3, 2, 0, 1), b).permute(0, 2, 3, 1)


def mars_moon(params, x, periodic, slope=0.3):
    act = lambda t: F.leaky_relu(t, slope)
    h = act(conv(x, params[0], params[1], periodic))
    for k in range(5):
        a = act(conv(h, params[2 + 4 * k], params[3 + 4 * k], periodic))
        h = act(h + conv(a, params[4 + 4 * k], params[5 + 4 * k], periodic))
    return conv(h, params[22], params[23], periodic)


def mercury(params, x, periodic):
    h = F.relu(conv(x, params[0], params[1], periodic))
    h = F.relu(conv(h, params[2], params[3], periodic))
    return conv(h, params[4], params[5], periodic)


def network(params, x, periodic):
    """the network the parameter list belongs to (24 tensors: mars_moon, 6: mercury); periodic = (False, False) is zero padding"""
    return (mercury if len(params) == 6 else mars_moon)(params, x, periodic)


def net_params(name, seed=0, last_scale=1.0, bias=0.0):
    """float32-valued float64 parameters of `name`, the last kernel scaled by last_scale, the biases seeded normal x `bias` (non-zero
    biases: a halo or pad cell that is not refreshed would carry them into the next layer's stencil)"""
    ps = [p.float().double() for p in (o.init_params_mercury(seed) if name == "mercury" else o.init_params(seed))]
    ps[-2] = (ps[-2] * last_scale).float().double()
    if bias:
        g = torch.Generator().manual_seed(1000 + seed)
        for k in range(1, len(ps), 2):
            ps[k] = (bias * torch.randn(ps[k].shape, generator=g, dtype=torch.float64)).float().double()
    return ps


# the whole-network cases of the GPU test: (B, H, W), periodic -> seed of the input.  The LeakyReLU / ReLU kinks make the gradient
# discontinuous: a seed is kept when the float32 reference alone holds the tolerances against float64 (the CPU test; never the device code)
NET_CASES = [((2, 32, 16), (False, True)), ((2, 16, 16), (True, True)), ((2, 40, 24), (True, False))]
NET_SEEDS = {}
NET_DEFAULT_SEED = 7


def net_case(name, shape, periodic):
    """(params, x, w_out) of a whole-network case, float32 values in float64"""
    B, H, W = shape
    seed = NET_SEEDS.get((name, shape, periodic), NET_DEFAULT_SEED)
    return net_params(name, 5, bias=0.1), smooth_input(B, H, W, 3, seed), smooth_input(B, H, W, 2, seed + 100)


def net_reference(params, x, w_out, periodic, dtype=torch.float64):
    """out = network(x), and the gradients of <out, w_out> with respect to x and the parameters (flat, Keras order)"""
    ps = [p.detach().to(dtype).requires_grad_(True) for p in params]
    xl = x.detach().to(dtype).requires_grad_(True)
    out = network(ps, xl, periodic)
    (out * w_out.to(dtype)).sum().backward()
    return out.detach().double(), xl.grad.double(), torch.cat([p.grad.reshape(-1) for p in ps]).double()


def smooth_input(B, H, W, c, seed):
    """seeded input of order one with float32 values, [B,H,W,c] float64"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, H, W, c, generator=g, dtype=torch.float64).float().double()


# ---- the corrected step and the trainer problem ---------------------------------------------------------------------------------------
def correction(params, vy, vx, re, periodic, padding):
    """sol_oracle.correction with the network padded circularly along the periodic axes (padding="circular") or with zeros"""
    sv = pc.TRAINER_STD_V
    feat = o.to_feature(vy, vx, re) / torch.tensor([sv[0], sv[1], o.STD_RE], dtype=vy.dtype)
    out = network(params, feat, periodic if padding == CIRCULAR else (False, False)) * torch.tensor([sv[0], sv[1]], dtype=vy.dtype)
    return o.to_staggered(out)


def corrected_step(params, d, vy, vx, re, g, per, padding):
    """solver step, correction (the duplicate plane gets none), seam sync: periodic_cases.corrected_step with the padding chosen"""
    d, vy, vx = pc.periodic_step(d, vy, vx, re, g, per)
    cy, cx = correction(params, vy, vx, re, per, padding)
    vy, vx = pc.seam_sync(vy + cy, vx + cx, per)
    return d, vy, vx


# The last layer of the trainer problem is scaled by this factor (periodic_cases.trainer_problem: 0.01).  A condition, checked by the CPU
# test: at this scale the circular and the zero-padded references differ by more than 100 x tolerance in the loss or the gradient.
LAST_SCALE = 0.01
# scene -> (grid, seed): chosen by the CPU test's float32-against-float64 run of this reference (never by the device code)
PROBLEMS = {"A": (pc.TRAINER_GRID, pc.TRAINER_SEED), "E": ((16, 16), pc.TRAINER_SEED)}


@functools.lru_cache(maxsize=None)
def scene(name, Y, X):
    """(oracle geometry, periodic).  "A": periodic_cases' scene A -- x periodic, empty, the standard velBC and inflow.  "E": doubly
    periodic and empty like periodic_cases' scene E, but WITH the standard velBC and inflow: the trainers take their scene from
    KarmanFlow, whose inflow box is not optional, and refuse masks that describe another one."""
    if name == "A":
        return pc.scene_geometry("A", Y, X), pc.periodic_of("A")
    assert name == "E"
    return pc.geometry(Y, X, pc.scene_active("none", Y, X)), (True, True)


def trainer_problem(name="A"):
    """periodic_cases.trainer_problem's recipe in the scene `name` (for "A" it is that problem): a state spun up by one float64 periodic
    step, ground truth = the roll-out of the perturbed state, mars_moon with the last kernel x LAST_SCALE, msteps = 2"""
    r32 = lambda t: t.detach().float().double()
    (Y, X), seed = PROBLEMS[name]
    g, per = scene(name, Y, X)
    d, vy, vx = o.synthetic_state(pc.B, Y, X, seed, project_it=False)
    re = torch.tensor([o.RE_TRAIN[i % 6] for i in range(pc.B)], dtype=torch.float64)
    with torch.no_grad():
        d, vy, vx = (r32(t) for t in pc.periodic_step(d, vy, vx, re, g, per))
        _, qy, qx = o.synthetic_state(pc.B, Y, X, 4321 + seed, project_it=False)
        gd = d
        gy, gx = pc.seam_sync(r32(vy + 0.05 * (qy - 1.0)), r32(vx + 0.05 * qx), per)
        gts_y, gts_x = [], []
        for _ in range(pc.TRAINER_MS):
            gd, gy, gx = (r32(t) for t in pc.periodic_step(gd, gy, gx, re, g, per))
            gts_y.append(gy)
            gts_x.append(gx)
    return {"g": g, "periodic": per, "d": d, "vy": vy, "vx": vx, "re": re, "gt_vy": gts_y, "gt_vx": gts_x,
            "params": [q.clone().requires_grad_(True) for q in net_params("mars_moon", 0, LAST_SCALE)]}


def trainer_reference(p, padding=CIRCULAR, dtype=torch.float64):
    """(loss, per-step losses, flat weight gradient, final state) of the unrolled loss: periodic_cases.trainer_reference's recipe"""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        params = [q.detach().to(dtype).requires_grad_(True) for q in p["params"]]
        d, vy, vx, re = (p[k].to(dtype) for k in ("d", "vy", "vx", "re"))
        sv = torch.tensor(pc.TRAINER_STD_V, dtype=dtype)
        losses = []
        for gy, gx in zip(p["gt_vy"], p["gt_vx"]):
            d, vy, vx = corrected_step(params, d, vy, vx, re, p["g"], p["periodic"], padding)
            diff = (o.staggered_tensor(gy.to(dtype), gx.to(dtype)) - o.staggered_tensor(vy, vx)) / sv
            losses.append(0.5 * (diff * diff).sum())
        loss = torch.stack(losses).sum() / len(losses)
        loss.backward()
    finally:
        torch.set_default_dtype(prev)
    return (float(loss.detach()), [float(l.detach()) for l in losses], torch.cat([q.grad.reshape(-1) for q in params]).double(),
            tuple(t.detach().double() for t in (d, vy, vx)))


def rollout_reference(p, steps, padding=CIRCULAR, dtype=torch.float64):
    rd, ry, rx, re = (p[k].to(dtype) for k in ("d", "vy", "vx", "re"))
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        with torch.no_grad():
            params = [q.detach().to(dtype) for q in p["params"]]
            for _ in range(steps):
                rd, ry, rx = corrected_step(params, rd, ry, rx, re, p["g"], p["periodic"], padding)
    finally:
        torch.set_default_dtype(prev)
    return rd.double(), ry.double(), rx.double()
