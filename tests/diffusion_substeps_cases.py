"""Float64 reference, inputs and cached reference results of the karman-2d diffusion-substep tests (test_gpu_karman2d_diffusion_substeps.py
and its CPU twin test_karman2d_diffusion_substeps_cpu.py).  A plain module: importing it touches no device.

The reference needs nothing new in the oracle.  With a = dt res^2 / (n re) per simulation,
    repeat n - 1 times:  vy += a * o.laplace_replicate(vy);  vx += a * o.laplace_replicate(vx)
    o.karman_step(d, vy, vx, re * n, g, ...)          (buoyancy_cases.buoyant_step for the buoyant case)
i.e. n explicit substeps of alpha / n and the boundary blend once, after the last one.  Gradients are torch autograd through that, in
float64, re.grad included.

The Reynolds numbers are chosen so that the single stencil is UNSTABLE (alpha = dt res^2 / re between 0.42 and 0.85, distinct per
simulation: re = res^2 / alpha rounded to fp32): a surface that ignores the parameter computes something else entirely.  The scenes,
cotangents and metrics are the buoyancy suite's (buoyancy_cases.SCENES, large2d_scenes); the state seeds are SEED for one step and
CHAIN_SEED for two chained steps, chosen like that suite's: test_karman2d_diffusion_substeps_cpu.py measures the reference in float32
against float64 on every case the GPU tests use and pins the figures (its docstring lists them)."""
import functools
import os
import sys

import numpy as np
import torch

import sol_oracle as o

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buoyancy_cases as bc
from density_adjoint_cases import w_dens
from large2d_scenes import cotangent_at, state, table_geometry

ALPHAS = (0.85, 0.6, 0.42)            # dt res^2 / re of simulation 0, 1, 2: all beyond the single stencil's bound 1/4
SEED = 11
CHAIN_SEED = 13
B = bc.B                              # the step cases (the buoyancy suite's scenes)
FORCE = bc.FORCES[1]                  # the buoyant case: (0.3, -0.2)
# the pre-diffusion alone: (Y, X) and the n of diffusion_substeps; B = 3
PRE_SHAPES = ((16, 16), (40, 24), (130, 65))
PRE_N = (2, 3, 9, 12)                 # 1 pre-substep, one chunk, exactly S_MAX = 8, two chunks
PRE_B = 3
STEP_N = (2, 5)
SMALL = ((64, 32), (32, 16))          # one-workgroup grids (ops.karman_step), n = 3
SMALL_N = 3
STABILITY = dict(Y=32, X=16, alpha=0.85, steps=40, n=4)


def re_of(res, batch):
    """[batch] float64 holding fp32 values: re_b = res^2 / ALPHAS[b]"""
    return torch.tensor([float(np.float32(res * res / ALPHAS[b % len(ALPHAS)])) for b in range(batch)], dtype=torch.float64)


def pre_diffuse(vy, vx, re, res, n, dt=1.0):
    """M^(n-1) (vy, vx), M = I + (dt res^2 / (n re)) L"""
    a = (dt * res * res / (n * re)).reshape(-1, 1, 1)
    for _ in range(n - 1):
        vy = vy + a * o.laplace_replicate(vy)
        vx = vx + a * o.laplace_replicate(vx)
    return vy, vx


def sub_step(d, vy, vx, re, g, n, force=None, inflow_order="after", dt=1.0):
    """one step with n diffusion substeps (force: the buoyant step)"""
    vy, vx = pre_diffuse(vy, vx, re, g.X, n, dt)
    if force is None:
        return o.karman_step(d, vy, vx, re * n, g, dt=dt, inflow_order=inflow_order)
    return bc.buoyant_step(d, vy, vx, re * n, g, force, dt=dt, inflow_order=inflow_order)


def pre_inputs(Y, X, seed=7, dtype=torch.float64):
    """seeded normal (vy, vx) [PRE_B, ...] of magnitude ~1 (every mode of the stencil is present) and re: fp32 values"""
    gen = torch.Generator().manual_seed(seed)
    vy = torch.randn(PRE_B, Y + 1, X, generator=gen, dtype=torch.float64).float()
    vx = torch.randn(PRE_B, Y, X + 1, generator=gen, dtype=torch.float64).float()
    return vy.to(dtype), vx.to(dtype), re_of(X, PRE_B).to(dtype)


@functools.lru_cache(maxsize=None)
def pre_reference(Y, X, n, seed=7, dtype=torch.float64):
    vy, vx, re = pre_inputs(Y, X, seed, dtype)
    return tuple(t.double() for t in pre_diffuse(vy, vx, re, X, n))


def start_state(name, dtype=torch.float64, steps=1):
    """(d, vy, vx, re) of a buoyancy_cases scene: large2d_scenes.state spun up in the scene, with this module's Reynolds numbers"""
    Y, X = bc.SCENES[name][:2]
    d, vy, vx, _ = state(B, Y, X, SEED if steps == 1 else CHAIN_SEED, bc.geometry_of(name))
    return d.to(dtype), vy.to(dtype), vx.to(dtype), re_of(X, B).to(dtype)


def small_state(Y, X, dtype=torch.float64):
    g = o.KarmanGeometry(Y, X)
    d, vy, vx, _ = state(B, Y, X, SEED, g)
    return g, (d.to(dtype), vy.to(dtype), vx.to(dtype), re_of(X, B).to(dtype))


def small_cotangents(Y, X, dtype=torch.float64):
    wy, wx = cotangent_at(B, Y, X)
    return wy.to(dtype), wx.to(dtype)


def needs_trim(kind, steps):
    """True where the GPU tests (and the float32 pin) apply the trimmed gradient metric: a velocity cotangent through one step's advection
    adjoint from SEED (as in the buoyancy suite)"""
    return steps == 1 and kind != "dens"


def _loss(out, wd, wy, wx):
    loss = 0.0
    if wd is not None:
        loss = loss + (out[0] * wd).sum()
    if wy is not None:
        loss = loss + (out[1] * wy).sum() + (out[2] * wx).sum()
    return loss


@functools.lru_cache(maxsize=None)
def reference(name, n, kind="vel", steps=1, re_grad=False, force=None, dtype=torch.float64):
    """The reference's autograd through `steps` chained steps with n substeps -> ((d, vy, vx) after the last step, (g_d, g_vy, g_vx[, g_re])
    with respect to the initial state), float64 tensors.  kind: "vel" | "dens" | "both" (buoyancy_cases.cotangents).  Cached, shared,
    never modified."""
    g, order = bc.geometry_of(name), bc.SCENES[name][3]
    d, vy, vx, re = start_state(name, dtype, steps)
    leaves = [t.clone().requires_grad_(True) for t in ((d, vy, vx, re) if re_grad else (d, vy, vx))]
    cd, cy, cx = leaves[:3]
    r = leaves[3] if re_grad else re
    for _ in range(steps):
        cd, cy, cx = sub_step(cd, cy, cx, r, g, n, force, order)
    _loss((cd, cy, cx), *bc.cotangents(name, kind, dtype)).backward()
    zero = lambda t, like: torch.zeros_like(like) if t is None else t
    return (tuple(t.detach().double() for t in (cd, cy, cx)), tuple(zero(p.grad, p).double() for p in leaves))


@functools.lru_cache(maxsize=None)
def small_reference(Y, X, n, re_grad=False, dtype=torch.float64):
    """one step on a one-workgroup grid, velocity cotangent -> ((d, vy, vx), (g_vy, g_vx[, g_re]))"""
    g, (d, vy, vx, re) = small_state(Y, X, dtype)
    leaves = [t.clone().requires_grad_(True) for t in ((vy, vx, re) if re_grad else (vy, vx))]
    out = sub_step(d, leaves[0], leaves[1], leaves[2] if re_grad else re, g, n)
    wy, wx = small_cotangents(Y, X, dtype)
    ((out[1] * wy).sum() + (out[2] * wx).sum()).backward()
    return tuple(t.detach().double() for t in out), tuple(p.grad.double() for p in leaves)


def stability_run(n, dtype=torch.float64, Y=None, X=None):
    """max|v| before and after STABILITY['steps'] steps without a network at alpha = STABILITY['alpha'] -> (initial, final)"""
    Y, X = STABILITY["Y"] if Y is None else Y, STABILITY["X"] if X is None else X
    g = o.KarmanGeometry(Y, X)
    d, vy, vx, _ = state(1, Y, X, SEED, g)
    d, vy, vx = d.to(dtype), vy.to(dtype), vx.to(dtype)
    re = torch.tensor([float(np.float32(X * X / STABILITY["alpha"]))], dtype=dtype)
    first = max(float(vy.abs().max()), float(vx.abs().max()))
    with torch.no_grad():
        for _ in range(STABILITY["steps"]):
            d, vy, vx = sub_step(d, vy, vx, re, g, n)
            if not bool(torch.isfinite(vy).all()):
                return first, float("inf")
    return first, max(float(vy.abs().max()), float(vx.abs().max()))


# ---- the LargeGridTrainer / LargeGridRollout problem: the smallest grid the trainer accepts (any_width=True), B = 1 ---------------------
TRAINER_GRID, TRAINER_STD_V, TRAINER_N, TRAINER_ALPHA = (144, 72), (0.2, 0.2), 4, 0.85


def unrolled_loss(params, d0, vy0, vx0, re, gt_vy, gt_vx, g, std_v, std_re, n):
    """o.unrolled_loss with n diffusion substeps: (loss, per-step losses, (d, vy, vx) after the last corrected step)"""
    d, vy, vx = d0, vy0, vx0
    losses = []
    sv = torch.tensor([std_v[0], std_v[1]], dtype=vy0.dtype)
    for i in range(len(gt_vy)):
        d, vy, vx = sub_step(d, vy, vx, re, g, n)
        cy, cx = o.correction(params, vy, vx, re, std_v, std_re)
        vy, vx = vy + cy, vx + cx
        diff = (o.staggered_tensor(gt_vy[i], gt_vx[i]) - o.staggered_tensor(vy, vx)) / sv
        losses.append(0.5 * (diff * diff).sum())
    return torch.stack(losses).sum() / len(gt_vy), losses, (d, vy, vx)


def trainer_problem(ms=2, seed=SEED, dtype=torch.float64):
    """buoyancy_cases.trainer_problem's recipe at TRAINER_GRID with the substep step and re = res^2 / TRAINER_ALPHA"""
    Y, X = TRAINER_GRID
    r32 = lambda t: t.detach().float().double()
    g = table_geometry("default", Y, X)
    d, vy, vx, _ = state(1, Y, X, seed, g)
    re = torch.tensor([float(np.float32(X * X / TRAINER_ALPHA))], dtype=torch.float64)
    with torch.no_grad():
        _, py, px = o.synthetic_state(1, Y, X, 4321 + seed, project_it=False)
        gd, gy, gx = d, r32(vy + 0.05 * (py - 1.0)), r32(vx + 0.05 * px)
        gts_y, gts_x = [], []
        for _ in range(ms):
            gd, gy, gx = (r32(t) for t in sub_step(gd, gy, gx, re, g, TRAINER_N))
            gts_y.append(gy)
            gts_x.append(gx)
    params = [r32(p) for p in o.init_params(0)]
    params[-2] = r32(params[-2] * 0.01)
    cast = lambda t: t.to(dtype)
    return {"g": g, "d": cast(d), "vy": cast(vy), "vx": cast(vx), "re": cast(re), "gt_vy": [cast(t) for t in gts_y],
            "gt_vx": [cast(t) for t in gts_x], "params": [cast(p).requires_grad_(True) for p in params]}


def trainer_reference(p, n, dtype=torch.float64):
    """(loss, per-step losses, flat weight gradient, final state) of unrolled_loss on a trainer_problem with n substeps, in `dtype`"""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        for q in p["params"]:
            q.grad = None
        loss, losses, fin = unrolled_loss(p["params"], p["d"], p["vy"], p["vx"], p["re"], p["gt_vy"], p["gt_vx"], p["g"], TRAINER_STD_V,
                                          o.STD_RE, n)
        loss.backward()
    finally:
        torch.set_default_dtype(prev)
    return (float(loss.detach()), [float(l.detach()) for l in losses], torch.cat([q.grad.reshape(-1) for q in p["params"]]).double(),
            tuple(t.detach().double() for t in fin))


def rollout_reference(p, n, steps, dtype=torch.float64):
    """`steps` steps of solver step (n substeps) + correction from a trainer_problem's start -> (d, vy, vx)"""
    rd, ry, rx, re = (p[k].to(dtype) for k in ("d", "vy", "vx", "re"))
    with torch.no_grad():
        params = [q.detach().to(dtype) for q in p["params"]]
        for _ in range(steps):
            rd, ry, rx = sub_step(rd, ry, rx, re, p["g"], n)
            cy, cx = o.correction(params, ry, rx, re, TRAINER_STD_V, o.STD_RE)
            ry, rx = ry + cy, rx + cx
    return rd.double(), ry.double(), rx.double()
