"""Float64 reference, inputs and cached reference results of the karman-2d MacCormack advection tests (test_gpu_karman2d_maccormack.py and
its CPU twin test_karman2d_maccormack_cpu.py).  A plain module: importing it touches no device.

The reference step is o.diffuse_bc -> the definition of include/sol_hip.h ("MACCORMACK ADVECTION on the large-grid step"), written with
the oracle's own o._points / o._local / o._sample and a twin of o._sample that also returns the min / max of the four values it read ->
(the buoyancy term of buoyancy_cases) -> o.project; the pre-diffusion of diffusion_substeps_cases in front for n substeps.  With c the
post-diffusion velocity, f one advected array, u = c at the array's sample points, S_g the bilinear sample of g in the array's mode:
    h = S_f(x - u dt),  b = S_h(x + u dt),  cor = h + (s / 2)(f - b),  out = cor where lo <= cor <= hi else h
Gradients are float64 autograd; torch.where freezes the limiter's decision, floor and clamp freeze themselves.

Scenes, seeds, cotangents and metrics are the buoyancy suite's (buoyancy_cases.SCENES at B = 2, seed 11 for one step and 13 for two
chained steps, large2d_scenes.cotangent_at, density_adjoint_cases.w_dens, TOL_FIELD, TOL_GRAD, trimmed_rel with the cap TRIM).  The
limiter and the clamped edges tie exactly in places and fp32 decides a few entries the other way, so EVERY MacCormack gradient comparison
uses the trimmed metric with the cap as a condition (k <= int(TRIM n)); test_karman2d_maccormack_cpu.py measures the reference in float32
against float64 on every case the GPU tests use and pins the figures (its docstring lists them)."""
import functools
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

import sol_oracle as o

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buoyancy_cases as bc
import diffusion_substeps_cases as ds
from large2d_scenes import cfl_scaled, state, table_geometry

B = bc.B
SEED, CHAIN_SEED = bc.SEED, bc.CHAIN_SEED
FORCE = bc.FORCES[1]                  # the buoyant composition: (0.3, -0.2)
NSUB = 2                              # the diffusion-substep composition
STAGE_SHAPES = ((16, 16), (40, 24), (130, 65))      # the stage alone: one tile, ragged tiles, several tiles
STAGE_B = 3
STRENGTHS = (1.0, 0.5)
BLOB = dict(Y=64, X=64, sigma=3.0, u=(0.37, 0.21), start=(14.0, 20.0), steps=100)


def sample_minmax(fld, ly, lx, mode):
    """o._sample(fld, ly, lx, mode) for mode "replicate" / "zero", and the min and max of the four values it read (after clamping; the
    zeros of the ghost ring count)"""
    Bn, H, W = fld.shape
    if mode == "zero":
        fld = F.pad(fld, (1, 1, 1, 1))
        ly, lx, H, W = ly + 1.0, lx + 1.0, H + 2, W + 2
    elif mode != "replicate":
        raise ValueError(mode)
    fy, fx = torch.floor(ly), torch.floor(lx)
    wy, wx = ly - fy, lx - fx
    y0, x0 = fy.long(), fx.long()
    y1, x1 = (y0 + 1).clamp(0, H - 1), (x0 + 1).clamp(0, W - 1)
    y0, x0 = y0.clamp(0, H - 1), x0.clamp(0, W - 1)
    flat = fld.reshape(Bn, -1)
    g = lambda yy, xx: torch.gather(flat, 1, (yy * W + xx).reshape(Bn, -1)).reshape(ly.shape)
    f00, f01, f10, f11 = g(y0, x0), g(y0, x1), g(y1, x0), g(y1, x1)
    val = (1 - wy) * ((1 - wx) * f00 + wx * f01) + wy * ((1 - wx) * f10 + wx * f11)
    four = torch.stack([f00, f01, f10, f11])
    return val, four.min(dim=0).values, four.max(dim=0).values


def advect(d, cy, cx, dt, dx, s=1.0, scheme="mac_cormack", stats=None):
    """(d, c_y, c_x) advected by c: the definition above for scheme "mac_cormack", o.advect_mac's values for "semi_lagrangian".  d may be
    None.  stats (a list): receives the share of entries the limiter reverted, per array."""
    Bn, Yp1, X = cy.shape
    Y = Yp1 - 1
    out = []
    for kind, f, mode in (("c", d, "zero"), ("y", cy, "replicate"), ("x", cx, "replicate")):
        if f is None:
            out.append(None)
            continue
        py, px = (t.unsqueeze(0).expand(Bn, -1, -1) for t in o._points(kind, Y, X, dx, cy))
        uy = o._sample(cy, *o._local("y", py, px, dx), "replicate")
        ux = o._sample(cx, *o._local("x", py, px, dx), "replicate")
        h, lo, hi = sample_minmax(f, *o._local(kind, py - uy * dt, px - ux * dt, dx), mode)
        if scheme == "semi_lagrangian":
            out.append(h)
            continue
        b = o._sample(h, *o._local(kind, py + uy * dt, px + ux * dt, dx), mode)
        cor = h + (0.5 * s) * (f - b)
        keep = (lo <= cor) & (cor <= hi)
        if stats is not None:
            stats.append(1.0 - float(keep.double().mean()))
        out.append(torch.where(keep, cor, h))
    return tuple(out)


def stage(d, cy, cx, g, s=1.0, scheme="mac_cormack", inflow_order="after", dt=1.0, stats=None):
    """the stage as sol_karman_advect runs it: inflow before / after, velocity times the hard-BC face masks"""
    infl = o._t(g.inflow, cy)
    d2, ay, ax = advect(d + infl if inflow_order == "before" else d, cy, cx, dt, g.dx, s, scheme, stats)
    if inflow_order == "after":
        d2 = d2 + infl * dt
    return d2, ay * o._t(g.my, cy), ax * o._t(g.mx, cy)


def step(d, vy, vx, re, g, s=1.0, scheme="mac_cormack", force=None, n=1, inflow_order="after", dt=1.0, stats=None):
    """one solver step with the chosen advection (force: the buoyancy term of buoyancy_cases; n: diffusion substeps)"""
    if n > 1:
        vy, vx = ds.pre_diffuse(vy, vx, re, g.X, n, dt)
        re = re * n
    cy, cx = o.diffuse_bc(vy, vx, re, g.X, dt, g)
    infl = o._t(g.inflow, vy)
    d2, ay, ax = advect(d + infl if inflow_order == "before" else d, cy, cx, dt, g.dx, s, scheme, stats)
    if inflow_order == "after":
        d2 = d2 + infl * dt
    if force is not None:
        dz = F.pad(d2, (1, 1, 1, 1))
        ay = ay + (dt * force[0]) * (0.5 * (dz[:, :-1, 1:-1] + dz[:, 1:, 1:-1]))
        ax = ax + (dt * force[1]) * (0.5 * (dz[:, 1:-1, :-1] + dz[:, 1:-1, 1:]))
    py, px = o.project(ay, ax, g)
    return d2, py, px


def start_state(name, dtype=torch.float64, steps=1, cfl=None):
    """the buoyancy suite's state of the scene (its Reynolds numbers too, with or without diffusion substeps: the substep suite's unstable
    ones leave a checkerboard in the velocity on which the limiter ties everywhere, and the reference in float32 then misses its own
    float64 by 7e-5 in the fields); cfl: its velocity scaled to that CFL number"""
    Y, X = bc.SCENES[name][:2]
    g = bc.geometry_of(name)
    st = state(B, Y, X, SEED if steps == 1 else CHAIN_SEED, g)
    if cfl is not None:
        st = cfl_scaled(st, g, cfl)[0]
    return tuple(t.to(dtype) for t in st)


@functools.lru_cache(maxsize=None)
def reference(name, s=1.0, kind="both", steps=1, force=None, n=1, re_grad=False, cfl=None, dtype=torch.float64):
    """The reference's autograd through `steps` chained MacCormack steps -> ((d, vy, vx) after the last step, (g_d, g_vy, g_vx[, g_re])
    with respect to the initial state, the limiter's reverted shares), float64 tensors.  Cached: computed once, shared, never modified."""
    g = bc.geometry_of(name)
    order = bc.SCENES[name][3]
    d, vy, vx, re = start_state(name, dtype, steps, cfl)
    leaves = [t.clone().requires_grad_(True) for t in ((d, vy, vx, re) if re_grad else (d, vy, vx))]
    cd, cy, cx = leaves[:3]
    r = leaves[3] if re_grad else re
    stats = []
    for _ in range(steps):
        cd, cy, cx = step(cd, cy, cx, r, g, s, force=force, n=n, inflow_order=order, stats=stats)
    wd, wy, wx = bc.cotangents(name, kind, dtype)
    loss = 0.0
    if wd is not None:
        loss = loss + (cd * wd).sum()
    if wy is not None:
        loss = loss + (cy * wy).sum() + (cx * wx).sum()
    loss.backward()
    zero = lambda t, like: torch.zeros_like(like) if t is None else t
    return (tuple(t.detach().double() for t in (cd, cy, cx)), tuple(zero(p.grad, p).double() for p in leaves), tuple(stats))


# ---- the stage alone: seeded normal fields ----
@functools.lru_cache(maxsize=None)
def stage_geometry(Y, X):
    """what the stage reads of a scene, for any Y x X (o.KarmanGeometry takes Y = 2 X only): dx, a block obstacle, an inflow patch and the
    hard-BC face masks of the obstacle (a face is open iff both cells it separates are accessible; outside the domain counts as accessible)"""
    active = np.ones((Y, X))
    active[Y // 3:Y // 3 + max(2, Y // 8), X // 4:X // 4 + max(2, X // 6)] = 0.0
    inflow = np.zeros((Y, X))
    inflow[1:max(3, Y // 10), X // 4:3 * X // 4] = 1.0
    acc = np.pad(active, 1, mode="edge")
    return types.SimpleNamespace(Y=Y, X=X, dx=100.0 / X, active=active, inflow=inflow,
                                 my=np.minimum(acc[0:Y + 1, 1:X + 1], acc[1:Y + 2, 1:X + 1]), mx=np.minimum(acc[1:Y + 1, 0:X + 1], acc[1:Y + 1, 1:X + 2]))


def stage_inputs(Y, X, cfl=None, seed=23, dtype=torch.float64):
    """seeded normal (d, c_y, c_x) [STAGE_B, ...] and cotangents (g_d, g_ay, g_ax): fp32 values.  The velocity has magnitude ~1 cell per
    step (CFL up to ~4 at the tails); cfl: multiplied so that max |c| dt/dx is that number"""
    gen = torch.Generator().manual_seed(seed)
    shapes = ((STAGE_B, Y, X), (STAGE_B, Y + 1, X), (STAGE_B, Y, X + 1))
    d, cy, cx, gd, gy, gx = (torch.randn(*sh, generator=gen, dtype=torch.float64) for sh in shapes + shapes)
    dx = stage_geometry(Y, X).dx
    scale = dx if cfl is None else cfl * dx / max(float(cy.abs().max()), float(cx.abs().max()))
    return tuple(t.float().to(dtype) for t in (d, cy * scale, cx * scale, gd, gy, gx))


@functools.lru_cache(maxsize=None)
def stage_reference(Y, X, s=1.0, inflow_order="after", cfl=None, scheme="mac_cormack", dtype=torch.float64):
    """((d_out, a_y, a_x), (g_d, g_cy, g_cx), reverted shares) of the stage on stage_inputs, float64 tensors; cached"""
    g = stage_geometry(Y, X)
    d, cy, cx, gd, gy, gx = stage_inputs(Y, X, cfl, dtype=dtype)
    leaves = [t.clone().requires_grad_(True) for t in (d, cy, cx)]
    stats = []
    out = stage(*leaves, g, s, scheme, inflow_order, stats=stats)
    ((out[0] * gd).sum() + (out[1] * gy).sum() + (out[2] * gx).sum()).backward()
    return tuple(t.detach().double() for t in out), tuple(p.grad.double() for p in leaves), tuple(stats)


# ---- the blob experiment: what the scheme is for ----
def blob_inputs(dtype=torch.float64):
    """a Gaussian density blob in a uniform flow on an obstacle-free box, dx = 1: (d [1,Y,X], c_y, c_x)"""
    Y, X, sig = BLOB["Y"], BLOB["X"], BLOB["sigma"]
    jj, ii = torch.meshgrid(torch.arange(Y, dtype=torch.float64), torch.arange(X, dtype=torch.float64), indexing="ij")
    d = torch.exp(-((jj - BLOB["start"][0]) ** 2 + (ii - BLOB["start"][1]) ** 2) / (2 * sig * sig)).reshape(1, Y, X)
    cy = torch.full((1, Y + 1, X), BLOB["u"][0], dtype=torch.float64)
    cx = torch.full((1, Y, X + 1), BLOB["u"][1], dtype=torch.float64)
    return tuple(t.float().to(dtype) for t in (d, cy, cx))


@functools.lru_cache(maxsize=None)
def blob_peak(scheme):
    """the peak the blob keeps after BLOB["steps"] steps in float64"""
    d, cy, cx = blob_inputs()
    for _ in range(BLOB["steps"]):
        d = advect(d, cy, cx, 1.0, 1.0, 1.0, scheme)[0]
    return float(d.max())


FIELD_PIN, GRAD_PIN, RE_PIN = 6e-6, 5e-5, 6e-6      # float32 against float64 of the reference: about 2.5 x the measured worst (see the CPU twin)


# ---- the LargeGridTrainer / LargeGridRollout problem: the smallest grid the trainer accepts (any_width=True), B = 1, SOL-2 -------------
TRAINER_GRID, TRAINER_STD_V = ds.TRAINER_GRID, ds.TRAINER_STD_V


def corrected_step(params, d, vy, vx, re, g, scheme):
    d, vy, vx = step(d, vy, vx, re, g, scheme=scheme)
    cy, cx = o.correction(params, vy, vx, re, TRAINER_STD_V, o.STD_RE)
    return d, vy + cy, vx + cx


def trainer_problem(ms=2, seed=SEED, dtype=torch.float64):
    """buoyancy_cases.trainer_problem's recipe at TRAINER_GRID with the MacCormack step (the buoyancy suite's Reynolds number)"""
    Y, X = TRAINER_GRID
    r32 = lambda t: t.detach().float().double()
    g = table_geometry("default", Y, X)
    d, vy, vx, re = state(1, Y, X, seed, g)
    with torch.no_grad():
        _, py, px = o.synthetic_state(1, Y, X, 4321 + seed, project_it=False)
        gd, gy, gx = d, r32(vy + 0.05 * (py - 1.0)), r32(vx + 0.05 * px)
        gts_y, gts_x = [], []
        for _ in range(ms):
            gd, gy, gx = (r32(t) for t in step(gd, gy, gx, re, g))
            gts_y.append(gy)
            gts_x.append(gx)
    params = [r32(p) for p in o.init_params(0)]
    params[-2] = r32(params[-2] * 0.01)
    cast = lambda t: t.to(dtype)
    return {"g": g, "d": cast(d), "vy": cast(vy), "vx": cast(vx), "re": cast(re), "gt_vy": [cast(t) for t in gts_y],
            "gt_vx": [cast(t) for t in gts_x], "params": [cast(p).requires_grad_(True) for p in params]}


def trainer_reference(p, scheme="mac_cormack", dtype=torch.float64):
    """(loss, per-step losses, flat weight gradient, final state) of the unrolled loss (o.unrolled_loss with the chosen step) in `dtype`"""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        for q in p["params"]:
            q.grad = None
        d, vy, vx = (p[k].to(dtype) for k in ("d", "vy", "vx"))
        params, re = [q if dtype == torch.float64 else q.detach().to(dtype).requires_grad_(True) for q in p["params"]], p["re"].to(dtype)
        sv = torch.tensor(TRAINER_STD_V, dtype=dtype)
        losses = []
        for gy, gx in zip(p["gt_vy"], p["gt_vx"]):
            d, vy, vx = corrected_step(params, d, vy, vx, re, p["g"], scheme)
            diff = (o.staggered_tensor(gy.to(dtype), gx.to(dtype)) - o.staggered_tensor(vy, vx)) / sv
            losses.append(0.5 * (diff * diff).sum())
        loss = torch.stack(losses).sum() / len(losses)
        loss.backward()
    finally:
        torch.set_default_dtype(prev)
    return (float(loss.detach()), [float(l.detach()) for l in losses], torch.cat([q.grad.reshape(-1) for q in params]).double(),
            tuple(t.detach().double() for t in (d, vy, vx)))


def rollout_reference(p, steps, dtype=torch.float64):
    """`steps` steps of MacCormack solver step + correction from a trainer_problem's start -> (d, vy, vx)"""
    rd, ry, rx, re = (p[k].to(dtype) for k in ("d", "vy", "vx", "re"))
    with torch.no_grad():
        params = [q.detach().to(dtype) for q in p["params"]]
        for _ in range(steps):
            rd, ry, rx = corrected_step(params, rd, ry, rx, re, p["g"], "mac_cormack")
    return rd.double(), ry.double(), rx.double()
