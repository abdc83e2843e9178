"""Grids, scenes, seeds and float64 references of the karman-2d multi_launch tests (test_gpu_karman2d_solve_one_wg.py,
test_gpu_karman2d_multi_launch.py and their CPU twin test_karman2d_multi_launch_cpu.py): SceneMasks(multi_launch=True) runs the
multi-launch path on the grids the one-workgroup kernels would serve.  A plain module: importing it touches no device.

Scenes are the oracle's (sol_oracle.geometry on any grid: the default sphere, the inflow box and the velocity BC keep their physical
definitions); TWO_BOXES is a custom obstacle whose support set spans more than 32 cells, so the one-window blob takes the 64-cell window.
States: large2d_scenes.state (spun up in the scene, fp32 values), cotangents large2d_scenes.cotangent_at / density_adjoint_cases.w_dens.
SEEDS: per (grid, physics) the first seed of (77, 11, 5, 7, 13) at which the float32 reference agrees with the float64 reference to a
quarter of TOL_FIELD / TOL_GRAD (the rule of karman2d_small_shapes.SEEDS; the MacCormack gradients in the trimmed metric with the cap
large2d_scenes.TRIM as a condition, as everywhere in maccormack_cases); the CPU twin measures and pins them."""
import functools
import os
import sys

import numpy as np
import torch

import sol_oracle as o

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buoyancy_cases as bc
import maccormack_cases as mc
from density_adjoint_cases import w_dens
from large2d_scenes import TOL_FIELD, TOL_GRAD, TRIM, active_of, cotangent_at, geometry, rel, state, trimmed_rel  # noqa: F401

B = 2
CANDIDATES = (77, 11, 5, 7, 13)
TWO_BOXES = ["box:40:50,20:30", "box:110:120,60:70"]

# ---- the solve kernel's shape table: id -> (Y, X, obstacle specs | None (the default sphere), what it reaches) ---------------------------
SOLVE_CASES = {
    "16x16": (16, 16, None, "window = whole grid"),
    "48x32": (48, 32, None, "Y != 2 X"),
    "32x64": (32, 64, None, "Y < X, SP = 128, the sphere is cut by the wall"),
    "40x24": (40, 24, None, "ragged on both axes"),
    "96x48": (96, 48, None, "a width no entry took before"),
    "128x64": (128, 64, None, "8192 cells, the default sphere"),
    "128x64_two_boxes": (128, 64, TWO_BOXES, "win = 64, the LDS worst case"),
    "512x16": (512, 16, None, "the tallest Y"),
    # beyond the issue's table: Y, X no multiples of 4 -- the kernel's instantiation with guarded element loads and padded LDS pitches
    "49x31": (49, 31, None, "odd on both axes: guarded loads, LDS pitches 52 and 32"),
    "130x63": (130, 63, None, "8190 cells, no multiple of 4: the largest LDS images (64 x 132 floats each)"),
}
# (wy0, wx0, nS, SP, win) of precond.direct_solver_blob(active, 64), pinned by the CPU twin
SOLVE_WINDOWS = {
    "16x16": (0, 0, 24, 64, 16), "48x32": (12, 12, 52, 64, 16), "32x64": (16, 25, 82, 128, 16), "40x24": (9, 8, 32, 64, 16),
    "96x48": (18, 18, 104, 128, 16), "128x64": (25, 25, 164, 192, 16), "128x64_two_boxes": (25, 0, 137, 192, 64),
    "512x16": (5, 0, 24, 64, 16), "49x31": (11, 11, 49, 64, 16), "130x63": (24, 24, 157, 192, 16),
}


@functools.lru_cache(maxsize=None)
def solve_geometry(case):
    Y, X, specs, _ = SOLVE_CASES[case]
    return o.geometry(Y, X) if specs is None else geometry(Y, X, active_of(specs, Y, X))


def one_wg_supported(Y, X, win):
    """replica of sol_karman_solve_one_wg_supported (csrc/karman_solve_small.hip)"""
    return Y >= 16 and X >= 16 and Y * X <= 8192 and X <= 64 and win in (16, 32, 64) and win <= Y and win <= X


# ---- the step's cases: (grid, advection strength | None, force | None, diffusion substeps) -> seed -----------------------------------------
PLAIN = [(64, 32), (48, 32)]
MAC = [((48, 32), 1.0, None, 1), ((48, 32), 0.5, None, 1), ((96, 48), 1.0, None, 1), ((96, 48), 0.5, None, 1),
       ((48, 32), None, bc.FORCES[1], 1), ((48, 32), None, None, 3), ((48, 32), 1.0, bc.FORCES[1], 3)]
CG_GRIDS = [(96, 32), (16, 64)]
SCATTERED_GRID = (64, 32)
SEEDS = {}
for _g in PLAIN + CG_GRIDS:
    SEEDS[(_g, None, None, 1)] = 77
for _c in MAC:
    SEEDS[_c] = 77
SEEDS[((48, 32), 1.0, None, 1, "density")] = 77
SEEDS[((48, 32), 1.0, None, 1, "re")] = 77


def step_of(adv, force, n):
    """the reference step of a case: o.karman_step for the plain physics, else maccormack_cases.step (which holds the buoyancy term of
    buoyancy_cases and the pre-diffusion of diffusion_substeps_cases)"""
    if adv is None and force is None and n == 1:
        return lambda d, vy, vx, re, g: o.karman_step(d, vy, vx, re, g)
    scheme = "semi_lagrangian" if adv is None else "mac_cormack"
    return lambda d, vy, vx, re, g: mc.step(d, vy, vx, re, g, 1.0 if adv is None else adv, scheme, force, n)


@functools.lru_cache(maxsize=None)
def reference(grid, adv=None, force=None, n=1, kind="velocity", seed=None, dtype=torch.float64):
    """One step and its autograd -> ((d, vy, vx), (g_d, g_vy, g_vx, g_re), state, cotangents (wd | None, wy, wx)), float64 tensors.
    kind "velocity": loss <vy, wy> + <vx, wx>; "density": plus <d, wd>; "re": the velocity loss, gradient in re as well.
    Cached: computed once, shared, never modified."""
    Y, X = grid
    key = (grid, adv, force, n) if kind == "velocity" else (grid, adv, force, n, kind)
    g = o.geometry(Y, X)
    st = tuple(t.to(dtype) for t in state(B, Y, X, SEEDS[key] if seed is None else seed, g))
    leaves = [t.clone().requires_grad_(True) for t in st]
    out = step_of(adv, force, n)(*leaves, g)
    wy, wx = (t.to(dtype) for t in cotangent_at(B, Y, X))
    wd = w_dens(B, Y, X, g).to(dtype) if kind == "density" else None
    loss = (out[1] * wy).sum() + (out[2] * wx).sum()
    if wd is not None:
        loss = loss + (out[0] * wd).sum()
    loss.backward()
    grads = tuple(torch.zeros_like(p).double() if p.grad is None else p.grad.double() for p in leaves)
    return tuple(t.detach().double() for t in out), grads, tuple(t.double() for t in st), (wd, wy.double(), wx.double())


def grad_error(got, ref, trimmed):
    """relative L2 of a gradient, in the trimmed metric (cap TRIM, a condition) where the case needs it -> (value, entries left out)"""
    if not trimmed:
        return rel(got, ref), 0
    v, k, _ = trimmed_rel(got, ref)
    assert k <= int(TRIM * ref.numel())
    return v, k


# ---- the trainer / roll-out problem: mars_moon, SOL-2, MacCormack + buoyancy + two diffusion substeps ---------------------------------------
TRAINER_FORCE, TRAINER_NSUB, TRAINER_STD_V = bc.FORCES[1], 2, mc.TRAINER_STD_V


def corrected_step(params, d, vy, vx, re, g, force, n):
    d, vy, vx = mc.step(d, vy, vx, re, g, force=force, n=n)
    cy, cx = o.correction(params, vy, vx, re, TRAINER_STD_V, o.STD_RE)
    return d, vy + cy, vx + cx


TRAINER_SEED = 77        # (seed 11, the MacCormack suite's: at 64 x 32 the float32 reference alone misses its float64 by 9e-5 in the second step's loss)
TRAINER_CASES = [((64, 32), 2), ((96, 48), 1)]           # (grid, simulations); the roll-out: 64 x 32, B = 2, MacCormack alone, four steps


def trainer_problem(Y, X, nb, ms=2, seed=TRAINER_SEED, force=TRAINER_FORCE, n=TRAINER_NSUB):
    """maccormack_cases.trainer_problem's recipe on a Y x X grid with nb simulations and the full physics"""
    r32 = lambda t: t.detach().float().double()
    g = o.geometry(Y, X)
    d, vy, vx, re = state(nb, Y, X, seed, g)
    with torch.no_grad():
        _, py, px = o.synthetic_state(nb, Y, X, 4321 + seed, project_it=False)
        gd, gy, gx = d, r32(vy + 0.05 * (py - 1.0)), r32(vx + 0.05 * px)
        gts_y, gts_x = [], []
        for _ in range(ms):
            gd, gy, gx = (r32(t) for t in mc.step(gd, gy, gx, re, g, force=force, n=n))
            gts_y.append(gy)
            gts_x.append(gx)
    params = [r32(p) for p in o.init_params(0)]
    params[-2] = r32(params[-2] * 0.01)
    return {"g": g, "d": d, "vy": vy, "vx": vx, "re": re, "gt_vy": gts_y, "gt_vx": gts_x, "force": force, "n": n,
            "params": [p.clone().requires_grad_(True) for p in params]}


def trainer_reference(p, dtype=torch.float64):
    """(loss, per-step losses, flat weight gradient, final state) of the unrolled loss in `dtype`"""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        params = [q.detach().to(dtype).requires_grad_(True) for q in p["params"]]
        d, vy, vx, re = (p[k].to(dtype) for k in ("d", "vy", "vx", "re"))
        sv = torch.tensor(TRAINER_STD_V, dtype=dtype)
        losses = []
        for gy, gx in zip(p["gt_vy"], p["gt_vx"]):
            d, vy, vx = corrected_step(params, d, vy, vx, re, p["g"], p["force"], p["n"])
            diff = (o.staggered_tensor(gy.to(dtype), gx.to(dtype)) - o.staggered_tensor(vy, vx)) / sv
            losses.append(0.5 * (diff * diff).sum())
        loss = torch.stack(losses).sum() / len(losses)
        loss.backward()
    finally:
        torch.set_default_dtype(prev)
    return (float(loss.detach()), [float(l.detach()) for l in losses], torch.cat([q.grad.reshape(-1) for q in params]).double(),
            tuple(t.detach().double() for t in (d, vy, vx)))


def rollout_reference(p, steps, dtype=torch.float64):
    rd, ry, rx, re = (p[k].to(dtype) for k in ("d", "vy", "vx", "re"))
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        with torch.no_grad():
            params = [q.detach().to(dtype) for q in p["params"]]
            for _ in range(steps):
                rd, ry, rx = corrected_step(params, rd, ry, rx, re, p["g"], p["force"], p["n"])
    finally:
        torch.set_default_dtype(prev)
    return rd.double(), ry.double(), rx.double()


def adam_reference(w, g, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """one TF-Adam step from zero moments in float64"""
    m, v = (1 - beta1) * g, (1 - beta2) * g * g
    return w - lr * np.sqrt(1 - beta2) / (1 - beta1) * m / (np.sqrt(v) + eps)
