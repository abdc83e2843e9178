"""Scenes, states and metrics shared by the large-grid karman-2d tests (test_gpu_karman2d_obstacles.py,
test_gpu_karman2d_large_adjoint.py, test_gpu_karman2d_large_shapes.py and its CPU twin test_karman2d_large_shapes_cpu.py).  A plain
module: importing it touches no device."""
import functools

import numpy as np
import torch

import sol_oracle as o
from sol_amd import fluid, karman, ops

DEV = "cuda"
TOL_FIELD = 1e-5
TOL_GRAD = 1e-4
CG_RTOL = 1e-7                                       # the oracle comparisons: solves converged below the field tolerance
TRIM = 1e-3                                          # trimmed gradient metric: a cap, not a tuning knob (test_gpu_karman2d_large_adjoint.py)
TWO = ["sphere:50,50,10", "sphere:120,50,10"]       # two cylinders in tandem
PLATE = ["box:70:73,20:80"]                          # a plate across the channel

# ---- the ragged-shape table (test_gpu_karman2d_large_shapes.py, pinned by test_karman2d_large_shapes_cpu.py) -----------------------
# 130 x 65: the smallest large grid, Y % 16 = 2 and X % 16 = 1 (the last adjoint tile row is 2 cells + face row Y, the last tile column
# 1 cell + face column X);  144 x 72: Y % 16 = 0, X % 16 = 8, % 64 = 16 and 8 (GEMM edge tiles; full adjoint tile rows, a half tile
# column);  160 x 80: X % 16 = 0, X % 64 = 16.
SHAPES = [(130, 65), (144, 72), (160, 80)]
SCENE_SPECS = {"default": None,                       # the oracle's default sphere
               "small": ["sphere:50,50,4"],
               "big": ["sphere:60,50,22"],
               "corner": ["box:188:200,88:100"],      # touches the top and the right edge: the window is clamped to the domain
               "top_edge": ["sphere:195,50,6"],
               "two": TWO}
# (wy0, wx0, nS, SP, win) of precond.direct_solver_blob(active, max_window=64); None: the one-window blob refuses the scene
WINDOWS = {
    ("default", 130): (25, 25, 177, 192, 16), ("default", 144): (28, 28, 208, 256, 16), ("default", 160): (31, 31, 256, 256, 32),
    ("small", 130): (29, 29, 37, 64, 16), ("small", 144): (32, 32, 40, 64, 16), ("small", 160): (36, 36, 52, 64, 16),
    ("big", 130): (24, 17, 722, 768, 32), ("big", 144): (26, 8, 884, 896, 64), ("big", 160): (29, 16, 1068, 1088, 64),
    ("corner", 130): (114, 49, 80, 128, 16), ("corner", 144): (128, 56, 99, 128, 16), ("corner", 160): (144, 64, 120, 128, 16),
    ("top_edge", 130): (114, 28, 64, 64, 16), ("top_edge", 144): (128, 31, 76, 128, 16), ("top_edge", 160): (144, 34, 94, 128, 16),
    ("two", 130): (25, 1, 348, 384, 64), ("two", 144): None, ("two", 160): None,
}


def rel(a, b):
    a = torch.as_tensor(np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a), dtype=torch.float64)
    b = torch.as_tensor(np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b), dtype=torch.float64)
    return float((a - b).norm() / (b.norm() + 1e-300))


def trimmed_rel(a, b, frac=TRIM):
    """relative L2 of a against b after leaving out the floor(frac * n) entries with the largest |a - b| (the norm of b is taken over
    the entries kept) -> (value, entries left out, largest deviation left out)"""
    a = torch.as_tensor(np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a), dtype=torch.float64).reshape(-1)
    b = torch.as_tensor(np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b), dtype=torch.float64).reshape(-1)
    dev = (a - b).abs()
    k = int(frac * dev.numel())
    if k == 0:
        return float(dev.norm() / (b.norm() + 1e-300)), 0, 0.0
    order = torch.argsort(dev)
    keep, drop = order[:-k], order[-k:]
    return float(dev[keep].norm() / (b[keep].norm() + 1e-300)), k, float(dev[drop].max())


def check_grads(got, ref, trimmed, what):
    for name, a, b in zip(("g_vy", "g_vx"), got, ref):
        full = rel(a, b)
        if trimmed:
            v, k, worst = trimmed_rel(a, b)
            print("%s %s: rel L2 %.3e untrimmed, %.3e after leaving out %d of %d entries (largest deviation left out %.3e)"
                  % (what, name, full, v, k, b.numel(), worst))
            assert k <= int(TRIM * b.numel())
            assert v < TOL_GRAD, (what, name, v, full)
        else:
            print("%s %s: rel L2 %.3e" % (what, name, full))
            assert full < TOL_GRAD, (what, name, full)


def f32(t):
    return torch.as_tensor(np.asarray(t), dtype=torch.float32).to(DEV).contiguous()


def active_of(specs, Y, X):
    dom = fluid.Domain([Y, X], box=fluid.box[0:200, 0:100])
    return karman.KarmanFlow(obstacles=karman.parse_obstacles(specs)).scene_arrays(dom)[0]


def geometry(Y, X, active):
    """The oracle's KarmanGeometry (a fresh instance, never the cached one) with the masks of a custom obstacle."""
    g = o.KarmanGeometry(Y, X)
    g.active = np.asarray(active, dtype=np.float64)
    g.obstacle = 1.0 - g.active
    acc = np.pad(g.active, 1, mode="edge")
    g.my = np.minimum(acc[0:Y + 1, 1:X + 1], acc[1:Y + 2, 1:X + 1])
    g.mx = np.minimum(acc[1:Y + 1, 0:X + 1], acc[1:Y + 1, 1:X + 2])
    g.diag = np.minimum(-(acc[0:Y, 1:X + 1] + acc[2:Y + 2, 1:X + 1] + acc[1:Y + 1, 0:X] + acc[1:Y + 1, 2:X + 2]), -1.0)
    return g


def masks(g, solver="auto"):
    return ops.SceneMasks(g.active, g.inflow, g.bc_mask, g.bc_mask, DEV, pressure_solver=solver)


def state(B, Y, X, seed, g=None):
    """seeded smooth noise; with a geometry: spun up by one float64 oracle step in that scene (divergence free, consistent with
    its obstacles -- the state a data-generation run steps), rounded to fp32 values"""
    d, vy, vx = o.synthetic_state(B, Y, X, seed, project_it=False)
    re = torch.tensor([o.RE_TRAIN[i % 6] for i in range(B)], dtype=torch.float64)
    if g is not None:
        with torch.no_grad():
            d, vy, vx = (t.float().double() for t in o.karman_step(d, vy, vx, re, g))
    return d, vy, vx, re


@functools.lru_cache(maxsize=None)
def table_geometry(name, Y, X):
    """the oracle geometry of a SCENE_SPECS scene at Y x X (one instance per cell of the table: it keeps the sparse LU of its matrix)"""
    return o.KarmanGeometry(Y, X) if SCENE_SPECS[name] is None else geometry(Y, X, active_of(SCENE_SPECS[name], Y, X))


def cotangent_at(B, Y, X, seed=3):
    """seeded normal cotangents of magnitude ~1 for (v_y, v_x), fp32 values held in float64 (the cotangent of the 256 x 128 tests)"""
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(B, Y + 1, X, generator=gen, dtype=torch.float64).float().double(),
            torch.randn(B, Y, X + 1, generator=gen, dtype=torch.float64).float().double())


def step_like_rhs(B, Y, X, seed=4):
    """B right-hand sides the step's solve sees: -div of unprojected seeded noise, fp32 values held in float64"""
    _, vy, vx = o.synthetic_state(B, Y, X, seed, project_it=False)
    return (-((vy[:, 1:] - vy[:, :-1]) + (vx[:, :, 1:] - vx[:, :, :-1]))).float().double()


def cfl_scaled(st, g, target):
    """st with its velocity multiplied by one factor (fp32 values) so that max |u| dt/dx of the post-diffusion velocity -- the field the
    advection and its adjoint trace back along -- is about `target`  ->  (state, the value reached)"""
    d, vy, vx, re = st
    dtdx = 1.0 / g.dx

    def reached(y, x):
        cy, cx = o.diffuse_bc(y, x, re, g.X, 1.0, g)
        return max(float(cy.abs().max()), float(cx.abs().max())) * dtdx

    s = float(np.float32(target / reached(vy, vx)))
    sy, sx = (vy * s).float().double(), (vx * s).float().double()
    return (d, sy, sx, re), reached(sy, sx)
