"""Scenes, states and metrics shared by the large-grid karman-2d GPU tests (test_gpu_karman2d_obstacles.py,
test_gpu_karman2d_large_adjoint.py).  A plain module: importing it touches no device."""
import numpy as np
import torch

import sol_oracle as o
from sol_amd import fluid, karman, ops

DEV = "cuda"
TOL_FIELD = 1e-5
TOL_GRAD = 1e-4
CG_RTOL = 1e-7                                       # the oracle comparisons: solves converged below the field tolerance
TWO = ["sphere:50,50,10", "sphere:120,50,10"]       # two cylinders in tandem
PLATE = ["box:70:73,20:80"]                          # a plate across the channel


def rel(a, b):
    a = torch.as_tensor(np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a), dtype=torch.float64)
    b = torch.as_tensor(np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b), dtype=torch.float64)
    return float((a - b).norm() / (b.norm() + 1e-300))


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
