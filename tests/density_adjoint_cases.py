"""Inputs and float64-oracle references of the karman-2d density-adjoint tests (test_gpu_karman2d_density_adjoint.py and its CPU twin
test_karman2d_density_adjoint_cpu.py).  A plain module: importing it touches no device.

The inputs are FIXED.  The step's gradient jumps where a departure point crosses a cell boundary, so a test input must keep every
departure point clear of one:
  * state seed 11 (large2d_scenes.state): with it the oracle in float32 agrees with the oracle in float64, untrimmed, to 8.3e-6 on every
    gradient component at every shape used here (seeds 5 and 7 flip one cell on some shapes);
  * the density cotangent is masked with the scene's `active`: deep inside the obstacle the saved velocity is exactly 0, the departure
    point sits exactly ON a cell boundary, and which side the oracle takes depends on the rounding of (j + 1/2) dx / dx when dx is not
    representable (X = 65); the kernel always takes floorf(0) = 0.
test_karman2d_density_adjoint_cpu.py pins that condition (float32 against float64 below 2e-5)."""
import functools
import os
import sys

import torch

import sol_oracle as o

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from large2d_scenes import cotangent_at, state

SEED = 11


@functools.lru_cache(maxsize=None)
def scene(Y, X):
    return o.KarmanGeometry(Y, X)


def w_dens(B, Y, X, g):
    """seeded normal density cotangent (seed 3) times the active mask, fp32 values held in float64"""
    gen = torch.Generator().manual_seed(3)
    w = torch.randn(B, Y, X, generator=gen, dtype=torch.float64).float().double()
    return w * torch.as_tensor(g.active, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def oracle_case(Y, X, B, steps=1, with_velocity=False, inflow_order="after", dtype=torch.float64):
    """the oracle's autograd through `steps` chained o.karman_step: loss = <d_last, w_d> (+ <vy_last, w_y> + <vx_last, w_x> with
    with_velocity) -> ((d, vy, vx) after the last step, (g_d, g_vy, g_vx) with respect to the initial state), float64 tensors.  Cached:
    computed once, shared, never modified."""
    g = scene(Y, X)
    d, vy, vx, re = (t.to(dtype) for t in state(B, Y, X, SEED, g))
    rd, ry, rx = (t.clone().requires_grad_(True) for t in (d, vy, vx))
    cd, cy, cx = rd, ry, rx
    for _ in range(steps):
        cd, cy, cx = o.karman_step(cd, cy, cx, re, g, inflow_order=inflow_order)
    loss = (cd * w_dens(B, Y, X, g).to(dtype)).sum()
    if with_velocity:
        wy, wx = cotangent_at(B, Y, X)
        loss = loss + (cy * wy.to(dtype)).sum() + (cx * wx.to(dtype)).sum()
    loss.backward()
    zero = lambda t, like: torch.zeros_like(like) if t is None else t
    return (tuple(t.detach().double() for t in (cd, cy, cx)),
            tuple(zero(p.grad, p).double() for p in (rd, ry, rx)))
