"""Inputs and oracle references of the karman-3d density / Reynolds-number adjoint tests (test_gpu_karman3d_density_re_adjoint.py and its
CPU twin test_karman3d_density_re_adjoint_cpu.py).  A plain module: importing it touches no device.

The inputs are FIXED.  The step's gradient jumps where a departure point crosses a cell boundary, so a test input must keep every
departure point clear of one: with o.synthetic_state(B, Y, X, Z, 13) and the cases below the oracle in float32 agrees with the oracle in
float64, UNTRIMMED, below 2e-5 on every gradient component (the CPU test pins it for every case; seed 11 flips a cell in the combined
cases, and 32 x 16 x 16 at its natural velocity has three cells within 1e-6 of a boundary).  The density cotangent is masked with the
scene's `active`: inside the obstacle the saved velocity is exactly 0 and the departure point sits exactly ON a cell boundary.

A case = the shape, a factor on the velocity, the time step, the Reynolds numbers, the step's options, the number of chained steps and
which cotangents the loss carries:  loss = <d_last, w_d> [density]  +  sum_c <v_c_last, w_c> [velocity]."""
import functools

import torch

import sol_oracle3d as o

SEED = 13
NAMES = ("g_d", "g_vy", "g_vx", "g_vz", "g_re")

CASES = {
    # 16 x 8 x 8, B = 2: the minimum grid, a batch
    "16_dens": dict(shape=(2, 16, 8, 8), density=True),
    "16_vel": dict(shape=(2, 16, 8, 8), velocity=True),
    "16_comb": dict(shape=(2, 16, 8, 8), density=True, velocity=True),
    "16_two": dict(shape=(2, 16, 8, 8), density=True, velocity=True, steps=2),
    "16_before": dict(shape=(2, 16, 8, 8), density=True, kw=dict(inflow_order="before")),
    "16_dirichlet": dict(shape=(2, 16, 8, 8), density=True, velocity=True, kw=dict(grad_pad="dirichlet0")),
    "16_lowre": dict(shape=(2, 16, 8, 8), density=True, velocity=True, re=(2000.0, 4000.0)),      # alpha = 0.032, 0.016: alpha L matters
    # 20 x 10 x 10: tiles that end inside the grid, the extra face rows
    "20_dens": dict(shape=(1, 20, 10, 10), density=True),
    "20_comb": dict(shape=(1, 20, 10, 10), density=True, velocity=True),
    # 32 x 16 x 16, velocity x 3.5: |v| dt = 4 length units, 0.64 cells ...
    "32_x35": dict(shape=(1, 32, 16, 16), density=True, scale=3.5),
    # ... and with dt = 4: departure points up to 2.6 CELLS away (cfl_of), targets beyond the scatter's LDS window of two halo columns
    "32_cfl": dict(shape=(1, 32, 16, 16), density=True, scale=3.5, dt=4.0),
}


def case(name):
    c = dict(scale=1.0, dt=1.0, re=None, kw={}, steps=1, density=False, velocity=False)
    c.update(CASES[name])
    return c


def geometry(name):
    _, Y, X, Z = case(name)["shape"]
    return o.geometry(Y, X, Z)


@functools.lru_cache(maxsize=None)
def state(name):
    """(d, (vy, vx, vz), re) of the case: float64 tensors holding fp32 values.  Shared, never modified."""
    c = case(name)
    B, Y, X, Z = c["shape"]
    d, v = o.synthetic_state(B, Y, X, Z, SEED)
    v = tuple((t * c["scale"]).float().double() for t in v)
    re = torch.tensor(c["re"] if c["re"] is not None else o.RE_TRAIN[:B], dtype=torch.float64)
    return d.float().double(), v, re


def cfl_of(name):
    """max |v| dt / dx of the case's input velocity"""
    c = case(name)
    _, v, _ = state(name)
    return max(float(t.abs().max()) for t in v) * c["dt"] / geometry(name).dx


@functools.lru_cache(maxsize=None)
def w_dens(name):
    """seeded normal density cotangent (seed 3) times the active mask, fp32 values held in float64"""
    B, Y, X, Z = case(name)["shape"]
    gen = torch.Generator().manual_seed(3)
    w = torch.randn(B, Y, X, Z, generator=gen, dtype=torch.float64).float().double()
    return w * torch.as_tensor(geometry(name).active, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def w_vel(name):
    """seeded normal velocity cotangents (seed 3), fp32 values held in float64"""
    B, Y, X, Z = case(name)["shape"]
    gen = torch.Generator().manual_seed(3)
    return tuple(torch.randn(s, generator=gen, dtype=torch.float64).float().double()
                 for s in ((B, Y + 1, X, Z), (B, Y, X + 1, Z), (B, Y, X, Z + 1)))


def step(d, v, re, name):
    """the oracle's step with the case's time step and options"""
    c = case(name)
    return o.karman3d_step(d, v, re, geometry(name), dt=c["dt"], **c["kw"])


@functools.lru_cache(maxsize=None)
def oracle_case(name, dtype=torch.float64):
    """the oracle's autograd through the case's chained o.karman3d_step -> ((d, vy, vx, vz) after the last step, (g_d, g_vy, g_vx, g_vz,
    g_re) with respect to the initial state and re), float64 tensors.  Cached: computed once, shared, never modified."""
    c = case(name)
    d, v, re = state(name)
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in (d, *v, re)]
    cd, cv = leaves[0], tuple(leaves[1:4])
    for _ in range(c["steps"]):
        cd, cv = step(cd, cv, leaves[4], name)
    loss = 0.0
    if c["density"]:
        loss = loss + (cd * w_dens(name).to(dtype)).sum()
    if c["velocity"]:
        loss = loss + sum((a * w.to(dtype)).sum() for a, w in zip(cv, w_vel(name)))
    loss.backward()
    zero = lambda p: torch.zeros_like(p) if p.grad is None else p.grad
    return (tuple(t.detach().double() for t in (cd, *cv)), tuple(zero(p).double() for p in leaves))
