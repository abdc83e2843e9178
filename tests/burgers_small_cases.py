"""Cases, inputs and metrics shared by the one-workgroup Burgers tests (test_gpu_burgers_small_shapes.py and its CPU twin
test_burgers_small_shapes_cpu.py).  A plain module: importing it touches no device.

Inputs follow test_gpu_burgers_large_adjoint.py: B = 2, nu = 0.1, v = 0.8 * smooth(randn), f = 0.2 * smooth(randn), cotangents randn,
drawn in the order vy, vx, fy, fx, wy, wx from one seeded generator and rounded to fp32 values.  A case with a target CFL multiplies
the velocity by ONE fp32 factor so that max |v| dt / dx reaches the target (the way large2d_scenes.cfl_scaled does) and rounds again."""
import functools

import numpy as np
import torch

import sol_oracle as o

B, NU, AMP = 2, 0.1, 0.8
TOL_FIELD = 1e-5                                     # large2d_scenes.TOL_FIELD
TOL_GRAD = 1e-4                                      # large2d_scenes.TOL_GRAD
TRIM = 1e-3                                          # at most 0.1 % of a component's entries left out: a cap, not a tuning knob
SEED = 3

# (Y, X, dx, dt, target CFL or None = the amplitude as drawn)
TINY = [(2, 2, 1.0, 0.5, 6.0), (3, 5, 1.0, 0.5, 6.0), (5, 3, 1.0, 0.5, 6.0), (2, 64, 1.0, 0.5, 6.0), (64, 2, 1.0, 0.5, 6.0)]
RAGGED = [(Y, X, 32.0 / Y, 0.1, None) for Y, X in ((33, 17), (7, 64), (64, 7), (63, 64), (64, 63), (16, 48))]
FULL = [(64, 64, 32.0 / 64, 0.5, 3.0)]               # the largest shape that fits, several cells per step: the most arrivals per cell
CASES = TINY + RAGGED + FULL
TALL, WIDE = (64, 7, 32.0 / 64, 0.1, None), (7, 64, 32.0 / 7, 0.1, None)      # the two cases that also go through the other surfaces
assert TALL in CASES and WIDE in CASES


def case_id(c):
    return "%dx%d-dt%g-%s" % (c[0], c[1], c[3], "drawn" if c[4] is None else "cfl%g" % c[4])


def rel(a, b):
    a = torch.as_tensor(np.asarray(a.detach().cpu()), dtype=torch.float64)
    b = torch.as_tensor(np.asarray(b.detach().cpu()), dtype=torch.float64)
    return float((a - b).norm() / (b.norm() + 1e-300))


def trimmed_rel(a, b, frac=TRIM):
    """relative L2 of a against b after leaving out the floor(frac * n) entries with the largest |a - b| (the norm of b is taken over
    the entries kept) -> (value, entries left out, entries in all).  A component with fewer than 1 / frac entries leaves none out."""
    a = torch.as_tensor(np.asarray(a.detach().cpu()), dtype=torch.float64).reshape(-1)
    b = torch.as_tensor(np.asarray(b.detach().cpu()), dtype=torch.float64).reshape(-1)
    dev = (a - b).abs()
    k = int(frac * dev.numel())
    if k == 0:
        return float(dev.norm() / (b.norm() + 1e-300)), 0, dev.numel()
    keep = torch.argsort(dev)[:-k]
    return float(dev[keep].norm() / (b[keep].norm() + 1e-300)), k, dev.numel()


def check_grad(name, got, ref):
    """the trimmed metric below TOL_GRAD, the cap asserted; -> the trimmed value"""
    t, k, n = trimmed_rel(got, ref)
    print("%s: trimmed %.3e (left out %d of %d), untrimmed %.3e" % (name, t, k, n, rel(got, ref)))
    assert k <= TRIM * n and (n >= 1000 or k == 0), (name, k, n)
    assert t < TOL_GRAD, (name, t)
    return t


@functools.lru_cache(maxsize=None)
def inputs(Y, X, dx, dt, cfl, seed=SEED):
    """vy, vx, fy, fx, wy, wx (float64 tensors holding fp32 values) and the CFL number max |v| dt / dx they reach"""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    r32 = lambda t: t.float().double()
    vy, vx = r32(AMP * o._smooth(rn(B, Y + 1, X))), r32(AMP * o._smooth(rn(B, Y, X + 1)))
    fy, fx = r32(0.2 * o._smooth(rn(B, Y + 1, X))), r32(0.2 * o._smooth(rn(B, Y, X + 1)))
    wy, wx = r32(rn(B, Y + 1, X)), r32(rn(B, Y, X + 1))
    reached = lambda: max(float(vy.abs().max()), float(vx.abs().max())) * dt / dx
    if cfl is not None:
        s = float(np.float32(cfl / reached()))
        vy, vx = r32(vy * s), r32(vx * s)
    return dict(vy=vy, vx=vx, fy=fy, fx=fx, wy=wy, wx=wx, cfl=reached())


def oracle(c, dx, dt, force, dtype=torch.float64, sims=slice(None)):
    """(vy, vx) after o.burgers_step in `dtype` and the gradient of sum(out * w) with respect to the input velocity"""
    t = lambda k: c[k][sims].to(dtype)
    ay, ax = t("vy").clone().requires_grad_(True), t("vx").clone().requires_grad_(True)
    ry, rx = o.burgers_step(ay, ax, dt, NU, t("fy") if force else None, t("fx") if force else None, dx=dx)
    ((ry * t("wy")).sum() + (rx * t("wx")).sum()).backward()
    return ry.detach(), rx.detach(), ay.grad, ax.grad


@functools.lru_cache(maxsize=None)
def reference(Y, X, dx, dt, cfl, seed=SEED):
    """the inputs of a case with the float64 oracle's outputs and gradients, with and without force; computed once, never modified"""
    c = dict(inputs(Y, X, dx, dt, cfl, seed))
    c["ref"] = {force: oracle(c, dx, dt, force) for force in (True, False)}
    return c
