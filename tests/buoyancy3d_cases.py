"""Float64 reference, inputs and cached reference results of the karman-3d buoyancy tests (test_gpu_karman3d_buoyancy.py and its CPU twin
test_karman3d_buoyancy_cpu.py).  A plain module: importing it touches no device.

The reference step is composed from the 3-D oracle's own stages (o.diffuse_bc, o.advect_mac, o.project) and the face average of the
definition (include/sol_hip.h, "BUOYANCY on the karman-3d step"): with c the post-diffusion velocity and F = (F_y, F_x, F_z)
    d_out = SL(d_in [+ inflow], c) [+ inflow dt]
    a_y[jf,i,k] = SL_y(c)[jf,i,k] + dt F_y (dz(jf-1,i,k) + dz(jf,i,k)) / 2,   a_x, a_z likewise,   dz = d_out with a zero ghost ring
    v_out = project(a)        (o.project applies the hard-BC face masks first, then subtracts mask * grad p)
The inputs are FIXED, those of karman3d_adjoint_cases.py: o.synthetic_state(B, Y, X, Z, 13), the seeded velocity cotangents w_vel and the
density cotangent w_dens masked with the scene's `active`.  The step's gradient jumps where a departure point crosses a cell boundary, and
the force moves the second step's departure points: test_karman3d_buoyancy_cpu.py measures how far the reference in float32 is from the
reference in float64 on every case the GPU tests use, in the metric both files assert -- max |a - b| / max |b| (maxrel), untrimmed.  Seed 11
is not used: with it several cases sit 2e-4 .. 1.5e-3 apart.  What was measured is in that file's docstring; the pins below are the worst
figure times about 2.5, and the GPU tests allow MARGIN times the pin (the ratio of the 3-D adjoint tests' tolerance, TOL_GRAD = 1e-4, to
their own pin of 2e-5)."""
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

import sol_oracle3d as o

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))        # make_golden.k3d_params: the golden network weights
import karman3d_adjoint_cases as kc

FORCES = ((0.981, 0.0, 0.0), (0.3, -0.2, 0.15))
# forward cases (fields): the step's options and the three shapes; adjoint cases (gradients): 16 x 8 x 8 with B = 2 and 32 x 16 x 16, v x 3.5
FORWARD_CASES = ("16_comb", "16_before", "16_dirichlet", "20_comb", "32_x35")
ADJOINT_CASES = ("16_comb", "32_x35")
KINDS = ("dens", "vel", "both")
NAMES = kc.NAMES

FIELD_PIN, GRAD_PIN, RE_PIN = 3e-6, 1e-5, 4e-5      # float32 against float64 of the reference (maxrel): the measured worst times about 2.5
MARGIN = 5.0                                        # GPU bound = MARGIN x pin


def maxrel(a, b):
    """max |a - b| / max |b| in float64 on the host"""
    a, b = (torch.as_tensor(t).detach().double().cpu() for t in (a, b))
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def wall_mask(Y, X, Z):
    """`active` of a box with an obstacle that touches the low x wall and the high z wall (grids below 3 cells per axis: no obstacle)"""
    act = np.ones((Y, X, Z))
    if min(Y, X, Z) < 3:
        return act
    act[Y // 3:Y // 3 + max(Y // 4, 1), :max(X // 2, 1), Z - max(Z // 3, 1):] = 0.0
    return act


def face_masks(act):
    """the hard-BC face masks of an `active` array as the oracle's geometry forms them ('boundary' extrapolation: edge value outside)"""
    a = np.pad(act, 1, mode="edge")
    c = slice(1, -1)
    return (a[:-1, c, c] * a[1:, c, c], a[c, :-1, c] * a[c, 1:, c], a[c, c, :-1] * a[c, c, 1:])


def face_average(d):
    """the three face averages of a cell field with a zero ghost ring: [B,Y+1,X,Z], [B,Y,X+1,Z], [B,Y,X,Z+1]"""
    dz = F.pad(d, (1, 1, 1, 1, 1, 1))
    c = slice(1, -1)
    return (0.5 * (dz[:, :-1, c, c] + dz[:, 1:, c, c]), 0.5 * (dz[:, c, :-1, c] + dz[:, c, 1:, c]), 0.5 * (dz[:, c, c, :-1] + dz[:, c, c, 1:]))


def add_term(d, masks, f):
    """the term alone on a zero velocity: mask_c f_c avg_c(d) for the three components, in d's dtype"""
    return tuple(o._t(m, d) * (fc * a) for m, fc, a in zip(masks, f, face_average(d)))


def add_term_transpose(g, masks, f):
    """the transpose of add_term applied to face fields g = (g_y, g_x, g_z): a cell field"""
    m = [o._t(mk, g[0]) * gc for mk, gc in zip(masks, g)]
    return (f[0] * 0.5 * (m[0][:, :-1] + m[0][:, 1:]) + f[1] * 0.5 * (m[1][:, :, :-1] + m[1][:, :, 1:]) +
            f[2] * 0.5 * (m[2][:, :, :, :-1] + m[2][:, :, :, 1:]))


def buoyant_step(d, v, re, geom, force, dt=1.0, res=None, grad_pad="replicate", inflow_order="after"):
    """o.karman3d_step with the buoyancy term between the advection and the projection"""
    res = geom.X if res is None else res
    c = o.diffuse_bc(v, re, res, dt, geom)
    infl = o._t(geom.inflow, v[0])
    if inflow_order == "before":
        d = d + infl
    d2, a = o.advect_mac(d, c, dt, geom.dx)
    if inflow_order == "after":
        d2 = d2 + infl * dt
    a = tuple(ac + (dt * fc) * avg for ac, fc, avg in zip(a, force, face_average(d2)))
    return d2, o.project(a, geom, grad_pad=grad_pad)


def step_of(name, force):
    """buoyant_step with the case's time step and options: (d, v, re) -> (d, v)"""
    c = kc.case(name)
    return lambda d, v, re: buoyant_step(d, v, re, kc.geometry(name), force, dt=c["dt"], **c["kw"])


@functools.lru_cache(maxsize=None)
def reference(name, force, kind="both", steps=1, dtype=torch.float64):
    """The reference's autograd through `steps` chained buoyant steps from the case's state -> ((d, vy, vx, vz) after the last step,
    (g_d, g_vy, g_vx, g_vz, g_re) with respect to the initial state and re), float64 tensors.  kind: "dens" (loss = <d, w_dens>), "vel"
    (sum_c <v_c, w_c>) or "both".  Cached: computed once, shared, never modified."""
    d, v, re = kc.state(name)
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in (d, *v, re)]
    cd, cv = leaves[0], tuple(leaves[1:4])
    step = step_of(name, force)
    for _ in range(steps):
        cd, cv = step(cd, cv, leaves[4])
    loss = 0.0
    if kind in ("dens", "both"):
        loss = loss + (cd * kc.w_dens(name).to(dtype)).sum()
    if kind in ("vel", "both"):
        loss = loss + sum((a * w.to(dtype)).sum() for a, w in zip(cv, kc.w_vel(name)))
    loss.backward()
    zero = lambda p: torch.zeros_like(p) if p.grad is None else p.grad
    return (tuple(t.detach().double() for t in (cd, *cv)), tuple(zero(p).double() for p in leaves))


# ---- trainer and roll-out ------------------------------------------------------------------------------------------------------------
TRAINER_SHAPE, TRAINER_STD_V, TRAINER_FORCE = (2, 32, 16, 16), (0.2, 0.25, 0.3), FORCES[0]


def unrolled_loss(params, d, v, re, gts, geom, std_v, std_re, force):
    """o.unrolled_loss with the buoyant step: (loss, per-step losses, (d, v) after the last corrected step)"""
    losses = []
    for gt in gts:
        d, v = buoyant_step(d, v, re, geom, force)
        c = o.correction(params, v, re, std_v, std_re)
        v = tuple(a + b for a, b in zip(v, c))
        losses.append(sum(0.5 * (((g - a) / s) ** 2).sum() for g, a, s in zip(gt, v, std_v)))
    return torch.stack(losses).sum() / len(gts), losses, (d, v)


def trainer_problem(ms=2):
    """The recipe of test_gpu_karman3d.test_karman3d_trainer_sol2_against_oracle: o.synthetic_state(seed 77) at 32 x 16 x 16, B = 2, ground
    truth = o.synthetic_state(500 + i), the golden network weights; fp32 values held in float64"""
    import make_golden as mg
    B, Y, X, Z = TRAINER_SHAPE
    d, v = o.synthetic_state(B, Y, X, Z, 77)
    d, v = d.float().double(), tuple(c.float().double() for c in v)
    gts = [tuple(c.float().double() for c in o.synthetic_state(B, Y, X, Z, 500 + i)[1]) for i in range(ms)]
    return {"g": o.geometry(Y, X, Z), "d": d, "v": v, "re": torch.tensor(o.RE_TRAIN[:B], dtype=torch.float64), "gts": gts,
            "params": [p.clone() for p in mg.k3d_params()]}


@functools.lru_cache(maxsize=None)
def trainer_reference(force=TRAINER_FORCE, ms=2):
    """(loss, per-step losses, flat weight gradient, (d, vy, vx, vz) after the last step) of unrolled_loss on trainer_problem, float64"""
    p = trainer_problem(ms)
    params = [q.clone().requires_grad_(True) for q in p["params"]]
    loss, losses, (d, v) = unrolled_loss(params, p["d"], p["v"], p["re"], p["gts"], p["g"], TRAINER_STD_V, o.STD_RE, force)
    loss.backward()
    return (float(loss.detach()), [float(l.detach()) for l in losses], torch.cat([q.grad.reshape(-1) for q in params]).double(),
            tuple(t.detach().double() for t in (d, *v)))


def rollout_reference(params, d, v, re, geom, std_v, std_re, force, nsteps):
    """o.rollout with the buoyant step -> (d, v) after the last corrected step"""
    with torch.no_grad():
        for _ in range(nsteps):
            d, v = buoyant_step(d, v, re, geom, force)
            c = o.correction(params, v, re, std_v, std_re)
            v = tuple(a + b for a, b in zip(v, c))
    return d, v
