"""Float64 reference, inputs and cached reference results of the karman-3d diffusion-substep tests
(test_gpu_karman3d_diffusion_substeps.py and its CPU twin test_karman3d_diffusion_substeps_cpu.py).  A plain module: importing it touches
no device.

The reference needs nothing new in the oracle.  With a = dt res^2 / (n re) per simulation,
    repeat n - 1 times:  v_c += a * o.laplace_replicate(v_c)    for the three components
    o.karman3d_step(d, v, re * n, geom, dt, **kw)               (buoyancy3d_cases.buoyant_step for the buoyant case)
i.e. n explicit substeps of alpha / n and the boundary blend once, after the last one.  Gradients are torch autograd through that, in
float64, re.grad included.

States, cotangents and the metric (maxrel, untrimmed) are those of karman3d_adjoint_cases.py / buoyancy3d_cases.py.  The Reynolds numbers
are replaced so that the single stencil is UNSTABLE: re_b = float32(X^2 / ALPHAS[b]), alpha = 0.45 and 0.3, both beyond the bound 1/6 --
a surface that ignores the parameter computes something else entirely.

The step's gradient jumps where a departure point crosses a cell boundary; the diffusion moves the departure points, so which (case, n,
steps) are usable is MEASURED: test_karman3d_diffusion_substeps_cpu.py runs the reference in float32 against float64 on every case below
and refuses a case whose density or velocity gradients sit more than 1e-4 apart (a flipped cell: 16_* and 32_x35 with n = 3 are).  Its
docstring lists the figures; the pins below are the worst figure times about 2.5 and the GPU tests allow MARGIN times the pin."""
import functools
import os
import sys

import numpy as np
import torch

import sol_oracle3d as o

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buoyancy3d_cases as bc
import karman3d_adjoint_cases as kc

ALPHAS = (0.45, 0.3)                  # dt res^2 / re of simulation 0 and 1: both beyond the single stencil's bound 1/6
FORCE = bc.FORCES[1]                  # the buoyant case: (0.3, -0.2, 0.15)
MARGIN = bc.MARGIN
maxrel = bc.maxrel
NAMES = kc.NAMES

# fields of one step: (case, n)
FIELD_CASES = tuple((name, n) for name in bc.FORWARD_CASES for n in (3, 5))
# gradients (loss = density + velocity cotangents): (case, n, chained steps, force) -- the clean rows of the measurement
GRAD_CASES = (("20_comb", 3, 1, None), ("20_comb", 5, 1, None), ("16_comb", 5, 2, None), ("16_before", 5, 2, None),
              ("16_dirichlet", 5, 2, None), ("20_comb", 5, 2, None), ("20_comb", 5, 1, FORCE), ("16_comb", 5, 2, FORCE), ("32_x35", 5, 2, FORCE),
              ("32_x35_a9", 6, 2, None))
# A row of GRAD_CASES has its g_re asserted, so it must be well conditioned in fp32: kappa 2^-24 < RE_PIN (re_condition, from the float64
# reference alone; the CPU twin asserts it for every row: kappa 21 .. 117).  One step of 32_x35 is not, at any alpha and n tried (alpha 0.2
# .. 1.2, n 4 .. 9: kappa 193 .. 5476, at alpha 0.45, n = 5 the terms cancel to 1 / 5476 of their magnitude), so the 32 x 16 x 16 rows that
# carry g_re are two chained steps: with the force, and without it at alpha = 0.9, n = 6 ("32_x35_a9": kappa 65, no flipped cell).
# GRAD_CASES_NO_RE: rows kept for their fields and their density and velocity gradients alone, run with re_grad off
GRAD_CASES_NO_RE = (("32_x35", 5, 1, None),)
CASE_ALPHAS = {"32_x35_a9": (0.9,)}   # a case name of this module = a karman3d_adjoint_cases case with other Reynolds numbers
CG_CASE = ("16_wall", 5, 2, None)     # a scene the direct solve does not take: buoyancy3d_cases.wall_mask at 16 x 8 x 8, pressure_solver="cg"

# the pre-diffusion alone: (Y, X, Z), B = 3; the last shape ends inside a tile on every axis for any tile of 4 .. 32 faces a side
PRE_SHAPES = ((16, 8, 8), (20, 10, 10), (18, 10, 70), (17, 11, 37))
PRE_B = 3
PRE_ALPHAS = (0.45, 0.3, 0.9)
STABILITY = dict(shape=(16, 8, 8), alpha=0.45, steps=40, n=3, seed=kc.SEED)

# float32 against float64 of the reference (maxrel), measured by test_karman3d_diffusion_substeps_cpu.py: the worst figure times about 2.5
PRE_PIN = 1.3e-6                      # the pre-diffusion alone (worst 5.3e-7)
FIELD_PIN, GRAD_PIN, RE_PIN = 2.7e-6, 8e-6, 1e-5      # worst 1.1e-6, 4.7e-6 (3.2e-6 but for g_d of 32_x35_a9: the pin was not widened for it), 3.7e-6


def re_of(X, batch, alphas=ALPHAS):
    """[batch] float64 holding fp32 values: re_b = X^2 / alphas[b]"""
    return torch.tensor([float(np.float32(X * X / alphas[b % len(alphas)])) for b in range(batch)], dtype=torch.float64)


def pre_diffuse(v, re, res, n, dt=1.0):
    """M^(n-1) (vy, vx, vz), M = I + (dt res^2 / (n re)) L"""
    a = (dt * res * res / (n * re)).reshape(-1, 1, 1, 1)
    v = tuple(v)
    for _ in range(n - 1):
        v = tuple(c + a * o.laplace_replicate(c) for c in v)
    return v


def sub_step(d, v, re, geom, n, force=None, dt=1.0, **kw):
    """one step with n diffusion substeps (force: the buoyant step)"""
    v = pre_diffuse(v, re, geom.X, n, dt)
    if force is None:
        return o.karman3d_step(d, v, re * n, geom, dt=dt, **kw)
    return bc.buoyant_step(d, v, re * n, geom, force, dt=dt, **kw)


# ---- the pre-diffusion alone ----------------------------------------------------------------------------------------------------------
def pre_inputs(shape, seed=7, dtype=torch.float64):
    """seeded normal (vy, vx, vz) [PRE_B, ...] of magnitude ~1 (every mode of the stencil is present) and re: fp32 values"""
    Y, X, Z = shape
    gen = torch.Generator().manual_seed(seed)
    v = tuple(torch.randn(PRE_B, *s, generator=gen, dtype=torch.float64).float().to(dtype) for s in ((Y + 1, X, Z), (Y, X + 1, Z), (Y, X, Z + 1)))
    return v, re_of(X, PRE_B, PRE_ALPHAS).to(dtype)


@functools.lru_cache(maxsize=None)
def pre_reference(shape, n, seed=7, dtype=torch.float64):
    v, re = pre_inputs(shape, seed, dtype)
    return tuple(t.double() for t in pre_diffuse(v, re, shape[1], n))


# ---- the step ---------------------------------------------------------------------------------------------------------------------------
def wall_geometry(Y, X, Z):
    """the oracle's geometry with buoyancy3d_cases.wall_mask as its `active` (masks and pressure diagonal re-derived as the class does)"""
    g = o.Karman3DGeometry(Y, X, Z)
    act = bc.wall_mask(Y, X, Z)
    acc = np.pad(act, 1, mode="edge")
    c = slice(1, -1)
    nacc = (acc[:-2, c, c] + acc[2:, c, c] + acc[c, :-2, c] + acc[c, 2:, c] + acc[c, c, :-2] + acc[c, c, 2:])
    g.active, g.obstacle, g.masks, g.diag = act, 1.0 - act, bc.face_masks(act), np.minimum(-nacc, -1.0)
    return g


def base(name):
    """the karman3d_adjoint_cases case whose inputs a case of this module takes"""
    return {"16_wall": "16_comb", "32_x35_a9": "32_x35"}.get(name, name)


@functools.lru_cache(maxsize=None)
def case(name):
    """karman3d_adjoint_cases.case; "16_wall": 16_comb's inputs in the wall_mask scene; "32_x35_a9": 32_x35's at alpha = 0.9"""
    return kc.case(base(name))


@functools.lru_cache(maxsize=None)
def geometry(name):
    return wall_geometry(*case(name)["shape"][1:]) if name == "16_wall" else kc.geometry(base(name))


@functools.lru_cache(maxsize=None)
def state(name):
    """(d, (vy, vx, vz), re): karman3d_adjoint_cases.state with this module's Reynolds numbers.  Shared, never modified."""
    d, v, _ = kc.state(base(name))
    B, _, X, _ = case(name)["shape"]
    return d, v, re_of(X, B, CASE_ALPHAS.get(name, ALPHAS))


def w_dens(name):
    """the density cotangent, masked with the scene's `active` as in karman3d_adjoint_cases"""
    if name == "16_wall":
        gen = torch.Generator().manual_seed(3)
        B, Y, X, Z = case(name)["shape"]
        w = torch.randn(B, Y, X, Z, generator=gen, dtype=torch.float64).float().double()
        return w * torch.as_tensor(geometry(name).active, dtype=torch.float64)
    return kc.w_dens(base(name))


def w_vel(name):
    return kc.w_vel(base(name))


@functools.lru_cache(maxsize=None)
def reference(name, n, steps=1, force=None, dtype=torch.float64):
    """The reference's autograd through `steps` chained steps with n substeps, loss = <d, w_dens> + sum_c <v_c, w_c>  ->  ((d, vy, vx, vz)
    after the last step, (g_d, g_vy, g_vx, g_vz, g_re) with respect to the initial state and re), float64 tensors.  Cached, shared, never
    modified."""
    c = case(name)
    d, v, re = state(name)
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in (d, *v, re)]
    cd, cv = leaves[0], tuple(leaves[1:4])
    for _ in range(steps):
        cd, cv = sub_step(cd, cv, leaves[4], geometry(name), n, force, dt=c["dt"], **c["kw"])
    loss = (cd * w_dens(name).to(dtype)).sum() + sum((a * w.to(dtype)).sum() for a, w in zip(cv, w_vel(name)))
    loss.backward()
    return (tuple(t.detach().double() for t in (cd, *cv)), tuple(p.grad.double() for p in leaves))


def re_condition(name, n, steps=1, force=None):
    """How well g_re of a case is conditioned in ANY fp32 evaluation, from the float64 reference alone: per simulation
        kappa_b = sum_e |g'_e (L u)_e| / |sum_e g'_e (L u)_e|
    over the faces of the three components and the chained steps, u = M^(n-1) v the pre-diffused velocity and g' the cotangent of
    u + a L u -- the terms the library's reduction adds (g_re = -n a / re times that sum).  One rounding of each term (2^-24), aligned,
    already moves g_re by kappa 2^-24 relative; a relative error of the cotangent (the fp32 pressure solve's, which the reference in
    float32 does not have: its solve runs in float64) is amplified by the same factor.  The step is composed here from the oracle's stages
    as o.karman3d_step / buoyancy3d_cases.buoyant_step compose it, with the diffused field as a graph node; fields and g_re are asserted
    equal to reference()'s.  -> [kappa_b]"""
    c, g = case(name), geometry(name)
    d, v, re = state(name)
    dt = c["dt"]
    a = (dt * g.X ** 2 / (n * re)).reshape(-1, 1, 1, 1)
    order, grad_pad = c["kw"].get("inflow_order", "after"), c["kw"].get("grad_pad", "replicate")
    cd, cv = d, tuple(t.clone().requires_grad_(True) for t in v)
    keep = []
    for _ in range(steps):
        u = pre_diffuse(cv, re, g.X, n, dt)
        lap = [o.laplace_replicate(t) for t in u]
        diff = [t + a * l for t, l in zip(u, lap)]
        for t in diff:
            t.retain_grad()
        keep.append((diff, [l.detach() for l in lap]))
        m = o._t(g.bc_mask, diff[0])
        cc = (diff[0] * (1.0 - m) + m, diff[1], diff[2])
        infl = o._t(g.inflow, cc[0])
        d2, adv = o.advect_mac(cd + infl if order == "before" else cd, cc, dt, g.dx)
        if order == "after":
            d2 = d2 + infl * dt
        if force is not None:
            adv = tuple(ac + (dt * fc) * avg for ac, fc, avg in zip(adv, force, bc.face_average(d2)))
        cd, cv = d2, o.project(adv, g, grad_pad=grad_pad)
    ref_out, ref_g = reference(name, n, steps, force)
    assert max(maxrel(x, y) for x, y in zip((cd, *cv), ref_out)) < 1e-12
    ((cd * w_dens(name)).sum() + sum((x * w).sum() for x, w in zip(cv, w_vel(name)))).backward()
    B = d.shape[0]
    num, net = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    for diff, lap in keep:
        for t, l in zip(diff, lap):
            p = (t.grad * l).reshape(B, -1)
            num += p.abs().sum(1)
            net += p.sum(1)
    assert maxrel(-(dt * g.X ** 2 / (re * re)) * net, ref_g[4]) < 1e-10
    return (num / net.abs()).tolist()


def stability_run(n, dtype=torch.float64):
    """max|v| before and after STABILITY['steps'] steps without a network at alpha = STABILITY['alpha'] -> (initial, final)"""
    Y, X, Z = STABILITY["shape"]
    g = o.geometry(Y, X, Z)
    d, v = o.synthetic_state(1, Y, X, Z, STABILITY["seed"])
    d, v = d.float().to(dtype), tuple(t.float().to(dtype) for t in v)
    re = re_of(X, 1, (STABILITY["alpha"],)).to(dtype)
    first = max(float(t.abs().max()) for t in v)
    with torch.no_grad():
        for _ in range(STABILITY["steps"]):
            d, v = sub_step(d, v, re, g, n)
            if not all(bool(torch.isfinite(t).all()) for t in v):
                return first, float("inf")
    return first, max(float(t.abs().max()) for t in v)


# ---- trainer and roll-out: buoyancy3d_cases.trainer_problem with unstable Reynolds numbers ---------------------------------------------
TRAINER_SHAPE, TRAINER_STD_V, TRAINER_N = bc.TRAINER_SHAPE, bc.TRAINER_STD_V, 4
# float32 against float64 of the reference's unrolled loss on this problem (test_karman3d_diffusion_substeps_cpu.py): worst times about 2.5
# (loss and per-step losses relative; weight gradient, its worst layer and the final state in relative L2: worst 6.3e-8, 8.1e-7, 1.8e-5, 1.2e-6)
TRAINER_LOSS_PIN, TRAINER_GRAD_PIN, TRAINER_LAYER_PIN, TRAINER_FINAL_PIN = 1.6e-7, 2e-6, 4.5e-5, 3e-6


def unrolled_loss(params, d, v, re, gts, geom, std_v, std_re, n):
    """o.unrolled_loss with n diffusion substeps: (loss, per-step losses, (d, v) after the last corrected step)"""
    losses = []
    for gt in gts:
        d, v = sub_step(d, v, re, geom, n)
        c = o.correction(params, v, re, std_v, std_re)
        v = tuple(a + b for a, b in zip(v, c))
        losses.append(sum(0.5 * (((g - a) / s) ** 2).sum() for g, a, s in zip(gt, v, std_v)))
    return torch.stack(losses).sum() / len(gts), losses, (d, v)


def trainer_problem(ms=2):
    p = bc.trainer_problem(ms)
    p["re"] = re_of(TRAINER_SHAPE[2], TRAINER_SHAPE[0])
    return p


@functools.lru_cache(maxsize=None)
def trainer_reference(n=TRAINER_N, ms=2, dtype=torch.float64):
    """(loss, per-step losses, flat weight gradient, (d, vy, vx, vz) after the last step) of unrolled_loss on trainer_problem in `dtype`"""
    p = trainer_problem(ms)
    cast = lambda t: t.to(dtype)
    params = [cast(q).clone().requires_grad_(True) for q in p["params"]]
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        loss, losses, (d, v) = unrolled_loss(params, cast(p["d"]), tuple(cast(t) for t in p["v"]), cast(p["re"]),
                                             [tuple(cast(t) for t in g) for g in p["gts"]], p["g"], TRAINER_STD_V, o.STD_RE, n)
        loss.backward()
    finally:
        torch.set_default_dtype(prev)
    return (float(loss.detach()), [float(l.detach()) for l in losses], torch.cat([q.grad.reshape(-1) for q in params]).double(),
            tuple(t.detach().double() for t in (d, *v)))


def rollout_reference(params, d, v, re, geom, std_v, std_re, n, nsteps):
    """nsteps x [step with n substeps -> correction -> add] -> (d, v)"""
    with torch.no_grad():
        for _ in range(nsteps):
            d, v = sub_step(d, v, re, geom, n)
            c = o.correction(params, v, re, std_v, std_re)
            v = tuple(a + b for a, b in zip(v, c))
    return d, v
