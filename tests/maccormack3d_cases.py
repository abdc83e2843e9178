"""Float64 reference, inputs and cached reference results of the karman-3d MacCormack advection tests (test_gpu_karman3d_maccormack.py and
its CPU twin test_karman3d_maccormack_cpu.py).  A plain module: importing it touches no device.

The reference step is o.diffuse_bc -> the definition of include/sol_hip.h ("MACCORMACK ADVECTION on the karman-3d step"), written with the
oracle's own o._points / o._local / o._sample and a twin of o._sample that also returns the min / max of the eight values it read -> (the
buoyancy term: buoyancy3d_cases.face_average) -> o.project; diffusion_substeps3d_cases.pre_diffuse in front for n substeps.  With c the
post-diffusion velocity, f one advected array, u = c at the array's sample points, S_g the trilinear sample of g in the array's mode:
    h = S_f(x - u dt),  b = S_h(x + u dt),  cor = h + (s / 2)(f - b),  out = cor where lo <= cor <= hi else h
Gradients are float64 autograd; torch.where freezes the limiter's decision, floor and clamp freeze themselves.

States and cotangents are those of karman3d_adjoint_cases (state, w_dens, w_vel; its own Reynolds numbers) and
diffusion_substeps3d_cases.wall_geometry ("16_wall").  The limiter and the clamped edges tie exactly in places and fp32 decides a few
entries the other way, so EVERY MacCormack gradient comparison uses the trimmed metric of large2d_scenes with the cap as a condition
(k <= int(TRIM n)).  Which (case, s, steps, force, n) are usable is MEASURED: test_karman3d_maccormack_cpu.py runs this reference in
float32 against float64 on every row of STEP_CASES and refuses a row whose fields sit further than FIELD_ADMIT apart or whose trimmed
gradients sit further than GRAD_ADMIT apart (a fifth of the GPU bounds TOL_FIELD / TOL_GRAD); a row's g_re is asserted only where the
row says so (RE_ADMIT).  Its docstring lists the figures."""
import functools
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

import sol_oracle3d as o

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buoyancy3d_cases as bc
import diffusion_substeps3d_cases as ds
import karman3d_adjoint_cases as kc
from large2d_scenes import TOL_FIELD, TOL_GRAD, TRIM, trimmed_rel      # noqa: F401  (the GPU bounds and the metric, re-exported)

FIELD_ADMIT, GRAD_ADMIT, RE_ADMIT = 2e-6, 2e-5, 2e-5      # float32 against float64 of the reference: what a usable case stays within
FORCE = bc.FORCES[1]                  # the buoyant composition: (0.3, -0.2, 0.15)
STRENGTHS = (1.0, 0.5)
NAMES = kc.NAMES
MARGIN = bc.MARGIN

# (case, s, chained steps, force, n, g_re asserted) -- the usable rows; the float32 reference holds g_re within RE_ADMIT on every one of
# them (worst: 20_comb at 1.9e-5), so every row asserts it.  NOT usable (a limiter decision flips in float32): two chained
# steps of 32_x35 (fields 5.7e-4 apart) and of 16_comb with the force (4.7e-4), two chained steps of 20_comb (trimmed gradient 5e-5), the
# substep suite's unstable Reynolds numbers (2.4e-5 .. 7e-5).
STEP_CASES = (
    ("16_comb", 1.0, 1, None, 1, True), ("16_comb", 0.5, 1, None, 1, True), ("16_before", 1.0, 1, None, 1, True),
    ("16_dirichlet", 1.0, 1, None, 1, True), ("20_comb", 1.0, 1, None, 1, True), ("32_x35", 1.0, 1, None, 1, True),
    ("32_cfl", 1.0, 1, None, 1, True), ("16_wall", 1.0, 1, None, 1, True), ("16_lowre", 1.0, 1, None, 1, True),
    ("16_comb", 1.0, 1, FORCE, 1, True), ("32_x35", 1.0, 1, FORCE, 1, True), ("16_lowre", 1.0, 1, FORCE, 3, True),
    ("16_comb", 1.0, 2, None, 1, True), ("16_lowre", 1.0, 2, None, 1, True), ("16_comb", 0.5, 2, None, 1, True),
    ("16_wall", 1.0, 2, FORCE, 1, True),
)
KIND_CASE = ("16_comb", 1.0, 1, None, 1, True)   # the row that runs with the three kinds of loss and the gradient modes on and off
KINDS = bc.KINDS


def case_id(row):
    name, s, steps, force, n, _ = row
    return "%s-s%g-x%d%s%s" % (name, s, steps, "-force" if force is not None else "", "-n%d" % n if n > 1 else "")


def sample_minmax(fld, loc, mode):
    """o._sample(fld, loc, mode) for mode "replicate" / "zero", and the min and max of the eight values it read (after clamping; the zeros
    of the ghost ring count)"""
    if mode == "zero":
        fld = F.pad(fld, (1, 1, 1, 1, 1, 1))
        loc = tuple(l + 1.0 for l in loc)
    elif mode != "replicate":
        raise ValueError(mode)
    Bn, n = fld.shape[0], fld.shape[1:]
    fl = [torch.floor(l) for l in loc]
    w = [l - f for l, f in zip(loc, fl)]
    idx = [(f.long().clamp(0, m - 1), (f.long() + 1).clamp(0, m - 1)) for f, m in zip(fl, n)]
    flat, shp = fld.reshape(Bn, -1), loc[0].shape
    out, vals = 0.0, []
    for a in (0, 1):                  # (o._sample's own loop: the semi-Lagrangian branch below equals o.advect_mac exactly)
        for b in (0, 1):
            for c in (0, 1):
                lin = (idx[0][a] * n[1] + idx[1][b]) * n[2] + idx[2][c]
                val = torch.gather(flat, 1, lin.reshape(Bn, -1)).reshape(shp)
                wt = (w[0] if a else 1 - w[0]) * (w[1] if b else 1 - w[1]) * (w[2] if c else 1 - w[2])
                out = out + wt * val
                vals.append(val)
    eight = torch.stack(vals)
    return out, eight.min(dim=0).values, eight.max(dim=0).values


def advect(d, v, dt, dx, s=1.0, scheme="mac_cormack", stats=None):
    """(d, (c_y, c_x, c_z)) advected by c: the definition above for scheme "mac_cormack", o.advect_mac's values for "semi_lagrangian".  d
    may be None.  stats (a list): receives the share of entries the limiter reverted, per array."""
    Bn = v[0].shape[0]
    n = (v[1].shape[1], v[0].shape[2], v[0].shape[3])
    out = []
    for kind, f, mode in (("c", d, "zero"), (0, v[0], "replicate"), (1, v[1], "replicate"), (2, v[2], "replicate")):
        if f is None:
            out.append(None)
            continue
        p = [q.unsqueeze(0).expand(Bn, -1, -1, -1) for q in o._points(kind, n, dx, v[0])]
        u = [o._sample(v[a], o._local(a, p, dx), "replicate") for a in range(3)]
        h, lo, hi = sample_minmax(f, o._local(kind, [p[a] - u[a] * dt for a in range(3)], dx), mode)
        if scheme == "semi_lagrangian":
            out.append(h)
            continue
        b = o._sample(h, o._local(kind, [p[a] + u[a] * dt for a in range(3)], dx), mode)
        cor = h + (0.5 * s) * (f - b)
        keep = (lo <= cor) & (cor <= hi)
        if stats is not None:
            stats.append(1.0 - float(keep.double().mean()))
        out.append(torch.where(keep, cor, h))
    return out[0], tuple(out[1:])


def stage(d, c, g, s=1.0, scheme="mac_cormack", inflow_order="after", dt=1.0, stats=None):
    """the stage as sol_karman3d_advect runs it: inflow before / after, velocity times the hard-BC face masks (g.masks)"""
    infl = o._t(g.inflow, c[0])
    d2, a = advect(d + infl if inflow_order == "before" else d, c, dt, g.dx, s, scheme, stats)
    if inflow_order == "after":
        d2 = d2 + infl * dt
    return d2, tuple(ac * o._t(m, c[0]) for ac, m in zip(a, g.masks))


def step(d, v, re, g, s=1.0, scheme="mac_cormack", force=None, n=1, dt=1.0, grad_pad="replicate", inflow_order="after", stats=None):
    """one solver step with the chosen advection (force: the buoyancy term of buoyancy3d_cases; n: diffusion substeps)"""
    if n > 1:
        v = ds.pre_diffuse(v, re, g.X, n, dt)
        re = re * n
    c = o.diffuse_bc(v, re, g.X, dt, g)
    infl = o._t(g.inflow, v[0])
    d2, a = advect(d + infl if inflow_order == "before" else d, c, dt, g.dx, s, scheme, stats)
    if inflow_order == "after":
        d2 = d2 + infl * dt
    if force is not None:
        a = tuple(ac + (dt * fc) * avg for ac, fc, avg in zip(a, force, bc.face_average(d2)))
    return d2, o.project(a, g, grad_pad=grad_pad)


def state(name):
    """(d, (vy, vx, vz), re) of a case: karman3d_adjoint_cases' state ("16_wall": 16_comb's) with ITS Reynolds numbers"""
    return kc.state(ds.base(name))


@functools.lru_cache(maxsize=None)
def reference(name, s=1.0, steps=1, force=None, n=1, kind="both", scheme="mac_cormack", dtype=torch.float64):
    """The reference's autograd through `steps` chained steps -> ((d, vy, vx, vz) after the last step, (g_d, g_vy, g_vx, g_vz, g_re) with
    respect to the initial state and re, the limiter's reverted shares), float64 tensors.  kind: "dens" (loss = <d, w_dens>), "vel"
    (sum_c <v_c, w_c>) or "both".  Cached: computed once, shared, never modified."""
    c, g = ds.case(name), ds.geometry(name)
    d, v, re = state(name)
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in (d, *v, re)]
    cd, cv = leaves[0], tuple(leaves[1:4])
    stats = []
    for _ in range(steps):
        cd, cv = step(cd, cv, leaves[4], g, s, scheme, force, n, dt=c["dt"], stats=stats, **c["kw"])
    loss = 0.0
    if kind in ("dens", "both"):
        loss = loss + (cd * ds.w_dens(name).to(dtype)).sum()
    if kind in ("vel", "both"):
        loss = loss + sum((a * w.to(dtype)).sum() for a, w in zip(cv, ds.w_vel(name)))
    loss.backward()
    zero = lambda p: torch.zeros_like(p) if p.grad is None else p.grad
    return tuple(t.detach().double() for t in (cd, *cv)), tuple(zero(p).double() for p in leaves), tuple(stats)


# ---- the stage alone: seeded normal fields ----
STAGE_SHAPES = ((16, 8, 8), (20, 10, 10), (17, 11, 37), (18, 10, 70))      # minimum; tiles that end inside; ragged on every axis; Z > 64: two lane passes
STAGE_B = 3
# (shape, s, inflow order, CFL or None = about one cell per step as drawn): both strengths and both inflow orders at every shape, one run
# scaled to CFL 2.5
STAGE_CASES = tuple((sh, s, order, None) for sh in STAGE_SHAPES for s, order in ((1.0, "after"), (0.5, "before"))) + (((20, 10, 10), 1.0, "after", 2.5),)
STAGE_DX = 2.0                        # the stage's cell size: see stage_geometry


def stage_id(c):
    return "%dx%dx%d-s%g-%s%s" % (*c[0], c[1], c[2], "" if c[3] is None else "-cfl%g" % c[3])


@functools.lru_cache(maxsize=None)
def stage_geometry(Y, X, Z):
    """what the stage reads of a scene, for any Y x X x Z: dx, a block obstacle, an inflow patch and the hard-BC face masks.
    dx = STAGE_DX = 2, a power of two (the scene's length is 2 X): the reference samples at PHYSICAL coordinates, and with the scenes'
    dx = 100 / X its float32 run rounds the sample points, x - u dt and the division by dx -- at Z = 37 and 70 that alone put its fields
    2.2e-6 .. 3.1e-6 from float64, beyond FIELD_ADMIT.  With a power of two the points and the division are exact and the one rounding of
    x - u dt is left (<= 1.8e-6 at Z = 70).  The kernels read dt / dx alone (0.5 here; the step cases run 100 / X)."""
    active = np.ones((Y, X, Z))
    active[Y // 3:Y // 3 + max(2, Y // 8), X // 4:X // 4 + max(2, X // 6), Z // 3:Z // 3 + max(2, Z // 5)] = 0.0
    inflow = np.zeros((Y, X, Z))
    inflow[1:max(3, Y // 10), X // 4:3 * X // 4, Z // 4:3 * Z // 4] = 1.0
    return types.SimpleNamespace(Y=Y, X=X, Z=Z, dx=STAGE_DX, length=STAGE_DX * X, active=active, inflow=inflow, masks=bc.face_masks(active))


def stage_inputs(shape, cfl=None, seed=23, B=STAGE_B, dtype=torch.float64):
    """seeded normal (d, c_y, c_x, c_z) [B, ...] and cotangents (g_d, g_ay, g_ax, g_az): fp32 values.  The velocity has magnitude ~1 cell
    per step (CFL up to ~4 at the tails); cfl: multiplied so that max |c| dt/dx is that number"""
    Y, X, Z = shape
    gen = torch.Generator().manual_seed(seed)
    shapes = ((B, Y, X, Z), (B, Y + 1, X, Z), (B, Y, X + 1, Z), (B, Y, X, Z + 1))
    t = [torch.randn(*sh, generator=gen, dtype=torch.float64) for sh in shapes + shapes]
    dx = stage_geometry(Y, X, Z).dx
    scale = dx if cfl is None else cfl * dx / max(float(c.abs().max()) for c in t[1:4])
    return tuple(x.float().to(dtype) for x in (t[0], t[1] * scale, t[2] * scale, t[3] * scale, *t[4:]))


@functools.lru_cache(maxsize=None)
def stage_reference(shape, s=1.0, inflow_order="after", cfl=None, scheme="mac_cormack", dtype=torch.float64):
    """((d_out, a_y, a_x, a_z), (g_d, g_cy, g_cx, g_cz), reverted shares) of the stage on stage_inputs, float64 tensors; cached"""
    g = stage_geometry(*shape)
    d, cy, cx, cz, *w = stage_inputs(shape, cfl, dtype=dtype)
    leaves = [t.clone().requires_grad_(True) for t in (d, cy, cx, cz)]
    stats = []
    d2, a = stage(leaves[0], tuple(leaves[1:]), g, s, scheme, inflow_order, stats=stats)
    sum((x * y).sum() for x, y in zip((d2, *a), w)).backward()
    return tuple(t.detach().double() for t in (d2, *a)), tuple(p.grad.double() for p in leaves), tuple(stats)


# ---- the blob experiment: what the scheme is for ----
BLOB = dict(N=32, sigma=3.0, u=(0.37, 0.21, 0.13), start=(9.0, 10.0, 11.0), steps=40)
BLOB_PEAKS = {"semi_lagrangian": 0.431, "mac_cormack": 0.829}      # float64, to three digits (pinned by the CPU twin)


def blob_inputs(dtype=torch.float64):
    """a Gaussian density blob in a uniform flow on an obstacle-free box, dx = 1: (d [1,N,N,N], (c_y, c_x, c_z))"""
    N, sig, (y0, x0, z0) = BLOB["N"], BLOB["sigma"], BLOB["start"]
    jj, ii, kk = torch.meshgrid(*(torch.arange(N, dtype=torch.float64),) * 3, indexing="ij")
    d = torch.exp(-((jj - y0) ** 2 + (ii - x0) ** 2 + (kk - z0) ** 2) / (2 * sig * sig)).reshape(1, N, N, N)
    c = tuple(torch.full(sh, u, dtype=torch.float64) for sh, u in zip(((1, N + 1, N, N), (1, N, N + 1, N), (1, N, N, N + 1)), BLOB["u"]))
    return d.float().to(dtype), tuple(t.float().to(dtype) for t in c)


@functools.lru_cache(maxsize=None)
def blob_peak(scheme):
    """the peak the blob keeps after BLOB["steps"] steps in float64"""
    d, c = blob_inputs()
    for _ in range(BLOB["steps"]):
        d = advect(d, c, 1.0, 1.0, 1.0, scheme)[0]
    return float(d.max())


# ---- trainer and roll-out: buoyancy3d_cases.trainer_problem with the MacCormack step, SOL-2 ------------------------------------------
TRAINER_SHAPE, TRAINER_STD_V = bc.TRAINER_SHAPE, bc.TRAINER_STD_V
# float32 against float64 of the reference's unrolled loss on this problem (test_karman3d_maccormack_cpu.py): the worst times about 2.5
# (loss and per-step losses relative; weight gradient, its worst layer and the final state in relative L2)
# worst 3.6e-7 / 5.7e-7, 4.6e-6, 4.5e-5, 1.4e-4 -- the final state carries entries whose limiter decision float32 takes the other way
TRAINER_LOSS_PIN, TRAINER_GRAD_PIN, TRAINER_LAYER_PIN, TRAINER_FINAL_PIN = 1.5e-6, 1.2e-5, 1.1e-4, 3.5e-4


def unrolled_loss(params, d, v, re, gts, geom, std_v, std_re, s=1.0):
    """o.unrolled_loss with the MacCormack step: (loss, per-step losses, (d, v) after the last corrected step)"""
    losses = []
    for gt in gts:
        d, v = step(d, v, re, geom, s)
        c = o.correction(params, v, re, std_v, std_re)
        v = tuple(a + b for a, b in zip(v, c))
        losses.append(sum(0.5 * (((g - a) / sd) ** 2).sum() for g, a, sd in zip(gt, v, std_v)))
    return torch.stack(losses).sum() / len(gts), losses, (d, v)


@functools.lru_cache(maxsize=None)
def trainer_reference(s=1.0, ms=2, dtype=torch.float64):
    """(loss, per-step losses, flat weight gradient, (d, vy, vx, vz) after the last step) of unrolled_loss on bc.trainer_problem in `dtype`"""
    p = bc.trainer_problem(ms)
    cast = lambda t: t.to(dtype)
    params = [cast(q).clone().requires_grad_(True) for q in p["params"]]
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        loss, losses, (d, v) = unrolled_loss(params, cast(p["d"]), tuple(cast(t) for t in p["v"]), cast(p["re"]),
                                             [tuple(cast(t) for t in g) for g in p["gts"]], p["g"], TRAINER_STD_V, o.STD_RE, s)
        loss.backward()
    finally:
        torch.set_default_dtype(prev)
    return (float(loss.detach()), [float(l.detach()) for l in losses], torch.cat([q.grad.reshape(-1) for q in params]).double(),
            tuple(t.detach().double() for t in (d, *v)))


def rollout_reference(params, d, v, re, geom, std_v, std_re, s, nsteps):
    """nsteps x [MacCormack step -> correction -> add] -> (d, v)"""
    with torch.no_grad():
        for _ in range(nsteps):
            d, v = step(d, v, re, geom, s)
            c = o.correction(params, v, re, std_v, std_re)
            v = tuple(a + b for a, b in zip(v, c))
    return d, v


def layer_slices(params):
    """the flat weight gradient's slice of every parameter tensor"""
    out, at = [], 0
    for q in params:
        out.append(slice(at, at + q.numel()))
        at += q.numel()
    return out
