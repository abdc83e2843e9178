"""Float64 reference, scenes, states and cases of the periodic karman-2d tests (test_gpu_karman2d_periodic.py and its CPU twin
test_karman2d_periodic_cpu.py).  A plain module: importing it touches no device.

periodic_step restates the step of include/sol_hip.h ("Forward step for grids beyond the one-workgroup kernels", "PERIODIC BOUNDARIES")
in torch, differentiable by autograd: the oracle's step (sol_oracle.karman_step, which the CPU twin ties it to at periodic = (False,
False)) with every clamped or zero-ghost index taken modulo n over the unique planes of a periodic axis.  Array shapes are the open
step's: on a periodic axis the last face plane is a duplicate of plane 0 -- never read on input, written equal to plane 0 on output.
The pressure solve is a float64 solve of precond.scene_matrix(active, periodic): dense up to DENSE_MAX cells, above that the sparse LU
of the SAME matrix (a dense inverse of the 8450 cells of 130 x 65 would take minutes); doubly periodic: the singular system is solved
for the zero-mean pressure of the mean-free right-hand side (one cell pinned, then the mean removed -- the pseudo-inverse).

Tolerances, batch size, metrics and generators are large2d_scenes' (TOL_FIELD, TOL_GRAD, TRIM, rel, trimmed_rel, cotangent_at, cfl_scaled).
"""
import functools
import os
import sys

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla
import torch

import sol_oracle as o
from sol_amd import precond

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diffusion_substeps_cases as _ds
from large2d_scenes import TOL_FIELD, TOL_GRAD, TRIM, cfl_scaled, cotangent_at, geometry, rel, trimmed_rel  # noqa: F401

B = 2
DENSE_MAX = 1024
OPEN, PER = "open", "periodic"


# ---- index helpers ---------------------------------------------------------------------------------------------------------------------
def _map(idx, n, periodic):
    """an index along an axis of n unique planes: modulo n when periodic, clamped to [0, n - 1] when open"""
    return idx % n if periodic else idx.clamp(0, n - 1)


def _shift(f, dim, s, periodic):
    n = f.shape[dim]
    return f.index_select(dim, _map(torch.arange(n) + s, n, periodic))


def _lap(f, periodic):
    """5-point Laplacian of f [B,H,W] (unique planes): wrapped along a periodic axis, replicate padded along an open one"""
    py, px = periodic
    return _shift(f, 1, 1, py) + _shift(f, 1, -1, py) + _shift(f, 2, 1, px) + _shift(f, 2, -1, px) - 4.0 * f


def _at(f, jj, ii):
    """f [B,H,W] at integer index tensors jj, ii [B,h,w] (already mapped into range)"""
    Bn, H, W = f.shape
    return torch.gather(f.reshape(Bn, -1), 1, (jj * W + ii).reshape(Bn, -1)).reshape(jj.shape)


def unique(vy, vx, periodic):
    """the unique planes of a staggered velocity: the duplicate plane of a periodic axis dropped"""
    py, px = periodic
    return (vy[:, :-1] if py else vy), (vx[:, :, :-1] if px else vx)


def with_duplicates(uy, ux, periodic):
    py, px = periodic
    return (torch.cat([uy, uy[:, :1]], 1) if py else uy), (torch.cat([ux, ux[:, :, :1]], 2) if px else ux)


def seam_sync(vy, vx, periodic):
    """plane 0 copied onto the duplicate plane (differentiable): the adjoint is the seam fold"""
    return with_duplicates(*unique(vy, vx, periodic), periodic)


def face_masks(active, periodic):
    """hard-BC face masks of the unique faces: my [UH,X], mx [Y,UW] (accessible = the active mask, wrapped / edge-extended)"""
    act = (np.asarray(active, dtype=np.float64) != 0).astype(np.float64)
    Y, X = act.shape
    acc = precond._accessible(act, periodic)
    my = acc[0:Y + 1, 1:X + 1] * acc[1:Y + 2, 1:X + 1]
    mx = acc[1:Y + 1, 0:X + 1] * acc[1:Y + 1, 1:X + 2]
    return (my[:-1] if periodic[0] else my), (mx[:, :-1] if periodic[1] else mx)


# ---- the pressure solve ----------------------------------------------------------------------------------------------------------------------
class _Solve(torch.autograd.Function):
    """p = M^+ rhs in float64 for the symmetric M = precond.scene_matrix(active, periodic); backward = the same solve"""

    @staticmethod
    def forward(ctx, rhs, solver):
        ctx.solver = solver
        Bn = rhs.shape[0]
        return torch.as_tensor(solver(rhs.detach().double().reshape(Bn, -1).numpy()), dtype=rhs.dtype).reshape(rhs.shape)

    @staticmethod
    def backward(ctx, g):
        return _Solve.apply(g, ctx.solver), None


def make_solver(active, periodic):
    """rows [B, N] -> M^+ rows, float64 numpy.  Dense (numpy.linalg.solve / lstsq) up to DENSE_MAX cells, else the sparse LU of the same
    matrix.  Doubly periodic: M is singular (constants); the zero-mean solution of the mean-free right-hand side."""
    act = np.asarray(active, dtype=np.float64)
    N = act.size
    M = precond.scene_matrix(act, periodic)
    singular = all(periodic)
    if N <= DENSE_MAX:
        if singular:
            Mp = np.linalg.pinv(M, hermitian=True)
            return lambda r: r @ Mp
        Mi = np.linalg.inv(M)
        return lambda r: r @ Mi.T
    Ms = sp.csc_matrix(M)
    del M
    if singular:
        lu = spla.splu(Ms[1:, 1:].tocsc())

        def solve(r):
            r = r - r.mean(axis=1, keepdims=True)
            p = np.concatenate([np.zeros((r.shape[0], 1)), lu.solve(r[:, 1:].T).T], axis=1)
            return p - p.mean(axis=1, keepdims=True)
        return solve
    lu = spla.splu(Ms)
    return lambda r: lu.solve(r.T).T


def solver_of(geom, periodic):
    key = "_periodic_solver_%d%d" % (int(periodic[0]), int(periodic[1]))
    if not hasattr(geom, key):
        setattr(geom, key, make_solver(geom.active, periodic))
    return getattr(geom, key)


# ---- the step --------------------------------------------------------------------------------------------------------------------------------
def periodic_step(d, vy, vx, re, geom, periodic=(False, False), dt=1.0, res=None, grad_pad="replicate", inflow_order="after",
                  return_pressure=False):
    """One solver step with the axes of `periodic` = (py, px) wrapped.  d [B,Y,X], vy [B,Y+1,X], vx [B,Y,X+1], re [B]; geom: an oracle
    KarmanGeometry (active, inflow, bc_mask -- velBCy = velBCyMask = bc_mask -- and dx are read)."""
    py, px = periodic = (bool(periodic[0]), bool(periodic[1]))
    Bn, Y, X = d.shape
    res = geom.X if res is None else res
    T = lambda a: torch.as_tensor(np.asarray(a), dtype=vy.dtype)
    uy, ux = unique(vy, vx, periodic)                   # [B,UH,X], [B,Y,UW]
    UH, UW = uy.shape[1], ux.shape[2]
    # diffusion + velocity BC
    alpha = (1.0 / re * dt * res * res).reshape(-1, 1, 1)
    m = T(geom.bc_mask)[:UH]
    cy = (uy + alpha * _lap(uy, periodic)) * (1.0 - m) + m
    cx = ux + alpha * _lap(ux, periodic)
    dtdx = dt / geom.dx
    ar = lambda n: torch.arange(n)

    def grid(h, w):
        jj, ii = torch.meshgrid(ar(h), ar(w), indexing="ij")
        return jj.unsqueeze(0).expand(Bn, -1, -1), ii.unsqueeze(0).expand(Bn, -1, -1)

    def bilinear(f, j, i, vy_pt, vx_pt, zero_ghost=False):
        """f [B,H,W] (unique planes) sampled at (j, i) - (vy_pt, vx_pt) dt/dx: floor and weights of the offset as the kernels form them"""
        H, W = f.shape[1:]
        oy, ox = -vy_pt * dtdx, -vx_pt * dtdx
        fy, fx = torch.floor(oy), torch.floor(ox)
        wy, wx = oy - fy, ox - fx
        j0, i0 = j + fy.long(), i + fx.long()
        out = 0.0
        for dj, bwy in ((0, 1.0 - wy), (1, wy)):
            for di, bwx in ((0, 1.0 - wx), (1, wx)):
                jj, ii = j0 + dj, i0 + di
                ok = torch.ones_like(wy)
                if zero_ghost:                      # the density: one ring of zero ghost cells along an OPEN axis
                    if not py:
                        ok = ok * ((jj >= 0) & (jj < H)).to(wy.dtype)
                    if not px:
                        ok = ok * ((ii >= 0) & (ii < W)).to(wy.dtype)
                out = out + bwy * bwx * ok * _at(f, _map(jj, H, py), _map(ii, W, px))
        return out

    # advecting velocity at the faces and the cell centres: face averages with wrapped / clamped neighbours
    jy, iy = grid(UH, X)
    u_x_at_y = 0.25 * (_at(cx, _map(jy - 1, Y, py), iy) + _at(cx, _map(jy - 1, Y, py), _map(iy + 1, UW, px)) +
                       _at(cx, _map(jy, Y, py), iy) + _at(cx, _map(jy, Y, py), _map(iy + 1, UW, px)))
    ay = bilinear(cy, jy, iy, cy, u_x_at_y)
    jx, ix = grid(Y, UW)
    u_y_at_x = 0.25 * (_at(cy, jx, _map(ix - 1, X, px)) + _at(cy, jx, _map(ix, X, px)) +
                       _at(cy, _map(jx + 1, UH, py), _map(ix - 1, X, px)) + _at(cy, _map(jx + 1, UH, py), _map(ix, X, px)))
    ax = bilinear(cx, jx, ix, u_y_at_x, cx)
    jc, ic = grid(Y, X)
    u_y_c = 0.5 * (_at(cy, jc, ic) + _at(cy, _map(jc + 1, UH, py), ic))
    u_x_c = 0.5 * (_at(cx, jc, ic) + _at(cx, jc, _map(ic + 1, UW, px)))
    infl = T(geom.inflow)
    d_src = d + infl if inflow_order == "before" else d
    d2 = bilinear(d_src, jc, ic, u_y_c, u_x_c, zero_ghost=True)
    if inflow_order == "after":
        d2 = d2 + infl * dt
    # projection
    my, mx = (T(a) for a in face_masks(geom.active, periodic))
    ay, ax = ay * my, ax * mx
    hi_y = ay.index_select(1, _map(ar(Y) + 1, UH, py))
    hi_x = ax.index_select(2, _map(ar(X) + 1, UW, px))
    div = (hi_y - ay[:, :Y]) + (hi_x - ax[:, :, :X])
    p = _Solve.apply(-div, solver_of(geom, periodic))        # M p = -div
    # face differences of p: wrapped along a periodic axis (no boundary face); along an open one zero (replicate) or +-p (dirichlet0)
    if py:
        gy = p - _shift(p, 1, -1, True)
    else:
        pad = torch.zeros_like(p[:, :1])
        inner = p[:, 1:] - p[:, :-1]
        gy = torch.cat([p[:, :1] if grad_pad == "dirichlet0" else pad, inner, -p[:, -1:] if grad_pad == "dirichlet0" else pad], 1)
    if px:
        gx = p - _shift(p, 2, -1, True)
    else:
        pad = torch.zeros_like(p[:, :, :1])
        inner = p[:, :, 1:] - p[:, :, :-1]
        gx = torch.cat([p[:, :, :1] if grad_pad == "dirichlet0" else pad, inner, -p[:, :, -1:] if grad_pad == "dirichlet0" else pad], 2)
    oy, ox = with_duplicates(ay - my * gy, ax - mx * gx, periodic)
    return (d2, oy, ox, p) if return_pressure else (d2, oy, ox)


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------------
# name -> (boundaries (by, bx), obstacle, velBC, inflow, pressure_solver of the masks)
SCENES = {
    "A": ((OPEN, PER), "none", "standard", "standard", "auto"),
    "A0": ((OPEN, PER), "none", "zero", "none", "auto"),               # translation invariant along x (the CPU twin's equivariance test)
    "B": ((OPEN, PER), "interior", "standard", "standard", "auto"),
    "C": ((OPEN, PER), "seam_x", "standard", "standard", "direct_scattered"),
    "D": ((PER, OPEN), "seam_y", "zero", "standard", "direct_scattered"),
    "E": ((PER, PER), "none", "zero", "none", "auto"),
}


def periodic_of(name):
    return tuple(b == PER for b in SCENES[name][0])


def scene_active(kind, Y, X):
    act = np.ones((Y, X))
    if kind == "interior":                  # a box well inside: one 16-cell window
        act[Y // 2 - 3:Y // 2 + 3, X // 2 - 2:X // 2 + 3] = 0.0
    elif kind == "seam_x":                  # three columns on either side of the x seam
        act[Y // 2 - 3:Y // 2 + 3, :3] = 0.0
        act[Y // 2 - 3:Y // 2 + 3, X - 3:] = 0.0
    elif kind == "seam_y":                  # three rows on either side of the y seam, left of the inflow box
        act[:3, 1:5] = 0.0
        act[Y - 3:, 1:5] = 0.0
    else:
        assert kind == "none"
    return act


@functools.lru_cache(maxsize=None)
def scene_geometry(name, Y, X):
    """the oracle geometry (a fresh instance) carrying the scene's active mask, velBC mask and inflow"""
    _, obstacle, velbc, inflow, _ = SCENES[name]
    g = geometry(Y, X, scene_active(obstacle, Y, X))
    if velbc == "zero":
        g.bc_mask = np.zeros_like(g.bc_mask)
    if inflow == "none":
        g.inflow = np.zeros_like(g.inflow)
    return g


def state(Y, X, seed, name, cfl=None):
    """seeded smooth noise spun up by one float64 periodic step in the scene (consistent duplicate planes, divergence free), fp32 values;
    cfl: the velocity scaled by one factor so that max |u| dt/dx of the post-diffusion velocity is about `cfl` (large2d_scenes.cfl_scaled)"""
    g, per = scene_geometry(name, Y, X), periodic_of(name)
    d, vy, vx = o.synthetic_state(B, Y, X, seed, project_it=False)
    re = torch.tensor([o.RE_TRAIN[i % 6] for i in range(B)], dtype=torch.float64)
    with torch.no_grad():
        d, vy, vx = (t.float().double() for t in periodic_step(d, vy, vx, re, g, per))
    st, reached = (d, vy, vx, re), None
    if cfl is not None:
        st, reached = cfl_scaled(st, g, cfl)
        sy, sx = seam_sync(st[1], st[2], per)          # (the scaling kept the planes equal; spelled out)
        st = (st[0], sy, sx, st[3])
    return st, reached


# ---- cases -------------------------------------------------------------------------------------------------------------------------------------
# (scene, (Y, X)): each scene at (40, 24); A and E at all three shapes; C at (130, 65)
SHAPES = [(16, 16), (40, 24), (130, 65)]
CASES = [("A", (16, 16)), ("A", (40, 24)), ("A", (130, 65)), ("B", (40, 24)), ("C", (40, 24)), ("C", (130, 65)), ("D", (40, 24)),
         ("E", (16, 16)), ("E", (40, 24)), ("E", (130, 65))]
CFLS = (0.8, 2.5)
# seed per (scene, shape, cfl): chosen by the CPU twin's float32-against-float64 run of this reference (never by the device code)
DEFAULT_SEED = 77
SEEDS = {}
# gradient cases that need the trimmed metric (cap TRIM as a condition), as measured by the CPU twin
TRIMMED = set()


def seed_of(name, shape, cfl):
    return SEEDS.get((name, shape, cfl), DEFAULT_SEED)


@functools.lru_cache(maxsize=None)
def reference(name, shape, cfl, dtype=torch.float64):
    """One periodic step and its autograd for the cotangent cotangent_at -> ((d, vy, vx), (g_vy, g_vx), state, (wy, wx), cfl reached).
    Cached: computed once, shared, never modified."""
    Y, X = shape
    g, per = scene_geometry(name, Y, X), periodic_of(name)
    st, reached = state(Y, X, seed_of(name, shape, cfl), name, cfl)
    st = tuple(t.to(dtype) for t in st)
    leaves = [t.clone().requires_grad_(i in (1, 2)) for i, t in enumerate(st)]
    out = periodic_step(*leaves, g, per)
    wy, wx = (t.to(dtype) for t in cotangent_at(B, Y, X))
    ((out[1] * wy).sum() + (out[2] * wx).sum()).backward()
    grads = (leaves[1].grad.double(), leaves[2].grad.double())
    return tuple(t.detach().double() for t in out), grads, tuple(t.double() for t in st), (wy.double(), wx.double()), reached


def periodic_rhs(name, Y, X, seed=4):
    """B right-hand sides the periodic step's solve sees: -div (wrapped) of masked seeded noise, fp32 values held in float64"""
    per = periodic_of(name)
    g = scene_geometry(name, Y, X)
    return field_rhs(g.active, per, Y, X, seed)


def field_rhs(active, per, Y, X, seed=4):
    _, vy, vx = o.synthetic_state(B, Y, X, seed, project_it=False)
    uy, ux = unique(vy, vx, per)
    my, mx = (torch.as_tensor(a) for a in face_masks(active, per))
    uy, ux = uy * my, ux * mx
    hi_y = uy.index_select(1, _map(torch.arange(Y) + 1, uy.shape[1], per[0]))
    hi_x = ux.index_select(2, _map(torch.arange(X) + 1, ux.shape[2], per[1]))
    return (-((hi_y - uy[:, :Y]) + (hi_x - ux[:, :, :X]))).float().double()


# ---- the trainer / roll-out problem: scene A at 32 x 16, mars_moon, msteps = 2 -------------------------------------------------------------------
TRAINER_GRID, TRAINER_MS, TRAINER_SEED, TRAINER_STD_V = (32, 16), 2, 77, _ds.TRAINER_STD_V


def corrected_step(params, d, vy, vx, re, g, per):
    """solver step, correction (the duplicate plane gets none), seam sync"""
    d, vy, vx = periodic_step(d, vy, vx, re, g, per)
    cy, cx = o.correction(params, vy, vx, re, TRAINER_STD_V, o.STD_RE)
    vy, vx = seam_sync(vy + cy, vx + cx, per)
    return d, vy, vx


def trainer_problem(name="A", grid=TRAINER_GRID, ms=TRAINER_MS, seed=TRAINER_SEED):
    r32 = lambda t: t.detach().float().double()
    Y, X = grid
    g, per = scene_geometry(name, Y, X), periodic_of(name)
    (d, vy, vx, re), _ = state(Y, X, seed, name)
    with torch.no_grad():
        _, qy, qx = o.synthetic_state(B, Y, X, 4321 + seed, project_it=False)
        gd = d
        gy, gx = seam_sync(r32(vy + 0.05 * (qy - 1.0)), r32(vx + 0.05 * qx), per)
        gts_y, gts_x = [], []
        for _ in range(ms):
            gd, gy, gx = (r32(t) for t in periodic_step(gd, gy, gx, re, g, per))
            gts_y.append(gy)
            gts_x.append(gx)
    params = [r32(p) for p in o.init_params(0)]
    params[-2] = r32(params[-2] * 0.01)
    return {"g": g, "periodic": per, "d": d, "vy": vy, "vx": vx, "re": re, "gt_vy": gts_y, "gt_vx": gts_x,
            "params": [p.clone().requires_grad_(True) for p in params]}


def trainer_reference(p, dtype=torch.float64):
    """(loss, per-step losses, flat weight gradient, final state) of the unrolled loss in `dtype`: solver step, correction, seam sync,
    l2 loss -- karman2d_multi_launch_cases.trainer_reference's recipe"""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        params = [q.detach().to(dtype).requires_grad_(True) for q in p["params"]]
        d, vy, vx, re = (p[k].to(dtype) for k in ("d", "vy", "vx", "re"))
        sv = torch.tensor(TRAINER_STD_V, dtype=dtype)
        losses = []
        for gy, gx in zip(p["gt_vy"], p["gt_vx"]):
            d, vy, vx = corrected_step(params, d, vy, vx, re, p["g"], p["periodic"])
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
                rd, ry, rx = corrected_step(params, rd, ry, rx, re, p["g"], p["periodic"])
    finally:
        torch.set_default_dtype(prev)
    return rd.double(), ry.double(), rx.double()
