"""Float64 reference, scenes, states and cases of the z-periodic karman-3d tests (test_gpu_karman3d_periodic.py and its CPU twin
test_karman3d_periodic_cpu.py).  A plain module: importing it touches no device.

periodic3d_step restates the step of include/sol_hip.h ("PERIODIC SPANWISE BOUNDARIES on the karman-3d step") in torch, differentiable
by autograd, the way periodic_cases.periodic_step does for 2-D: the oracle's step (sol_oracle3d.karman3d_step, which the CPU twin ties
it to with pz off) with every clamped or zero-ghost z index taken modulo the Z unique planes.  Array shapes are the open step's: v_z
[B,Y,X,Z+1], plane Z a duplicate of plane 0 -- never read on input, written equal to plane 0 on output.  The pressure solve is a float64
sparse LU of precond3d.scene_matrix3d(active, pz) up to LU_MAX_CELLS cells (the oracle's bound); above that the float64 restatement of
the device algorithm on the periodic blob (precond3d.periodic_solve_reference3d; the CPU twin ties it to the LU at the small cells).

States, metrics and tolerances are karman3d_shapes': synthetic_state spun up by one float64 step in the scene, scaled to CFL_TARGET =
3.0; rel, trimmed_rel; TOL_FIELD = 1e-5, TOL_GRAD = 1e-4, TRIM = 1e-3 (a cap, not a knob: the CPU twin shows that the float32 run of
this reference alone stays inside them on every case).
"""
import functools

import numpy as np
import scipy.sparse.linalg as spla
import torch

import sol_oracle3d as o
from sol_amd import precond3d
from karman3d_shapes import CFL_TARGET, SEED, TOL_FIELD, TOL_GRAD, TRIM, W_SEED, cotangent, face_shapes, rel, reynolds, sid, trimmed_rel  # noqa: F401

B = 2
LU_MAX_CELLS = o.LU_MAX_CELLS

# cell (Y, X, Z) -> the path it reaches (csrc/karman3d.hip, csrc/karman3d_periodic.hip).  On a periodic blob every transform of the solve
# is the fp64-accumulating GEMM (k_p_gemm) whatever the options say: the grids at which an OPEN blob runs k3_tzx / k3_ty (16 x 8 x 8) or
# the matrix-core transforms (32 x 32 x 32) stay in the table because the dispatch must NOT reach those kernels there -- the forward test
# asserts it by name under every transform setting
CELLS = {
    (16, 8, 8): "k_p_gemm where an open blob runs k3_tzx / k3_ty",
    (22, 10, 12): "k_p_gemm chain with ragged tiles; ragged advection and adjoint tiles",
    (32, 32, 32): "k_p_gemm where an open blob runs the MFMA transforms; extruded SP2 = 64",
    (24, 12, 72): "Z > 64: adjoint on global atomics",
    (18, 10, 84): "forward tile falls back to k3p_advect",
}
ODD = (16, 9, 9)                    # odd Z: forward only
# (cell, obstacle): every cell runs the cylinder on the extruded blob; 22 x 10 x 12 also the sphere (dense blob) and the empty box
SCENES = [(c, "cylinder") for c in CELLS] + [((22, 10, 12), "sphere"), ((22, 10, 12), "empty")]
SOLVER = {"cylinder": "direct_extruded", "sphere": "direct", "empty": "direct"}
# seed per (cell, obstacle): chosen by the CPU twin's float32-against-float64 run of this reference (never by the device code).  A case
# that does not stay inside the bounds gets another seed here, not a looser bound; the replacement is recorded with its reason.
DEFAULT_SEED = SEED
SEEDS = {}


def seed_of(cell, obstacle):
    return SEEDS.get((tuple(cell), obstacle), DEFAULT_SEED)


# ---- index helpers ---------------------------------------------------------------------------------------------------------------------
def _map(idx, n, periodic):
    """an index along an axis of n unique planes: modulo n when periodic, clamped to [0, n - 1] when open"""
    return idx % n if periodic else idx.clamp(0, n - 1)


def _shift(f, dim, s, periodic):
    n = f.shape[dim]
    return f.index_select(dim, _map(torch.arange(n) + s, n, periodic))


def _lap(f, per):
    """7-point Laplacian of f [B,n0,n1,n2] (unique planes): wrapped along a periodic axis, replicate padded along an open one"""
    out = -6.0 * f
    for a in range(3):
        out = out + _shift(f, a + 1, 1, per[a]) + _shift(f, a + 1, -1, per[a])
    return out


def _at(f, idx):
    """f [B,n0,n1,n2] at integer index tensors idx = (jj, ii, kk), each [B,...] (already mapped into range)"""
    Bn, n0, n1, n2 = f.shape
    lin = (idx[0] * n1 + idx[1]) * n2 + idx[2]
    return torch.gather(f.reshape(Bn, -1), 1, lin.reshape(Bn, -1)).reshape(idx[0].shape)


def unique(v, pz):
    """the unique planes of a staggered velocity: the duplicate plane of v_z dropped on a z-periodic scene"""
    return [v[0], v[1], v[2][..., :-1] if pz else v[2]]


def with_duplicate(uz, pz):
    return torch.cat([uz, uz[..., :1]], 3) if pz else uz


def seam_sync(v, pz):
    """plane 0 of v_z copied onto the duplicate plane (differentiable): the adjoint is the seam fold"""
    return (v[0], v[1], with_duplicate(unique(v, pz)[2], pz))


def face_masks(active, pz):
    """hard-BC face masks of the unique faces: my [Y+1,X,Z], mx [Y,X+1,Z], mz [Y,X,Z+1] (Z when periodic); accessible = the active mask,
    edge-extended along an open axis, wrapped along a periodic z"""
    act = (np.asarray(active, dtype=np.float64) != 0).astype(np.float64)
    acc = precond3d._accessible3d(act, pz)
    c = slice(1, -1)
    my = acc[:-1, c, c] * acc[1:, c, c]
    mx = acc[c, :-1, c] * acc[c, 1:, c]
    mz = acc[c, c, :-1] * acc[c, c, 1:]
    return my, mx, (mz[..., :-1] if pz else mz)


# ---- the pressure solve ------------------------------------------------------------------------------------------------------------------
class _Solve(torch.autograd.Function):
    """p = M^-1 rhs in float64 for the symmetric M = precond3d.scene_matrix3d(active, pz); backward = the same solve"""

    @staticmethod
    def forward(ctx, rhs, solver):
        ctx.solver = solver
        return torch.as_tensor(solver(rhs.detach().double().numpy()), dtype=rhs.dtype)

    @staticmethod
    def backward(ctx, g):
        return _Solve.apply(g, ctx.solver), None


def make_solver(active, pz):
    """rhs [B,Y,X,Z] float64 numpy -> M^-1 rhs.  Sparse LU up to LU_MAX_CELLS cells; above, the float64 restatement of the device
    algorithm on the periodic blob (the extruded one where it builds, else the dense one)"""
    act = np.asarray(active, dtype=np.float64)
    if act.size <= LU_MAX_CELLS or not pz:
        lu = spla.splu(precond3d.scene_matrix3d(act, pz))
        return lambda r: lu.solve(r.reshape(r.shape[0], -1).T).T.reshape(r.shape)
    blob = precond3d.extruded_solver_blob3d(act, periodic=True)
    if blob is None:
        blob = precond3d.periodic_solver_blob3d(act)
    assert blob is not None
    return lambda r: np.stack([precond3d.periodic_solve_reference3d(blob, q) for q in r])


def solver_of(geom, pz):
    key = "_periodic3d_solver_%d" % int(pz)
    if not hasattr(geom, key):
        setattr(geom, key, make_solver(geom.active, pz))
    return getattr(geom, key)


# ---- the step --------------------------------------------------------------------------------------------------------------------------------
def diffused(v, re, geom, pz, dt=1.0, res=None):
    """the post-diffusion velocity on the unique planes: explicit 7-point diffusion + the velocity BC blend on the flow component"""
    per = (False, False, bool(pz))
    res = geom.X if res is None else res
    u = unique(v, pz)
    alpha = (1.0 / re * dt * res * res).reshape(-1, 1, 1, 1)
    c = [f + alpha * _lap(f, per) for f in u]
    m = torch.as_tensor(np.asarray(geom.bc_mask), dtype=u[0].dtype)
    c[0] = c[0] * (1.0 - m) + m
    return c


def periodic3d_step(d, v, re, geom, pz=False, dt=1.0, res=None, grad_pad="replicate", inflow_order="after", return_pressure=False):
    """One solver step with the z axis wrapped when pz.  d [B,Y,X,Z], v = (vy [B,Y+1,X,Z], vx [B,Y,X+1,Z], vz [B,Y,X,Z+1]), re [B]; geom:
    an oracle Karman3DGeometry (active, inflow, bc_mask -- velBCy = velBCyMask = bc_mask -- and dx are read)  ->  d, (vy, vx, vz)"""
    pz = bool(pz)
    per = (False, False, pz)
    Bn, Y, X, Z = d.shape
    n = (Y, X, Z)
    dtype = v[0].dtype
    T = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    c = diffused(v, re, geom, pz, dt, res)
    U = tuple(c[a].shape[a + 1] for a in range(3))          # unique faces of component a along its own axis
    dtdx = dt / geom.dx

    def lattice(shape):
        g = torch.meshgrid(*(torch.arange(s) for s in shape), indexing="ij")
        return [t.unsqueeze(0).expand(Bn, -1, -1, -1) for t in g]

    def vel_at(kind, b, idx):
        """component b of the advecting velocity at the points of lattice `kind` (0, 1, 2: the faces of that component; "c": the cells):
        the stored value, or the average of the surrounding faces with wrapped / clamped neighbours"""
        if kind == b:
            return _at(c[b], idx)
        out = 0.0
        if kind == "c":
            for db in (0, 1):
                q = list(idx)
                q[b] = _map(idx[b] + db, U[b], per[b])
                out = out + _at(c[b], q)
            return 0.5 * out
        a = kind
        for da in (-1, 0):
            for db in (0, 1):
                q = list(idx)
                q[a] = _map(idx[a] + da, n[a], per[a])
                q[b] = _map(idx[b] + db, U[b], per[b])
                out = out + _at(c[b], q)
        return 0.25 * out

    def trilinear(f, idx, u, zero_ghost=False):
        """f [B,n0,n1,n2] (unique planes) sampled at idx - u dt/dx: floor and weights of the offset as the kernels form them"""
        off = [-u[a] * dtdx for a in range(3)]
        fl = [torch.floor(t) for t in off]
        w = [t - g for t, g in zip(off, fl)]
        base = [idx[a] + fl[a].long() for a in range(3)]
        out = 0.0
        for cj in (0, 1):
            for ci in (0, 1):
                for ck in (0, 1):
                    q, wt = [], 1.0
                    for a, cc in enumerate((cj, ci, ck)):
                        ia = base[a] + cc
                        if zero_ghost and not per[a]:           # the density: one ring of zero ghost cells along an OPEN axis
                            wt = wt * ((ia >= 0) & (ia < f.shape[a + 1])).to(dtype)
                        wt = wt * (w[a] if cc else 1.0 - w[a])
                        q.append(_map(ia, f.shape[a + 1], per[a]))
                    out = out + wt * _at(f, q)
        return out

    adv = []
    for a in range(3):
        idx = lattice(c[a].shape[1:])
        adv.append(trilinear(c[a], idx, [vel_at(a, b, idx) for b in range(3)]))
    idx = lattice(n)
    infl = T(geom.inflow)
    d_src = d + infl if inflow_order == "before" else d
    d2 = trilinear(d_src, idx, [vel_at("c", b, idx) for b in range(3)], zero_ghost=True)
    if inflow_order == "after":
        d2 = d2 + infl * dt
    # projection
    m = [T(a) for a in face_masks(geom.active, pz)]
    adv = [f * mk for f, mk in zip(adv, m)]
    hi_z = adv[2].index_select(3, _map(torch.arange(Z) + 1, U[2], pz))
    div = (adv[0][:, 1:] - adv[0][:, :-1]) + (adv[1][:, :, 1:] - adv[1][:, :, :-1]) + (hi_z - adv[2][..., :Z])
    p = _Solve.apply(-div, solver_of(geom, pz))             # M p = -div
    gy, gx, gz = o.grad_p(p, grad_pad)                      # (M = -A: this p is the oracle's)
    if pz:
        gz = p - _shift(p, 3, -1, True)                     # no boundary face along z: grad_pad is not read
    out = (adv[0] - m[0] * gy, adv[1] - m[1] * gx, with_duplicate(adv[2] - m[2] * gz, pz))
    return (d2, out, p) if return_pressure else (d2, out)


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------------
def bc_mask(cell, pz):
    """velBCyMask of the scene: the oracle's, without the z walls on a periodic span (karman3d.velocity_bc_masks3d)"""
    Y, X, Z = cell
    vn = np.zeros((Y + 1, X, Z))
    vn[0:2] = 1.0
    vn[:, 0] = 1.0
    vn[:, -1] = 1.0
    if not pz:
        vn[:, :, 0] = 1.0
        vn[:, :, -1] = 1.0
    return vn


@functools.lru_cache(maxsize=None)
def scene_geometry(cell, obstacle, pz=True):
    """the oracle geometry (a fresh instance) of a cell with the scene's obstacle ("sphere", "cylinder", "empty") and velBC mask"""
    g = o.Karman3DGeometry(*cell, obstacle_kind="sphere" if obstacle == "empty" else obstacle)
    if obstacle == "empty":
        g.obstacle = np.zeros(cell)
        g.active = np.ones(cell)
    g.bc_mask = bc_mask(cell, pz)
    g.masks = g.diag = None                                 # (the open scene's: nothing here reads them)
    return g


def cfl_of(v, re, g, pz):
    return max(float(t.abs().max()) for t in diffused(v, re, g, pz)) / g.dx


def state(cell, obstacle, seed=None, cfl=CFL_TARGET, pz=True):
    """seeded smooth noise spun up by one float64 periodic step in the scene (consistent duplicate plane, divergence free), fp32 values;
    the velocity scaled by one factor so that max |u| dt/dx of the post-diffusion velocity is about `cfl`  ->  ((d, v, re), cfl reached)"""
    g = scene_geometry(tuple(cell), obstacle, pz)
    d, v = o.synthetic_state(B, *cell, seed_of(cell, obstacle) if seed is None else seed)
    re = reynolds(B)
    with torch.no_grad():
        d, v = periodic3d_step(d, v, re, g, pz)
    d, v = d.float().double(), tuple(t.float().double() for t in v)
    if cfl is not None:
        s = float(np.float32(cfl / cfl_of(v, re, g, pz)))
        v = seam_sync(tuple((t * s).float().double() for t in v), pz)
    return (d, v, re), cfl_of(v, re, g, pz)


Z_DRIFT = 10.5                      # cells per step: more than the 8 planes of a period at 16 x 8 x 8


def drift_state(cell=(16, 8, 8), obstacle="cylinder"):
    """the CFL_TARGET state of the cell with a uniform z drift of Z_DRIFT cells per step added to v_z: the true-modulo case.
    REPLACEMENT, recorded: the drift was first added to the unscaled spun-up state (lateral |v_x| about 0.6 against v_z = 131).  The
    float32 run of this reference ALONE then reads 1.55e-5 on v_x against float64 (the rounding of v_z, 131 x 6e-8, reaches v_x through
    the pressure solve), beyond TOL_FIELD for any float32 step.  On the scaled state (|v_y| up to 38, |v_x| up to 18) it reads 3.4e-7 /
    1.3e-7 / 5.7e-7 / 5.4e-8 (d, v_y, v_x, v_z); test_karman3d_periodic_cpu.py holds it to the bound."""
    g = scene_geometry(tuple(cell), obstacle)
    (d, v, re), _ = state(cell, obstacle)
    return d, seam_sync((v[0], v[1], (v[2] + Z_DRIFT * g.dx).float().double()), True), re


@functools.lru_cache(maxsize=None)
def reference(cell, obstacle, dtype=torch.float64):
    """One periodic step and its autograd for the cotangent karman3d_shapes.cotangent  ->  ((d, vy, vx, vz) out, (g_vy, g_vx, g_vz),
    state, (w_vy, w_vx, w_vz), cfl reached).  Cached: computed once, shared, never modified."""
    g = scene_geometry(tuple(cell), obstacle)
    st, reached = state(cell, obstacle)
    d, v, re = st
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in v]
    od, ov = periodic3d_step(d.to(dtype), tuple(leaves), re.to(dtype), g, True)
    w, _ = cotangent(B, cell)
    sum((a * b.to(dtype)).sum() for a, b in zip(ov, w)).backward()
    return (od.detach().double(),) + tuple(t.detach().double() for t in ov), tuple(t.grad.double() for t in leaves), st, w, reached


def periodic_rhs(cell, obstacle, seed=4):
    """B right-hand sides the periodic step's solve sees: -div (wrapped) of masked seeded noise, fp32 values held in float64"""
    g = scene_geometry(tuple(cell), obstacle)
    _, v = o.synthetic_state(B, *cell, seed)
    u = [f * torch.as_tensor(m) for f, m in zip(unique(v, True), face_masks(g.active, True))]
    Z = cell[2]
    hi_z = u[2].index_select(3, (torch.arange(Z) + 1) % Z)
    return (-((u[0][:, 1:] - u[0][:, :-1]) + (u[1][:, :, 1:] - u[1][:, :, :-1]) + (hi_z - u[2]))).float().double()


# ---- the trainer / roll-out problem: the cylinder at 16 x 8 x 8, msteps = 2 ---------------------------------------------------------------------
TRAINER_CELL, TRAINER_MS, TRAINER_STD_V = (16, 8, 8), 2, (0.8, 0.6, 0.5)


def corrected_step(params, d, v, re, g, std_v=TRAINER_STD_V):
    """solver step, correction (the duplicate plane gets none), seam sync"""
    d, v = periodic3d_step(d, v, re, g, True)
    corr = o.correction(params, v, re, std_v, o.STD_RE)
    return d, seam_sync(tuple(a + c for a, c in zip(v, corr)), True)


def trainer_problem(cell=TRAINER_CELL, ms=TRAINER_MS, seed=SEED):
    r32 = lambda t: t.detach().float().double()
    g = scene_geometry(tuple(cell), "cylinder")
    (d, v, re), _ = state(cell, "cylinder", seed, cfl=None)
    with torch.no_grad():
        _, q = o.synthetic_state(B, *cell, 4321 + seed)
        gd = d
        gv = seam_sync((r32(v[0] + 0.05 * (q[0] - 1.0)), r32(v[1] + 0.05 * q[1]), r32(v[2] + 0.05 * q[2])), True)
        gts = []
        for _ in range(ms):
            gd, gv = periodic3d_step(gd, gv, re, g, True)
            gd, gv = r32(gd), tuple(r32(t) for t in gv)
            gts.append(gv)
    params = [r32(p) for p in o.init_params(0)]
    params[-2] = r32(params[-2] * 0.01)
    return {"g": g, "d": d, "v": v, "re": re, "gts": gts, "params": params}


def trainer_reference(p, dtype=torch.float64):
    """(loss, per-step losses, flat weight gradient, final state) of the unrolled loss in `dtype`: solver step, correction, seam sync, l2
    loss over the stored faces (sol_oracle3d.unrolled_loss's recipe)"""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        params = [q.detach().to(dtype).requires_grad_(True) for q in p["params"]]
        d, re = p["d"].to(dtype), p["re"].to(dtype)
        v = tuple(t.to(dtype) for t in p["v"])
        sv = torch.tensor(TRAINER_STD_V, dtype=dtype)
        losses = []
        for gt in p["gts"]:
            d, v = corrected_step(params, d, v, re, p["g"])
            losses.append(sum(0.5 * (((gt[c].to(dtype) - v[c]) / sv[c]) ** 2).sum() for c in range(3)))
        loss = torch.stack(losses).sum() / len(losses)
        loss.backward()
    finally:
        torch.set_default_dtype(prev)
    return (float(loss.detach()), [float(l.detach()) for l in losses], torch.cat([q.grad.reshape(-1) for q in params]).double(),
            (d.detach().double(),) + tuple(t.detach().double() for t in v))


def rollout_reference(p, steps, dtype=torch.float64):
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        with torch.no_grad():
            params = [q.detach().to(dtype) for q in p["params"]]
            d, re = p["d"].to(dtype), p["re"].to(dtype)
            v = tuple(t.to(dtype) for t in p["v"])
            for _ in range(steps):
                d, v = corrected_step(params, d, v, re, p["g"])
    finally:
        torch.set_default_dtype(prev)
    return (d.double(),) + tuple(t.double() for t in v)
