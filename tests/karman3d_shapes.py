"""The shape table, states and metrics of the karman-3d shape tests (test_gpu_karman3d_shapes.py and its CPU twin
test_karman3d_shapes_cpu.py).  A plain module: importing it touches no device.

The rest of the 3-D suite runs the step at (2r, r, r) grids only: 16 x 8 x 8, 20 x 10 x 10, 32 x 16 x 16 and 128 x 64 x 64.  The table
lists the smallest grids that reach the other paths of csrc/karman3d.hip, csrc/pcg.hip and csrc/karman3d_density_bwd.hip; which
transform kernel a cell runs follows from k3_apply_G's predicate, restated here as transform_path().  The scenes are the oracle's
(sol_oracle3d.geometry on any grid: dx = length / X, the inflow box and the obstacle keep their physical definitions), passed to
Scene3D as active= / inflow=."""
import functools

import numpy as np
import torch

import sol_oracle3d as o
from large2d_scenes import CG_RTOL, DEV, TOL_FIELD, TOL_GRAD, TRIM, f32, rel, trimmed_rel   # noqa: F401  (re-exported: one definition)

SEED = 5                            # state seed
W_SEED = 3                          # cotangent seed
CFL_TARGET = 3.0                    # max |u| dt/dx of the scaled state: beyond the halo of 2 of the advection and of the adjoint tiles

# cell (Y, X, Z) -> what it reaches
CELLS = {
    (32, 32, 32): "k3_tzx_mfma<16,16>, k3_ty_mfma<16>; sphere nS 256 / SP 256",
    (64, 32, 64): "k3_tzx_mfma<16,32>, k3_ty_mfma<32>",
    (64, 64, 32): "k3_tzx_mfma<32,16>, k3_ty_mfma<32>; the sphere is cut by the z wall (nS 784, SP 832)",
    (128, 8, 8): "k3_ty at Y = 128 (LDS opt-in), k3_tzx at 8 x 8; the sphere has no cell, the cylinder nS 96 / SP 128",
    (48, 24, 8): "k3_tzx with X != Z; k3_ty with Y = 48 (idle row groups), 6 column slabs; the sphere lies beyond the z wall",
    (22, 10, 12): "GEMM path; adjoint tiles leave 2 rows and 2 columns plus the face row and column, advection tiles 6 and 2; "
                  "sphere nS 32 -> SP 64, half padding",
    (21, 10, 12): "odd Y: accepted, forward and backward",
    (24, 12, 72): "Z in (64, 82]: GEMMs, adjoint on global atomics, advection tile still in LDS",
    (18, 10, 84): "Z > 82: the advection tile falls back under k3d_tile = 1",
    (16, 9, 9): "two odd extents: the forward step runs, every adjoint entry refuses with the face-count message",
}
ODD = (16, 9, 9)
ADJ_CELLS = [c for c in CELLS if c != ODD]
RAGGED = [(22, 10, 12), (21, 10, 12)]
DENS_CELLS = [(22, 10, 12), (24, 12, 72), (64, 32, 64)]      # the density adjoint and the gradient in Re
# (nS, SP) of precond3d.direct_solver_blob3d on the oracle geometry
BLOBS = {
    ((32, 32, 32), "sphere"): (256, 256), ((32, 32, 32), "cylinder"): (1664, 1664),
    ((64, 32, 64), "sphere"): (256, 256), ((64, 32, 64), "cylinder"): (3328, 3328),
    ((64, 64, 32), "sphere"): (784, 832), ((64, 64, 32), "cylinder"): (5248, 5248),
    ((128, 8, 8), "sphere"): (0, 0), ((128, 8, 8), "cylinder"): (96, 128),
    ((48, 24, 8), "sphere"): (0, 0), ((48, 24, 8), "cylinder"): (256, 256),
    ((22, 10, 12), "sphere"): (32, 64), ((22, 10, 12), "cylinder"): (144, 192),
    ((21, 10, 12), "sphere"): (32, 64), ((21, 10, 12), "cylinder"): (144, 192),
    ((24, 12, 72), "sphere"): (32, 64), ((24, 12, 72), "cylinder"): (864, 896),
    ((18, 10, 84), "sphere"): (32, 64), ((18, 10, 84), "cylinder"): (1008, 1024),
    ((16, 9, 9), "sphere"): (7, 64), ((16, 9, 9), "cylinder"): (45, 64),
}
# the obstacle of a cell's step and adjoint tests: the sphere where it has a cell, else the cylinder
OBSTACLE = {c: ("sphere" if BLOBS[(c, "sphere")][0] else "cylinder") for c in CELLS}
# building the blob of these takes 7 s and 23 s of float64 numpy: the CPU twin pins them, the GPU tests run the cylinder there on CG
SLOW_BLOBS = {((64, 32, 64), "cylinder"), ((64, 64, 32), "cylinder")}

# one-hot cotangents at 22 x 10 x 12 (sphere): (component, j, i, k), the state of the case, and in ONE_HOT_ALONE the oracle-alone UNTRIMMED
# value of the case: the largest over the gradient components of float32 oracle against float64 oracle (test_karman3d_shapes_cpu.py
# measures and pins it); the GPU bound is ten times that.
# (a) runs at drift_state: the face lies on the wall column X - 1, where the boundary condition prescribes v_y, so at the spun-up state
# (lateral |u| dt/dx about 2e-3) its value hardly depends on the input -- the largest entry of the reference gradient is 5e-6, every entry
# is a slope of post-diffusion values near 1 times a weight, and the float32 oracle ALONE reads 1.76e-4 / 2.35e-5 / 9.07e-5 in the trimmed
# metric (g_vy / g_vx / g_vz; 11 / 7 / 7 non-zero entries, 5 left out): beyond TOL_GRAD, no float32 step can be held to it there.  With
# the drift the departure point leaves the wall column and the gradient has entries of 0.08: oracle alone 6.4e-7 / 2.7e-6 / 2.4e-6.
ONE_HOT = {
    "a_vy_Y_Xm1_Zm1": (0, 22, 9, 11, "drift"),
    "b_vx_Ym1_X_0": (1, 21, 10, 0, "spun_up"),
    "c_vz_0_0_Z": (2, 0, 0, 12, "spun_up"),
    "d_vx_beside_the_obstacle": (1, 5, 3, 5, "spun_up"),
}
# measured, untrimmed: (a) 7.79e-7 / 2.75e-6 / 2.92e-6 (g_vy / g_vx / g_vz; 22 / 14 / 14 non-zero entries), (b) 0 / 6.14e-7 / 2.30e-7
# (0 / 27 / 7), (c) 0 / 8.45e-7 / 4.40e-7 (0 / 7 / 16), (d) 4.57e-7 / 6.01e-7 / 6.91e-6 (dense through the pressure solve)
ONE_HOT_ALONE = {"a_vy_Y_Xm1_Zm1": 3.0e-6, "b_vx_Ym1_X_0": 6.2e-7, "c_vz_0_0_Z": 8.5e-7, "d_vx_beside_the_obstacle": 7.0e-6}


def one_hot_case(which, B=2):
    """(state, geometry, cotangent) of a one-hot case"""
    cell = (22, 10, 12)
    g = geometry(cell, "sphere")
    comp, j, i, k, name = ONE_HOT[which]
    st = drift_state(B, cell, SEED, g) if name == "drift" else state(B, cell, SEED, g)
    w = [torch.zeros(s, dtype=torch.float64) for s in face_shapes(B, cell)]
    w[comp][:, j, i, k] = 1.0
    return st, g, w


def sid(c):
    return "%dx%dx%d" % tuple(c)


def transform_path(Y, X, Z):
    """k3_apply_G's predicate (csrc/karman3d.hip) -> "mfma", "lds" or "gemm": the transform kernels a grid runs under the default options"""
    fused = X <= 64 and Z <= 64 and Y <= 128 and X % 4 == 0 and Z % 4 == 0 and Y % 16 == 0 and (X * Z) % 32 == 0
    if not fused:
        return "gemm"
    return "mfma" if X in (32, 64) and Z in (32, 64) and Y in (32, 64, 128) else "lds"


def transform_settings(Y, X, Z):
    """the settings of (k3d_mfma_tf, k3d_fused_tf) that run distinct kernels at this grid"""
    path = transform_path(Y, X, Z)
    return {"mfma": [(1, 1), (0, 1), (1, 0)], "lds": [(1, 1), (1, 0)], "gemm": [(1, 1)]}[path]


def advect_tile_fits(Z, TR=12):
    """step_fwd3d's tile_lds <= 160 KB with the tile of 8 x 8 columns + a halo of 2: 1968 Z + 576 <= 163840"""
    return ((TR + 1) * TR * Z + TR * (TR + 1) * Z + TR * TR * (Z + 1)) * 4 + TR * TR * Z <= 160 * 1024


def geometry(cell, obstacle):
    return o.geometry(*cell, obstacle=obstacle)


@functools.lru_cache(maxsize=None)
def empty_geometry(cell):
    """the all-fluid scene of a cell (a fresh instance, never the cached one)"""
    g = o.Karman3DGeometry(*cell)
    g.obstacle = np.zeros(cell)
    g.active = np.ones(cell)
    g.masks = tuple(np.ones(s) for s in ((cell[0] + 1, cell[1], cell[2]), (cell[0], cell[1] + 1, cell[2]), (cell[0], cell[1], cell[2] + 1)))
    g.diag = np.full(cell, -6.0)
    return g


def reynolds(B):
    return torch.tensor([o.RE_TRAIN[i % 6] for i in range(B)], dtype=torch.float64)


def state(B, cell, seed=SEED, g=None):
    """(d, (vy, vx, vz), re): seeded smooth noise; with a geometry: spun up by one float64 oracle step in that scene (divergence free,
    consistent with its obstacle), rounded to fp32 values held in float64"""
    d, v = o.synthetic_state(B, *cell, seed)
    re = reynolds(B)
    if g is not None:
        with torch.no_grad():
            d, v = o.karman3d_step(d, v, re, g)
    return d.float().double(), tuple(t.float().double() for t in v), re


DRIFT = 0.3                         # cells per step


def drift_state(B, cell, seed=SEED, g=None):
    """the seeded noise with a uniform lateral drift of DRIFT cells per step on v_x and v_z (fp32 values held in float64).  The plain
    state's lateral |u| dt/dx is about 2e-3, so some of its 1e4 ... 1e6 departure points lie within float32 rounding of a cell boundary,
    where the step's gradient jumps: the trimmed metric absorbs those few entries of a field gradient, but g_re is ONE sum per simulation
    and moves by 1e-4 ... 1e-2 in the oracle alone (float32 against float64, density cotangent on uniform-noise density).  With the
    drift every departure point is 0.05 cells or more away from a boundary (test_karman3d_shapes_cpu.py pins the oracle-alone g_re)."""
    d, v = o.synthetic_state(B, *cell, seed)
    dx = (g.dx if g is not None else 100.0 / cell[1])
    v = (v[0], v[1] + DRIFT * dx, v[2] + DRIFT * dx)
    return d.float().double(), tuple(t.float().double() for t in v), reynolds(B)


W_DENS = 8.0                        # weight of the density term of energy_cotangent: the density path is then 1 ... 25 % of g_re


def energy_cotangent(st, g):
    """the cotangents of the loss 1/2 |v_out|^2 + W_DENS/2 |active d_out|^2 at the float64 oracle's outputs (fp32 values held in
    float64): (w_vy, w_vx, w_vz), w_d.  With a seeded-noise cotangent g_re is a sum of terms of either sign that cancel to 1e-9 (a
    relative error of 1e-4 in the oracle alone); diffusion lowers the energy everywhere, so these terms have one sign and the sum is
    well conditioned."""
    with torch.no_grad():
        od, ov = o.karman3d_step(st[0], st[1], st[2], g)
    return tuple(t.float().double() for t in ov), (W_DENS * od * torch.as_tensor(g.active)).float().double()


def face_shapes(B, cell):
    Y, X, Z = cell
    return (B, Y + 1, X, Z), (B, Y, X + 1, Z), (B, Y, X, Z + 1)


def cotangent(B, cell, seed=W_SEED, g=None):
    """seeded normal cotangents of magnitude ~1: (w_vy, w_vx, w_vz) and, drawn after them, w_d (times the scene's active mask: inside the
    obstacle the departure point sits exactly on a cell boundary, karman3d_adjoint_cases.py); fp32 values held in float64"""
    gen = torch.Generator().manual_seed(seed)
    w = tuple(torch.randn(s, generator=gen, dtype=torch.float64).float().double() for s in face_shapes(B, cell))
    wd = torch.randn((B,) + tuple(cell), generator=gen, dtype=torch.float64).float().double()
    if g is not None:
        wd = wd * torch.as_tensor(g.active, dtype=torch.float64)
    return w, wd


def step_like_rhs(B, cell, seed=4):
    """B right-hand sides the step's solve sees: -div of unprojected seeded noise, fp32 values held in float64"""
    _, v = o.synthetic_state(B, *cell, seed)
    return (-o.divergence(v)).float().double()


def white_rhs(B, cell, seed=6):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn((B,) + tuple(cell), generator=gen, dtype=torch.float64).float().double()


def rect_solve(b, cell):
    """float64 empty-box solve M_r p = b of the oracle; b [B,Y,X,Z] tensor -> numpy"""
    return o.rect_solve(np.asarray(b, dtype=np.float64), o._rect_eigenvalues(tuple(cell)))


def oracle_solve(rhs, g):
    """float64 p with M p = rhs, M = -A of the scene: the oracle's own solve (sparse LU below LU_MAX_CELLS, else its PCG)"""
    with torch.no_grad():
        return -o._PressureSolve.apply(torch.as_tensor(rhs, dtype=torch.float64), g)


def oracle_grad(st, g, w, wd=None, re_grad=False, dtype=torch.float64, **kw):
    """one oracle step in `dtype` and the gradient of <v_out, w> (+ <d_out, wd>) -> ((d, vy, vx, vz) out, (g_d, g_vy, g_vx, g_vz, g_re)),
    float64 tensors; g_d / g_re are zero where the loss does not reach them"""
    d, v, re = st
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in (d, *v)] + [re.to(dtype).clone().requires_grad_(re_grad)]
    od, ov = o.karman3d_step(leaves[0], tuple(leaves[1:4]), leaves[4], g, **kw)
    loss = sum((a * b.to(dtype)).sum() for a, b in zip(ov, w))
    if wd is not None:
        loss = loss + (od * wd.to(dtype)).sum()
    loss.backward()
    zero = lambda p: torch.zeros_like(p) if p.grad is None else p.grad
    return tuple(t.detach().double() for t in (od, *ov)), tuple(zero(p).double() for p in leaves)


def cfl_of(v, re, g, dt=1.0):
    """max |u| dt/dx of the post-diffusion velocity: the field the advection and its adjoint trace back along"""
    c = o.diffuse_bc(v, re, g.X, dt, g)
    return max(float(t.abs().max()) for t in c) * dt / g.dx


def cfl_scaled(st, g, target=CFL_TARGET):
    """st with its velocity multiplied by one factor (fp32 values) so that cfl_of is about `target` -> (state, the value reached)"""
    d, v, re = st
    s = float(np.float32(target / cfl_of(v, re, g)))
    sv = tuple((t * s).float().double() for t in v)
    return (d, sv, re), cfl_of(sv, re, g)


def check_fields(out, ref, what, names=("d", "v_y", "v_x", "v_z")):
    errs = [rel(a, b) for a, b in zip(out, ref)]
    print("%s: %s against the oracle: %s" % (what, "/".join(names), ", ".join("%.3e" % e for e in errs)))
    assert max(errs) < TOL_FIELD, (what, errs)
    return errs


def check_grads(got, ref, what, names=("g_vy", "g_vx", "g_vz"), tol=TOL_GRAD):
    """the trimmed metric on every component: at most floor(TRIM n) entries left out -> [(trimmed, untrimmed)]"""
    res = []
    for name, a, b in zip(names, got, ref):
        full = rel(a, b)
        v, k, worst = trimmed_rel(a, b)
        print("%s %s: rel L2 %.3e untrimmed, %.3e after leaving out %d of %d entries (largest deviation left out %.3e)"
              % (what, name, full, v, k, b.numel(), worst))
        assert k <= int(TRIM * b.numel())
        assert v < tol, (what, name, v, full)
        res.append((v, full))
    return res
