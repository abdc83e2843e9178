"""karman-3d (BASELINE.json configs[4]): host surface of the 3-D forward path.

The reference has no 3-D code (/root/reference/README.md:37-38).  This module is the dimension-generic twin of karman.py /
model.py / trainer.SolRollout: the same scene (karman-2d/karman_train.py:166-171, 363-373) with a third axis, the same step
(`KarmanFlow.step`, :173-185), `model_mars_moon` (:101-138) with Conv3D(5) layers over 4 input channels (three velocity
components + Re) and 3 output channels, and the roll-out loop of karman_apply.py:138-158.  Forward only in this version.

Layout: density [B,Y,X,Z], v_y [B,Y+1,X,Z], v_x [B,Y,X+1,Z], v_z [B,Y,X,Z+1] (y = flow direction, z contiguous); CNN
tensors [B,Y,X,Z,C].  Everything calls libsol_hip.so (csrc/karman3d.hip); there is no CPU implementation.

Training (SOL-n, the reverse sweep of karman_train.py:397-457 in 3-D): `Karman3DTrainer` runs a hand-written schedule over the C ABI
(forward unroll + reverse sweep, no autograd graph; `schedule="autograd"` keeps the torch composition as the cross-check).  How the network
is launched -- its packed weights, the twelve forward launches, the reverse sweep and the weight-gradient partials -- is written once, in
schedule3d.NetSchedule3D: the trainer, the autograd node of `MarsMoon3D.__call__` and `Karman3DRollout` (train=False) all run one, and it re-packs
when `MarsMoon3D.params_key()` has moved.  For other hosts
`Karman3DFlow.step` and `conv3d` are also torch.autograd Functions over the HIP adjoints (sol_karman3d_step_bwd; Conv3D backward-data = sol_conv3d on flipped weights, weight gradient
= five passes of the 2-D weight-gradient kernels), composed by `Karman3DTrainer` exactly as the reference composes its graph.
"""
import ctypes as C
import math
import weakref
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import Karman3DCfg, check, ptr, stream

EPI_NONE, EPI_LRELU, EPI_DLRELU = 0, 1, 2


def scene_arrays3d(Y, X, Z, length=100.0, obstacle="sphere"):
    """(active, inflow) [Y,X,Z] float64: Inflow(box[5:10, 25:75, 25:75]) and Obstacle(Sphere([50, 50, 50], 10)) -- the
    dimension-generic form of karman_train.py:169-170 -- on the domain box[0:2*len, 0:len, 0:len] (:363).  Cell centres
    inside count (inclusive box bounds, dist^2 <= r^2), as in the 2-D scene."""
    if obstacle != "sphere":
        raise NotImplementedError("the HIP path takes window-sized obstacles (sphere); obstacle=%r is an oracle-only option" % (obstacle,))
    if not (Y == 2 * X and Z == X):
        raise ValueError("karman-3d domain is box[0:2*len, 0:len, 0:len]: resolution must be (2*res, res, res)")
    dx = length / X
    c = [(np.arange(n) + 0.5) * dx for n in (Y, X, Z)]
    YC, XC, ZC = np.meshgrid(*c, indexing="ij")
    s = length / 100.0
    inflow = ((YC >= 5 * s) & (YC <= 10 * s) & (XC >= 25 * s) & (XC <= 75 * s) & (ZC >= 25 * s) & (ZC <= 75 * s)).astype(np.float64)
    obst = (((YC - 50 * s) ** 2 + (XC - 50 * s) ** 2 + (ZC - 50 * s) ** 2) <= (10 * s) ** 2).astype(np.float64)
    return 1.0 - obst, inflow


def extrude_mask(mask2d, Z):
    """[Y,X] -> [Y,X,Z] float64: the 2-D mask repeated along z (mask[:, :, k] = mask2d for every k): the scenes the extruded direct solve
    (Scene3D(pressure_solver="direct_extruded")) takes"""
    m = np.asarray(mask2d, dtype=np.float64)
    if m.ndim != 2 or isinstance(Z, bool) or not isinstance(Z, (int, np.integer)) or Z < 1:
        raise ValueError("extrude_mask: mask2d must be [Y,X] and Z a positive integer (got shape %s, Z %r)" % (m.shape, Z))
    return np.ascontiguousarray(np.broadcast_to(m[:, :, None], m.shape + (int(Z),)))


def cylinder_arrays3d(Y, X, Z, length=100.0):
    """(active, inflow) [Y,X,Z] float64 of the wake scene: scene_arrays3d's inflow box and, in place of the sphere, the disc
    Sphere([50, 50], 10) of the 2-D scene extruded along z (cell centres inside count, dist^2 <= r^2).  Any grid: dx = length / X, the
    domain is box[0:Y dx, 0:X dx, 0:Z dx] and the inflow box and the obstacle keep their physical definitions (coordinates of a domain
    of length 100: `length` sets dx alone), so a coarse or short grid may hold no inflow cell."""
    dx = length / X
    yc, xc, zc = ((np.arange(n) + 0.5) * dx for n in (Y, X, Z))
    inflow = ((yc >= 5.0) & (yc <= 10.0))[:, None, None] & ((xc >= 25.0) & (xc <= 75.0))[None, :, None] & ((zc >= 25.0) & (zc <= 75.0))[None, None, :]
    disc = ((yc[:, None] - 50.0) ** 2 + (xc[None, :] - 50.0) ** 2) <= 10.0 ** 2
    return extrude_mask(1.0 - disc, Z), inflow.astype(np.float64)


def velocity_bc_masks3d(Y, X, Z, periodic_z=False):
    """velBCy / velBCyMask of karman_train.py:366-373 with the third axis: the two inflow-side planes and the four lateral
    walls of the flow component, [Y+1,X,Z], values 1.  periodic_z: a periodic span has no z walls -- the two x walls only."""
    vn = np.zeros((Y + 1, X, Z))
    vn[0:2, :, :] = 1.0
    vn[:, 0, :] = 1.0
    vn[:, -1, :] = 1.0
    if not periodic_z:
        vn[:, :, 0] = 1.0
        vn[:, :, -1] = 1.0
    return vn, np.copy(vn)


PERIODIC_Z = 8                  # Scene3D.periodic_bits of a z-periodic scene: header word 6 of its blob (precond3d.PERIODIC_Z, SOL_K3_PERIODIC_Z)
BOUNDARIES3D_MESSAGE = "%s must be 'open', 'periodic-z' or a triple (by, bx, bz) of 'open' / 'periodic' (got %r)"


def boundaries_arg3d(b, who="boundaries"):
    """"open", "periodic-z" or a triple (by, bx, bz) of "open" / "periodic" (the words of ops.boundaries_arg)  ->  (py, px, pz), True for a
    periodic axis.  Only z is built: a periodic y or x is refused by name.  Anything else raises ValueError."""
    if isinstance(b, str):
        if b not in ("open", "periodic-z"):
            raise ValueError(BOUNDARIES3D_MESSAGE % (who, b))
        return False, False, b == "periodic-z"
    try:
        by, bx, bz = b
    except (TypeError, ValueError):
        raise ValueError(BOUNDARIES3D_MESSAGE % (who, b)) from None
    for v in (by, bx, bz):
        if not isinstance(v, str) or v not in ("open", "periodic"):
            raise ValueError(BOUNDARIES3D_MESSAGE % (who, b))
    for name, v in (("y", by), ("x", bx)):
        if v == "periodic":
            raise ValueError("%s: a periodic %s axis is not built for karman-3d: only the spanwise axis is ('periodic-z')" % (who, name))
    return False, False, bz == "periodic"


def boundaries_name3d(periodic):
    """(py, px, pz) back as a word boundaries_arg3d takes"""
    return "periodic-z" if periodic[2] else "open"


def _not_periodic(scene, what):
    """ValueError, by name, for what is not built for z-periodic scenes"""
    if getattr(scene, "periodic_bits", 0):
        raise ValueError("%s is not built for periodic scenes (Scene3D(boundaries='periodic-z')): the plain step, its velocity adjoint and the "
                         "pressure solve are" % what)


def buoyancy_force3d(buoyancy=None, buoyancy_factor=None, gravity=(-9.81, 0.0, 0.0)):
    """The force per unit density F = (fy, fx, fz) of the buoyant 3-D step, or None (off): ops.buoyancy_force's conventions with a third
    component.  `buoyancy`: F itself, one number (fy) or up to three (missing components are 0); else PhiFlow's spelling, F = -gravity *
    buoyancy_factor (Gravity() = -9.81 along y: F = (9.81 beta, 0, 0)).  A force of (0, 0, 0) is kept as given: the entry points take it
    and issue the plain launches."""
    if buoyancy is not None and buoyancy_factor is not None:
        raise ValueError("give buoyancy=(fy, fx, fz) or buoyancy_factor (with gravity), not both")
    if buoyancy is None and buoyancy_factor is None:
        return None
    if buoyancy is None:
        g = (float(gravity), 0.0, 0.0) if np.isscalar(gravity) else tuple(float(v) for v in gravity)
        if len(g) != 3:
            raise ValueError("gravity must be (gy, gx, gz), got %r" % (gravity,))
        buoyancy = tuple(-c * float(buoyancy_factor) for c in g)
    f = (float(buoyancy),) if np.isscalar(buoyancy) else tuple(float(v) for v in buoyancy)
    if not 1 <= len(f) <= 3 or not all(np.isfinite(f)):
        raise ValueError("buoyancy must be a finite force (fy, fx, fz), got %r" % (buoyancy,))
    return f + (0.0,) * (3 - len(f))


def _buoyant3d(buoyancy):
    """True for a force that moves the velocity: the density is then part of the dynamics"""
    return buoyancy is not None and any(v != 0.0 for v in buoyancy)


class StepPhysics3D(NamedTuple):
    """The physics of one 3-D step beyond the plain one, as every internal call carries it (the sibling of ops.StepPhysics).  The default
    is the plain step: the launches and the bits of a call without either keyword.  The two compose with each other, with density_grad
    and re_grad, both solvers and feat_out (whose fourth channel stays the true re).
    buoyancy = (fy, fx, fz), a force per unit density, or None: the step's OUTPUT density pushes the velocity (sol_karman3d_step_fwd_buoy:
    one launch more).  The density is then part of the dynamics: a differentiable step keeps it in the graph whatever density_grad says.
    nsub = n >= 1, the diffusion substeps (PhiFlow's diffuse(field, amount, substeps)): n explicit substeps of alpha / n, alpha = dt res^2
    / Re, the boundary blend after the last one -- diffuse_sub (M^(n-1) v), then the step's launches on Karman3DFlow.sub_cfg(n).  The
    single stencil is stable only while alpha <= 1/6 (min_diffusion_substeps3d gives the n a run needs)."""
    buoyancy: Optional[tuple] = None
    nsub: int = 1

    @classmethod
    def of(cls, buoyancy=None, buoyancy_factor=None, gravity=(-9.81, 0.0, 0.0), diffusion_substeps=1, who="diffusion_substeps", keep_zero_force=False):
        """From the user-facing keywords, validated (ValueError) by buoyancy_force3d and ops.diffusion_substeps_arg (`who` is how its message
        names the count).  A force of (0, 0, 0) becomes None, the plain step; keep_zero_force (torch.ops.sol.karman3d_step_buoy without a
        gradient) keeps it as given: the _buoy entry point takes it and issues the plain launches."""
        from .ops import diffusion_substeps_arg
        n = diffusion_substeps_arg(diffusion_substeps, who)
        f = buoyancy_force3d(buoyancy, buoyancy_factor, gravity)
        return cls(f if keep_zero_force or _buoyant3d(f) else None, n)

    def moving(self):
        """self, a kept force of (0, 0, 0) normalised to None: what a differentiable step runs on"""
        return self if self.buoyancy is None or _buoyant3d(self.buoyancy) else self._replace(buoyancy=None)

    mode = property(lambda self: "" if self.buoyancy is None else "_buoy", doc='the entry points of the step and its velocity adjoint: "" or "_buoy"')
    force_tail = property(lambda self: () if self.buoyancy is None else tuple(float(v) for v in self.buoyancy),
                          doc="the three floats a _buoy entry point takes after its plain sibling's arguments; () in the plain mode")


def _adv_workspace_bytes(lib, cfg):
    """the workspace the _adv entry points take under the MacCormack advection, the largest over the step, its velocity adjoint and its
    density adjoint, with and without re"""
    c = C.byref(cfg)
    return max(lib.sol_karman3d_step_fwd_adv_workspace_bytes(c, 1), lib.sol_karman3d_step_bwd_adv_workspace_bytes(c, 1, 1),
               lib.sol_karman3d_density_bwd_adv_workspace_bytes(c, 1, 1))


def _adv_tail(adv):
    """the two arguments an _adv entry point takes last: advection = 1 and the correction strength `adv` (ops.advection_arg's float)"""
    return (1, float(adv))


def _adjoint_entry(lib, half, mode="", re=False):
    """The lookup of an adjoint's entry point, sol_karman3d_<half><mode>[_re]: half "step_bwd" (mode: StepPhysics3D.mode) or "density_bwd" (none)"""
    return getattr(lib, "sol_karman3d_" + half + mode + ("_re" if re else ""))


# ---------------------------------------------------------------------------------------------------------------------
# diffusion substeps (include/sol_hip.h, "DIFFUSION SUBSTEPS of the karman-3d step"; csrc/karman3d_diffuse_sub.hip)
# ---------------------------------------------------------------------------------------------------------------------
def min_diffusion_substeps3d(re_min, res, dt=1.0):
    """The smallest n with dt res^2 / (n re_min) <= 1/6: the explicit 3-D diffusion stencil v += a Lap(v) is a convex combination of a
    face and its six neighbours exactly while a <= 1/6 (the 2-D bound, ops.min_diffusion_substeps, is 1/4).  re_min: the smallest
    Reynolds number of the run."""
    re_min, res, dt = float(re_min), float(res), float(dt)
    if not (re_min > 0 and res > 0 and dt > 0) or not np.isfinite(dt * res * res / re_min):
        raise ValueError("min_diffusion_substeps3d: re_min, res and dt must be positive and finite (got %r, %r, %r)" % (re_min, res, dt))
    alpha = dt * res * res / re_min
    n = max(1, int(np.ceil(6.0 * alpha)))
    while alpha / n > 1.0 / 6.0:
        n += 1
    while n > 1 and alpha / (n - 1) <= 1.0 / 6.0:
        n -= 1
    return n


def diffusion_sub_res(res, n):
    """`res` of the cfg the existing launches and the pre-diffusion run on under diffusion_substeps = n: float32(res / sqrt(n)), so that
    their own expression dt * res * res / re[b] is the substep's coefficient (ops.diffusion_sub_cfg's idea; res enters the 3-D kernels
    through that product alone).  re is NOT scaled: the feature channel keeps the true Reynolds number.  n = 1: res itself."""
    return float(res) if n == 1 else float(np.float32(float(res) / np.sqrt(float(n))))


def diffuse_sub_max3d():
    """S_MAX: the most substeps one launch of sol_karman3d_diffuse_sub runs"""
    return int(_lib.load().sol_karman3d_diffuse_sub_max())


# substeps per launch of the pre-diffusion where the caller names none (1 .. diffuse_sub_max3d()); the bits do not depend on it.
# Measured at 128 x 64 x 64, B = 1 (tools/k3d_substeps_time.py -> profiles/k3d_substeps_time.json): two substeps fused tie with two
# launches of one, three fused LOSE to three launches of one (supposed, not measured: the box of three faces a side is 3.6 times the
# tile's volume and leaves two workgroups a CU) -- so one substep per launch is the default; the fused path stays for callers that name a chunk.
DIFFUSE_SUB_CHUNK3D = 1


def diffuse_sub(sim, vy, vx, vz, re, nsub, chunk=None):
    """The pre-diffusion of a step with diffusion_substeps = nsub (sol_karman3d_diffuse_sub): (vy, vx, vz) -> M^(nsub-1) (vy, vx, vz),
    M = I + (alpha / nsub) L with alpha = dt res^2 / re of `sim` (a Karman3DFlow: its own, unscaled res) and L the 7-point Laplacian with
    replicate padding on each face grid.  M^(nsub-1) is symmetric: applied to a cotangent this is also the adjoint.  chunk: the most
    substeps per launch, 1 .. diffuse_sub_max3d() (None = DIFFUSE_SUB_CHUNK3D); the bits do not depend on it.  More than one launch
    ping-pongs through sim's pre-diffusion workspace (Karman3DFlow._sub_workspace: the static one of sim's own count, else a buffer of this
    call alone).  nsub = 1: no launch, the inputs are returned."""
    from .ops import diffusion_substeps_arg
    _not_periodic(getattr(sim, "scene", None), "diffuse_sub")
    n = diffusion_substeps_arg(nsub, "diffuse_sub: nsub")
    smax = diffuse_sub_max3d()
    chunk = DIFFUSE_SUB_CHUNK3D if chunk is None else chunk
    if isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or not 1 <= chunk <= smax:
        raise ValueError("diffuse_sub: chunk must be None or an integer in [1, %d] (got %r)" % (smax, chunk))
    _lib.require_gpu()
    vy, vx, vz, re = (_lib.f32(t) for t in (vy, vx, vz, re))
    if n == 1:
        return vy, vx, vz
    s, B = sim.scene, sim.B
    Y, X, Z = s.Y, s.X, s.Z
    if vy.shape != (B, Y + 1, X, Z) or vx.shape != (B, Y, X + 1, Z) or vz.shape != (B, Y, X, Z + 1) or re.shape != (B,):
        raise ValueError("diffuse_sub: vy %s, vx %s, vz %s, re %s are not [B,Y+1,X,Z], [B,Y,X+1,Z], [B,Y,X,Z+1], [B] of the scene (B, Y, X, Z) = "
                         "(%d, %d, %d, %d)" % (tuple(vy.shape), tuple(vx.shape), tuple(vz.shape), tuple(re.shape), B, Y, X, Z))
    cfg = sim.sub_cfg(n)
    ws, nbytes = sim._sub_workspace(cfg, n - 1, int(chunk))
    out = [torch.empty_like(t) for t in (vy, vx, vz)]
    check(sim.lib.sol_karman3d_diffuse_sub(C.byref(cfg), stream(), ptr(vy), ptr(vx), ptr(vz), ptr(re), ptr(out[0]), ptr(out[1]), ptr(out[2]),
                                           n - 1, int(chunk), ptr(ws), nbytes))
    return tuple(out)


PRESSURE_SOLVERS3D = ("auto", "direct", "cg", "direct_extruded")
CG_MAX_ITER3D = 120             # launch budget of the CG solve: 28-87 iterations measured at rtol 1e-6


class Scene3D:
    """Device-resident constants of a karman-3d scene: masks + the pressure-solver blob (precond3d).

    active [Y,X,Z] (1 = fluid, 0 = solid; default: scene_arrays3d's sphere) and inflow [Y,X,Z] (default: its inflow box).
    pressure_solver: "direct" = the capacitance-corrected direct solve (ValueError where precond3d.direct_solver_blob3d refuses
    the mask), "cg" = the preconditioned CG solve (any mask; the blob without capacitance part), "auto" = direct where the blob
    builds, else CG.  "direct_extruded" (opt-in; "auto" never picks it) = the direct solve for an obstacle extruded along z, active[j, i, k]
    = a2[j, i] for every k -- the cylinder of the wake, which the dense blob refuses at 128 x 64 x 64: Z capacitance systems on the in-plane
    set between two sine transforms of the support columns (precond3d.extruded_solver_blob3d; ValueError with its reason where it refuses:
    a mask that depends on z, no obstacle, size, conditioning).  The choice is `self.pressure_solver` ("direct", "cg" or
    "direct_extruded"); everything that takes a scene treats "direct_extruded" as it treats "direct": no iteration, no report, capturable.

    boundaries: "open" (default), "periodic-z" or a triple (by, bx, bz) of "open" / "periodic" (boundaries_arg3d; a periodic y or x is
    refused by name) -> self.periodic = (py, px, pz), self.periodic_bits (0 or PERIODIC_Z).  A z-periodic scene (include/sol_hip.h,
    "PERIODIC SPANWISE BOUNDARIES"): the default velBC mask has no z walls, and the blob is a periodic one -- "direct": precond3d.
    periodic_solver_blob3d, "direct_extruded": extruded_solver_blob3d(periodic=True), "auto": the dense direct solve where it builds,
    else a ValueError that names direct_extruded; "cg" is refused by name.  Array shapes do not change: v_z[..., Z] duplicates plane 0."""

    def __init__(self, Y, X, Z, length=100.0, device="cuda", velBCy=None, velBCyMask=None, active=None, inflow=None, pressure_solver="auto",
                 boundaries="open"):
        from .precond3d import direct_solver_blob3d, extruded_solver_blob3d, periodic_solver_blob3d
        if pressure_solver not in PRESSURE_SOLVERS3D:
            raise ValueError("pressure_solver must be one of %s, got %r" % (PRESSURE_SOLVERS3D, pressure_solver))
        self.periodic = boundaries_arg3d(boundaries, "Scene3D: boundaries")
        self.periodic_bits = PERIODIC_Z if self.periodic[2] else 0
        if self.periodic_bits and pressure_solver == "cg":
            raise ValueError("pressure_solver='cg' is not built for periodic scenes (boundaries=%r): 'direct' and 'direct_extruded' are" % (boundaries,))
        self.Y, self.X, self.Z = Y, X, Z
        self.dx = length / X
        if active is None or inflow is None:
            act0, inf0 = scene_arrays3d(Y, X, Z, length)
            active = act0 if active is None else active
            inflow = inf0 if inflow is None else inflow
        active = np.asarray(active, dtype=np.float64)
        inflow = np.asarray(inflow, dtype=np.float64)
        if active.shape != (Y, X, Z) or inflow.shape != (Y, X, Z):
            raise ValueError("active / inflow must be [Y,X,Z] = %s, got %s / %s" % ((Y, X, Z), active.shape, inflow.shape))
        if not np.all((active == 0.0) | (active == 1.0)):
            raise ValueError("active must hold 0 (solid) and 1 (fluid) only")
        bcv, bcm = velocity_bc_masks3d(Y, X, Z, self.periodic[2])
        if velBCy is not None:
            bcv, bcm = np.asarray(velBCy, dtype=np.float64), np.asarray(velBCyMask, dtype=np.float64)
        n = (Y + 1) * X * Z
        if bcv.size % n or bcv.size != bcm.size:
            raise ValueError("velBCy / velBCyMask must be [Y+1,X,Z] or [B,Y+1,X,Z]")
        self.bc_stride = 0 if bcv.size == n else n
        self.active_np = active
        self.active = _lib.f32(active, device)
        self.inflow = _lib.f32(inflow, device)
        self.velBCy = _lib.f32(bcv, device)
        self.velBCyMask = _lib.f32(bcm, device)
        if pressure_solver == "direct_extruded":
            why = []
            blob = extruded_solver_blob3d(active, why, **({"periodic": True} if self.periodic_bits else {}))
            if blob is None:
                raise ValueError("pressure_solver='direct_extruded' does not support this scene (%dx%dx%d): %s" % (Y, X, Z, why[0]))
        elif self.periodic_bits:
            why = []
            blob = periodic_solver_blob3d(active, why)
            if blob is None:
                raise ValueError("the direct pressure solver does not support this z-periodic scene (%dx%dx%d): %s%s" % (
                    Y, X, Z, why[0], "; pressure_solver='direct_extruded' takes an obstacle extruded along z" if pressure_solver == "auto" else ""))
        else:
            blob = direct_solver_blob3d(active) if pressure_solver != "cg" else None
        if blob is None and pressure_solver == "direct":
            raise ValueError("the direct pressure solver does not support this scene (%dx%dx%d)" % (Y, X, Z))
        self.pressure_solver = "direct_extruded" if pressure_solver == "direct_extruded" else ("direct" if blob is not None else "cg")
        if blob is None:
            blob = direct_solver_blob3d(np.ones_like(active))        # the CG preconditioner: the empty-box solve (nS = 0)
        self.direct = torch.from_numpy(blob).to(device)
        self.direct_header = np.ascontiguousarray(blob[:16].view(np.int32))


class Karman3DFlow:
    """`simulator.step(...)` of the 3-D scene: one sol_karman3d_step_fwd.

    cg_rtol / cg_atol / cg_max_iter: the CG solve of a scene with pressure_solver == "cg" (names and tolerances of the 2-D
    KarmanFlow; cg_max_iter is the fixed launch budget).  After a forward step on such a scene `solve_info` holds "iterations"
    and "converged" (device int32 [B]); the adjoint adds "iterations_bwd" and "converged_bwd".  The direct solve reports nothing.

    density_grad=True (opt-in): the density output of `step` is differentiable too.  re_grad=True (opt-in): a tensor `re` that requires
    a gradient receives one.  With both off the density is a passive tracer and `re` is data (_step_adjoint3d describes the modes).

    buoyancy=(fy, fx, fz), a force per unit density, or PhiFlow's spelling buoyancy_factor=beta with gravity=(gy, gx, gz): F = -gravity *
    beta (buoyancy_force3d), and diffusion_substeps=n are kept as `self.physics`, one StepPhysics3D built here (see there; a force of
    zero is none).  The defaults issue the launches the step always did.

    advection="mac_cormack", correction_strength=s (0 <= s <= 1): the MacCormack advection (include/sol_hip.h, "MACCORMACK ADVECTION on the
    karman-3d step") in place of the semi-Lagrangian one, forward and adjoint; validated by ops.advection_arg before the device is asked
    for and kept as `self.adv` (None for "semi_lagrangian", else the float s) BESIDE the physics value, which has no field for it.  It
    composes with everything above."""

    buoyancy = property(lambda self: self.physics.buoyancy)
    nsub = property(lambda self: self.physics.nsub)

    def __init__(self, scene, batch_size, dt=1.0, res=None, grad_pad="replicate", inflow_order="after",
                 cg_rtol=1e-6, cg_atol=1e-9, cg_max_iter=CG_MAX_ITER3D, density_grad=False, re_grad=False,
                 buoyancy=None, buoyancy_factor=None, gravity=(-9.81, 0.0, 0.0), diffusion_substeps=1,
                 advection="semi_lagrangian", correction_strength=1.0):
        from .ops import advection_arg
        self.physics = StepPhysics3D.of(buoyancy, buoyancy_factor, gravity, diffusion_substeps, "Karman3DFlow: diffusion_substeps")
        self.adv = advection_arg(advection, correction_strength, "Karman3DFlow: advection")
        if getattr(scene, "periodic_bits", 0):      # what is not built for z-periodic scenes, by name
            for on, what in ((self.adv is not None, "advection='mac_cormack'"), (self.physics.buoyancy is not None, "a non-zero buoyancy"),
                             (self.physics.nsub > 1, "diffusion_substeps > 1"), (density_grad, "density_grad"), (re_grad, "re_grad")):
                if on:
                    _not_periodic(scene, "Karman3DFlow: " + what)
        _lib.require_gpu()
        self.lib = _lib.load()
        self.scene, self.B = scene, batch_size
        self.density_grad, self.re_grad = bool(density_grad), bool(re_grad)
        s = scene
        self.cg = s.pressure_solver == "cg"
        self.cfg = Karman3DCfg(batch_size, s.Y, s.X, s.Z, float(s.dx), float(dt), float(s.X if res is None else res),
                               {"replicate": 0, "dirichlet0": 1}[grad_pad], {"after": 0, "before": 1}[inflow_order],
                               s.direct.numel(), s.direct.data_ptr(),
                               1 if self.cg else 0, int(cg_max_iter), float(cg_rtol), float(cg_atol), None)
        nbytes = max(self.lib.sol_karman3d_step_workspace_bytes(C.byref(self.cfg)), self.lib.sol_karman3d_step_bwd_workspace_bytes(C.byref(self.cfg)))
        if self.adv is not None:            # the MacCormack launches' parts, every mode: sized once, here (a captured graph bakes the address in)
            nbytes = max(nbytes, _adv_workspace_bytes(self.lib, self.cfg))
        self.workspace = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=s.active.device)
        self.workspace_bytes = nbytes
        self.solve_info = {}
        # the pre-diffusion's ping-pong buffers for this simulator's own count: allocated once, here, and never replaced (a captured graph
        # bakes their address in)
        nbytes = self.lib.sol_karman3d_diffuse_sub_workspace_bytes(C.byref(self.cfg), self.nsub - 1, DIFFUSE_SUB_CHUNK3D) if self.nsub > 1 else 0
        self._sub_ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=s.active.device) if nbytes else None
        self._sub_ws_bytes = nbytes

    def _sub_workspace(self, cfg, m, chunk):
        """(workspace, bytes) of sol_karman3d_diffuse_sub(cfg, m substeps, chunk): (None, 0) for a single launch, the simulator's static
        buffer where it is large enough (its own count), else a buffer of this call alone (another count through diffuse_sub or the torch
        op on a simulator built without one: the static buffer is never grown or replaced)"""
        nbytes = self.lib.sol_karman3d_diffuse_sub_workspace_bytes(C.byref(cfg), m, chunk)
        if nbytes == 0:
            return None, 0
        if nbytes <= self._sub_ws_bytes:
            return self._sub_ws, self._sub_ws_bytes
        return torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=self.scene.active.device), nbytes

    def sub_cfg(self, n):
        """The cfg the existing launches (_fwd, _bwd, density_bwd) and the pre-diffusion run on under diffusion_substeps = n: a COPY whose
        res is diffusion_sub_res(res, n), so that their own dt res^2 / re[b] is the substep's coefficient alpha / n; n = 1: the
        simulator's own cfg.  The simulator's cfg is never modified."""
        if n == 1:
            return self.cfg
        c = Karman3DCfg.from_buffer_copy(self.cfg)
        c.res = diffusion_sub_res(self.cfg.res, n)
        return c

    def _cg_info(self, cfg):
        """a fresh device report [B][2] for the next call on `cfg` (a captured graph keeps its own), or None for the direct solve"""
        if not self.cg:
            cfg.cg_info = None
            return None
        info = torch.empty(self.B, 2, dtype=torch.int32, device=self.scene.active.device)      # (every solve writes it)
        cfg.cg_info = info.data_ptr()
        return info

    def _forward(self, ph, d, vy, vx, vz, re, saved=None, feat_out=None, feat_scale=None, pre_diffuse=True, adv=None):
        """THE forward launch site: one step under the StepPhysics3D `ph`  ->  ((d, vy, vx, vz) after the step, the velocity the launches
        read).  ph.nsub > 1: the pre-diffusion (diffuse_sub; not with pre_diffuse=False: the caller has run it), then the launches on
        sub_cfg(ph.nsub) -- the velocity handed back is then M^(n-1) v, "the input velocity" the re mode saves.  ph.buoyancy:
        sol_karman3d_step_fwd_buoy (a kept force of zero issues the plain call's launches).  adv = s (ops.advection_arg: a float for
        "mac_cormack", None for "semi_lagrangian"): sol_karman3d_step_fwd_adv with the force, or a zero force, then (1, s)."""
        if ph.buoyancy is not None or ph.nsub > 1 or adv is not None:
            _not_periodic(self.scene, "Karman3DFlow: a step with buoyancy, diffusion substeps or MacCormack advection")
        if pre_diffuse and ph.nsub > 1:
            vy, vx, vz = diffuse_sub(self, vy, vx, vz, re, ph.nsub)
        cfg = self.sub_cfg(ph.nsub)
        s, B = self.scene, self.B
        Y, X, Z = s.Y, s.X, s.Z
        assert d.shape == (B, Y, X, Z) and vy.shape == (B, Y + 1, X, Z) and vx.shape == (B, Y, X + 1, Z) and vz.shape == (B, Y, X, Z + 1)
        assert re.shape == (B,)
        out = [torch.empty_like(t) for t in (d, vy, vx, vz)]
        fs = None
        if feat_out is not None:
            assert feat_out.shape == (B, Y, X, Z, 4) and feat_out.is_contiguous()
            fs = (C.c_float * 4)(*[float(v) for v in feat_scale])
        sv = saved if saved is not None else (None, None, None)
        info = self._cg_info(cfg)
        entry, tail = getattr(self.lib, "sol_karman3d_step_fwd" + (ph.mode if adv is None else "_adv")), ph.force_tail
        if adv is not None:
            self._ws(self.lib.sol_karman3d_step_fwd_adv_workspace_bytes(C.byref(cfg), 1))
            tail = (tail or (0.0, 0.0, 0.0)) + _adv_tail(adv)
        check(entry(C.byref(cfg), stream(), ptr(d), ptr(vy), ptr(vx), ptr(vz), ptr(re),
                    ptr(s.active), ptr(s.inflow), ptr(s.velBCy), ptr(s.velBCyMask), s.bc_stride,
                    ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), ptr(sv[0]), ptr(sv[1]), ptr(sv[2]), ptr(feat_out), fs,
                    s.direct_header.ctypes.data_as(C.c_void_p), ptr(self.workspace), self.workspace_bytes, *tail))
        if info is not None:
            self.solve_info = {"iterations": info[:, 0], "converged": info[:, 1]}
        return tuple(out), (vy, vx, vz)

    def _fwd(self, d, vy, vx, vz, re, saved=None, feat_out=None, feat_scale=None, buoyancy=None, nsub=1, physics=None, pre_diffuse=False, adv=None):
        """the step's outputs of _forward's launches alone (the caller has pre-diffused the velocity); `physics` replaces buoyancy= / nsub="""
        ph = physics if physics is not None else StepPhysics3D(buoyancy, nsub)
        return self._forward(ph, d, vy, vx, vz, re, saved, feat_out, feat_scale, pre_diffuse, adv=adv)[0]

    def _fwd_sub(self, *args, **kw):
        """_fwd with the pre-diffusion"""
        return self._fwd(*args, pre_diffuse=True, **kw)

    def _ws(self, nbytes):
        """the workspace, grown to nbytes where a call needs more than the step and its velocity adjoint (the opt-in adjoints)"""
        if nbytes > self.workspace_bytes:
            self.workspace = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=self.scene.active.device)
            self.workspace_bytes = nbytes
        return self.workspace

    def _re_tail(self, saved, vel_in, g_re):
        """the five arguments an _re entry point takes after its plain sibling's: the step's INPUT velocity, g_re [B] (the caller's buffer
        to add onto, or None for a fresh one to write) and accumulate_re  ->  (arguments, g_re)"""
        vel_in = [_lib.f32(t) for t in vel_in]
        if [t.shape for t in vel_in] != [t.shape for t in saved]:
            raise ValueError("the step's input velocity must have the saved velocity's shapes")
        accumulate = g_re is not None
        if not accumulate:
            g_re = torch.empty(self.B, dtype=torch.float32, device=saved[0].device)
        elif g_re.shape != (self.B,):
            raise ValueError("g_re must be [B] = (%d,), got %s" % (self.B, tuple(g_re.shape)))
        return (ptr(vel_in[0]), ptr(vel_in[1]), ptr(vel_in[2]), ptr(g_re), int(accumulate)), g_re

    def _bwd(self, saved, re, gvy, gvx, gvz, vel_in=None, g_re=None, buoyancy=None, g_d=None, nsub=1, physics=None, adv=None):
        """the velocity adjoint, the direct call (sol_karman3d_step_bwd); vel_in = the step's input velocity: also the gradient with respect
        to re (sol_karman3d_step_bwd_re; the velocity gradients are the plain call's bits) -> [g_vy, g_vx, g_vz] (+ [g_re]).
        buoyancy = (fy, fx, fz): the buoyant step's (sol_karman3d_step_bwd_buoy(_re): the same launches and bits, then the transpose of the
        force term); g_d [B,Y,X,Z] = the cotangent of the step's output density (None = zero) -> ... + [g_dsum], which the caller hands to
        density_bwd as its g_d, accumulating onto the velocity gradients returned here.  `physics` replaces buoyancy= / nsub=.
        adv = s (the MacCormack step's): the _adv entries, sol_karman3d_step_bwd_adv(_re), which take the force (zero, with NULL g_d /
        g_dsum, where there is none) and then (1, s); the list returned is the same.
        _step_adjoint3d composes this with density_bwd and the substep tail, and is the one place that takes this list apart."""
        s = self.scene
        ph = physics if physics is not None else StepPhysics3D(buoyancy, nsub)
        if ph.buoyancy is not None or ph.nsub > 1 or adv is not None or vel_in is not None:
            _not_periodic(s, "Karman3DFlow: the adjoint of a step with buoyancy, diffusion substeps or MacCormack advection, and the gradient in re (re_grad)")
        cfg = self.sub_cfg(ph.nsub)         # (nsub > 1: `saved` / vel_in are the pre-diffused step's; the result is the cotangent of M^(n-1) v, g_re 1/n)
        gi = [torch.empty_like(t) for t in saved]
        info = self._cg_info(cfg)
        buoy = ph.buoyancy is not None
        entry, tail = _adjoint_entry(self.lib, "step_bwd", ph.mode if adv is None else "_adv", vel_in is not None), ()
        if adv is not None:
            self._ws(self.lib.sol_karman3d_step_bwd_adv_workspace_bytes(C.byref(self.cfg), int(vel_in is not None), 1))
        if vel_in is not None:
            self._ws(self.lib.sol_karman3d_step_bwd_re_workspace_bytes(C.byref(self.cfg)))
            tail, g_re = self._re_tail(saved, vel_in, g_re)
        g_dsum = None
        if buoy:
            if g_d is not None:
                g_d = _lib.f32(g_d)
                if g_d.shape != (self.B, s.Y, s.X, s.Z):
                    raise ValueError("g_d must be [B,Y,X,Z] = %s, got %s" % ((self.B, s.Y, s.X, s.Z), tuple(g_d.shape)))
            g_dsum = torch.empty(self.B, s.Y, s.X, s.Z, dtype=torch.float32, device=saved[0].device)
            tail = tuple(tail) + ph.force_tail + (ptr(g_d), ptr(g_dsum))
        elif adv is not None:
            tail = tuple(tail) + (0.0, 0.0, 0.0, None, None)
        if adv is not None:
            tail = tuple(tail) + _adv_tail(adv)
        check(entry(C.byref(cfg), stream(), ptr(saved[0]), ptr(saved[1]), ptr(saved[2]), ptr(re),
                    ptr(s.active), ptr(s.velBCyMask), s.bc_stride, ptr(gvy), ptr(gvx), ptr(gvz),
                    ptr(gi[0]), ptr(gi[1]), ptr(gi[2]),
                    s.direct_header.ctypes.data_as(C.c_void_p), ptr(self.workspace), self.workspace_bytes, *tail))
        if info is not None:
            self.solve_info = dict(self.solve_info, iterations_bwd=info[:, 0], converged_bwd=info[:, 1])
        res = gi if vel_in is None else gi + [g_re]
        return res + [g_dsum] if buoy else res

    def pressure_solve(self, rhs):
        """The step's pressure solve alone (sol_karman3d_pressure_solve): p with M p = rhs, M = -A for the scene's mask; rhs [B,Y,X,Z].
        No gradient.  A CG scene reports to solve_info["iterations"] / ["converged"]."""
        s = self.scene
        rhs = _lib.f32(rhs)
        assert rhs.shape == (self.B, s.Y, s.X, s.Z)
        p = torch.empty_like(rhs)
        info = self._cg_info(self.cfg)
        check(self.lib.sol_karman3d_pressure_solve(C.byref(self.cfg), stream(), ptr(s.active), ptr(rhs), ptr(p),
                                                   s.direct_header.ctypes.data_as(C.c_void_p), ptr(self.workspace), self.workspace_bytes))
        if info is not None:
            self.solve_info = {"iterations": info[:, 0], "converged": info[:, 1]}
        return p

    def step(self, d, vy, vx, vz, re, feat_out=None, feat_scale=None):
        """(d, vy, vx, vz) -> new tensors after one solver step.  Differentiable with respect to the velocity when a velocity input requires
        grad -- and to the density (density_grad, or a buoyancy force: taken when any of d, vy, vx, vz requires a gradient) and to a tensor
        `re` that requires one (re_grad): _step_adjoint3d.  feat_out [B,Y,X,Z,4] (optional, no-grad use) receives the scaled features."""
        d, vy, vx, vz, re = (_lib.f32(t) for t in (d, vy, vx, vz, re))
        grad = torch.is_grad_enabled()
        want_re = self.re_grad and grad and re.requires_grad
        density = self.density_grad or self.physics.buoyancy is not None
        if grad and (vy.requires_grad or vx.requires_grad or vz.requires_grad or (density and d.requires_grad) or want_re):
            if feat_out is not None:
                raise ValueError("feat_out is the fused no-grad feature output: build the features with to_feature3d() when training")
            return _Karman3DStepFn.apply(self, d, vy, vx, vz, re, density, want_re, self.physics, self.adv)
        return self._forward(self.physics, d, vy, vx, vz, re, None, feat_out, feat_scale, adv=self.adv)[0]


def density_bwd(sim, d_in, saved, re, g_d, g_v=None, vel_in=None, g_re=None, nsub=1, adv=None):
    """Adjoint of the 3-D step's marker density (sol_karman3d_density_bwd), the direct call: (g_d_in, g_vy_in, g_vx_in, g_vz_in) from the
    step's input density `d_in`, the saved post-diffusion velocity `saved` = (svy, svx, svz), `re` and the gradient `g_d` with respect
    to the step's output density; `sim` = the Karman3DFlow (scene, cfg, workspace).  g_v = (g_vy, g_vx, g_vz): buffers that already hold
    the velocity adjoint's result; the density's part is added onto them in place (one fp32 add per face) and they are returned.  Without
    them the density's part alone is written to fresh tensors.  vel_in = (vy, vx, vz), the step's INPUT velocity: the gradient with
    respect to re as well (sol_karman3d_density_bwd_re), returned fifth; g_re [B]: a buffer to add onto, else a fresh one is written.
    nsub (diffusion substeps: StepPhysics3D.nsub): the launches run on sim.sub_cfg(nsub); `saved` / vel_in are then those of
    the pre-diffused velocity, the velocity gradients are the cotangent of M^(n-1) v and g_re is 1/n of the gradient -- a g_re to add onto
    must hold such a part too (the factor n is applied once, afterwards: _step_adjoint3d).  adv = s (the MacCormack step's): the _adv
    entries, sol_karman3d_density_bwd_adv(_re), which take (1, s) last."""
    _not_periodic(getattr(sim, "scene", None), "density_bwd")
    _lib.require_gpu()
    s, B = sim.scene, sim.B
    Y, X, Z = s.Y, s.X, s.Z
    d_in, re, g_d = (_lib.f32(t) for t in (d_in, re, g_d))
    saved = [_lib.f32(t) for t in saved]
    shapes = (("d_in", d_in, (B, Y, X, Z)), ("g_d", g_d, (B, Y, X, Z)), ("svy", saved[0], (B, Y + 1, X, Z)), ("svx", saved[1], (B, Y, X + 1, Z)),
              ("svz", saved[2], (B, Y, X, Z + 1)), ("re", re, (B,)))
    for name, t, shape in shapes:
        if t.shape != shape:
            raise ValueError("density_bwd: %s is %s, not %s of the scene" % (name, tuple(t.shape), shape))
    accumulate = g_v is not None
    if accumulate and [t.shape for t in g_v] != [t.shape for t in saved]:
        raise ValueError("density_bwd: g_v must have the velocity's shapes")
    want_re = vel_in is not None
    entry, tail = _adjoint_entry(sim.lib, "density_bwd", "" if adv is None else "_adv", want_re), ()
    nbytes = (sim.lib.sol_karman3d_density_bwd_re_workspace_bytes if want_re else sim.lib.sol_karman3d_density_bwd_workspace_bytes)(C.byref(sim.cfg))
    if adv is not None:
        nbytes = sim.lib.sol_karman3d_density_bwd_adv_workspace_bytes(C.byref(sim.cfg), int(want_re), 1)
    if want_re:
        tail, g_re = sim._re_tail(saved, vel_in, g_re)
    if adv is not None:
        tail = tuple(tail) + _adv_tail(adv)
    gi = list(g_v) if accumulate else [torch.empty_like(t) for t in saved]
    od = torch.empty_like(d_in)
    ws = sim._ws(nbytes)
    check(entry(C.byref(sim.sub_cfg(nsub)), stream(), ptr(d_in), ptr(s.inflow), ptr(saved[0]), ptr(saved[1]), ptr(saved[2]), ptr(re),
                ptr(s.velBCyMask), s.bc_stride, ptr(g_d), ptr(od), ptr(gi[0]), ptr(gi[1]), ptr(gi[2]), int(accumulate),
                ptr(ws), sim.workspace_bytes, *tail))
    return (od, *gi) if vel_in is None else (od, *gi, g_re)


def _advect3d_inputs(who, sim, d, svy, svx, svz):
    s, B = sim.scene, sim.B
    Y, X, Z = s.Y, s.X, s.Z
    d, svy, svx, svz = (_lib.f32(t) for t in (d, svy, svx, svz))
    if d.shape != (B, Y, X, Z) or svy.shape != (B, Y + 1, X, Z) or svx.shape != (B, Y, X + 1, Z) or svz.shape != (B, Y, X, Z + 1):
        raise ValueError("%s: d %s, svy %s, svx %s, svz %s are not [B,Y,X,Z], [B,Y+1,X,Z], [B,Y,X+1,Z], [B,Y,X,Z+1] of the scene (B, Y, X, Z) = "
                         "(%d, %d, %d, %d)" % (who, tuple(d.shape), tuple(svy.shape), tuple(svx.shape), tuple(svz.shape), B, Y, X, Z))
    return d, svy, svx, svz


def _adv_pair(adv):
    """(advection, correction_strength) of the stage's entry points from ops.advection_arg's value"""
    return (0, 1.0) if adv is None else (1, float(adv))


def advect3d(sim, d, svy, svx, svz, adv=None):
    """The advection stage of the 3-D step alone (sol_karman3d_advect) on a given post-diffusion velocity (svy, svx, svz): -> (d_out, a_y,
    a_x, a_z), the velocity times the hard-BC face masks, the inflow added as the simulator's inflow_order says.  adv: None = the
    semi-Lagrangian launch of the step, a float s = MacCormack with that correction strength (ops.advection_arg).  Any Y, X, Z >= 8."""
    _not_periodic(getattr(sim, "scene", None), "advect3d")
    _lib.require_gpu()
    d, svy, svx, svz = _advect3d_inputs("advect3d", sim, d, svy, svx, svz)
    s = sim.scene
    advection, strength = _adv_pair(adv)
    nbytes = sim.lib.sol_karman3d_advect_workspace_bytes(C.byref(sim.cfg), advection)
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=d.device) if nbytes else None
    out = [torch.empty_like(t) for t in (d, svy, svx, svz)]
    check(sim.lib.sol_karman3d_advect(C.byref(sim.cfg), stream(), ptr(d), ptr(svy), ptr(svx), ptr(svz), ptr(s.active), ptr(s.inflow), advection, strength,
                                      ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), ptr(ws), nbytes))
    return tuple(out)


def advect3d_bwd(sim, d, svy, svx, svz, g_d, g_ay, g_ax, g_az, adv=None, tile_window=True):
    """The transpose of advect3d (sol_karman3d_advect_bwd): the cotangents of (d_out, a_y, a_x, a_z) -> (g_d_in, g_svy, g_svx, g_svz), every
    decision of the forward stage frozen.  tile_window: the semi-Lagrangian scatters go through their LDS windows (False: global atomics
    only; equal bits)."""
    _not_periodic(getattr(sim, "scene", None), "advect3d_bwd")
    _lib.require_gpu()
    d, svy, svx, svz = _advect3d_inputs("advect3d_bwd", sim, d, svy, svx, svz)
    g = [_lib.f32(t) for t in (g_d, g_ay, g_ax, g_az)]
    if [t.shape for t in g] != [t.shape for t in (d, svy, svx, svz)]:
        raise ValueError("advect3d_bwd: the cotangents must have the shapes of d, svy, svx, svz")
    s = sim.scene
    advection, strength = _adv_pair(adv)
    nbytes = sim.lib.sol_karman3d_advect_bwd_workspace_bytes(C.byref(sim.cfg))
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=d.device)
    out = [torch.empty_like(t) for t in (d, svy, svx, svz)]
    check(sim.lib.sol_karman3d_advect_bwd(C.byref(sim.cfg), stream(), ptr(d), ptr(svy), ptr(svx), ptr(svz), ptr(s.active), ptr(s.inflow), advection, strength,
                                          ptr(g[0]), ptr(g[1]), ptr(g[2]), ptr(g[3]), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]),
                                          int(bool(tile_window)), ptr(ws), nbytes))
    return tuple(out)


def _step_adjoint3d(sim, ph, density, d_in, saved, re, gd, gv, vel_in=None, through_substeps=True, adv=None):
    """THE adjoint of one step of `sim` under the StepPhysics3D `ph` (a moving force or none: StepPhysics3D.moving): the velocity half
    (Karman3DFlow._bwd, with the pressure solve), the density half (density_bwd) and the substep tail are composed here and nowhere else
    (_Karman3DStepFn.backward, the reverse sweep of Karman3DTrainer).  `saved` = the post-diffusion velocity the forward kept, d_in = the
    step's input density (the density half reads it), gd / gv = (gvy, gvx, gvz) = the cotangents of the step's outputs, None where none
    arrived; vel_in = the velocity the forward launches read: the gradient in re as well (the _re entries, the opt-in `want_re`)
    ->  (g_d, g_vy, g_vx, g_vz, g_re), None where nothing reaches it.
    Plain (no force, `density` and vel_in off): the velocity half runs unconditionally; the density is a passive tracer, re is data.
    `density` or vel_in: the velocity half runs only when a velocity cotangent arrived, the density half only when gd did (`density`);
    both together accumulate onto the velocity half's buffers and g_re.
    A force: whenever any cotangent arrived the velocity half runs through its buoyant entry (zeros for a missing velocity cotangent, gd =
    None a null pointer; the plain launches and the transpose of the force term, g_dsum = g_d + dt F . transpose(g_a)), then the density
    half on g_dsum, accumulating: a velocity-only loss yields a density gradient too.  No cotangent at all: nothing is launched.
    ph.nsub = n > 1: both halves ran on the scaled cfg, their velocity result is the cotangent of M^(n-1) v and g_re 1/n of the gradient;
    the tail is diffuse_sub on that cotangent (the operator is symmetric; not with through_substeps=False, for a caller that does not
    read it) and g_re times n (one fp32 multiply).
    adv = s (ops.advection_arg): the step ran the MacCormack advection; both halves are handed adv= (only then) and run their _adv entries."""
    moving, want_re = ph.buoyancy is not None, vel_in is not None
    akw = {} if adv is None else {"adv": adv}
    some_v = any(g is not None for g in gv)
    gd = None if gd is None else gd.contiguous()
    gi = g_re = od = None
    if (moving and gd is not None) or some_v or not (moving or density or want_re):
        res = sim._bwd(saved, re, *(torch.zeros_like(t) if g is None else g.contiguous() for g, t in zip(gv, saved)), vel_in=vel_in,
                       g_d=gd if moving else None, physics=ph, **akw)
        gi, g_re = res[:3], (res[3] if want_re else None)
        gd = res[-1] if moving else gd                  # g_dsum
    if (moving or density) and gd is not None:
        od, *gi = density_bwd(sim, d_in, saved, re, gd, gi, vel_in, g_re, nsub=ph.nsub, **akw)
        g_re = gi.pop() if want_re else None
    if ph.nsub > 1:
        if through_substeps and gi is not None:
            gi = diffuse_sub(sim, gi[0], gi[1], gi[2], re, ph.nsub)
        if g_re is not None:
            g_re = g_re * float(ph.nsub)
    return (od, *(gi if gi is not None else (None,) * 3), g_re)


class _Karman3DStepFn(torch.autograd.Function):
    """One solver step under a StepPhysics3D with its hand-written adjoint: Karman3DFlow._forward, which also hands back the velocity its
    launches read ("the input velocity" the `want_re` mode saves beside the post-diffusion one), and _step_adjoint3d, which describes the
    modes.  `density`: the density output stays in the graph (always under a force)."""

    @staticmethod
    def forward(ctx, sim, d, vy, vx, vz, re, density, want_re, ph=StepPhysics3D(), adv=None):
        vel = [vy.contiguous(), vx.contiguous(), vz.contiguous()]
        saved = [torch.empty_like(t) for t in vel]
        density = bool(density) or ph.buoyancy is not None
        out, vel = sim._forward(ph, d, *vel, re, saved, adv=adv)
        ctx.sim, ctx.density, ctx.want_re, ctx.physics, ctx.adv = sim, density, want_re, ph, adv
        ctx.save_for_backward(re, *saved, *((d,) if density else ()), *(vel if want_re else ()))
        if not density:
            ctx.mark_non_differentiable(out[0])
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, gd, gvy, gvx, gvz):
        re, sy, sx, sz, *rest = ctx.saved_tensors
        d_in = rest[0] if ctx.density else None
        vel_in = tuple(rest[-3:]) if ctx.want_re else None
        return (None, *_step_adjoint3d(ctx.sim, ctx.physics, ctx.density, d_in, (sy, sx, sz), re, gd, (gvy, gvx, gvz), vel_in, adv=ctx.adv),
                None, None, None, None)


def _seam3d(entry, scene, vz):
    if vz.dtype != torch.float32 or not vz.is_contiguous() or vz.dim() != 4 or vz.shape[1:] != (scene.Y, scene.X, scene.Z + 1):
        raise ValueError("%s: v_z must be a contiguous float32 [B,Y,X,Z+1] tensor of the scene, got %s %s" % (entry, vz.dtype, tuple(vz.shape)))
    _lib.require_gpu()
    check(getattr(_lib.load(), entry)(stream(), ptr(vz), vz.shape[0], scene.Y, scene.X, scene.Z, scene.periodic_bits))
    return vz


def seam_sync3d(scene, vz):
    """In place on a z-periodic scene (sol_karman3d_seam_sync): plane 0 of v_z [B,Y,X,Z+1] copied onto the duplicate plane Z -- after a
    correction, which leaves the duplicate plane behind.  An open scene: nothing is launched.  Returns vz."""
    return _seam3d("sol_karman3d_seam_sync", scene, vz)


def seam_fold3d(scene, g_vz):
    """In place, the adjoint of seam_sync3d (sol_karman3d_seam_fold): g[..., 0] += g[..., Z], then g[..., Z] = 0.  Returns g_vz."""
    return _seam3d("sol_karman3d_seam_fold", scene, g_vz)


class _SeamSync3DFn(torch.autograd.Function):
    """seam_sync3d out of place, with seam_fold3d as its backward (the autograd schedule of Karman3DTrainer)"""

    @staticmethod
    def forward(ctx, vz, scene):
        ctx.scene = scene
        return seam_sync3d(scene, _lib.dclone(vz.contiguous()))

    @staticmethod
    def backward(ctx, g):
        return seam_fold3d(ctx.scene, _lib.dclone(g.contiguous())), None


class _ToFeature3DFn(torch.autograd.Function):
    """to_feature3d as one node with a backward made of kernels only: the autograd backward of `vy[:, :Y]` is zeros + a copy into a
    narrow, and with B = 1 that narrow is contiguous -- a hipMemcpyAsync, i.e. a memcpy node per unrolled step in the captured trainer
    (refused by sol_graph_check).  Here: zero-padding of the strided channel slices (fill + strided copy kernels).  A tensor `re` that
    requires a gradient stays in the graph: its gradient is the sum of the fourth channel's per simulation (taken only then)."""

    @staticmethod
    def forward(ctx, vy, vx, vz, re):
        Y, X, Z = vx.shape[1], vy.shape[2], vy.shape[3]
        ctx.re_meta = (re.shape, re.dtype)
        st = torch.stack([vy[:, :Y], vx[:, :, :X], vz[..., :Z]], dim=-1)
        return torch.cat([st, re.reshape(-1, 1, 1, 1, 1).expand(-1, Y, X, Z, 1).to(st.dtype)], dim=-1)

    @staticmethod
    def backward(ctx, g):
        g_re = None
        if ctx.needs_input_grad[3]:
            shape, dtype = ctx.re_meta
            g_re = g[..., 3].sum(dim=(1, 2, 3)).reshape(shape).to(dtype)
        return _lib.pad_high(g[..., 0], 1), _lib.pad_high(g[..., 1], 2), _lib.pad_high(g[..., 2], 3), g_re


def to_feature3d(vy, vx, vz, re):
    """karman_train.py:77-86 with three components: [B,Y,X,Z,4] = the components at the low faces of every cell + Re."""
    return _ToFeature3DFn.apply(vy, vx, vz, re)


def to_staggered3d(t):
    """karman_train.py:88-90 with three components: zero padding at the high end of each component's own axis."""
    # (cat with zeros, not F.pad: its backward clone()s a narrow of the gradient -- contiguous at B = 1, i.e. a memcpy node: _lib.pad_high)
    return _lib.pad_high(t[..., 0], 1), _lib.pad_high(t[..., 1], 2), _lib.pad_high(t[..., 2], 3)


# ---------------------------------------------------------------------------------------------------------------------
# model_mars_moon with Conv3D(5) layers
# ---------------------------------------------------------------------------------------------------------------------
def net3d_shape_reason(Y, X, Z, train=True):
    """None where the correction network runs on a [Y, X, Z] grid, else the reason it does not (a pure function: no device, no library).
    The network's convolutions run over the (X, Z) planes with Z as the row: check_shape of csrc/conv5x5.hip takes rows that divide 64
    -- 64 / Z image rows then share a tile, so X must be a multiple of 64 / Z -- or that are a multiple of 64 pixels long; the Conv3D entry
    points need three planes (sol_conv3d: D >= 3); and the batched weight gradients of the reverse sweep take rows up to 64 pixels
    (bww_launch of csrc/conv5x5.hip), so beyond Z = 64 only the forward network (a roll-out) runs."""
    Y, X, Z = int(Y), int(X), int(Z)
    if Y < 3 or X < 1:
        return "Y = %d, X = %d: the 5 x 5 x 5 convolutions need Y >= 3 planes of X >= 1 rows" % (Y, X)
    if Z < 4 or not ((Z <= 64 and 64 % Z == 0) or Z % 64 == 0):
        return "Z = %d: the rows of the (X, Z) planes must be 4, 8, 16, 32 or 64 pixels long, or a multiple of 64" % Z
    if Z < 64 and X % (64 // Z) != 0:
        return "X = %d with Z = %d: 64/Z = %d rows of a plane share one tile, so X must be a multiple of 64/Z" % (X, Z, 64 // Z)
    if train and Z > 64:
        return ("Z = %d: the weight gradients of the reverse sweep take Z <= 64 (the batched forms of the 5 x 5 weight gradient); "
                "a roll-out (Karman3DRollout, NetSchedule3D(train=False)) runs at this width" % Z)
    return None


def circular_rows3d(X, Z):
    """HB, the row count of the circular network's buffers [B, Y, HB, X, C]: the Z planes and two halo rows on either side, rounded up to
    a multiple of the 64 / X rows that share a tile when X < 64 (check_shape of csrc/conv5x5.hip: H % (64 / W) == 0)"""
    q = 64 // int(X) if int(X) < 64 else 1
    return -(-(int(Z) + 4) // q) * q


def net3d_circular_shape_reason(Y, X, Z, train=True):
    """net3d_shape_reason for the network with circular z padding (conv_padding="circular"): it runs on the transposed volume -- depth y,
    image rows z (Z + 4 of them with the halo, padded up to circular_rows3d(X, Z)), pixels x --, so X takes the pixel rule and Z is free."""
    Y, X, Z = int(Y), int(X), int(Z)
    if Y < 3 or Z < 2:
        return "Y = %d, Z = %d: the circular 5 x 5 x 5 convolutions need Y >= 3 planes and Z >= 2 periodic planes" % (Y, Z)
    if X < 4 or not ((X <= 64 and 64 % X == 0) or X % 64 == 0):
        return ("X = %d: with circular z padding x is the pixel axis of a row, which must be 4, 8, 16, 32 or 64 pixels long, or a multiple "
                "of 64" % X)
    if train and X > 64:
        return ("X = %d: the weight gradients of the reverse sweep take rows up to 64 pixels, with circular z padding X <= 64; "
                "a roll-out (Karman3DRollout, NetSchedule3D(train=False)) runs at this width" % X)
    return None


def conv_padding_arg3d(conv_padding, scene, who, train=True):
    """the conv_padding keyword of Karman3DTrainer / Karman3DRollout, checked by name before any device call: "zeros" or "circular", the
    latter on a z-periodic scene whose grid net3d_circular_shape_reason takes"""
    if conv_padding not in ("zeros", "circular"):
        raise _lib.SolError("%s: conv_padding must be 'zeros' or 'circular' (got %r)" % (who, conv_padding))
    if conv_padding == "circular":
        if not scene.periodic_bits:
            raise _lib.SolError("%s: conv_padding='circular' needs a z-periodic scene (Scene3D(boundaries='periodic-z')); this scene's "
                                "boundaries are open" % who)
        why = net3d_circular_shape_reason(scene.Y, scene.X, scene.Z, train)
        if why is not None:
            raise _lib.SolError("%s: conv_padding='circular' at %d x %d x %d: %s" % (who, scene.Y, scene.X, scene.Z, why))
    return conv_padding


class MarsMoon3D:
    """12 Conv3D(5, padding='same') layers, 32 features, five residual blocks (karman_train.py:101-138 in 3-D): 4 -> 32,
    10 x 32 -> 32, 32 -> 3; 1 308 355 parameters in ONE flat fp32 buffer in Keras get_weights() order (kernels DHWIO).
    Keras defaults: glorot_uniform kernels, zero biases, LeakyReLU(alpha=0.3)."""
    name = "mars_moon3d"
    slope = 0.3

    def __init__(self, cin=4, cout=3, seed=0, device="cuda"):
        self.cin, self.cout = cin, cout
        chans = [cin] + [32] * 11 + [cout]
        self.chans = chans
        self.shapes = []
        for l in range(12):
            self.shapes += [(5, 5, 5, chans[l], chans[l + 1]), (chans[l + 1],)]
        self.offsets = np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in self.shapes])]).astype(np.int64)
        gen = torch.Generator().manual_seed(seed)
        parts = []
        for s in self.shapes:
            if len(s) == 5:
                lim = math.sqrt(6.0 / (125 * (s[3] + s[4])))
                parts.append(((torch.rand(s, generator=gen, dtype=torch.float64) * 2 - 1) * lim).reshape(-1))
            else:
                parts.append(torch.zeros(s, dtype=torch.float64))
        self.params = torch.cat(parts).to(device=device, dtype=torch.float32).contiguous()
        self._generation = 0
        self._schedules = {}

    def params_key(self):
        """Identity of the weight buffer's CONTENT, the ONE staleness rule of the packed weights: a schedule (schedule3d.NetSchedule3D)
        re-packs when this differs from the key it packed at.  An optimizer that updates `params` in place through torch bumps
        `_version`; writes torch does not see (the library's own Adam, ctypes) are announced with invalidate()."""
        return (self.params.data_ptr(), self.params._version, self._generation)

    def invalidate(self):
        """Mark every schedule's packed weights stale.  MUST be called by whoever changes the CONTENT of `params` in a way torch's version
        counter does not see: writes through `params.data` (`p.data.add_()`, `load_state_dict`-style `.data.copy_`), ctypes / HIP writes
        into the buffer (the library's own Adam: Karman3DTrainer.apply_gradients calls this), external kernels.  `set_weights` calls it
        itself; in-place torch ops on `params` bump `_version` and need nothing."""
        self._generation += 1

    def schedule(self, B, Y, X, Z, padding="zeros"):
        """the training schedule (launch sequence, packed weights, weight-gradient partials) of this network at one shape, built once
        (it refers back to the net weakly: no reference cycle, the buffers go with the net).  padding="circular": the schedule with
        circular z padding, kept beside the zero-padded one of the same shape"""
        from .schedule3d import NetSchedule3D
        shape = (int(B), int(Y), int(X), int(Z))
        key = shape if padding == "zeros" else shape + (padding,)
        if key not in self._schedules:
            self._schedules[key] = NetSchedule3D(weakref.proxy(self), *shape, padding=padding)
        return self._schedules[key]

    fused_backward = True      # one autograd node with a hand-written reverse sweep (False: one node per layer, torch glue)

    def __call__(self, x, padding="zeros"):
        """Differentiable forward (training): x [B,Y,X,Z,4] -> [B,Y,X,Z,cout]; gradients flow to self.params (set
        `net.params.requires_grad_(True)`) and to x.  padding="circular": the convolutions wrap along z (a z-periodic scene)."""
        if self.fused_backward:
            return _MarsMoon3DFn.apply(x, self.params, self, padding)
        p = self.tensors()
        if padding != "zeros":
            if padding != "circular":
                raise _lib.SolError("MarsMoon3D: padding must be 'zeros' or 'circular' (got %r)" % (padding,))
            lr = lambda t: torch.nn.functional.leaky_relu(t, self.slope)
            h = lr(conv3d_circular(x, p[0], p[1]))
            for k in range(5):
                a = lr(conv3d_circular(h, p[2 + 4 * k], p[3 + 4 * k]))
                h = lr(conv3d_circular(a, p[4 + 4 * k], p[5 + 4 * k]) + h)
            return conv3d_circular(h, p[22], p[23])
        pk = self.schedule(*x.shape[:4]).layer_packs()
        sl = self.slope
        h = conv3d_fn(x, p[0], p[1], None, True, sl, pk[0])
        for k in range(5):
            a = conv3d_fn(h, p[2 + 4 * k], p[3 + 4 * k], None, True, sl, pk[1 + 2 * k])
            h = conv3d_fn(a, p[4 + 4 * k], p[5 + 4 * k], h, True, sl, pk[2 + 2 * k])
        return conv3d_fn(h, p[22], p[23], None, False, sl, pk[11])

    def activations(self, x):
        """The eleven 32-channel activations h0, a1, h1, ..., a5, h5 of the forward pass (no gradient; the same launches as
        __call__) -- for checks that need the LeakyReLU masks the backward pass will use."""
        with torch.no_grad():
            _, (_, _, acts) = self.schedule(*x.shape[:4]).forward(x)
        return acts

    @property
    def n_params(self):
        return int(self.offsets[-1])

    def tensors(self):
        from .ops import split_flat
        return [t.reshape(s) for t, s in zip(split_flat(self.params, self.offsets), self.shapes)]

    def get_weights(self):
        return [t.detach().cpu().numpy() for t in self.tensors()]

    def set_weights(self, weights):
        flat = np.concatenate([np.asarray(w, dtype=np.float32).reshape(-1) for w in weights])
        assert flat.size == self.n_params, "weight list does not match %s" % self.name
        with torch.no_grad():
            self.params.copy_(torch.as_tensor(flat, device=self.params.device))
        self.invalidate()


def conv3d(x, packed, bias, residual, cout, lrelu, slope, x_absmax=None, y_absmax=None, out=None, act_ref=None):
    """sol_conv3d: x [B,Y,X,Z,cin] -> [B,Y,X,Z,cout].  act_ref: the result (conv + residual) is multiplied by LeakyReLU'(act_ref)
    (SOL_EPI_DLRELU, the backward pass's fused form) instead of being activated."""
    lib = _lib.load()
    B, D, H, W, cin = x.shape
    y = out if out is not None else torch.empty(B, D, H, W, cout, dtype=torch.float32, device=x.device)
    epi = EPI_DLRELU if act_ref is not None else (EPI_LRELU if lrelu else EPI_NONE)
    check(lib.sol_conv3d(stream(), ptr(x), ptr(packed), ptr(bias), ptr(residual), ptr(act_ref), ptr(y), B, D, H, W, cin, cout,
                         epi, float(slope), ptr(x_absmax), ptr(y_absmax)))
    return y


def conv3d_thin(x4, packed, bias, lrelu, slope, y_absmax=None, act_ref=None, out=None, ws=None):
    """sol_conv3d_thin: x4 [B,Y,X,Z,4] (zero padded input channels) -> [B,Y,X,Z,32]; the depth taps are gathered into the channel axis
    (scratch: 32 channels of the volume) and the layer runs as ONE 2-D 32 -> 32 convolution over the (X, Z) planes."""
    lib = _lib.load()
    B, D, H, W, c = x4.shape
    assert c == 4, "conv3d_thin reads four (zero padded) input channels"
    y = out if out is not None else torch.empty(B, D, H, W, 32, dtype=torch.float32, device=x4.device)
    if ws is None:
        ws = torch.empty(lib.sol_conv3d_thin_ws_floats(B, D, H, W), dtype=torch.float32, device=x4.device)
    assert ws.numel() >= lib.sol_conv3d_thin_ws_floats(B, D, H, W)
    epi = EPI_DLRELU if act_ref is not None else (EPI_LRELU if lrelu else EPI_NONE)
    check(lib.sol_conv3d_thin(stream(), ptr(x4), ptr(packed), ptr(bias), ptr(act_ref), ptr(y), ptr(ws), B, D, H, W, epi, float(slope), ptr(y_absmax)))
    return y


def conv3d_thin_out(x, packed, bias, cout, x_absmax=None, out=None, ws=None):
    """y [B,D,H,W,cout (<= 4)] = conv3d(x [B,D,H,W,32], w) + bias with the depth taps packed into the OUTPUT channel axis: one 2-D 32 -> 32
    launch + a gather over five planes (sol_conv3d_thin_out; `packed` from _pack3d_thin_out).  No activation."""
    lib = _lib.load()
    B, D, H, W, c = x.shape
    assert c == 32 and 1 <= cout <= 4
    y = out if out is not None else torch.empty(B, D, H, W, cout, dtype=torch.float32, device=x.device)
    if ws is None:
        ws = torch.empty(lib.sol_conv3d_thin_ws_floats(B, D, H, W), dtype=torch.float32, device=x.device)
    check(lib.sol_conv3d_thin_out(stream(), ptr(x), ptr(packed), ptr(bias), ptr(y), ptr(ws), B, D, H, W, cout, ptr(x_absmax)))
    return y


def _pack3d_thin_out(w, cr, mode, out=None):
    """sol_conv3d_thin_out_pack: w = the FORWARD kernel ([5,5,5,32,cr] for mode 0, [5,5,5,cr,32] for mode 1 = backward-data), cr <= 4"""
    lib = _lib.load()
    buf = out if out is not None else torch.empty(lib.sol_conv3d_thin_packed_floats(), dtype=torch.float32, device=w.device)
    check(lib.sol_conv3d_thin_out_pack(stream(), ptr(w.contiguous()), cr, mode, ptr(buf)))
    return buf


def _pack3d_thin(w, cin_run, mode, out=None):
    """w: the FORWARD kernel ([5,5,5,cin_run,32] for mode 0, [5,5,5,32,cin_run] for mode 1 = backward-data)"""
    lib = _lib.load()
    buf = out if out is not None else torch.empty(lib.sol_conv3d_thin_packed_floats(), dtype=torch.float32, device=w.device)
    check(lib.sol_conv3d_thin_pack(stream(), ptr(w.contiguous()), cin_run, mode, ptr(buf)))
    return buf


def _pack3d(w, cin_run, cout_run, mode, out=None):
    """sol_conv3d_pack of the FORWARD kernel w for a convolution that runs cin_run -> cout_run channels (mode 1: backward-data);
    out: the buffer to pack into (a schedule's persistent one), else a fresh one"""
    lib = _lib.load()
    buf = out if out is not None else torch.empty(lib.sol_conv3d_packed_floats(cin_run, cout_run), dtype=torch.float32, device=w.device)
    check(lib.sol_conv3d_pack(stream(), ptr(w.contiguous()), cin_run, cout_run, mode, ptr(buf)))
    return buf


def _absmax(x):
    """absmax slots of x (sol_absmax: one pass at HBM speed; the tensor must stay referenced by the caller until the consumer is enqueued)"""
    slots = torch.empty(256, dtype=torch.int32, device=x.device)
    check(_lib.load().sol_absmax(stream(), ptr(x), x.numel(), ptr(slots)))
    return slots


def _pad_ch(x, c):
    return x.contiguous() if x.shape[-1] == c else torch.nn.functional.pad(x, (0, c - x.shape[-1])).contiguous()


def _acc_buffers(name, acc, shape_key, alloc):
    """(buffers, first, last) of a weight-gradient call.  acc = (state dict, first, last): the partial sums of a reverse sweep live in the
    caller's state dict -- alloc() fills a fresh one --, they belong to ONE shape and to a sequence that was opened with first=True (the C
    entry point cannot see the size of `partial`, so a mismatch would overrun it or add onto stale sums).  acc = None: one call on its own."""
    if acc is None:
        return alloc(), True, True
    st, first, last = acc
    if "part" in st:
        if st.get("shape") != shape_key:
            raise _lib.SolError("%s: the accumulation state was allocated for %s, this call has %s" % (name, st.get("shape"), shape_key))
        if not first and not st.get("open"):
            raise _lib.SolError("%s: first=False on a state whose sequence is not open (the previous sweep ended with last=True)" % name)
    else:
        if not first:
            raise _lib.SolError("%s: the first call on a fresh accumulation state must have first=True (nothing to add onto yet)" % name)
        st.update(alloc(), shape=shape_key)
    st["open"] = not last
    return st, first, last


def conv3d_thin_bwd_weight(x4, dz, cin, zmax=None, acc=None, thin_out=False):
    """dW [5,5,5,cin,32], db [32] of a thin-input layer y = conv3d(x, W) + b from x4 [B,D,H,W,4] (zero padded) and dz [B,D,H,W,32], W == 64:
    sol_conv3d_thin_bwd_weight_acc -- the depth taps packed into the channel axis, ONE pass of the 2-D 32 -> 32 weight-gradient kernel.
    thin_out=True: the thin-OUTPUT layer (32 -> cin <= 4 channels; `x4` is then the zero-padded output gradient [B,D,H,W,4], `dz` the layer's
    32-channel input and `zmax` its absmax slots): dW [5,5,5,32,cin], db [cin] (sol_conv3d_thin_out_bwd_weight_acc).
    acc = (state dict, first, last) as in conv3d_bwd_weight."""
    lib = _lib.load()
    B, D, H, W, c = x4.shape
    assert c == 4 and dz.shape[-1] == 32 and W == 64
    dev = x4.device
    shape_key = ("thin_out" if thin_out else "thin", B, D, H, W, cin, str(dev))
    f = lambda *n: torch.empty(*n, dtype=torch.float32, device=dev)
    st, first, last = _acc_buffers("conv3d_thin_bwd_weight", acc, shape_key, lambda: dict(
        part=f(lib.sol_conv3d_thin_bwd_weight_ws_floats(B, D, H, W)), ws=f(lib.sol_conv3d_thin_ws_floats(B, D, H, W)),
        dW=f(5, 5, 5, 32, cin) if thin_out else f(5, 5, 5, cin, 32), db=f(cin if thin_out else 32)))
    part, dW, db, ws = (st[k] for k in ("part", "dW", "db", "ws"))
    if thin_out:
        check(lib.sol_conv3d_thin_out_bwd_weight_acc(stream(), ptr(dz), ptr(zmax), ptr(x4), ptr(ws), ptr(part), ptr(dW), ptr(db), B, D, H, W, cin,
                                                     0 if first else 1, 1 if last else 0))
    else:
        check(lib.sol_conv3d_thin_bwd_weight_acc(stream(), ptr(x4), ptr(dz), ptr(zmax), ptr(ws), ptr(part), ptr(dW), ptr(db), B, D, H, W, cin,
                                                 0 if first else 1, 1 if last else 0))
    return (dW, db) if last else (None, None)


def conv3d_bwd_weight(xk, dz, cin, cout, xmax=None, zmax=None, acc=None):
    """dW [5,5,5,cin,cout], db [cout] of y = conv3d(x, W) + b from xk [B,D,H,W,cin_k] (channels padded to 4 / 32) and dz
    [B,D,H,W,cout]: sol_conv3d_bwd_weight (five passes of the batched 2-D weight-gradient kernels over the shifted plane
    ranges; fp16 three-product operands for the 32 -> 32 case, scaled by the absmax of x and dz).
    acc = (state dict, first, last): the unrolled trainer's form (sol_conv3d_bwd_weight_acc) -- the partial sums of this layer live in
    `state` across the calls of a reverse sweep, the first call overwrites them, the last one reduces; returns (None, None) before the
    last call and the sum over all calls with it."""
    lib = _lib.load()
    B, D, H, W, cin_k = xk.shape
    co_k = cout if cout in (2, 32) else 32                 # the 2-D weight-gradient kernels take 2 or 32 output channels
    dzk = _pad_ch(dz, co_k)
    dev = xk.device
    shape_key = (B, D, H, W, cin_k, co_k, cin, str(dev))
    f = lambda *n: torch.empty(*n, dtype=torch.float32, device=dev)
    st, first, last = _acc_buffers("conv3d_bwd_weight", acc, shape_key, lambda: dict(
        part=f(lib.sol_conv3d_bwd_weight_ws_floats(B, D, H, W, cin_k, co_k)), dW=f(5, 5, 5, cin, co_k), db=f(co_k), scratch=f(5 * co_k)))
    part, dW, db, scratch = (st[k] for k in ("part", "dW", "db", "scratch"))
    both32 = cin_k == 32 and co_k == 32
    # (the slot tensors must outlive the call: a temporary inside ptr(...) is freed -- and its block handed to the next
    # allocation -- before the launch is even enqueued)
    # (xmax / zmax given: the slots the producing conv launches published -- no pass over the tensors)
    xmax = (xmax if xmax is not None else _absmax(xk)) if both32 else None
    zmax = (zmax if zmax is not None and dzk is dz else _absmax(dzk)) if both32 else None
    if acc is not None:
        check(lib.sol_conv3d_bwd_weight_acc(stream(), ptr(xk), ptr(dzk), ptr(xmax), ptr(zmax), ptr(part), ptr(dW), ptr(db), ptr(scratch),
                                            B, D, H, W, cin_k, co_k, cin, co_k, 0 if first else 1, 1 if last else 0))
        if not last:
            return None, None
    else:
        check(lib.sol_conv3d_bwd_weight(stream(), ptr(xk), ptr(dzk), ptr(xmax), ptr(zmax),
                                        ptr(part), ptr(dW), ptr(db), ptr(scratch), B, D, H, W, cin_k, co_k, cin, co_k))
    return (dW if co_k == cout else dW[..., :cout].contiguous()), (db if co_k == cout else _lib.dclone(db[:cout]))


class _Conv3DFn(torch.autograd.Function):
    """y = act(conv3d_same(x, w) + b (+ residual)), NDHWC, w in Keras DHWIO layout."""

    @staticmethod
    def forward(ctx, x, w, b, residual, lrelu, slope, packs):
        _lib.require_gpu()
        cin, cout = w.shape[3], w.shape[4]
        assert cin in (1, 2, 3, 4, 32), "conv3d supports <= 4 or 32 input channels"
        cin_k = 4 if cin <= 4 else 32
        xk = _pad_ch(_lib.f32(x), cin_k)
        if packs is not None and cin_k == cin:
            packed = packs[0]
        else:
            wk = _pad_ch(_lib.f32(w).permute(0, 1, 2, 4, 3), cin_k).permute(0, 1, 2, 4, 3).contiguous() if cin_k != cin else _lib.f32(w)
            packed = _pack3d(wk, cin_k, cout, 0)
        ctx.packed_bwd = packs[1] if packs is not None else None
        res = None if residual is None else _lib.f32(residual)
        # the operand's absmax selects the fp16 three-product kernels (and, for 32 -> 32 layers, the one-launch 5x5x5 kernel)
        if cin <= 4 and cout == 32 and res is None:      # the depth-packed one-launch form, as the fused network runs it
            y = conv3d_thin(xk, _pack3d_thin(_lib.f32(w), cin, 0), _lib.f32(b), lrelu, slope)
        elif cin == 32 and cout <= 4 and res is None and not lrelu:      # ... and the thin-output form
            y = conv3d_thin_out(xk, _pack3d_thin_out(_lib.f32(w), cout, 0), _lib.f32(b), cout, _absmax(xk))
        else:
            y = conv3d(xk, packed, _lib.f32(b), res, cout, lrelu, slope, _absmax(xk) if cin_k == 32 else None)
        ctx.save_for_backward(xk, w, y)
        ctx.meta = (cin, cout, cin_k, lrelu, slope, residual is not None)
        return y

    @staticmethod
    def backward(ctx, gy):
        xk, w, y = ctx.saved_tensors
        cin, cout, cin_k, lrelu, slope, has_res = ctx.meta
        dz = gy.contiguous()
        if lrelu:
            dz = dz * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope))
        if cin <= 4 and cout == 32 and xk.shape[3] == 64:
            dW, db = conv3d_thin_bwd_weight(xk, dz, cin)
        elif cin == 32 and cout <= 4 and xk.shape[3] == 64:
            dW, db = conv3d_thin_bwd_weight(_pad_ch(dz, 4), xk, cout, thin_out=True)
        else:
            dW, db = conv3d_bwd_weight(xk, dz, cin, cout)
        # data gradient: the flipped kernel, run channels (cout -> cin)
        co_k = 4 if cout <= 4 else 32
        packed = ctx.packed_bwd if ctx.packed_bwd is not None else _pack3d(_lib.f32(w), cout, cin, 1)
        dzk = _pad_ch(dz, co_k)
        if cout <= 4 and cin == 32:
            dx = conv3d_thin(dzk, _pack3d_thin(_lib.f32(w), cout, 1), None, False, slope)
        elif cin <= 4 and cout == 32:
            dx = conv3d_thin_out(dzk, _pack3d_thin_out(_lib.f32(w), cin, 1), None, 4, _absmax(dzk))[..., :cin]
        else:
            dx = conv3d(dzk, packed, None, None, cin, False, slope, _absmax(dzk) if co_k == 32 else None)
        return dx, dW, db, (dz if has_res else None), None, None, None


class _MarsMoon3DFn(torch.autograd.Function):
    """model_mars_moon (3-D) as ONE autograd node over the net's schedule of the input's shape (schedule3d.NetSchedule3D): its twelve forward
    launches and its hand-written reverse sweep, the weight gradients of this one call reduced at once."""

    @staticmethod
    def forward(ctx, x, params, net, padding="zeros"):
        ctx.net, ctx.sch = net, net.schedule(*x.shape[:4], padding=padding)
        out, (xk, amax, acts) = ctx.sch.forward(x)
        ctx.save_for_backward(xk, amax, *acts)
        return out

    @staticmethod
    def backward(ctx, g_out):
        xk, amax, *acts = ctx.saved_tensors
        dx, flat = ctx.sch.backward((xk, amax, acts), g_out)
        return dx[..., :ctx.net.cin], flat, None, None


def conv3d_fn(x, w, b, residual=None, lrelu=False, slope=0.3, packs=None):
    """packs: optional (forward-packed, backward-data-packed) weight buffers of this layer (NetSchedule3D.layer_packs)."""
    return _Conv3DFn.apply(x, w, b, residual, lrelu, slope, packs)


class _CircWrap3DFn(torch.autograd.Function):
    """x [B,Y,X,Z,C] -> the halo buffer [B,Y,HB,X,C] of the circular network (include/sol_hip.h, "CIRCULAR PADDING, KARMAN-3D"): planes
    transposed into rows [2, Z + 2), halo rows wrapped, pad rows zero.  C = 4: sol_conv3d_circ_pack; C = 32: a torch transpose and
    sol_conv3d_halo.  backward: the adjoint, every halo row folded onto the plane it copied."""

    @staticmethod
    def forward(ctx, x):
        _lib.require_gpu()
        lib = _lib.load()
        B, Y, X, Z, c = x.shape
        assert c in (4, 32), "the halo buffers hold 4 or 32 channels"
        HB = circular_rows3d(X, Z)
        ctx.Z = Z
        x = _lib.f32(x).contiguous()
        buf = torch.empty(B, Y, HB, X, c, dtype=torch.float32, device=x.device)
        if c == 4:
            check(lib.sol_conv3d_circ_pack(stream(), ptr(x), ptr(buf), B, Y, X, Z, HB, 4, 0))
        else:
            buf[:, :, 2:Z + 2] = x.permute(0, 1, 3, 2, 4)
            check(lib.sol_conv3d_halo(stream(), ptr(buf), B * Y, Z, HB, X, c, 0))
        return buf

    @staticmethod
    def backward(ctx, g):
        Z = ctx.Z
        gx = g[:, :, 2:Z + 2].clone()
        for r in (0, 1, Z + 2, Z + 3):
            gx[:, :, (r - 2) % Z] += g[:, :, r]
        return gx.permute(0, 1, 3, 2, 4).contiguous()


def conv3d_circular(x, w, b):
    """y [B,Y,X,Z,cout] = conv3d(x [B,Y,X,Z,cin], w [5,5,5,cin,cout] (Keras k_y, k_x, k_z, in, out)) + b with CIRCULAR padding along z and
    zero padding along y and x: one differentiable linear layer, the cross-check of NetSchedule3D(padding="circular").  The layer wraps x
    into the halo buffer, runs conv3d_fn there with kernel axes 1 and 2 swapped and crops the valid rows; autograd composes the adjoint
    (zero cotangent in halo rows -> weight gradient over valid rows; the data gradient's halo rows folded back by the wrap's adjoint)."""
    B, Y, X, Z, cin = x.shape
    why = net3d_circular_shape_reason(Y, X, Z, train=X <= 64)
    if why is not None:
        raise _lib.SolError("conv3d_circular at %d x %d x %d: %s" % (Y, X, Z, why))
    ck = 4 if cin <= 4 else 32
    xb = _CircWrap3DFn.apply(x if cin == ck else torch.nn.functional.pad(x, (0, ck - cin)))
    wk = w if cin == ck else torch.nn.functional.pad(w, (0, 0, 0, ck - cin))
    yb = conv3d_fn(xb, wk.permute(0, 2, 1, 3, 4), b)
    return yb[:, :, 2:Z + 2].permute(0, 1, 3, 2, 4).contiguous()


def ops_l2_loss(pred, gt, std):
    from .ops import l2_loss
    return l2_loss(pred, gt, std)


class Karman3DTrainer:
    """SOL-n training step of the 3-D scene: msteps x [solver step -> features / std -> mars_moon3d -> velocity += std *
    to_staggered(correction)], loss = sum_i l2_loss((gt_i - prd_i) / std_v) / msteps (karman_train.py:397-447 with three
    components), reverse sweep through the HIP adjoints by torch autograd, TF-Adam on the flat parameter buffer
    (sol_adam_tf_step).  gts: [msteps] of (vy, vx, vz) ground-truth frames."""

    buoyancy = property(lambda self: self.sim.physics.buoyancy)
    nsub = property(lambda self: self.sim.physics.nsub)

    def __init__(self, net, scene, B, msteps, std_v, std_re, dt=1.0, res=None, beta1=0.9, beta2=0.999, eps=1e-8, conv_precision="split",
                 use_graph=False, group=None, comm=None, schedule="manual", glue="fused", buoyancy=None, diffusion_substeps=1,
                 advection="semi_lagrangian", correction_strength=1.0, conv_padding="zeros", **solver):
        """schedule: "manual" (default) = the hand-written forward unroll + reverse sweep over the C ABI (_unrolled_schedule), "autograd" = the
        torch-autograd composition of the differentiable HIP ops (rounds 3-4; kept as the cross-check).
        use_graph: capture the whole forward unroll + reverse sweep ONCE into a hipGraph over static input buffers (the
        TF1 "build the graph, sess.run many" shape, as trainer.GraphTrainer does for the 2-D mercury model): a step then
        copies the batch in and replays ~3000 launches with one host call.
        buoyancy=(fy, fx, fz), diffusion_substeps=n: the StepPhysics3D of the simulator (self.sim.physics).  The schedule is unchanged; the
        solver pair is Karman3DFlow._forward and _step_adjoint3d under it: with a force each step's input density is kept and the density
        cotangent is carried to the next (earlier) step (None at the last step: the loss does not look at the density).  Kernel launches
        only, the pre-diffusion's ping-pong buffers are the simulator's static ones: use_graph stays a graph of kernel nodes.
        advection="mac_cormack", correction_strength=s: the simulator's scheme (self.sim.adv); both schedules hand it to the solver pair.  The
        MacCormack launches work in the simulator's workspace, sized at construction: kernel nodes only, as before.
        conv_padding="circular" (a z-periodic scene): the correction network pads circularly along z in the forward pass, the backward-data
        pass and the weight gradient (NetSchedule3D(padding="circular")), under both schedules, eager and captured; X then takes the
        pixel rule and Z is free (net3d_circular_shape_reason).  Kept as self.conv_padding."""
        from .trainer import _conv_precision_code
        from .dist import DPStep
        from .ops import advection_arg
        advection_arg(advection, correction_strength, "Karman3DTrainer: advection")       # (refused before the device is asked for)
        self.conv_padding = conv_padding_arg3d(conv_padding, scene, "Karman3DTrainer")     # (likewise)
        _lib.require_gpu()
        self.lib = _lib.load()
        self.net, self.scene, self.B, self.ms = net, scene, B, msteps
        # the network's launches, packed weights and weight-gradient partials at this shape -- first: a grid the network does not take
        # (net3d_shape_reason) is refused here, before a simulator or a buffer exists
        self.sch = net.schedule(B, scene.Y, scene.X, scene.Z, padding=self.conv_padding)
        assert glue in ("fused", "torch")
        self.glue = glue          # reverse-sweep glue of the manual schedule: sol_karman3d_correct_bwd / _feature_bwd, or the torch elementwise composition
        self.sim = Karman3DFlow(scene, B, dt=dt, res=res, buoyancy=buoyancy, diffusion_substeps=diffusion_substeps, advection=advection,
                                correction_strength=correction_strength, **solver)
        dev = scene.active.device
        self.std_v = torch.tensor([float(v) for v in std_v], dtype=torch.float32, device=dev)
        self._std_v_host = tuple(float(v) for v in std_v)
        self._std_in_host = tuple(float(v) for v in std_v) + (float(std_re),)
        self.std_in = torch.tensor([float(v) for v in std_v] + [float(std_re)], dtype=torch.float32, device=dev)
        self.conv_precision = _conv_precision_code(conv_precision)
        net.params.requires_grad_(True)
        self.m = torch.zeros_like(net.params.detach())
        self.v = torch.zeros_like(net.params.detach())
        self.t = 0
        self.beta1, self.beta2, self.eps = beta1, beta2, eps
        Y, X, Z = scene.Y, scene.X, scene.Z
        f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        # static buffers: inputs, ground-truth frames, outputs (the graph bakes their addresses in)
        self._in = [f(B, Y, X, Z), f(B, Y + 1, X, Z), f(B, Y, X + 1, Z), f(B, Y, X, Z + 1), f(B)]
        self._gt = [f(msteps, B, Y + 1, X, Z), f(msteps, B, Y, X + 1, Z), f(msteps, B, Y, X, Z + 1)]
        self.loss_steps = f(msteps)
        self._loss = f(())
        # gradient + one slot for the loss: the data-parallel exchange (B simulations per rank, BASELINE configs[4]: 8 GPUs) is ONE
        # all-reduce(SUM) of this buffer per training step, as for the 2-D trainers (dist.DPStep; group / comm as there)
        self._flat = f(net.n_params + 1)
        self._grads = self._flat[:net.n_params]
        self._dp = DPStep(lambda *b: (self.fwd_bwd(*b), self._grads), lambda g, lr: self.apply_gradients(lr), group=group, comm=comm, flat=self._flat)
        self._fin = [f(B, Y, X, Z), f(B, Y + 1, X, Z), f(B, Y, X + 1, Z), f(B, Y, X, Z + 1)]
        self.final = None
        self.use_graph, self._graph = bool(use_graph), None
        if schedule not in ("manual", "autograd"):
            raise ValueError("schedule must be 'manual' or 'autograd'")
        self.schedule = schedule

    def _unrolled(self):
        if self.schedule == "manual":
            with torch.no_grad():                   # nothing here is differentiated by torch: the reverse sweep is written out
                return self._unrolled_schedule()
        return self._unrolled_autograd()

    def _unrolled_schedule(self):
        """The SOL-n step as a HAND-WRITTEN schedule over the C ABI (karman_train.py:397-457 differentiated by hand, as train.hip does for
        the 2-D scene): forward unroll with everything the reverse sweep needs kept per step, then the reverse sweep -- no autograd
        graph, no torch op between the launches except a handful of elementwise kernels (slicing adds, one stack per step).
        Per unrolled step i, forward:   solver step (saves the post-diffusion velocity, writes the SCALED features itself) -> network
        (twelve launches, absmax handed from layer to layer) -> velocity += std * to_staggered(out) (sol_karman3d_correct) -> loss_i and
        d loss_i / d v_i in one pass (sol_l2_loss_fwd_bwd, gradient pre-scaled by 1 / msteps).
        Reverse, i = n-1 .. 0:   G = d loss_i / d v_i + (adjoint of step i+1 w.r.t. its input)  ->  d out = std * G at the corrected faces
        -> network reverse sweep (weight gradients accumulated over the steps, d features) -> G += d features / std_in at the low faces
        (to_feature's adjoint) -> solver adjoint (sol_karman3d_step_bwd)."""
        from .ops import l2_loss_fwd_bwd
        d, vy, vx, vz, re = self._in
        net, sim, sch, ms = self.net, self.sim, self.sch, self.ms
        sc = self.scene
        B, Y, X, Z = self.B, sc.Y, sc.X, sc.Z
        sch.begin_step()                            # the weights moved since the last step: re-pack once (inside the graph when captured)
        fs = [1.0 / t for t in self._std_in_host]          # (host copies: a .tolist() of a device tensor is a synchronising copy -- illegal inside a capture)
        sv = self._std_v_host
        v = (vy, vx, vz)
        ph, buoyant = sim.physics, sim.physics.buoyancy is not None
        akw = {} if sim.adv is None else {"adv": sim.adv}      # (the scheme travels beside the physics value, only where it is not the default)
        keep = []                                # per step: (saved velocities, network state, d loss_i / d v_i, input density (buoyant mode))
        losses = []
        for i in range(ms):
            saved = [torch.empty_like(t) for t in v]
            feat = torch.empty(B, Y, X, Z, 4, dtype=torch.float32, device=vy.device)
            d_in = d if buoyant else None
            d, *v = sim._forward(ph, d, v[0], v[1], v[2], re, saved, feat, fs, **akw)[0]
            out, state = sch.forward(feat)
            check(self.lib.sol_karman3d_correct(stream(), ptr(out), net.cout, sv[0], sv[1], sv[2], ptr(v[0]), ptr(v[1]), ptr(v[2]), B, Y, X, Z))
            if sc.periodic_bits:                    # the correction left the duplicate plane behind
                seam_sync3d(sc, v[2])
            li, gi = l2_loss_fwd_bwd(v, tuple(g[i] for g in self._gt), sv, gscale=1.0 / ms)
            losses.append(li.reshape(()))
            keep.append((saved, state, gi, d_in))
        flat = None
        gin = None
        g_d = None                                  # buoyant mode: the density cotangent carried from step i + 1 to step i
        inv_in = fs[:3]
        for i in range(ms - 1, -1, -1):
            saved, state, G, d_in = keep[i]
            if sc.periodic_bits:                    # the adjoint of the seam sync (gin's duplicate plane is exactly zero: folding G alone is folding G + gin)
                seam_fold3d(sc, G[2])
            # G += gin and the adjoint of  v += std * to_staggered(out):  d out[..., c] = std_c * G_c restricted to the faces that received a correction
            # (one launch, zero padded to the four channels the thin-layer launches read; glue="torch": the elementwise composition of rounds 5-6)
            fused_glue = self.glue == "fused" and net.cout == 3
            if fused_glue:
                dO = torch.empty(B, Y, X, Z, 4, dtype=torch.float32, device=G[0].device)
                gi = gin if gin is not None else (None, None, None)
                check(self.lib.sol_karman3d_correct_bwd(stream(), ptr(G[0]), ptr(G[1]), ptr(G[2]), ptr(gi[0]), ptr(gi[1]), ptr(gi[2]), sv[0], sv[1], sv[2], ptr(dO), B, Y, X, Z))
            else:
                if gin is not None:
                    for c in range(3):
                        G[c].add_(gin[c])
                dO = torch.stack([G[0][:, :Y] * sv[0], G[1][:, :, :X] * sv[1], G[2][..., :Z] * sv[2]], dim=-1)
            dx, gflat = sch.backward(state, dO, i == ms - 1, i == 0)      # (the weight gradients accumulate over the sweep: reduced once, at i = 0)
            flat = gflat if gflat is not None else flat
            # adjoint of the feature map (the three components at the low faces of every cell, divided by std_in; the Re channel has no gradient)
            if fused_glue and dx.shape[-1] == 4:
                check(self.lib.sol_karman3d_feature_bwd(stream(), ptr(dx), inv_in[0], inv_in[1], inv_in[2], ptr(G[0]), ptr(G[1]), ptr(G[2]), B, Y, X, Z))
            else:
                G[0][:, :Y].add_(dx[..., 0], alpha=inv_in[0])
                G[1][:, :, :X].add_(dx[..., 1], alpha=inv_in[1])
                G[2][..., :Z].add_(dx[..., 2], alpha=inv_in[2])
            # (nobody reads step 0's input cotangent: it is not taken through the pre-diffusion)
            g_d, *gin, _ = _step_adjoint3d(sim, ph, buoyant, d_in, saved, re, g_d, G, through_substeps=i > 0, **akw)
            keep[i] = None                          # (eager runs: the step's activations can go)
        losses = _lib.stack0(losses)
        loss = losses.sum() / ms
        # (kernel copies: a contiguous tensor.copy_ is a hipMemcpyAsync = a memcpy node, refused by the capture guard -- _lib.dcopy_)
        _lib.dcopy_(self.loss_steps, losses)
        _lib.dcopy_(self._loss, loss)
        _lib.dcopy_(self._grads, flat)
        for dst, src in zip(self._fin, (d,) + tuple(v)):
            _lib.dcopy_(dst, src)

    def _unrolled_autograd(self):
        """The same step as a torch-autograd composition of the differentiable HIP ops (schedule="autograd"): the cross-check of the
        hand-written schedule (test_karman3d_manual_schedule_equals_autograd_composition) and the form of rounds 3-4."""
        d, vy, vx, vz, re = self._in
        self.net.params.grad = None
        self.sch.begin_step()                       # the weights moved since the last step: re-pack once (inside the graph when captured)
        v = (_lib.dclone(vy).requires_grad_(True), vx, vz)     # the state enters the graph (the step's autograd Function needs a grad-requiring input)
        losses = []
        for i in range(self.ms):
            d, *v = self.sim.step(d, v[0], v[1], v[2], re)
            out = self.net(to_feature3d(v[0], v[1], v[2], re) / self.std_in, padding=self.conv_padding) * self.std_v
            v = tuple(a + c for a, c in zip(v, to_staggered3d(out)))
            if self.scene.periodic_bits:
                v = (v[0], v[1], _SeamSync3DFn.apply(v[2], self.scene))
            # (one kernel, no torch reduction: a multi-workgroup torch .sum() puts a memset node into the captured graph, ops.L2LossFn)
            losses.append(ops_l2_loss(v, tuple(g[i] for g in self._gt), self._std_v_host))
        losses = _lib.stack0(losses)
        loss = losses.sum() / self.ms
        loss.backward()
        # (kernel copies: a contiguous tensor.copy_ is a hipMemcpyAsync = a memcpy node, refused by the capture guard -- _lib.dcopy_)
        _lib.dcopy_(self.loss_steps, losses)
        _lib.dcopy_(self._loss, loss)
        _lib.dcopy_(self._grads, self.net.params.grad)
        for dst, src in zip(self._fin, (d,) + tuple(v)):
            _lib.dcopy_(dst, src)

    def fwd_bwd(self, d, vy, vx, vz, re, gts):
        """gts: [msteps] of (vy, vx, vz) frames, or the three stacked tensors [msteps, B, ...]."""
        from .trainer import _conv_precision_scope
        for dst, src in zip(self._in, (d, vy, vx, vz, re)):
            dst.copy_(_lib.f32(src), non_blocking=True)
        if isinstance(gts, (list, tuple)) and len(gts) == self.ms and isinstance(gts[0], (list, tuple)):
            for i, fr in enumerate(gts):
                for c in range(3):
                    self._gt[c][i].copy_(_lib.f32(fr[c]), non_blocking=True)
        else:
            for c in range(3):
                self._gt[c].copy_(_lib.f32(gts[c]), non_blocking=True)
        with _conv_precision_scope(self.conv_precision):
            if not self.use_graph:
                self._unrolled()
            else:
                if self._graph is None:
                    side = torch.cuda.Stream()
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):          # warm-up off the capture: library initialisation, allocator pools
                        self._unrolled()
                    torch.cuda.current_stream().wait_stream(side)
                    torch.cuda.synchronize()
                    self.net.params.grad = None
                    self._graph = _lib.capture_graph(self._unrolled, "Karman3DTrainer")      # kernel nodes only (sol_graph_check), then instantiated
                self._graph.replay()
        self.final = tuple(self._fin)
        return self._loss

    @property
    def grads(self):
        return self._grads

    def apply_gradients(self, lr):
        self.t += 1
        p = self.net.params.detach()
        check(self.lib.sol_adam_tf_step(stream(), ptr(p), ptr(self._grads), ptr(self.m), ptr(self.v),
                                        self.net.n_params, self.t, float(lr), self.beta1, self.beta2, self.eps, 0.0, None, 0, None))
        self.net.invalidate()                       # every schedule's packs are stale now (torch does not see this write)

    def train_step(self, d, vy, vx, vz, re, gts, lr):
        """One training step on this rank's simulations; returns the GLOBAL loss tensor (the sum over all ranks' simulations)."""
        return self._dp(d, vy, vx, vz, re, gts, lr=lr)


class Karman3DRollout:
    """No-grad roll-out: nsteps x [solver step -> features / std -> CNN -> velocity += std * correction]
    (karman_apply.py:138-158 / the forward half of karman_train.py:397-426, three components)."""

    buoyancy = property(lambda self: self.sim.physics.buoyancy)
    nsub = property(lambda self: self.sim.physics.nsub)

    def __init__(self, net, scene, B, std_v, std_re, dt=1.0, res=None, conv_precision="split", buoyancy=None, diffusion_substeps=1,
                 advection="semi_lagrangian", correction_strength=1.0, conv_padding="zeros", **solver):
        """buoyancy=(fy, fx, fz), diffusion_substeps=n: the StepPhysics3D of the simulator (self.sim.physics); the features keep the true re.
        advection="mac_cormack", correction_strength=s: the simulator's scheme (self.sim.adv)
        conv_padding="circular" (a z-periodic scene): the network pads circularly along z; X takes the pixel rule (a multiple of 64 runs
        here), Z is free.  Kept as self.conv_padding."""
        from .trainer import _conv_precision_code
        from .schedule3d import NetSchedule3D
        from .ops import advection_arg
        advection_arg(advection, correction_strength, "Karman3DRollout: advection")       # (refused before the device is asked for)
        self.conv_padding = conv_padding_arg3d(conv_padding, scene, "Karman3DRollout", train=False)     # (likewise)
        _lib.require_gpu()
        self.lib = _lib.load()
        self.net, self.scene, self.B = net, scene, B
        # forward only, in its own persistent buffers -- first: a grid the network does not take (net3d_shape_reason) is refused here
        self.sch = NetSchedule3D(net, B, scene.Y, scene.X, scene.Z, train=False, padding=self.conv_padding)
        self.sim = Karman3DFlow(scene, B, dt=dt, res=res, buoyancy=buoyancy, diffusion_substeps=diffusion_substeps, advection=advection,
                                correction_strength=correction_strength, **solver)
        self.std_v = tuple(float(v) for v in std_v)
        self.feat_scale = [1.0 / self.std_v[0], 1.0 / self.std_v[1], 1.0 / self.std_v[2], 1.0 / float(std_re)]
        self.conv_precision = _conv_precision_code(conv_precision)
        dev = scene.active.device
        Y, X, Z = scene.Y, scene.X, scene.Z
        self.feat = torch.empty(B, Y, X, Z, 4, dtype=torch.float32, device=dev)
        self.out = self.sch.out

    def correction(self):
        """self.feat -> self.out (the network), publishing / consuming the per-tensor absmax of every 32-channel tensor."""
        from .trainer import _conv_precision_scope
        with _conv_precision_scope(self.conv_precision):
            return self.sch.forward(self.feat)[0]

    def step(self, d, vy, vx, vz, re):
        d, vy, vx, vz = self.sim.step(d, vy, vx, vz, re, feat_out=self.feat, feat_scale=self.feat_scale)
        out = self.correction()
        s = self.scene
        check(self.lib.sol_karman3d_correct(stream(), ptr(out), self.net.cout, self.std_v[0], self.std_v[1], self.std_v[2],
                                            ptr(vy), ptr(vx), ptr(vz), self.B, s.Y, s.X, s.Z))
        if s.periodic_bits:
            seam_sync3d(s, vz)
        return d, vy, vx, vz

    def run(self, d, vy, vx, vz, re, nsteps):
        re = _lib.f32(re)
        for _ in range(nsteps):
            d, vy, vx, vz = self.step(d, vy, vx, vz, re)
        return d, vy, vx, vz
