"""Differentiable PyTorch-ROCm wrappers over the C ABI (one autograd.Function per op).

These are the composable building blocks behind the reference-shaped Python surface
(karman.py, burgers.py, model.py).  The fused whole-step entry point lives in trainer.py.
Every function here calls libsol_hip.so; there is no CPU implementation.
"""
import ctypes as C
import functools
import os
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import KarmanCfg, SolError, check, ptr, stream

EPI_NONE, EPI_LRELU, EPI_DLRELU = 0, 1, 2
CONV_FWD, CONV_BWD_DATA = 0, 1


def karman_cfg(B, Y, X, dx, dt=1.0, res=None, cg_rtol=1e-6, cg_atol=1e-9, cg_max_iter=2000,
               grad_pad="replicate", inflow_order="after", masks=None):
    """sol_karman_cfg; `masks` (SceneMasks) supplies the coarse inverse of the CG preconditioner."""
    cfg = KarmanCfg(B, Y, X, float(dx), float(dt), float(X if res is None else res),
                    float(cg_rtol), float(cg_atol), int(cg_max_iter),
                    {"replicate": 0, "dirichlet0": 1}[grad_pad], {"after": 0, "before": 1}[inflow_order], 0, None, 0, None)
    ci = getattr(masks, "coarse_inv", None)
    if ci is not None:
        cfg.coarse_n = ci.shape[0]
        cfg.coarse_inv = ci.data_ptr()
    db = getattr(masks, "direct", None)
    if db is not None:
        cfg.direct_n = db.numel()
        cfg.direct = db.data_ptr()
    cfg._keep = (ci, db)          # the struct holds raw device pointers
    return cfg


def beyond_one_workgroup(Y, X):
    """True for a grid the one-workgroup solver kernels (sol_karman_step_fwd / _bwd, the fused adjoint) do not take: more than 8192 cells
    or rows wider than 64 cells.  Such a grid runs the multi-launch path (karman_step_large, trainer.LargeGridTrainer)."""
    return Y * X > 8192 or X > 64


# word of the direct blob's HOST header copy that carries flags for the launch code (the device blob keeps 0 there), and its bit
# "built with multi_launch=True": sol_large_direct_solve may run the one-launch solve (csrc/karman_solve_small.hip, option k2d_solve_one_wg)
DIRECT_HEADER_FLAGS, DIRECT_ONE_WG = 8, 1

PRESSURE_SOLVERS = ("auto", "direct", "cg", "direct_scattered")

# header flag bits of a direct blob built for periodic axes (precond.PERIODIC_Y / _X, SOL_DIRECT_HDR_PERIODIC_Y / _X): also the
# `periodic_bits` of karman_seam_sync / karman_seam_fold
PERIODIC_Y, PERIODIC_X = 2, 4
BOUNDARIES = ("open", "periodic")


def boundaries_arg(b, who="boundaries"):
    """"open", "periodic" or a pair (by, bx) of those -> (py, px), True for a periodic axis.  One word applies to both axes.  Anything
    else raises ValueError."""
    pair = (b, b) if isinstance(b, str) else b
    try:
        by, bx = pair
    except (TypeError, ValueError):
        raise ValueError("%s must be 'open', 'periodic' or a pair (by, bx) of those (got %r)" % (who, b)) from None
    for v in (by, bx):
        if not isinstance(v, str) or v not in BOUNDARIES:
            raise ValueError("%s must be 'open', 'periodic' or a pair (by, bx) of those (got %r)" % (who, b))
    return by == "periodic", bx == "periodic"


def boundaries_name(periodic):
    """(py, px) back as the pair of words boundaries_arg takes"""
    return tuple("periodic" if p else "open" for p in periodic)


def periodic_bits(periodic):
    return PERIODIC_Y * bool(periodic[0]) + PERIODIC_X * bool(periodic[1])


def is_direct(pressure_solver):
    """True for the solvers without iteration (SceneMasks.pressure_solver "direct" or "direct_scattered"): capturable, no cg_info."""
    return pressure_solver in ("direct", "direct_scattered")


class SceneMasks:
    """Device-resident constant masks of a scene: active (1 - obstacle), inflow rate, velBCy,
    velBCyMask (reference: KarmanFlow.__init__ karman_train.py:166-171 and :366-373)."""

    def __init__(self, active, inflow, velBCy, velBCyMask, device="cuda", precondition=True, pressure_solver="auto", multi_launch=False,
                 boundaries="open"):
        """multi_launch=True (opt-in): the multi-launch path (karman_step_large and everything that keys on `large`) on a grid the
        one-workgroup kernels would serve, any Y, X >= 16 -- what buoyancy, mac_cormack and "direct_scattered" are built on.
        boundaries: "open" (default), "periodic" or a pair (by, bx) (boundaries_arg) -> self.periodic = (py, px).  A periodic scene runs
        the multi-launch path with a direct solve only: its blob carries the axes, and every call that takes the masks follows it."""
        self.periodic = boundaries_arg(boundaries, "SceneMasks: boundaries")
        self.periodic_bits = periodic_bits(self.periodic)
        self.active = _lib.f32(active, device)
        self.inflow = _lib.f32(inflow, device)
        self.velBCy = _lib.f32(velBCy, device)
        self.velBCyMask = _lib.f32(velBCyMask, device)
        Y, X = self.active.shape[-2:]
        n = (Y + 1) * X
        assert self.velBCy.numel() % n == 0 and self.velBCy.numel() == self.velBCyMask.numel()
        self.bc_stride = 0 if self.velBCy.numel() == n else n
        self.multi_launch = bool(multi_launch)
        if self.multi_launch and (Y < 16 or X < 16):
            raise ValueError("SceneMasks: multi_launch=True takes grids with Y, X >= 16 (the multi-launch kernels); this one is %dx%d" % (Y, X))
        self.large = self.multi_launch or beyond_one_workgroup(Y, X)      # the multi-launch path (karman_step_large)
        if self.periodic_bits and not self.large:
            raise ValueError("SceneMasks: periodic boundaries are built on the multi-launch path only; a %dx%d grid runs the fused one-workgroup "
                             "kernels (not ops.beyond_one_workgroup), which are open on all sides: pass multi_launch=True (Y, X >= 16)" % (Y, X))
        # two-level CG preconditioner (host-prepared dense coarse inverse), when the grid allows it
        self.coarse_inv = None
        if precondition and not os.environ.get("SOL_NO_PRECOND") and not self.large and _lib.load().sol_karman_precond_supported(Y, X):
            from .precond import coarse_inverse
            self.coarse_inv = _lib.f32(coarse_inverse(self.active.reshape(Y, X).cpu().numpy()), device)
        # direct pressure solver (fast diagonalisation + capacitance correction) where it is built and the
        # scene qualifies; pressure_solver="cg" (or SOL_PRESSURE_SOLVER=cg) keeps the (preconditioned) CG
        self.direct = None
        self.direct_header = None
        want = os.environ.get("SOL_PRESSURE_SOLVER", pressure_solver)
        if want not in PRESSURE_SOLVERS:
            raise ValueError("pressure_solver must be 'auto', 'direct', 'cg' or 'direct_scattered' (got %r)" % (want,))
        if self.periodic_bits:
            self._periodic_solver(want, Y, X, device)
        elif want == "direct_scattered":
            # opt-in: the capacitance solve on the support set's row and column lists (no window), large grids only
            if not self.large:
                raise ValueError("pressure_solver='direct_scattered' serves the large-grid path only (grids beyond the one-workgroup "
                                 "kernels, ops.beyond_one_workgroup); %dx%d is not large: use 'auto', 'direct' or 'cg'.  SceneMasks(multi_launch=True) "
                                 "runs the large-grid path on such a grid" % (Y, X))
            from .precond import scattered_solver_blob
            blob = scattered_solver_blob(self.active.reshape(Y, X).cpu().numpy())
            if blob is None:
                raise ValueError("the scattered direct pressure solver does not support this scene (%dx%d): no obstacle, more than "
                                 "4096 support cells, or an ill-conditioned capacitance system" % (Y, X))
            self.direct = torch.from_numpy(blob).to(device)
            self.direct_header = np.ascontiguousarray(blob[:16].view(np.int32))
        elif want != "cg" and (self.large or _lib.load().sol_karman_direct_supported(Y, X)):
            from .precond import direct_solver_blob
            blob = direct_solver_blob(self.active.reshape(Y, X).cpu().numpy(), max_window=64 if self.large else 16)
            if blob is not None:
                self.direct = torch.from_numpy(blob).to(device)
                self.direct_header = np.ascontiguousarray(blob[:16].view(np.int32))      # host copy: sizes the large-grid launches
                if self.multi_launch:
                    # a copy of its own (ascontiguousarray hands back a view of the blob), then the flag: the one-launch solve may serve this scene
                    self.direct_header = self.direct_header.copy()
                    self.direct_header[DIRECT_HEADER_FLAGS] |= DIRECT_ONE_WG
        if want == "direct" and self.direct is None:
            raise ValueError("the direct pressure solver does not support this scene (%dx%d)" % (Y, X))
        if self.periodic_bits and self.direct_header[0] == 0x46445331:
            want = "direct_scattered"
        # large grids without a direct blob ("cg", or a scene the blob refuses): the preconditioned CG solve of the large-grid step
        # (sol_karman_step_fwd_large_cg) with the empty-box solve as its preconditioner
        self.box = None
        self.box_header = None
        if self.large and self.direct is None:
            from .precond import box_solver_blob
            blob = box_solver_blob(Y, X)
            self.box = torch.from_numpy(blob).to(device)
            self.box_header = np.ascontiguousarray(blob[:16].view(np.int32))
        self.pressure_solver = want if want == "direct_scattered" else ("direct" if self.direct is not None else "cg")

    def _periodic_solver(self, want, Y, X, device):
        """The direct blob of a periodic scene: the one-window blob (an empty scene: the box blob with nS = 0) under "auto" / "direct",
        the scattered blob under "direct_scattered" or where the window refuses (an obstacle across the seam spans the whole axis).
        There is no CG solve on periodic scenes: "cg" and a scene both blobs refuse raise."""
        from .precond import direct_solver_blob, scattered_solver_blob
        if want == "cg":
            raise ValueError("SceneMasks: pressure_solver='cg' is not built for periodic boundaries; use 'auto', 'direct' or 'direct_scattered'")
        act = self.active.reshape(Y, X).cpu().numpy()
        blob = None
        if want != "direct_scattered":
            blob = direct_solver_blob(act, max_window=64, periodic=self.periodic)
        if blob is None and want != "direct":
            blob = scattered_solver_blob(act, periodic=self.periodic)
        if blob is None:
            raise ValueError("SceneMasks: no direct pressure solver takes this periodic scene (%dx%d, pressure_solver=%r): the one-window blob "
                             "needs the obstacle inside one 64 x 64 window away from the seam, the scattered blob ('direct_scattered') an obstacle "
                             "with at most 4096 support cells and a well-conditioned capacitance system; periodic scenes have no CG solve to "
                             "fall back to" % (Y, X, want))
        self.direct = torch.from_numpy(blob).to(device)
        self.direct_header = np.ascontiguousarray(blob[:16].view(np.int32)).copy()
        if self.multi_launch and self.direct_header[0] != 0x46445331 and self.direct_header[5] > 0:
            self.direct_header[DIRECT_HEADER_FLAGS] |= DIRECT_ONE_WG

    def staged_box(self):
        """(box blob, its host header) for the CG solve of the staged adjoint (sol_karman_step_bwd_large*), None for a scene with a
        direct blob.  A large CG scene built it in __init__; a one-workgroup CG scene needs it only under re_grad (the staged adjoint
        runs there instead of the fused one) and prepares it on first use."""
        if self.direct is not None:
            return None, None
        if self.box is None:
            from .precond import box_solver_blob
            Y, X = self.active.shape[-2:]
            blob = box_solver_blob(Y, X)
            self.box = torch.from_numpy(blob).to(self.active.device)
            self.box_header = np.ascontiguousarray(blob[:16].view(np.int32))
        return self.box, self.box_header


def _mac(physics):
    """1 for a StepPhysics with advection="mac_cormack", else 0 (None: the plain step): the `advection` argument of the size functions"""
    return int(physics is not None and physics.adv is not None)


def large_workspace_bytes(cfg, masks, physics=None, saved=False):
    """Device scratch of the large-grid step for the scene's solver (direct, scattered direct or CG) under `physics` (a StepPhysics;
    None: the plain step); saved: of karman_step_saved, the training form.  The _adv size functions serve every mode: with advection = 0
    they return the plain functions' bytes (tests/test_workspace_bytes_cpu.py)."""
    lib = _lib.load()
    fn = lib.sol_karman_step_fwd_large_saved_adv_workspace_bytes_for if saved and _mac(physics) else lib.sol_karman_step_fwd_large_adv_workspace_bytes_for
    return fn(C.byref(cfg), _hdr(masks.direct_header), _mac(physics))


def large_bwd_workspace_bytes(cfg, masks, physics=None, re=False):
    """Device scratch of the large-grid velocity adjoint (sol_karman_step_bwd_large and its siblings) for the scene's solver under
    `physics`; re: with the gradient with respect to the Reynolds number (the _re entry points)."""
    return _lib.load().sol_karman_step_bwd_large_adv_workspace_bytes_for(C.byref(cfg), _hdr(masks.direct_header), int(re), _mac(physics))


def density_bwd_workspace_bytes(cfg, physics=None, re=False):
    """Device scratch of the density adjoint (sol_karman_density_bwd and its siblings) under `physics`; re: the _re entry points."""
    return _lib.load().sol_karman_density_bwd_adv_workspace_bytes(C.byref(cfg), int(re), _mac(physics))


def _hdr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _workspace(nbytes, workspace, device):
    """`workspace` when it holds nbytes, else a fresh buffer that does"""
    if workspace is None or workspace.numel() * 4 < nbytes:
        workspace = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
    return workspace


def _cg_info(masks, B, device):
    """[2][B] int32 that the large-grid CG solve reports to; None for a scene with the direct solver"""
    return torch.empty(2, B, dtype=torch.int32, device=device) if masks.direct is None else None


def _publish_cg(info, cg_info, suffix=""):
    if info is not None and cg_info is not None:
        info["iterations" + suffix], info["converged" + suffix] = cg_info[0], cg_info[1]


def _step_fwd_args(d, vy, vx, re, cfg, masks, outs=None):
    """Outputs of the forward step (fresh unless given) and the fourteen arguments each of its entry points begins with"""
    if outs is None:
        outs = torch.empty_like(d), torch.empty_like(vy), torch.empty_like(vx)
    head = (C.byref(cfg), stream(), ptr(d), ptr(vy), ptr(vx), ptr(re), ptr(masks.active), ptr(masks.inflow), ptr(masks.velBCy),
            ptr(masks.velBCyMask), masks.bc_stride, *(ptr(t) for t in outs))
    return outs, head


def buoyancy_force(buoyancy=None, buoyancy_factor=None, gravity=(-9.81, 0.0)):
    """The force per unit density F = (fy, fx) of the buoyant step, or None (off).  `buoyancy`: F itself, one number (fy) or a pair;
    else PhiFlow's spelling, F = -gravity * buoyancy_factor (Gravity() = -9.81 along y: F = (9.81 beta, 0)).  A force of (0, 0) is kept
    as given: the entry points take it and issue the plain launches."""
    if buoyancy is not None and buoyancy_factor is not None:
        raise ValueError("give buoyancy=(fy, fx) or buoyancy_factor (with gravity), not both")
    if buoyancy is None and buoyancy_factor is None:
        return None
    if buoyancy is None:
        g = (float(gravity), 0.0) if np.isscalar(gravity) else tuple(float(v) for v in gravity)
        if len(g) != 2:
            raise ValueError("gravity must be (gy, gx), got %r" % (gravity,))
        buoyancy = (-g[0] * float(buoyancy_factor), -g[1] * float(buoyancy_factor))
    f = (float(buoyancy), 0.0) if np.isscalar(buoyancy) else tuple(float(v) for v in buoyancy)
    if len(f) != 2 or not all(np.isfinite(f)):
        raise ValueError("buoyancy must be a finite force (fy, fx), got %r" % (buoyancy,))
    return f


def _buoyant(buoyancy):
    """True for a force that moves the velocity: the density is then part of the dynamics"""
    return buoyancy is not None and (buoyancy[0] != 0.0 or buoyancy[1] != 0.0)


# --------------------------------------------------------------------------------------
# advection scheme (include/sol_hip.h, "MACCORMACK ADVECTION on the large-grid step"; csrc/karman_maccormack.hip)
# --------------------------------------------------------------------------------------
ADVECTIONS = ("semi_lagrangian", "mac_cormack")


def advection_arg(advection="semi_lagrangian", correction_strength=1.0, who="advection"):
    """The pair of keywords as the calls below carry it: None for "semi_lagrangian" (the existing entry points, launches and bits), the
    correction strength s as a float for "mac_cormack".  An unknown name, or an s outside [0, 1] or not finite, raises ValueError (s is
    checked for either scheme)."""
    if advection not in ADVECTIONS:
        raise ValueError("%s must be one of %s (got %r)" % (who, ", ".join(ADVECTIONS), advection))
    if isinstance(correction_strength, bool) or not isinstance(correction_strength, (int, float, np.integer, np.floating)):
        raise ValueError("correction_strength must be a number in [0, 1] (got %r)" % (correction_strength,))
    s = float(correction_strength)
    if not (np.isfinite(s) and 0.0 <= s <= 1.0):
        raise ValueError("correction_strength must be finite and lie in [0, 1] (got %r)" % (correction_strength,))
    return s if advection == "mac_cormack" else None


def _adv_grid(cfg, who):
    if cfg.Y < 16 or cfg.X < 16:
        raise SolError("%s: the advection stage (sol_karman_advect) takes grids with Y, X >= 16; this one is %dx%d" % (who, cfg.Y, cfg.X))


def _adv_inputs(who, cfg, d, svy, svx, active, inflow):
    B, Y, X = cfg.B, cfg.Y, cfg.X
    d, svy, svx, active, inflow = (_lib.f32(t) for t in (d, svy, svx, active, inflow))
    if d.shape != (B, Y, X) or svy.shape != (B, Y + 1, X) or svx.shape != (B, Y, X + 1) or active.numel() != Y * X or inflow.numel() != Y * X:
        raise ValueError("%s: d %s, svy %s, svx %s, active %s, inflow %s are not [B,Y,X], [B,Y+1,X], [B,Y,X+1], [Y,X], [Y,X] of the cfg "
                         "(B, Y, X) = (%d, %d, %d)" % (who, tuple(d.shape), tuple(svy.shape), tuple(svx.shape), tuple(active.shape),
                                                      tuple(inflow.shape), B, Y, X))
    return d, svy, svx, active, inflow


def _adv_boundaries(who, boundaries):
    if any(boundaries_arg(boundaries, "%s: boundaries" % who)):
        raise SolError("%s: the advection stage alone is not built for periodic boundaries; run the whole step (karman_step_large / "
                       "karman_step_saved on masks built with boundaries=...), or use boundaries='open'" % who)


def karman_advect(d, svy, svx, cfg, active, inflow, advection="semi_lagrangian", correction_strength=1.0, workspace=None, boundaries="open"):
    """The advection stage of the large-grid step alone (sol_karman_advect; any Y, X >= 16): (d, svy, svx) -- the density and the
    post-diffusion velocity -- -> (d_out, a_y, a_x): the advected density (+ inflow as cfg.inflow_before says) and the advected velocity
    times the hard-BC face masks of `active` [Y,X].  advection = "mac_cormack": the MacCormack scheme with the revert-to-semi-Lagrangian
    limiter (form selected by the option k2d_mc_tile, equal bits)."""
    s = advection_arg(advection, correction_strength, "karman_advect: advection")
    _adv_boundaries("karman_advect", boundaries)
    _adv_grid(cfg, "karman_advect")
    _lib.require_gpu()
    lib = _lib.load()
    d, svy, svx, active, inflow = _adv_inputs("karman_advect", cfg, d, svy, svx, active, inflow)
    nbytes = lib.sol_karman_advect_workspace_bytes(C.byref(cfg), int(s is not None))
    ws = _workspace(nbytes, workspace, d.device) if nbytes else None
    outs = torch.empty_like(d), torch.empty_like(svy), torch.empty_like(svx)
    check(lib.sol_karman_advect(C.byref(cfg), stream(), ptr(d), ptr(svy), ptr(svx), ptr(active), ptr(inflow), int(s is not None),
                                1.0 if s is None else s, *(ptr(t) for t in outs), ptr(ws), 0 if ws is None else ws.numel() * 4))
    return outs


def karman_advect_bwd(d, svy, svx, cfg, active, inflow, g_d, g_ay, g_ax, advection="semi_lagrangian", correction_strength=1.0,
                      tile=True, workspace=None, boundaries="open"):
    """The transpose of karman_advect (sol_karman_advect_bwd): the cotangents of (d_out, a_y, a_x) -> (g_d_in, g_svy, g_svx), every
    decision of the forward stage (floor, clamp, limiter) frozen.  64-bit fixed-point scatter: bit-reproducible; tile=False takes global
    atomics only (equal bits).  A non-finite cotangent makes every gradient of its simulation NaN."""
    s = advection_arg(advection, correction_strength, "karman_advect_bwd: advection")
    _adv_boundaries("karman_advect_bwd", boundaries)
    _adv_grid(cfg, "karman_advect_bwd")
    _lib.require_gpu()
    lib = _lib.load()
    d, svy, svx, active, inflow = _adv_inputs("karman_advect_bwd", cfg, d, svy, svx, active, inflow)
    g_d, g_ay, g_ax = (_lib.f32(t) for t in (g_d, g_ay, g_ax))
    if g_d.shape != d.shape or g_ay.shape != svy.shape or g_ax.shape != svx.shape:
        raise ValueError("karman_advect_bwd: the cotangents must have the shapes of d, svy, svx")
    ws = _workspace(lib.sol_karman_advect_bwd_workspace_bytes(C.byref(cfg)), workspace, d.device)
    outs = torch.empty_like(d), torch.empty_like(svy), torch.empty_like(svx)
    check(lib.sol_karman_advect_bwd(C.byref(cfg), stream(), ptr(d), ptr(svy), ptr(svx), ptr(active), ptr(inflow), int(s is not None),
                                    1.0 if s is None else s, ptr(g_d), ptr(g_ay), ptr(g_ax), *(ptr(t) for t in outs), int(bool(tile)),
                                    ptr(ws), ws.numel() * 4))
    return outs


# --------------------------------------------------------------------------------------
# diffusion substeps (include/sol_hip.h, "DIFFUSION SUBSTEPS"; csrc/karman_diffuse_sub.hip)
# --------------------------------------------------------------------------------------
def diffusion_substeps_arg(n, who="diffusion_substeps"):
    """n as an int >= 1; anything else (a float, a bool, None, n < 1) raises ValueError"""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
        raise ValueError("%s must be an integer >= 1 (got %r)" % (who, n))
    if n < 1:
        raise ValueError("%s must be an integer >= 1 (got %d)" % (who, n))
    return int(n)


def min_diffusion_substeps(re_min, res, dt=1.0):
    """The smallest n with dt res^2 / (n re_min) <= 1/4: the explicit diffusion stencil v += a Lap(v) is a convex combination of a face
    and its four neighbours exactly while a <= 1/4; beyond it the checkerboard mode grows.  re_min: the smallest Reynolds number of the
    run."""
    re_min, res, dt = float(re_min), float(res), float(dt)
    if not (re_min > 0 and res > 0 and dt > 0) or not np.isfinite(dt * res * res / re_min):
        raise ValueError("min_diffusion_substeps: re_min, res and dt must be positive and finite (got %r, %r, %r)" % (re_min, res, dt))
    alpha = dt * res * res / re_min
    n = max(1, int(np.ceil(4.0 * alpha)))
    while alpha / n > 0.25:
        n += 1
    while n > 1 and alpha / (n - 1) <= 0.25:
        n -= 1
    return n


def diffusion_sub_cfg(cfg, n):
    """The cfg the existing step, its adjoints and the pre-diffusion run on under diffusion_substeps = n: a copy whose res is
    float32(res / sqrt(n)), so that their own expression dt * res * res / re[b] is the substep's coefficient; n = 1: cfg itself."""
    if n == 1:
        return cfg
    c = KarmanCfg.from_buffer_copy(cfg)
    c.res = float(np.float32(float(cfg.res) / np.sqrt(float(n))))
    c._keep = getattr(cfg, "_keep", None)
    return c


def _require_sub_grid(cfg, who):
    if cfg.Y < 16 or cfg.X < 16:
        raise SolError("%s: diffusion substeps (sol_karman_diffuse_sub) take grids with Y, X >= 16; this one is %dx%d" % (who, cfg.Y, cfg.X))


class StepPhysics(NamedTuple):
    """The physics of one 2-D step beyond the plain one, as every internal call carries it.  The default is the plain step: the launches
    and the bits of a call without any of the keywords.
    buoyancy = (fy, fx), a force per unit density (large grids only), or None: the step's output density pushes the velocity
    (sol_karman_step_fwd_large_buoy / _saved_buoy: one launch more).  With a force that moves the velocity the density is part of the
    dynamics: a differentiable step keeps it in the graph whatever density_grad says, and a velocity-only loss yields a density gradient.
    nsub = n >= 1, the diffusion substeps (grids with Y, X >= 16): the velocity is diffused by n explicit substeps of alpha / n, the
    boundary blend after the last one -- karman_diffuse_sub, then the step's launches on diffusion_sub_cfg(cfg, n).
    adv = the correction strength s in [0, 1] of advection="mac_cormack" (large grids only), or None for "semi_lagrangian": velocity and
    density are advected by the MacCormack scheme with the revert-to-semi-Lagrangian limiter (the _adv entry points; the adjoint freezes
    the limiter's decisions).
    The three compose with each other, with density_grad and re_grad, and with the no-grad extras of karman_step_large."""
    buoyancy: Optional[tuple] = None
    nsub: int = 1
    adv: Optional[float] = None

    @classmethod
    def of(cls, buoyancy=None, buoyancy_factor=None, gravity=(-9.81, 0.0), diffusion_substeps=1, advection="semi_lagrangian",
           correction_strength=1.0, who="the step", keep_zero_force=False):
        """From the user-facing keywords, validated (ValueError): diffusion_substeps_arg, advection_arg (s is checked under either
        scheme), buoyancy_force.  A force of (0, 0) becomes None, the plain step; keep_zero_force (the direct calls karman_step_large,
        karman_step_saved, karman_step_large_bwd_buoy) keeps it as given: their buoyant entry points take it and issue the plain launches."""
        n = diffusion_substeps_arg(diffusion_substeps, "%s: diffusion_substeps" % who)
        adv = advection_arg(advection, correction_strength, "%s: advection" % who)
        f = buoyancy_force(buoyancy, buoyancy_factor, gravity)
        return cls(f if keep_zero_force or _buoyant(f) else None, n, adv)

    def on(self, masks):
        """self as the launches of `masks` take it: a periodic scene has no buoyant entry points, a kept force of (0, 0) becomes None there"""
        return self.moving() if getattr(masks, "periodic_bits", 0) else self

    def moving(self):
        """self, a kept force of (0, 0) normalised to None: what a differentiable step runs on"""
        return self if self.buoyancy is None or _buoyant(self.buoyancy) else self._replace(buoyancy=None)

    def require(self, cfg, masks, who):
        """The grid checks (SolError), before any device call: substeps take Y, X >= 16; the buoyancy force and the mac_cormack advection
        are built on the large-grid step only (masks.large)."""
        if self.nsub > 1:
            _require_sub_grid(cfg, who)
        if getattr(masks, "periodic_bits", 0):
            if _buoyant(self.buoyancy):
                raise SolError("%s: a buoyancy force is not built for periodic boundaries; use buoyancy=None on a periodic scene, or open boundaries" % who)
            if self.adv is not None:
                raise SolError("%s: advection='mac_cormack' is not built for periodic boundaries; use advection='semi_lagrangian' on a periodic "
                               "scene, or open boundaries" % who)
            if self.nsub > 1:
                raise SolError("%s: diffusion_substeps > 1 is not built for periodic boundaries; use diffusion_substeps=1 on a periodic scene, "
                               "or open boundaries" % who)
        if self.buoyancy is not None and not masks.large:
            raise SolError("%s: the buoyancy force is built on the multi-launch (large-grid) step only; a %dx%d grid runs the fused "
                           "one-workgroup kernels (not ops.beyond_one_workgroup), which have no buoyancy term.  Masks built with "
                           "multi_launch=True run the multi-launch step on such a grid" % (who, cfg.Y, cfg.X))
        if self.adv is not None and not masks.large:
            raise SolError("%s: the mac_cormack advection is built on the multi-launch (large-grid) step only; a %dx%d grid runs the fused "
                           "one-workgroup kernels (not ops.beyond_one_workgroup), which advect semi-Lagrangian.  Masks built with "
                           "multi_launch=True run the multi-launch step on such a grid" % (who, cfg.Y, cfg.X))

    @property
    def mode(self):
        """Which family of entry points runs the step and its velocity adjoint: "_adv", "_buoy" or "" (plain)"""
        return "_adv" if self.adv is not None else "_buoy" if self.buoyancy is not None else ""

    @property
    def force_tail(self):
        """The arguments a _buoy or _adv entry point ends with: the force ((0, 0) without one), then advection = 1 and s"""
        f = (0.0, 0.0) if self.buoyancy is None else (float(self.buoyancy[0]), float(self.buoyancy[1]))
        return f if self.adv is None else f + (1, self.adv)

    @property
    def advection_kw(self):
        """{} or the two advection keywords of the public calls"""
        return {} if self.adv is None else {"advection": "mac_cormack", "correction_strength": self.adv}


@functools.lru_cache(maxsize=64, typed=True)
def _physics_of(who, buoyancy, diffusion_substeps, advection, correction_strength, keep_zero_force):
    return StepPhysics.of(buoyancy, None, None, diffusion_substeps, advection, correction_strength, who, keep_zero_force)


def _physics(physics, who, buoyancy=None, diffusion_substeps=1, advection="semi_lagrangian", correction_strength=1.0, keep_zero_force=False):
    """The StepPhysics of a public call: `physics` where the caller built one (it then replaces the keywords), else from the keywords --
    built and validated once per distinct set of them (a loop of steps passes the same ones at every call), not per call"""
    if physics is not None:
        return physics
    try:
        return _physics_of(who, buoyancy, diffusion_substeps, advection, correction_strength, keep_zero_force)
    except TypeError:               # an unhashable spelling (a force given as a list): built per call
        return _physics_of.__wrapped__(who, buoyancy, diffusion_substeps, advection, correction_strength, keep_zero_force)


def diffuse_sub_max():
    """S_MAX: the most substeps one launch of sol_karman_diffuse_sub runs"""
    return int(_lib.load().sol_karman_diffuse_sub_max())


def diffuse_sub_workspace_bytes(cfg, nsub, chunk=None):
    """Device scratch of karman_diffuse_sub(.., cfg, nsub, chunk): 0 when its nsub - 1 substeps fit one launch"""
    if nsub <= 1:
        return 0
    return _lib.load().sol_karman_diffuse_sub_workspace_bytes(C.byref(cfg), nsub - 1, 0 if chunk is None else int(chunk))


def karman_diffuse_sub(vy, vx, re, cfg, nsub, chunk=None, workspace=None):
    """The pre-diffusion of a step with diffusion_substeps = nsub (sol_karman_diffuse_sub): (vy, vx) -> M^(nsub-1) (vy, vx), M = I +
    (alpha / nsub) L with alpha = dt res^2 / re of `cfg` (the step's own, unscaled cfg) and L the 5-point Laplacian with replicate padding.
    M^(nsub-1) is symmetric: applied to a cotangent this is also the adjoint.  chunk: the most substeps per launch, 1 .. diffuse_sub_max()
    (None = that maximum, the measured default: profiles/k2d_substeps_time.json); the bits do not depend on it.  nsub = 1: no launch, the inputs are returned."""
    n = diffusion_substeps_arg(nsub, "karman_diffuse_sub: nsub")
    if chunk is not None and (isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or not 1 <= chunk <= diffuse_sub_max()):
        raise ValueError("karman_diffuse_sub: chunk must be None or an integer in [1, %d] (got %r)" % (diffuse_sub_max(), chunk))
    _lib.require_gpu()
    vy, vx, re = (_lib.f32(t) for t in (vy, vx, re))
    if n == 1:
        return vy, vx
    _require_sub_grid(cfg, "karman_diffuse_sub")
    B, Y, X = cfg.B, cfg.Y, cfg.X
    if vy.shape != (B, Y + 1, X) or vx.shape != (B, Y, X + 1) or re.shape != (B,):
        raise ValueError("karman_diffuse_sub: vy %s, vx %s, re %s are not [B,Y+1,X], [B,Y,X+1], [B] of the cfg (B, Y, X) = (%d, %d, %d)"
                         % (tuple(vy.shape), tuple(vx.shape), tuple(re.shape), B, Y, X))
    sc = diffusion_sub_cfg(cfg, n)
    nbytes = diffuse_sub_workspace_bytes(sc, n, chunk)
    ws = _workspace(nbytes, workspace, vy.device) if nbytes else None
    oy, ox = torch.empty_like(vy), torch.empty_like(vx)
    check(_lib.load().sol_karman_diffuse_sub(C.byref(sc), stream(), ptr(vy), ptr(vx), ptr(re), ptr(oy), ptr(ox), n - 1,
                                             0 if chunk is None else int(chunk), ptr(ws), 0 if ws is None else ws.numel() * 4))
    return oy, ox


def _sub_adjoint(oy, ox, g_re, re, cfg, nsub):
    """The tail of an adjoint under diffusion_substeps = nsub: (oy, ox) and g_re (any of them None) are what the existing adjoints
    returned on diffusion_sub_cfg(cfg, nsub) -- the cotangent of M^(nsub-1) v and 1/nsub of the gradient in re.  -> (g_vy, g_vx, g_re):
    the cotangent taken through M^(nsub-1) (karman_diffuse_sub: the operator is symmetric) and g_re times nsub (one fp32 multiply)."""
    if nsub > 1:
        if oy is not None:
            oy, ox = karman_diffuse_sub(oy, ox, re, cfg, nsub)
        if g_re is not None:
            g_re = g_re * float(nsub)
    return oy, ox, g_re


def _pre_diffuse(vy, vx, re, cfg, nsub):
    """The head of a step with diffusion_substeps = nsub: (vy, vx, cfg) its launches run on -- M^(nsub-1) (vy, vx) (karman_diffuse_sub)
    and diffusion_sub_cfg(cfg, nsub); nsub = 1: the arguments, no launch"""
    if nsub == 1:
        return vy, vx, cfg
    return karman_diffuse_sub(vy, vx, re, cfg, nsub) + (diffusion_sub_cfg(cfg, nsub),)


def _fwd_large(head, cfg, masks, ph, workspace, info, saved=None, feat=None, fs=None, p_guess=None):
    """The one launch of the large-grid forward step: sol_karman_step_fwd_large + the scene's solver and ph.mode.  saved = (svy, svx):
    the training form (_saved, _saved_buoy, _saved_adv); else the roll-out form with its extras (the plain step keeps an entry point
    per solver: the direct one, _cg, and _cg_warm with p_guess; _buoy and _adv take either solver and the guess).  `head`: of
    _step_fwd_args; `info` receives the CG solve's counts."""
    dev = masks.active.device
    ws = _workspace(large_workspace_bytes(cfg, masks, ph, saved is not None), workspace, dev)
    cg_info = _cg_info(masks, cfg.B, dev)
    mode = ph.mode
    solver = (_hdr(masks.direct_header), ptr(masks.box), _hdr(masks.box_header), ptr(cg_info))
    tail = (ptr(ws), ws.numel() * 4) + (ph.force_tail if mode else ())
    if saved is not None:
        name, args = "_saved" + mode, (ptr(saved[0]), ptr(saved[1]), *solver, *tail)
    elif mode:
        name, args = mode, (ptr(feat), fs, *solver, ptr(p_guess), *tail)
    elif cg_info is None:
        name, args = "", (ptr(feat), fs, solver[0], *tail)
    else:
        name, args = ("_cg", (ptr(feat), fs, *solver[1:], *tail)) if p_guess is None else ("_cg_warm", (ptr(feat), fs, *solver[1:], ptr(p_guess), *tail))
    check(getattr(_lib.load(), "sol_karman_step_fwd_large" + name)(*head, *args))
    _publish_cg(info, cg_info)


def _refuse_periodic_grads(who, masks, density_grad, re_grad):
    """density_grad and re_grad on a periodic scene: not built (SolError), whatever requires a gradient"""
    if getattr(masks, "periodic_bits", 0):
        if density_grad:
            raise SolError("%s: density_grad is not built for periodic boundaries; use density_grad=False (the density is a passive tracer "
                           "there), or open boundaries" % who)
        if re_grad:
            raise SolError("%s: re_grad is not built for periodic boundaries; use re_grad=False (re is data there), or open boundaries" % who)


def karman_step_saved(d, vy, vx, re, cfg, masks, workspace=None, info=None, buoyancy=None, diffusion_substeps=1,
                      advection="semi_lagrangian", correction_strength=1.0, physics=None):
    """The differentiable form of the step without autograd, on any grid: ((d, vy, vx) after the step, saved vy, saved vx) -- the
    post-diffusion velocity the adjoints take.  A one-workgroup grid runs sol_karman_step_fwd (`info` receives "iterations"), a grid
    beyond them (masks.large) sol_karman_step_fwd_large_saved with `workspace` and `info` as in karman_step_large.
    buoyancy, diffusion_substeps, advection, correction_strength: see StepPhysics (physics: one built by the caller, in their place)."""
    ph = _physics(physics, "karman_step_saved", buoyancy=buoyancy, diffusion_substeps=diffusion_substeps, advection=advection,
                  correction_strength=correction_strength, keep_zero_force=True)
    ph.require(cfg, masks, "karman_step_saved")
    ph = ph.on(masks)
    _lib.require_gpu()
    d, vy, vx, re = (_lib.f32(t) for t in (d, vy, vx, re))
    B, Y, X = cfg.B, cfg.Y, cfg.X
    assert vy.shape == (B, Y + 1, X) and vx.shape == (B, Y, X + 1) and d.shape == (B, Y, X) and re.shape == (B,)
    vy, vx, cfg = _pre_diffuse(vy, vx, re, cfg, ph.nsub)
    outs, head = _step_fwd_args(d, vy, vx, re, cfg, masks)
    svy, svx = torch.empty_like(vy), torch.empty_like(vx)
    if masks.large:
        _fwd_large(head, cfg, masks, ph, workspace, info, saved=(svy, svx))
    else:
        iters = None if info is None else torch.empty(B, dtype=torch.int32, device=vy.device)      # the kernel only stores to it
        check(_lib.load().sol_karman_step_fwd(*head, ptr(svy), ptr(svx), None, None, ptr(iters)))
        if info is not None:
            info["iterations"] = iters
    return outs, svy, svx


karman_step_large_saved = karman_step_saved      # the name the large-grid callers know it by (trainer.LargeGridTrainer, tools)


def karman_step_large(d, vy, vx, re, cfg, masks, workspace=None, info=None, feat=None, feat_scale=None, p_guess=None, out=None,
                      density_grad=False, re_grad=False, buoyancy=None, diffusion_substeps=1, advection="semi_lagrangian", correction_strength=1.0,
                      physics=None):
    """The step for grids beyond the one-workgroup kernels (data generation at 256 x 128,
    /root/reference/karman-2d/karman.py:98-159): sol_karman_step_fwd_large (direct solve) or sol_karman_step_fwd_large_cg (CG solve,
    masks.pressure_solver == "cg").  Returns (d, vy, vx) after the step; with the CG solve, `info` (a dict) receives "iterations" and
    "converged", device int32 [B] each.  When grad is enabled and vy or vx requires a gradient the call goes through KarmanStepFn
    (same forward launches, plus the saved post-diffusion velocity) and `info` also receives "iterations_bwd" / "converged_bwd" after
    backward(); otherwise nothing is kept.
    No-grad extras (a roll-out, trainer.LargeGridRollout): `feat` [B,Y,X,4] receives the network's input, to_feature of the new velocity
    times `feat_scale` (three factors, 1 / std; channel 3 is zero); `p_guess` [B,Y,X] warm-starts the CG solve
    (sol_karman_step_fwd_large_cg_warm: read as the initial guess, overwritten with the step's pressure) and is an error on a scene with
    the direct solver; `out` = (d, vy, vx) buffers to write instead of fresh tensors (they must not be the inputs).
    density_grad=True (opt-in): the density output is differentiable too (KarmanStepFn's density mode: same forward launches; the
    differentiable form is taken when any of d, vy, vx requires a gradient).
    re_grad=True (opt-in): a tensor `re` that requires a gradient receives one (KarmanStepFn's re mode: same forward launches, the step's
    input velocity saved as well; composes with density_grad).  Without the flag `re` is data.
    buoyancy (see buoyancy_force), diffusion_substeps, advection, correction_strength: see StepPhysics; each composes with every mode
    and extra above (physics: a StepPhysics built by the caller, in their place)."""
    ph = _physics(physics, "karman_step_large", buoyancy=buoyancy, diffusion_substeps=diffusion_substeps, advection=advection,
                  correction_strength=correction_strength, keep_zero_force=True)
    ph.require(cfg, masks, "karman_step_large")
    ph = ph.on(masks)
    _refuse_periodic_grads("karman_step_large", masks, density_grad, re_grad)
    if p_guess is not None and masks.direct is not None:
        raise ValueError("karman_step_large: p_guess warm-starts the CG pressure solve; this scene runs the direct solver (no iteration to start)")
    differentiable, density, want_re = _step_mode(d, vy, vx, re, cfg, density_grad, re_grad, ph)
    _lib.require_gpu()
    d, vy, vx, re = (_lib.f32(t) for t in (d, vy, vx, re))
    B, Y, X = cfg.B, cfg.Y, cfg.X
    assert vy.shape == (B, Y + 1, X) and vx.shape == (B, Y, X + 1) and d.shape == (B, Y, X) and re.shape == (B,)
    if differentiable:
        if feat is not None or p_guess is not None or out is not None:
            raise ValueError("karman_step_large: feat / p_guess / out belong to the no-grad step (the differentiable step keeps its own state)")
        return KarmanStepFn.apply(d, vy, vx, re, cfg, masks, workspace, info, density, want_re, ph.moving())
    vy, vx, cfg = _pre_diffuse(vy, vx, re, cfg, ph.nsub)
    if (feat is None) != (feat_scale is None):
        raise ValueError("karman_step_large: feat and feat_scale go together")
    if feat is not None and (feat.shape != (B, Y, X, 4) or feat.device != vy.device):
        raise ValueError("karman_step_large: feat must be [B,Y,X,4] = %s on %s (got %s on %s)" % ((B, Y, X, 4), vy.device, tuple(feat.shape), feat.device))
    if p_guess is not None and (p_guess.shape != (B, Y, X) or p_guess.device != vy.device):
        raise ValueError("karman_step_large: p_guess must be [B,Y,X] = %s on %s (got %s on %s)" % ((B, Y, X), vy.device, tuple(p_guess.shape), p_guess.device))
    if out is None:
        outs, head = _step_fwd_args(d, vy, vx, re, cfg, masks)
    else:
        outs = tuple(out)
        if [tuple(t.shape) for t in outs] != [tuple(t.shape) for t in (d, vy, vx)]:
            raise ValueError("karman_step_large: out must be (d, vy, vx) buffers of the inputs' shapes")
        head = _step_fwd_args(d, vy, vx, re, cfg, masks, outs)[1]
    fs = None if feat_scale is None else (feat_scale if isinstance(feat_scale, C.Array) else _scale3(feat_scale))
    _fwd_large(head, cfg, masks, ph, workspace, info, feat=feat, fs=fs, p_guess=p_guess)
    return outs


def karman_correct(out, vy, vx, s, cor=None):
    """velocity += s * to_staggered(out) in place, one launch (sol_karman_correct; karman_train.py:88-90, 424-426): out [B,Y,X,2] the
    network's output, vy [B,Y+1,X] / vx [B,Y,X+1] whose last row / column get no correction, s = (s0, s1) the output scale per
    component.  cor = (cor_y, cor_x) of the velocity's shapes receive the applied correction (zero on that row / column)."""
    _lib.require_gpu()
    B, Y, X = vx.shape[0], vx.shape[1], vy.shape[2]
    if out.shape != (B, Y, X, 2) or vy.shape != (B, Y + 1, X) or vx.shape != (B, Y, X + 1):
        raise ValueError("karman_correct: out %s, vy %s, vx %s are not [B,Y,X,2], [B,Y+1,X], [B,Y,X+1]" % (tuple(out.shape), tuple(vy.shape), tuple(vx.shape)))
    cy, cx = (None, None) if cor is None else cor
    if cor is not None and (cy.shape != vy.shape or cx.shape != vx.shape):
        raise ValueError("karman_correct: cor must be (cor_y, cor_x) of the velocity's shapes")
    check(_lib.load().sol_karman_correct(stream(), ptr(out), ptr(vy), ptr(vx), ptr(cy), ptr(cx), B, Y, X, float(s[0]), float(s[1])))


def _seam(name, vy, vx, periodic):
    _lib.require_gpu()
    bits = periodic if isinstance(periodic, (int, np.integer)) and not isinstance(periodic, bool) else periodic_bits(periodic)
    B, Y, X = vx.shape[0], vx.shape[1], vy.shape[2]
    if vy.shape != (B, Y + 1, X) or vx.shape != (B, Y, X + 1) or vy.dtype != torch.float32 or vx.dtype != torch.float32 or \
            not (vy.is_contiguous() and vx.is_contiguous()):
        raise ValueError("%s: vy %s, vx %s must be contiguous float32 [B,Y+1,X], [B,Y,X+1]" % (name, tuple(vy.shape), tuple(vx.shape)))
    check(getattr(_lib.load(), "sol_" + name)(stream(), ptr(vy), ptr(vx), B, Y, X, int(bits)))
    return vy, vx


def karman_seam_sync(vy, vx, periodic):
    """In place: plane 0 copied onto the duplicate plane of a periodic axis (sol_karman_seam_sync) -- vy[:, Y, :] = vy[:, 0, :] when y is
    periodic, vx[:, :, X] = vx[:, :, 0] when x is.  periodic: (py, px) (SceneMasks.periodic) or the bits.  What follows karman_correct
    on a periodic scene, which leaves the duplicate plane stale.  Open scenes: nothing is launched."""
    return _seam("karman_seam_sync", vy, vx, periodic)


def karman_seam_fold(g_vy, g_vx, periodic):
    """In place, the adjoint of karman_seam_sync on a cotangent (sol_karman_seam_fold): g[plane 0] += g[duplicate], g[duplicate] = 0."""
    return _seam("karman_seam_fold", g_vy, g_vx, periodic)


class SeamSyncFn(torch.autograd.Function):
    """karman_seam_sync for autograd compositions (out of place): (vy, vx) -> copies with the duplicate planes equal to plane 0; backward
    = karman_seam_fold on copies of the cotangents"""

    @staticmethod
    def forward(ctx, vy, vx, bits):
        ctx.bits = int(bits)
        return karman_seam_sync(_lib.f32(vy).clone(), _lib.f32(vx).clone(), ctx.bits)

    @staticmethod
    def backward(ctx, gy, gx):
        return karman_seam_fold(_lib.f32(gy).contiguous().clone(), _lib.f32(gx).contiguous().clone(), ctx.bits) + (None,)


def pressure_solve_large(rhs, cfg, masks, workspace=None, info=None):
    """The large-grid step's pressure solve alone: p [B,Y,X] with M p = rhs, M = -A of the scene's mask (precond.scene_matrix).  CG scenes:
    sol_karman_pressure_solve_large, `info` receives "iterations" / "converged" (device int32 [B]).  Scenes with
    pressure_solver="direct_scattered": sol_karman_pressure_solve_large_direct (no iteration, `info` stays empty)."""
    _lib.require_gpu()
    lib = _lib.load()
    rhs = _lib.f32(rhs)
    B, Y, X = cfg.B, cfg.Y, cfg.X
    assert rhs.shape == (B, Y, X)
    if masks.pressure_solver == "direct_scattered":
        workspace = _workspace(large_workspace_bytes(cfg, masks), workspace, rhs.device)
        p = torch.empty_like(rhs)
        check(lib.sol_karman_pressure_solve_large_direct(C.byref(cfg), stream(), ptr(rhs), ptr(p), _hdr(masks.direct_header),
                                                         ptr(workspace), workspace.numel() * 4))
        return p
    if masks.box is None:
        raise ValueError("pressure_solve_large needs a scene prepared for the large-grid CG solve (SceneMasks.pressure_solver == 'cg') "
                         "or for the scattered direct solve ('direct_scattered')")
    workspace = _workspace(lib.sol_karman_step_large_cg_workspace_bytes(C.byref(cfg)), workspace, rhs.device)
    p = torch.empty_like(rhs)
    cg_info = _cg_info(masks, B, rhs.device)
    check(lib.sol_karman_pressure_solve_large(C.byref(cfg), stream(), ptr(masks.active), ptr(rhs), ptr(p), ptr(masks.box),
                                              masks.box_header.ctypes.data_as(C.c_void_p), ptr(cg_info), ptr(workspace),
                                              workspace.numel() * 4))
    _publish_cg(info, cg_info)
    return p


def karman_pressure_solve_large(rhs, cfg, masks, workspace=None, info=None):
    """pressure_solve_large for every solver of the multi-launch path: a scene with a direct blob, one-window or scattered, runs
    sol_karman_pressure_solve_large_direct (on masks built with multi_launch=True and the option k2d_solve_one_wg the one-launch solve
    of csrc/karman_solve_small.hip where it serves the grid), a CG scene sol_karman_pressure_solve_large."""
    if masks.direct is None or masks.pressure_solver == "direct_scattered":
        return pressure_solve_large(rhs, cfg, masks, workspace, info)
    if cfg.Y < 16 or cfg.X < 16:
        raise SolError("karman_pressure_solve_large: the multi-launch direct solve takes grids with Y, X >= 16; this one is %dx%d" % (cfg.Y, cfg.X))
    _lib.require_gpu()
    rhs = _lib.f32(rhs)
    assert rhs.shape == (cfg.B, cfg.Y, cfg.X)
    workspace = _workspace(large_workspace_bytes(cfg, masks), workspace, rhs.device)
    p = torch.empty_like(rhs)
    check(_lib.load().sol_karman_pressure_solve_large_direct(C.byref(cfg), stream(), ptr(rhs), ptr(p), _hdr(masks.direct_header),
                                                             ptr(workspace), workspace.numel() * 4))
    return p


def solve_one_wg_supported(Y, X, win):
    """True where the one-launch direct solve (sol_karman_solve_one_wg) serves a Y x X grid with a one-window blob of window `win`"""
    return bool(_lib.load().sol_karman_solve_one_wg_supported(int(Y), int(X), int(win)))


def _scale3(vals):
    return (C.c_float * 3)(*[float(v) for v in vals])


def _step_bwd(svy, svx, re, gvy, gvx, cfg, masks, info):
    """The one-workgroup velocity adjoint (sol_karman_step_bwd), pressure solve fused in"""
    lib = _lib.load()
    oy = torch.empty_like(svy)
    ox = torch.empty_like(svx)
    iters = torch.empty(cfg.B, dtype=torch.int32, device=svy.device)
    check(lib.sol_karman_step_bwd(C.byref(cfg), stream(), ptr(svy), ptr(svx), ptr(re), ptr(masks.active),
                                  ptr(masks.velBCyMask), masks.bc_stride, ptr(gvy), ptr(gvx), None, None,
                                  ptr(oy), ptr(ox), ptr(iters)))
    if info is not None:
        info["iterations_bwd"] = iters
    return oy, ox


def _require_staged(cfg, who):
    if cfg.Y < 16 or cfg.X < 16:
        raise SolError("%s: the gradient with respect to re runs the staged adjoint (sol_karman_step_bwd_large_re), which takes grids "
                       "with Y, X >= 16; this one is %dx%d" % (who, cfg.Y, cfg.X))


def _re_tail(who, re_in, svy, svx, B):
    """The four arguments an _re entry point takes after its plain sibling's, from re_in = (vy_in, vx_in, g_re): the step's INPUT
    velocity, and g_re [B], the caller's buffer to add onto (one fp32 add) or None for a fresh one to write  ->  (arguments, g_re)"""
    vy_in, vx_in, g_re = re_in
    vy_in, vx_in = _lib.f32(vy_in), _lib.f32(vx_in)
    if vy_in.shape != svy.shape or vx_in.shape != svx.shape:
        raise ValueError("%s: vy_in / vx_in must have the velocity's shapes" % who)
    accumulate = g_re is not None
    if not accumulate:
        g_re = torch.empty(B, dtype=torch.float32, device=svy.device)
    elif g_re.shape != (B,):
        raise ValueError("%s: g_re must be [B] = (%d,), got %s" % (who, B, tuple(g_re.shape)))
    return (ptr(vy_in), ptr(vx_in), ptr(g_re), int(accumulate)), g_re


def _velocity_bwd(who, svy, svx, re, gvy, gvx, gd, cfg, masks, ph, re_in, workspace, info, fused):
    """The velocity half of the step's adjoint on the cfg as given, the one launch site of sol_karman_step_bwd_large + ph.mode (+ _re with
    re_in = (vy_in, vx_in, g_re)): -> (g_vy_in, g_vx_in, g_re | None, g_dsum | None).  A missing cotangent counts as zero.  The _buoy and
    _adv entry points (the latter with a force of (0, 0) when there is none) also write g_dsum = gd + dt F . transpose of the face
    average of the cotangent, what the density half then runs on; under mac_cormack with neither a force nor gd nothing reaches the
    density and g_dsum is None.  The plain ones hand gd through.  fused (the autograd step): a one-workgroup grid without re_in runs
    sol_karman_step_bwd, the pressure solve fused in."""
    gvy = torch.zeros_like(svy) if gvy is None else _lib.f32(gvy)
    gvx = torch.zeros_like(svx) if gvx is None else _lib.f32(gvx)
    mode = ph.mode
    if fused and re_in is None and not mode and not masks.large:
        return _step_bwd(svy, svx, re, gvy, gvx, cfg, masks, info) + (None, gd)
    tail, g_re = ((), None) if re_in is None else _re_tail(who, re_in, svy, svx, cfg.B)
    g_dsum = gd
    if mode:
        g_dsum = torch.empty(cfg.B, cfg.Y, cfg.X, dtype=torch.float32, device=svy.device)
        force = ph.force_tail
        tail += force[:2] + (ptr(gd), ptr(g_dsum)) + force[2:]
    box, box_header = masks.staged_box()
    workspace = _workspace(large_bwd_workspace_bytes(cfg, masks, ph, re_in is not None), workspace, svy.device)
    oy, ox = torch.empty_like(svy), torch.empty_like(svx)
    cg_info = _cg_info(masks, cfg.B, svy.device)
    entry = getattr(_lib.load(), "sol_karman_step_bwd_large" + mode + ("" if re_in is None else "_re"))
    check(entry(C.byref(cfg), stream(), ptr(svy), ptr(svx), ptr(re), ptr(masks.active), ptr(masks.velBCyMask), masks.bc_stride,
                ptr(gvy), ptr(gvx), ptr(oy), ptr(ox), _hdr(masks.direct_header), ptr(box), _hdr(box_header), ptr(cg_info),
                ptr(workspace), workspace.numel() * 4, *tail))
    _publish_cg(info, cg_info, "_bwd")
    if ph.adv is not None and gd is None and force[:2] == (0.0, 0.0):
        g_dsum = None
    return oy, ox, g_re, g_dsum


def karman_step_large_bwd(svy, svx, re, gvy, gvx, cfg, masks, workspace=None, info=None, diffusion_substeps=1,
                          advection="semi_lagrangian", correction_strength=1.0, physics=None):
    """Adjoint of the large-grid step, the velocity's part (sol_karman_step_bwd_large; under advection="mac_cormack" _adv): (g_vy_in,
    g_vx_in) from the saved post-diffusion velocity and the gradient with respect to the step's output velocity.  With the CG solve,
    `info` receives "iterations_bwd" / "converged_bwd".  diffusion_substeps = n: the adjoint of karman_step_saved(.., diffusion_substeps=n),
    `cfg` the step's own, unscaled one (see _step_adjoint).  The density's part is karman_density_bwd with the same keywords."""
    ph = _physics(physics, "karman_step_large_bwd", diffusion_substeps=diffusion_substeps, advection=advection, correction_strength=correction_strength)
    return _step_adjoint("karman_step_large_bwd", None, svy, svx, re, None, gvy, gvx, cfg, masks, ph, False, None, None, workspace, info)[1:3]


def karman_step_large_bwd_re(svy, svx, re, gvy, gvx, vy_in, vx_in, cfg, masks, g_re=None, workspace=None, info=None, diffusion_substeps=1,
                             advection="semi_lagrangian", correction_strength=1.0, physics=None):
    """The staged velocity adjoint with the gradient with respect to re (sol_karman_step_bwd_large_re), on every grid with Y, X >= 16 --
    the one-workgroup grids included: (g_vy_in, g_vx_in, g_re) from the saved post-diffusion velocity, the cotangent of the step's output
    velocity and the step's INPUT velocity.  g_vy_in / g_vx_in are karman_step_large_bwd's bits.  g_re [B]: a buffer to add onto (one
    fp32 add), else a fresh one is written.
    diffusion_substeps = n > 1: as in karman_step_large_bwd; vy_in / vx_in are then the PRE-DIFFUSED input, karman_diffuse_sub(vy, vx, re,
    cfg, n), and the reduction's result is multiplied by n (a g_re to add onto is not taken: it would be scaled too; nor is one under
    advection="mac_cormack")."""
    ph = _physics(physics, "karman_step_large_bwd_re", diffusion_substeps=diffusion_substeps, advection=advection, correction_strength=correction_strength)
    if ph.nsub > 1 and g_re is not None:
        raise ValueError("karman_step_large_bwd_re: with diffusion_substeps > 1 the gradient in re is written to a fresh tensor (g_re=None)")
    if ph.adv is not None and g_re is not None:
        raise ValueError("karman_step_large_bwd_re: with advection='mac_cormack' the gradient in re is written to a fresh tensor (g_re=None)")
    return _step_adjoint("karman_step_large_bwd_re", None, svy, svx, re, None, gvy, gvx, cfg, masks, ph, False, (vy_in, vx_in), g_re, workspace, info)[1:]


def _density_bwd(who, d, svy, svx, re, g_d, cfg, masks, g_vy, g_vx, workspace, re_in=None, ph=StepPhysics()):
    """The density half of the step's adjoint on the cfg as given, the one launch site of sol_karman_density_bwd (+ _adv under
    ph.adv, + _re with re_in = (vy_in, vx_in, g_re)): -> (g_d_in, g_vy_in, g_vx_in[, g_re]), added onto g_vy / g_vx and g_re where given"""
    if ph.adv is not None:
        _adv_grid(cfg, who)
    _lib.require_gpu()
    if (g_vy is None) != (g_vx is None):
        raise ValueError("%s: g_vy and g_vx go together" % who)
    B, Y, X = cfg.B, cfg.Y, cfg.X
    d, svy, svx, re, g_d = (_lib.f32(t) for t in (d, svy, svx, re, g_d))
    for name, t, shape in (("d", d, (B, Y, X)), ("g_d", g_d, (B, Y, X)), ("svy", svy, (B, Y + 1, X)), ("svx", svx, (B, Y, X + 1)), ("re", re, (B,))):
        if t.shape != shape:
            raise ValueError("%s: %s is %s, not %s of the cfg (B, Y, X) = (%d, %d, %d)" % (who, name, tuple(t.shape), shape, B, Y, X))
    accumulate = g_vy is not None
    if accumulate and (g_vy.shape != svy.shape or g_vx.shape != svx.shape):
        raise ValueError("%s: g_vy / g_vx must have the velocity's shapes" % who)
    tail, g_re = ((), None) if re_in is None else _re_tail(who, re_in, svy, svx, B)
    if ph.adv is not None:
        tail += (1, ph.adv)
    oy, ox = (g_vy, g_vx) if accumulate else (torch.empty_like(svy), torch.empty_like(svx))
    od = torch.empty_like(d)
    workspace = _workspace(density_bwd_workspace_bytes(cfg, ph, re_in is not None), workspace, d.device)
    entry = getattr(_lib.load(), "sol_karman_density_bwd" + ("" if ph.adv is None else "_adv") + ("" if re_in is None else "_re"))
    check(entry(C.byref(cfg), stream(), ptr(d), ptr(masks.inflow), ptr(svy), ptr(svx), ptr(re), ptr(masks.velBCyMask), masks.bc_stride,
                ptr(g_d), ptr(od), ptr(oy), ptr(ox), int(accumulate), ptr(workspace), workspace.numel() * 4, *tail))
    return (od, oy, ox) if re_in is None else (od, oy, ox, g_re)


def karman_density_bwd(d, svy, svx, re, g_d, cfg, masks, g_vy=None, g_vx=None, workspace=None, advection="semi_lagrangian", correction_strength=1.0):
    """Adjoint of the step's marker density (sol_karman_density_bwd), on any grid: (g_d_in, g_vy_in, g_vx_in) from the step's input
    density `d`, the saved post-diffusion velocity and the gradient `g_d` with respect to the step's output density.  g_vy / g_vx (both
    or neither): buffers that already hold the velocity adjoint's result; the density's part is added onto them in place (one fp32 add
    per face) and they are returned.  Without them the density's part alone is written to fresh tensors.
    advection = "mac_cormack" (grids with Y, X >= 16): the adjoint of the MacCormack-advected density (sol_karman_density_bwd_adv)."""
    ph = _physics(None, "karman_density_bwd", advection=advection, correction_strength=correction_strength)
    return _density_bwd("karman_density_bwd", d, svy, svx, re, g_d, cfg, masks, g_vy, g_vx, workspace, None, ph)


def karman_density_bwd_re(d, svy, svx, re, g_d, vy_in, vx_in, cfg, masks, g_vy=None, g_vx=None, g_re=None, workspace=None,
                          advection="semi_lagrangian", correction_strength=1.0):
    """karman_density_bwd with the gradient with respect to re (sol_karman_density_bwd_re): (g_d_in, g_vy_in, g_vx_in, g_re).  The first
    three are karman_density_bwd's bits; g_re [B]: a buffer to add onto (the velocity adjoint's part), else a fresh one is written."""
    ph = _physics(None, "karman_density_bwd_re", advection=advection, correction_strength=correction_strength)
    return _density_bwd("karman_density_bwd_re", d, svy, svx, re, g_d, cfg, masks, g_vy, g_vx, workspace, (vy_in, vx_in, g_re), ph)


def karman_buoyancy_add(d, vy, vx, active, f):
    """The buoyancy term alone, in place (sol_karman_buoyancy_add): vy [B,Y+1,X], vx [B,Y,X+1] = (v + f * face average of d) * face mask,
    d [B,Y,X] with a zero ghost ring, active [Y,X], f = (fy dt, fx dt); a component with f = 0 is not touched.  Any Y, X >= 1."""
    _lib.require_gpu()
    B, Y, X = d.shape
    if vy.shape != (B, Y + 1, X) or vx.shape != (B, Y, X + 1) or active.numel() != Y * X:
        raise ValueError("karman_buoyancy_add: d %s, vy %s, vx %s, active %s are not [B,Y,X], [B,Y+1,X], [B,Y,X+1], [Y,X]"
                         % (tuple(d.shape), tuple(vy.shape), tuple(vx.shape), tuple(active.shape)))
    check(_lib.load().sol_karman_buoyancy_add(stream(), B, Y, X, ptr(active), ptr(d), float(f[0]), float(f[1]), ptr(vy), ptr(vx)))
    return vy, vx


def karman_buoyancy_add_bwd(gvy, gvx, active, f, gd=None):
    """The exact transpose of karman_buoyancy_add (sol_karman_buoyancy_add_bwd): g_dsum [B,Y,X] = gd (None = zero) + f . (face-to-cell
    transpose of the masked gvy [B,Y+1,X], gvx [B,Y,X+1]).  A gather in a fixed order: bit-reproducible."""
    _lib.require_gpu()
    B, Y, X = gvx.shape[0], gvx.shape[1], gvy.shape[2]
    if gvy.shape != (B, Y + 1, X) or gvx.shape != (B, Y, X + 1) or active.numel() != Y * X or (gd is not None and gd.shape != (B, Y, X)):
        raise ValueError("karman_buoyancy_add_bwd: gvy %s, gvx %s, active %s are not [B,Y+1,X], [B,Y,X+1], [Y,X] (gd: [B,Y,X])"
                         % (tuple(gvy.shape), tuple(gvx.shape), tuple(active.shape)))
    out = torch.empty(B, Y, X, dtype=torch.float32, device=gvy.device)
    check(_lib.load().sol_karman_buoyancy_add_bwd(stream(), B, Y, X, ptr(active), ptr(gvy), ptr(gvx), float(f[0]), float(f[1]), ptr(gd), ptr(out)))
    return out


def _step_adjoint(who, d, svy, svx, re, gd, gvy, gvx, cfg, masks, ph, density, vel_in=None, g_re=None, workspace=None, info=None,
                  density_workspace=None, fused=False):
    """THE adjoint of one step under ph, behind KarmanStepFn.backward and the direct calls karman_step_large_bwd / _bwd_re / _bwd_buoy:
    -> (g_d_in, g_vy_in, g_vx_in, g_re), each None where nothing reaches it.  From the step's input density `d`, the saved post-diffusion
    velocity, the cotangents gd, gvy, gvx of its outputs (None = zero) and `cfg`, the step's own (unscaled) one.
    - `density`: the density is in the graph (density_grad, or a force that moves the velocity); without it gd is ignored and the density
      half never runs.
    - The velocity half (_velocity_bwd, with its pressure solve) runs only when a velocity cotangent arrived.  Without one the density
      half runs on gd alone; with no cotangent at all every result is None.
    - The density half (_density_bwd) runs on what the velocity half left for it (g_dsum: gd, plus the force's part under _buoy / _adv)
      and adds onto the velocity half's buffers and onto g_re.
    - vel_in = (vy_in, vx_in), the step's input velocity (under substeps the PRE-DIFFUSED one), asks for g_re: the _re entry points on
      grids with Y, X >= 16.  g_re: a buffer to add onto (plain mode only).
    - ph.nsub = n > 1: both halves run on diffusion_sub_cfg(cfg, n); the velocity cotangent then goes through karman_diffuse_sub on cfg
      (M^(n-1) is symmetric) and g_re is multiplied by n, once (_sub_adjoint).
    `info` receives "iterations_bwd" / "converged_bwd"; workspace / density_workspace: scratch of the two halves; fused: see _velocity_bwd."""
    ph.require(cfg, masks, who)
    ph = ph.on(masks)
    _refuse_periodic_grads(who, masks, density, vel_in is not None)
    gd = gd if density else None
    od = oy = ox = None
    if gvy is None and gvx is None and gd is None:
        return None, None, None, None
    if vel_in is not None:
        _require_staged(cfg, who)
    _lib.require_gpu()
    sc = diffusion_sub_cfg(cfg, ph.nsub)
    svy, svx, re = (_lib.f32(t) for t in (svy, svx, re))
    g_dsum = gd = None if gd is None else _lib.f32(gd)
    if gvy is not None or gvx is not None:
        oy, ox, g_re, g_dsum = _velocity_bwd(who, svy, svx, re, gvy, gvx, gd, sc, masks, ph, None if vel_in is None else (*vel_in, g_re),
                                             workspace, info, fused)
    if density and g_dsum is not None:
        od, oy, ox, *g = _density_bwd(who, d, svy, svx, re, g_dsum, sc, masks, oy, ox, density_workspace,
                                      None if vel_in is None else (*vel_in, g_re), ph)
        g_re = g[0] if g else None
    return (od,) + _sub_adjoint(oy, ox, g_re, re, cfg, ph.nsub)


def karman_step_large_bwd_buoy(d, svy, svx, re, gvy, gvx, gd, cfg, masks, buoyancy, vel_in=None, workspace=None, info=None,
                               density_workspace=None, diffusion_substeps=1, advection="semi_lagrangian", correction_strength=1.0, physics=None):
    """Adjoint of the BUOYANT large-grid step (karman_step_saved(..., buoyancy=F)), the density in the graph: (g_d_in, g_vy_in, g_vx_in)
    -- with vel_in = (vy, vx), the step's input velocity, (g_d_in, g_vy_in, g_vx_in, g_re) -- from the step's input density `d`, the
    saved post-diffusion velocity and the cotangents gvy, gvx, gd of its outputs (None = zero): _step_adjoint, which describes the chain
    and the other keywords."""
    ph = _physics(physics, "karman_step_large_bwd_buoy", buoyancy=buoyancy, diffusion_substeps=diffusion_substeps, advection=advection,
                  correction_strength=correction_strength, keep_zero_force=True)
    res = _step_adjoint("karman_step_large_bwd_buoy", d, svy, svx, re, gd, gvy, gvx, cfg, masks, ph, True, vel_in, None, workspace, info,
                        density_workspace)
    return res if vel_in is not None else res[:3]


class KarmanStepFn(torch.autograd.Function):
    """(d, vy, vx) [B,Y,X] / [B,Y+1,X] / [B,Y,X+1] -> one simulator_lo.step(...) on any grid, with its hand-written adjoint; the forward
    launches are karman_step_saved's and the backward ones _step_adjoint's in every mode.  Plain: differentiable with respect to the
    velocity, the density is a passive tracer.  `density` (opt-in, density_grad=True): the density output is differentiable too.
    `want_re` (opt-in, re_grad=True; grids with Y, X >= 16, which _step_mode and the torch.ops.sol steps check): differentiable with
    respect to re as well, the step's input velocity saved beside the post-diffusion one.  `physics`: the StepPhysics, a force in it one
    that moves the velocity (StepPhysics.moving) -- the density is then in the graph whatever `density` says.
    backward returns (g_d_in | None, g_vy_in, g_vx_in, g_re | None)."""

    @staticmethod
    def forward(ctx, d, vy, vx, re, cfg, masks, workspace, info, density, want_re, physics):
        _lib.require_gpu()
        d, vy, vx, re = (_lib.f32(t) for t in (d, vy, vx, re))
        density = bool(density) or physics.buoyancy is not None
        _refuse_periodic_grads("KarmanStepFn", masks, density, want_re)
        ctx.cfg, ctx.masks, ctx.info, ctx.density, ctx.want_re, ctx.physics = cfg, masks, info, density, want_re, physics
        # under substeps the pre-diffused velocity M^(nsub-1) v is also the "input velocity" the re mode saves
        vy, vx, cfg = _pre_diffuse(vy, vx, re, cfg, physics.nsub)
        outs, svy, svx = karman_step_saved(d, vy, vx, re, cfg, masks, workspace, info, physics=physics._replace(nsub=1))
        ctx.save_for_backward(svy, svx, re, *((d, vy, vx) if want_re else (d,) if density else ()))
        if not density:
            ctx.mark_non_differentiable(outs[0])
        ctx.set_materialize_grads(False)
        return outs

    @staticmethod
    def backward(ctx, gd, gvy, gvx):
        svy, svx, re, *inputs = ctx.saved_tensors
        res = _step_adjoint("KarmanStepFn.backward", inputs[0] if ctx.density else None, svy, svx, re, gd, gvy, gvx, ctx.cfg, ctx.masks,
                            ctx.physics, ctx.density, tuple(inputs[1:]) if ctx.want_re else None, info=ctx.info, fused=True)
        return res + (None,) * 7


def _step_mode(d, vy, vx, re, cfg, density_grad, re_grad, ph=StepPhysics()):
    """(differentiable?, density, want_re) of a call of karman_step / karman_step_large, from its inputs as given and its two flags.
    re_grad with an `re` that requires no gradient is the plain mode.  A grid the staged adjoint does not take is refused here, before
    any device call."""
    needs = lambda t: isinstance(t, torch.Tensor) and t.requires_grad
    density = bool(density_grad) or _buoyant(ph.buoyancy)          # a force that moves the velocity: the density is always in the graph
    want_re = bool(re_grad) and torch.is_grad_enabled() and needs(re)
    if want_re:
        _require_staged(cfg, "re_grad")
    return torch.is_grad_enabled() and (needs(vy) or needs(vx) or (density and needs(d)) or want_re), density, want_re


def karman_step(d, vy, vx, re, cfg, masks, info=None, density_grad=False, re_grad=False, diffusion_substeps=1, physics=None):
    """One step on a one-workgroup grid.  density_grad=True (opt-in): the density output is differentiable too (KarmanStepFn's density
    mode), taken when any of d, vy, vx requires a gradient.  re_grad=True (opt-in): a tensor `re` that requires a gradient receives one
    (KarmanStepFn's re mode; grids with Y, X >= 16; composes with density_grad).  Without the flag `re` is data.
    diffusion_substeps = n > 1 (grids with Y, X >= 16): karman_diffuse_sub, then the fused kernel on diffusion_sub_cfg(cfg, n)."""
    ph = _physics(physics, "karman_step", diffusion_substeps=diffusion_substeps)
    ph.require(cfg, masks, "karman_step")
    _refuse_periodic_grads("karman_step", masks, density_grad, re_grad)
    differentiable, density, want_re = _step_mode(d, vy, vx, re, cfg, density_grad, re_grad)
    if not differentiable:
        return karman_step_saved(d, vy, vx, re, cfg, masks, None, info, physics=ph)[0]
    _lib.require_gpu()
    d, vy, vx, re = (_lib.f32(t) for t in (d, vy, vx, re))
    return KarmanStepFn.apply(d, vy, vx, re, cfg, masks, None, info, density, want_re, ph)


# --------------------------------------------------------------------------------------
# conv 5x5
# --------------------------------------------------------------------------------------
def _pack(w_hwio, cin_run, cout_run, mode):
    lib = _lib.load()
    n = lib.sol_conv5x5_packed_floats(cin_run, cout_run, mode)
    out = torch.empty(n, dtype=torch.float32, device=w_hwio.device)
    check(lib.sol_conv5x5_pack(stream(), ptr(w_hwio), cin_run, cout_run, mode, ptr(out)))
    return out


def _pad_channels(x, c):
    if x.shape[-1] == c:
        return x.contiguous()
    return torch.nn.functional.pad(x, (0, c - x.shape[-1])).contiguous()


def conv5x5_raw(x, packed, bias, residual, act_ref, cout, epilogue, slope):
    lib = _lib.load()
    B, H, W, cin = x.shape
    y = torch.empty(B, H, W, cout, dtype=torch.float32, device=x.device)
    check(lib.sol_conv5x5(stream(), ptr(x), ptr(packed), ptr(bias), ptr(residual), ptr(act_ref), ptr(y),
                          B, H, W, cin, cout, epilogue, float(slope)))
    return y


AMAX_SLOTS = 256         # SOL_AMAX_SLOTS of csrc/common.hpp (include/sol_hip.h: sol_conv5x5_scaled)


def absmax_slots(x):
    """[AMAX_SLOTS] int32 slots holding the bit pattern of max|x| (the form sol_conv5x5_scaled consumes).  In the fused
    trainer the producing kernel publishes this; here it costs one reduction pass."""
    assert _lib.load().sol_absmax_slots() == AMAX_SLOTS
    slots = torch.zeros(AMAX_SLOTS, dtype=torch.int32, device=x.device)
    slots[0] = x.detach().abs().max().to(torch.float32).view(torch.int32)
    return slots


def conv5x5_scaled_raw(x, packed, bias, residual, act_ref, cout, epilogue, slope, x_absmax, y_absmax=None):
    """sol_conv5x5_scaled: fp16 three-product MFMA path when x_absmax is given (32 input channels, W % 64 == 0)."""
    lib = _lib.load()
    B, H, W, cin = x.shape
    y = torch.empty(B, H, W, cout, dtype=torch.float32, device=x.device)
    check(lib.sol_conv5x5_scaled(stream(), ptr(x), ptr(packed), ptr(bias), ptr(residual), ptr(act_ref), ptr(y),
                                 B, H, W, cin, cout, epilogue, float(slope), ptr(x_absmax), ptr(y_absmax)))
    return y


def conv5x5_cols_raw(x, packed, bias, residual, act_ref, cout, epilogue, slope, wv, x_absmax=None, y_absmax=None, y=None):
    """sol_conv5x5_cols: sol_conv5x5_scaled on pitched rows -- x [B,H,W,cin] with W % 64 == 0 of which the first `wv` columns are data
    and the rest ZERO (the caller's duty, also for residual / act_ref); the pad columns of y are written as zeros and stay out of
    y_absmax.  y: an output buffer to write into (default: a new one)."""
    lib = _lib.load()
    B, H, W, cin = x.shape
    if y is None:
        y = torch.empty(B, H, W, cout, dtype=torch.float32, device=x.device)
    check(lib.sol_conv5x5_cols(stream(), ptr(x), ptr(packed), ptr(bias), ptr(residual), ptr(act_ref), ptr(y),
                               B, H, W, int(wv), cin, cout, epilogue, float(slope), ptr(x_absmax), ptr(y_absmax)))
    return y


class Conv5x5Fn(torch.autograd.Function):
    """y = act(conv5x5_same(x, w) + b (+ residual)), NHWC, w in Keras HWIO layout."""

    @staticmethod
    def forward(ctx, x, w, b, residual, lrelu, slope):
        _lib.require_gpu()
        cin, cout = w.shape[2], w.shape[3]
        x = _lib.f32(x); w = _lib.f32(w); b = _lib.f32(b)
        cin_k = 4 if cin <= 4 else 32
        assert cin in (1, 2, 3, 4, 32), "conv5x5 supports <=4 or 32 input channels"
        ctx.cin_w = cin
        xk = _pad_channels(x, cin_k)
        packed = _pack(w, cin, cout, CONV_FWD)
        res = None if residual is None else _lib.f32(residual)
        y = conv5x5_raw(xk, packed, b, res, None, cout, EPI_LRELU if lrelu else EPI_NONE, slope)
        ctx.save_for_backward(xk, w, y)
        ctx.meta = (cin, cout, cin_k, lrelu, slope, residual is not None)
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = _lib.load()
        xk, w, y = ctx.saved_tensors
        cin, cout, cin_k, lrelu, slope, has_res = ctx.meta
        B, H, W, _ = xk.shape
        dz = gy.contiguous()
        if lrelu:
            dz = dz * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope))
        # weight / bias gradient
        cout_k = cout if cout in (2, 32) else None
        assert cout_k is not None, "conv5x5 backward-weight supports 2 or 32 output channels"
        nws = lib.sol_conv5x5_bwd_weight_ws_floats(B, H, W, cin_k, cout)
        part = torch.zeros(nws, dtype=torch.float32, device=xk.device)
        check(lib.sol_conv5x5_bwd_weight(stream(), ptr(xk), ptr(dz), ptr(part), B, H, W, cin_k, cout))
        dw = torch.empty_like(w)
        db = torch.empty(cout, dtype=torch.float32, device=xk.device)
        check(lib.sol_conv5x5_bwd_weight_reduce(stream(), ptr(part), ptr(dw), ptr(db), B, H, W, cin, cout, 0))
        # data gradient: run-conv with cin_run = cout (padded to 4/32), cout_run = cin
        dzk = _pad_channels(dz, 4 if cout <= 4 else 32)
        packed = _pack(w, cout, cin, CONV_BWD_DATA)
        dx = conv5x5_raw(dzk, packed, None, None, None, cin, EPI_NONE, slope)
        return dx, dw, db, (dz if has_res else None), None, None


def conv5x5(x, w, b, residual=None, lrelu=False, slope=0.3):
    return Conv5x5Fn.apply(x, w, b, residual, lrelu, slope)


class Conv5x5ScaledFn(Conv5x5Fn):
    """Conv5x5Fn whose forward launch is sol_conv5x5_scaled with the absmax slots handed from layer to layer -- the launch
    schedule2d.NetSchedule2D's forward makes on 64-pixel rows (fp16 three-product kernels on the 32-channel layers), so that an autograd
    composition and the hand-written schedule see the same activations, LeakyReLU masks included.  The backward is Conv5x5Fn's."""

    @staticmethod
    def forward(ctx, x, w, b, residual, lrelu, slope, xmax, ymax):
        _lib.require_gpu()
        cin, cout = w.shape[2], w.shape[3]
        x = _lib.f32(x); w = _lib.f32(w); b = _lib.f32(b)
        cin_k = 4 if cin <= 4 else 32
        assert cin in (1, 2, 3, 4, 32), "conv5x5 supports <=4 or 32 input channels"
        ctx.cin_w = cin
        xk = _pad_channels(x, cin_k)
        packed = _pack(w, cin, cout, CONV_FWD)
        res = None if residual is None else _lib.f32(residual)
        y = conv5x5_scaled_raw(xk, packed, b, res, None, cout, EPI_LRELU if lrelu else EPI_NONE, slope, xmax, ymax)
        ctx.save_for_backward(xk, w, y)
        ctx.meta = (cin, cout, cin_k, lrelu, slope, residual is not None)
        return y

    @staticmethod
    def backward(ctx, gy):
        return Conv5x5Fn.backward(ctx, gy) + (None, None)


def conv5x5_scaled(x, w, b, residual=None, lrelu=False, slope=0.3, xmax=None, ymax=None):
    """conv5x5 through sol_conv5x5_scaled: xmax / ymax are rows of an [n, AMAX_SLOTS] int32 tensor zeroed by the caller (or None)."""
    return Conv5x5ScaledFn.apply(x, w, b, residual, lrelu, slope, xmax, ymax)


def conv_halo(buf, H, W, periodic, mode):
    """sol_conv_halo in place on buf [B, H + 4 py, P, C] (include/sol_hip.h, "CIRCULAR PADDING"): mode "wrap" / "zero".  periodic: the
    pair (py, px) or the bits 2 (y) | 4 (x).  -> buf"""
    bits = periodic if isinstance(periodic, int) else periodic_bits(periodic)
    B, _, P, c = buf.shape
    check(_lib.load().sol_conv_halo(stream(), ptr(buf), B, int(H), int(W), P, c, int(bits), {"wrap": 0, "zero": 1}[mode]))
    return buf


class Conv5x5CircularFn(torch.autograd.Function):
    """y = conv5x5(x, w) + b with CIRCULAR padding along the periodic axes: one linear layer, dense [B,H,W,c] in and out -- the
    cross-check of schedule2d.NetSchedule2D(padding="circular"), kept apart from its buffer handling on purpose.  It builds its own
    halo buffers (include/sol_hip.h, "CIRCULAR PADDING"): forward = wrap -> sol_conv5x5_cols -> crop; backward = zero -> weight gradient
    -> wrap -> backward-data convolution -> crop.  The skip and the activation of a network are torch operations around it."""

    @staticmethod
    def forward(ctx, x, w, b, bits):
        _lib.require_gpu()
        cin, cout = w.shape[2], w.shape[3]
        assert cin in (1, 2, 3, 4, 32), "conv5x5 supports <=4 or 32 input channels"
        x = _lib.f32(x); w = _lib.f32(w); b = _lib.f32(b)
        B, H, W, _ = x.shape
        r0, c0 = 2 * bool(bits & PERIODIC_Y), 2 * bool(bits & PERIODIC_X)
        geo = (B, H, W, r0, c0, 64 * ((W + 2 * c0 + 63) // 64))
        xb = Conv5x5CircularFn._halo_buffer(x, geo, 4 if cin <= 4 else 32)
        conv_halo(xb, H, W, bits, "wrap")
        yb = conv5x5_cols_raw(xb, _pack(w, cin, cout, CONV_FWD), b, None, None, cout, EPI_NONE, 0.0, W + 2 * c0)
        ctx.save_for_backward(xb, w)
        ctx.meta = (cin, cout, bits, geo)
        return yb[:, r0:r0 + H, c0:c0 + W].contiguous()

    @staticmethod
    def _halo_buffer(t, geo, c):
        """zeros [B, H + 2 r0, P, c] with t [B,H,W,<=c] in the valid pixels (a strided copy: a kernel)"""
        B, H, W, r0, c0, P = geo
        buf = torch.zeros(B, H + 2 * r0, P, c, dtype=torch.float32, device=t.device)
        buf[:, r0:r0 + H, c0:c0 + W, :t.shape[-1]].copy_(t)
        return buf

    @staticmethod
    def backward(ctx, gy):
        lib = _lib.load()
        xb, w = ctx.saved_tensors
        cin, cout, bits, geo = ctx.meta
        B, H, W, r0, c0, P = geo
        assert cout in (2, 32), "conv5x5 backward-weight supports 2 or 32 output channels"
        HB, cin_k = H + 2 * r0, xb.shape[-1]
        gb = Conv5x5CircularFn._halo_buffer(gy, geo, 4 if cout <= 4 else 32)
        # weight / bias gradient: x with its wrapped halo, dz zero in the halo -- the valid pixels only (the buffer is fresh, so the
        # launch changes nothing here; it is the schedule's sequence, run as the schedule runs it)
        conv_halo(gb, H, W, bits, "zero")
        dz = gb if gb.shape[-1] == cout else gb[..., :cout].contiguous()
        part = torch.zeros(lib.sol_conv5x5_bwd_weight_ws_floats(B, HB, P, cin_k, cout), dtype=torch.float32, device=xb.device)
        check(lib.sol_conv5x5_bwd_weight(stream(), ptr(xb), ptr(dz), ptr(part), B, HB, P, cin_k, cout))
        dw = torch.empty_like(w)
        db = torch.empty(cout, dtype=torch.float32, device=xb.device)
        check(lib.sol_conv5x5_bwd_weight_reduce(stream(), ptr(part), ptr(dw), ptr(db), B, HB, P, cin, cout, 0))
        # data gradient: the circular correlation = the backward-data convolution of the wrapped dz
        conv_halo(gb, H, W, bits, "wrap")
        dxb = conv5x5_cols_raw(gb, _pack(w, cout, cin, CONV_BWD_DATA), None, None, None, cin, EPI_NONE, 0.0, W + 2 * c0)
        return dxb[:, r0:r0 + H, c0:c0 + W].contiguous(), dw, db, None


def conv5x5_circular(x, w, b, periodic):
    """conv5x5(x, w) + b, NHWC, w in Keras HWIO layout, padded circularly along the axes of periodic = (py, px) and with zeros along the
    others; any H, W >= 1.  Differentiable in x, w and b."""
    bits = periodic_bits(periodic)
    if not bits:
        raise _lib.SolError("conv5x5_circular: periodic=%r names no periodic axis (ops.conv5x5 pads with zeros)" % (tuple(periodic),))
    return Conv5x5CircularFn.apply(x, w, b, bits)


# --------------------------------------------------------------------------------------
# Burgers step
# --------------------------------------------------------------------------------------
def circulant_diffusion_matrix(n, amount):
    """Real symmetric circulant matrix of PhiFlow's periodic diffusion along one axis of
    length n: ifft(fft(.) * exp(-(2 pi k)^2 amount)), k = fftfreq(n)  (dx = 1)."""
    k = np.fft.fftfreq(n)
    col = np.fft.ifft(np.exp(-(2 * np.pi) ** 2 * k ** 2 * amount)).real
    idx = (np.arange(n)[:, None] - np.arange(n)[None, :]) % n
    return col[idx]


BURGERS_LDS_MAX = 64      # largest grid edge of the one-workgroup Burgers kernels


def burgers_large_workspace_bytes(cfg):
    """Bytes of a workspace that serves sol_burgers_step_fwd_large AND sol_burgers_step_bwd_large (they never run at the same time)."""
    lib = _lib.load()
    return max(lib.sol_burgers_step_large_workspace_bytes(C.byref(cfg)), lib.sol_burgers_step_bwd_large_workspace_bytes(C.byref(cfg)))


def _burgers_fwd(vy, vx, fy, fx, cfg, circ, large, workspace):
    """(vy, vx) after the step: sol_burgers_step_fwd, or (large) sol_burgers_step_fwd_large with its workspace"""
    lib = _lib.load()
    oy, ox = torch.empty_like(vy), torch.empty_like(vx)
    head = (C.byref(cfg), stream(), ptr(vy), ptr(vx), ptr(fy), ptr(fx), ptr(circ[0]), ptr(circ[1]), ptr(circ[2]), ptr(circ[3]), ptr(oy), ptr(ox))
    if large:
        workspace = _workspace(lib.sol_burgers_step_large_workspace_bytes(C.byref(cfg)), workspace, vy.device)
        check(lib.sol_burgers_step_fwd_large(*head, ptr(workspace), workspace.numel() * 4))
    else:
        check(lib.sol_burgers_step_fwd(*head))
    return oy, ox


def burgers_step_large_bwd(vy, vx, gy, gx, cfg, circ, workspace=None):
    """Adjoint of the large-grid Burgers step (sol_burgers_step_bwd_large): (g_vy_in, g_vx_in) from the step's input velocity and the
    gradient with respect to its output velocity."""
    lib = _lib.load()
    workspace = _workspace(lib.sol_burgers_step_bwd_large_workspace_bytes(C.byref(cfg)), workspace, vy.device)
    oy, ox = torch.empty_like(vy), torch.empty_like(vx)
    check(lib.sol_burgers_step_bwd_large(C.byref(cfg), stream(), ptr(vy), ptr(vx), ptr(circ[0]), ptr(circ[1]), ptr(circ[2]), ptr(circ[3]),
                                         ptr(gy), ptr(gx), ptr(oy), ptr(ox), ptr(workspace), workspace.numel() * 4))
    return oy, ox


class BurgersStepFn(torch.autograd.Function):
    """The Burgers step with its hand-written adjoint: sol_burgers_step_fwd / sol_burgers_step_bwd on a one-workgroup grid, `large`:
    sol_burgers_step_fwd_large / sol_burgers_step_bwd_large.  d f = dt * g."""

    @staticmethod
    def forward(ctx, vy, vx, fy, fx, cfg, circ, large, workspace):
        oy, ox = _burgers_fwd(vy, vx, fy, fx, cfg, circ, large, workspace)
        ctx.save_for_backward(vy, vx)
        ctx.cfg, ctx.circ, ctx.large, ctx.workspace, ctx.has_f = cfg, circ, large, workspace, fy is not None
        ctx.set_materialize_grads(False)
        return oy, ox

    @staticmethod
    def backward(ctx, gy, gx):
        vy, vx = ctx.saved_tensors
        cfg, circ = ctx.cfg, ctx.circ
        gy = torch.zeros_like(vy) if gy is None else gy.contiguous()         # a missing cotangent counts as zero
        gx = torch.zeros_like(vx) if gx is None else gx.contiguous()
        if ctx.large:
            oy, ox = burgers_step_large_bwd(vy, vx, gy, gx, cfg, circ, ctx.workspace)
        else:
            oy, ox = torch.empty_like(vy), torch.empty_like(vx)
            check(_lib.load().sol_burgers_step_bwd(C.byref(cfg), stream(), ptr(vy), ptr(vx), ptr(circ[0]), ptr(circ[1]), ptr(circ[2]), ptr(circ[3]),
                                                   ptr(gy), ptr(gx), ptr(oy), ptr(ox)))
        return oy, ox, (gy * cfg.dt if ctx.has_f else None), (gx * cfg.dt if ctx.has_f else None), None, None, None, None


def burgers_circ(Y, X, amount, device="cuda"):
    mk = lambda n: torch.as_tensor(circulant_diffusion_matrix(n, amount), dtype=torch.float32, device=device).contiguous()
    return (mk(Y + 1), mk(X), mk(Y), mk(X + 1))


def _burgers_inputs(vy, vx, fy, fx):
    _lib.require_gpu()
    return _lib.f32(vy), _lib.f32(vx), None if fy is None else _lib.f32(fy), None if fx is None else _lib.f32(fx)


def burgers_step(vy, vx, fy, fx, cfg, circ):
    """Burgers step on a one-workgroup grid (edges up to BURGERS_LDS_MAX), differentiable through BurgersStepFn."""
    return BurgersStepFn.apply(*_burgers_inputs(vy, vx, fy, fx), cfg, circ, False, None)


def burgers_step_large(vy, vx, fy, fx, cfg, circ, workspace=None):
    """Burgers step for grids beyond the one-workgroup kernels (the reference's 128 x 128 data generation,
    /root/reference/burgers/Makefile:19-29): sol_burgers_step_fwd_large.  Returns (vy, vx) after the step.  When grad is enabled and an
    input requires a gradient the call goes through BurgersStepFn (same forward launches; the adjoint is
    sol_burgers_step_bwd_large, d f = dt * g); otherwise nothing is kept.  `workspace` (optional, fp32 words) serves both directions when
    it holds burgers_large_workspace_bytes(cfg)."""
    vy, vx, fy, fx = _burgers_inputs(vy, vx, fy, fx)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (vy, vx, fy, fx)):
        return BurgersStepFn.apply(vy, vx, fy, fx, cfg, circ, True, workspace)
    return _burgers_fwd(vy, vx, fy, fx, cfg, circ, True, workspace)


class SplitFlatFn(torch.autograd.Function):
    """1-D tensor -> its consecutive pieces flat[b[k]:b[k+1]] (views) as ONE autograd node whose backward assembles the gradient with
    KERNEL copies (_lib.dcopy_).  Why not plain slicing: the backward of a 1-D slice is zeros(n) + narrow.copy_(g), and a copy into a
    contiguous narrow is a hipMemcpyAsync -- one MEMCPY NODE per parameter tensor and unrolled step in a captured trainer (refused by
    sol_graph_check), next to an n-sized zero fill and an n-sized add each.  Used for the flat parameter buffer of the networks
    (ConvNet.tensors, MarsMoon3D.tensors) and for the 1-D halves model_mercury takes of a bias."""

    @staticmethod
    def forward(ctx, flat, bounds):
        ctx.bounds = tuple(int(b) for b in bounds)
        ctx.n = flat.numel()
        return tuple(flat[ctx.bounds[k]:ctx.bounds[k + 1]] for k in range(len(ctx.bounds) - 1))

    @staticmethod
    def backward(ctx, *gs):
        b = ctx.bounds
        ref = next(g for g in gs if g is not None)
        out = torch.empty(ctx.n, dtype=ref.dtype, device=ref.device)
        if b[0] > 0:
            out[:b[0]].zero_()
        if b[-1] < ctx.n:
            out[b[-1]:].zero_()
        for k, g in enumerate(gs):
            seg = out[b[k]:b[k + 1]]
            if g is None:
                seg.zero_()
            elif g.is_cuda and g.dtype in (torch.float32, torch.int32):
                _lib.dcopy_(seg, g.contiguous().reshape(-1))
            else:
                seg.copy_(g.reshape(-1))
        return out, None


def split_flat(flat, bounds):
    """pieces flat[bounds[k]:bounds[k+1]] of a 1-D tensor; differentiable through SplitFlatFn when `flat` requires grad"""
    if torch.is_grad_enabled() and flat.requires_grad:
        return SplitFlatFn.apply(flat, tuple(int(b) for b in bounds))
    return tuple(flat[int(bounds[k]):int(bounds[k + 1])] for k in range(len(bounds) - 1))


def l2_loss_fwd_bwd(pred, gt, std, gscale=1.0, want_grad=True, loss=None, grads=None):
    """sol_l2_loss_fwd_bwd: the loss of ONE unrolled step, karman_train.py:428-436 -- 0.5 * sum(((gt - pred) / std)^2) over the
    staggered components `pred` / `gt` (tuples of 1..3 device tensors, e.g. (v_y [B,Y+1,X], v_x [B,Y,X+1])), `std` one scale per
    component.  Returns (loss [1] device tensor, tuple of d loss / d pred times gscale, or None).  `loss` / `grads` given: accumulated into."""
    lib = _lib.load()
    nc = len(pred)
    assert 1 <= nc <= 3 and len(gt) == nc and len(std) == nc
    pred = [_lib.f32(t) for t in pred]
    gt = [_lib.f32(t) for t in gt]
    for c in range(nc):     # the kernel reads n[c] = pred[c].numel() elements of BOTH: a mismatch would be an out-of-bounds device read
        if gt[c].shape != pred[c].shape or gt[c].device != pred[c].device:
            raise SolError("l2_loss_fwd_bwd: component %d: gt %s on %s does not match pred %s on %s" % (
                c, tuple(gt[c].shape), gt[c].device, tuple(pred[c].shape), pred[c].device))
        if grads is not None and (grads[c].shape != pred[c].shape or grads[c].device != pred[c].device):
            raise SolError("l2_loss_fwd_bwd: component %d: grads %s does not match pred %s" % (c, tuple(grads[c].shape), tuple(pred[c].shape)))
    acc_g = grads is not None
    g = list(grads) if acc_g else ([torch.empty_like(t) for t in pred] if want_grad else None)
    acc_l = loss is not None
    if loss is None:
        loss = torch.empty(1, dtype=torch.float32, device=pred[0].device)
    scratch = torch.empty(lib.sol_l2_loss_scratch_floats(), dtype=torch.float32, device=pred[0].device)
    arr = lambda ts: (C.c_void_p * nc)(*[ptr(t) for t in ts])
    check(lib.sol_l2_loss_fwd_bwd(stream(), nc, arr(pred), arr(gt), arr(g) if g is not None else None,
                                  (C.c_int64 * nc)(*[t.numel() for t in pred]), (C.c_float * nc)(*[float(v) for v in std]),
                                  float(gscale), int(acc_g), ptr(loss), int(acc_l), ptr(scratch)))
    return loss, (tuple(g) if g is not None else None)


class L2LossFn(torch.autograd.Function):
    """tf.nn.l2_loss((gt - prd) / std) of one unrolled step over 1..3 staggered components (karman_train.py:428-436) as ONE
    autograd node: sol_l2_loss_fwd_bwd computes the value and d loss / d prd in one pass, backward scales the saved gradient.
    Why the trainers that are captured into a hipGraph use THIS and not `(diff * diff).sum()`: a torch reduction over more
    elements than one workgroup handles allocates semaphores and clears them with cudaMemsetAsync -- a MEMSET NODE in the captured
    graph, and memset nodes of a replayed hipGraph are unreliable on ROCm 7.2: after a few replays the
    reduction folded its partial sums early and the reported per-step losses were 0.5x / 2x the true values while state and
    gradient stayed right (found by the full-size SOL-16 test).  This kernel has no memset, no atomics and a fixed summation order."""

    @staticmethod
    def forward(ctx, std, n, *tensors):
        pred, gt = tensors[:n], tensors[n:]
        loss, g = l2_loss_fwd_bwd(pred, gt, std)
        ctx.save_for_backward(*g)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, gl):
        return (None, None) + tuple(gl * g for g in ctx.saved_tensors) + (None,) * len(ctx.saved_tensors)


def l2_loss(pred, gt, std):
    """0.5 * sum_c sum(((gt_c - pred_c) / std_c)^2), differentiable w.r.t. the `pred` tensors (tuples of 1..3 device tensors)."""
    pred = tuple(_lib.f32(t) for t in pred)
    gt = tuple(_lib.f32(t.detach()) for t in gt)
    return L2LossFn.apply(tuple(float(v) for v in std), len(pred), *pred, *gt)
