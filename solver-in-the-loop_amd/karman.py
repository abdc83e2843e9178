"""Reference-shaped Python surface of the karman-2d hot path.

Mirrors /root/reference/karman-2d/karman_train.py:
  to_feature (l.77-86), to_staggered (l.88-90), model_mercury / model_mars_moon (l.92-138),
  lr_schedule (l.146-163), KarmanFlow (l.166-185), velocity BC masks (l.366-373).
`simulator_lo.step(state, re=, res=, velBCy=, velBCyMask=)` keeps its call shape; under it a
single fused HIP kernel per direction (csrc/karman_step.hip) does the work.
"""
import numpy as np
import torch

from . import _lib, ops
from .fluid import (Box, Sphere, Inflow, Obstacle, Gravity, StaggeredGrid, CenteredGrid, box)


def velocity_bc_masks(Y, X, batch_size=None):
    """karman_train.py:366-373 -- returns (velBCy, velBCyMask) as numpy [B?,Y+1,X,1]."""
    shape = (Y + 1, X, 1) if batch_size is None else (batch_size, Y + 1, X, 1)
    vn = np.zeros(shape)
    vn[..., 0:2, 0:X - 1, 0] = 1.0
    vn[..., 0:Y + 1, 0:1, 0] = 1.0
    vn[..., 0:Y + 1, -1:, 0] = 1.0
    return vn, np.copy(vn)


DEFAULT_OBSTACLES = ("sphere:50,50,10",)       # KarmanFlow's Obstacle(Sphere([50, 50], 10)), karman_train.py:169


def _num(v):
    return "%g" % v


def parse_obstacles(spec):
    """Obstacles of a scene from their text form (the scripts' --obstacle): one spec string or a list of them, each
    `sphere:CY,CX,R` (centre and radius) or `box:Y0:Y1,X0:X1` (inclusive bounds), in domain coordinates (the domain is
    box[0:2*len, 0:len], y first); `none` (alone) = no obstacle.  Returns a list of Obstacle(Sphere | Box)."""
    specs = [spec] if isinstance(spec, str) else list(spec)
    if any(str(s).strip().lower() == "none" for s in specs):
        if len(specs) != 1:
            raise ValueError("obstacle spec 'none' cannot be combined with other obstacles (got %r)" % (specs,))
        return []
    out = []
    for s in specs:
        kind, _, args = str(s).strip().partition(":")
        kind = kind.lower()
        try:
            if kind == "sphere":
                vals = [float(v) for v in args.split(",")]
                if len(vals) != 3 or vals[2] <= 0:
                    raise ValueError
                out.append(Obstacle(Sphere(vals[:2], vals[2])))
            elif kind == "box":
                rng = [[float(v) for v in part.split(":")] for part in args.split(",")]
                if len(rng) != 2 or any(len(r) != 2 or r[1] < r[0] for r in rng):
                    raise ValueError
                out.append(Obstacle(Box([rng[0][0], rng[1][0]], [rng[0][1], rng[1][1]])))
            else:
                raise ValueError
        except ValueError:
            raise ValueError("bad obstacle spec %r: expected 'sphere:CY,CX,R' (R > 0), 'box:Y0:Y1,X0:X1' (Y0 <= Y1, X0 <= X1) "
                             "or 'none'" % (s,)) from None
    return out


def obstacle_spec(obstacles):
    """Inverse of parse_obstacles: the canonical spec strings of a list of Obstacle(Sphere | Box)."""
    out = []
    for ob in obstacles:
        g = ob.geometry if isinstance(ob, Obstacle) else ob
        if isinstance(g, Sphere):
            out.append("sphere:%s,%s,%s" % (_num(g.center[0]), _num(g.center[1]), _num(g.radius)))
        elif isinstance(g, Box):
            out.append("box:%s:%s,%s:%s" % (_num(g.lower[0]), _num(g.upper[0]), _num(g.lower[1]), _num(g.upper[1])))
        else:
            raise TypeError("obstacle geometry must be Sphere or Box, got %r" % (g,))
    return out


def _with_boundaries(rec, boundaries):
    """rec plus "boundaries": ("open" | "periodic", "open" | "periodic") -- only when an axis is periodic, so that the record of an open
    scene stays what it has always been (a record without the key reads as open: record_boundaries)"""
    if boundaries is not None and any(ops.boundaries_arg(boundaries, "scene_record: boundaries")):
        rec["boundaries"] = ops.boundaries_name(ops.boundaries_arg(boundaries))
    return rec


def record_boundaries(rec):
    """The (by, bx) words of a scene record; records written before the key existed are open"""
    return tuple(rec.get("boundaries", ("open", "open")))


def scene_record(obstacles=None, active=None, boundaries=None):
    """Picklable description of a scene (what the scripts store in params.pickle / dataStats.pickle): {"obstacles": canonical spec
    strings or None, "active": [Y, X] float32 mask or None}.  Neither given: the default sphere.  boundaries (ops.boundaries_arg) with
    a periodic axis adds "boundaries": (by, bx)."""
    if obstacles is not None and active is not None:
        raise ValueError("give obstacles or an active mask, not both")
    if active is not None:
        return _with_boundaries({"obstacles": None, "active": np.ascontiguousarray(np.asarray(active, dtype=np.float32))}, boundaries)
    if obstacles is None:
        return _with_boundaries({"obstacles": list(DEFAULT_OBSTACLES), "active": None}, boundaries)
    obs = parse_obstacles(obstacles) if isinstance(obstacles, str) or (obstacles and isinstance(obstacles[0], str)) else obstacles
    return _with_boundaries({"obstacles": obstacle_spec(obs), "active": None}, boundaries)


def scenes_equal(a, b):
    if record_boundaries(a) != record_boundaries(b):
        return False
    if (a["active"] is None) != (b["active"] is None):
        return False
    if a["active"] is not None:
        return a["active"].shape == b["active"].shape and bool(np.array_equal(a["active"], b["active"]))
    return list(a["obstacles"]) == list(b["obstacles"])


def describe_scene(rec):
    by, bx = record_boundaries(rec)
    tail = "" if (by, bx) == ("open", "open") else "; boundaries y %s, x %s" % (by, bx)
    if rec["active"] is not None:
        return "mask %dx%d (%d obstacle cells)" % (rec["active"].shape + (int((rec["active"] == 0).sum()),)) + tail
    return (", ".join(rec["obstacles"]) or "none") + tail


class KarmanFlow:
    """KarmanFlow(IncompressibleFlow), karman_train.py:166-185.

    obstacles: list of Obstacle(Sphere | Box) in domain coordinates (the PhiFlow-2 spelling, karman-2d-phi2/karman_train.py:162),
    resolution independent; [] = no obstacle.  active: a [Y, X] mask (1 = fluid) for exactly one grid.  Neither: the reference's
    Obstacle(Sphere([50, 50], 10))."""

    def __init__(self, pressure_solver=None, make_input_divfree=False, make_output_divfree=True,
                 cg_rtol=1e-6, cg_atol=1e-9, cg_max_iter=2000, grad_pad="replicate", inflow_order="after",
                 obstacles=None, active=None, density_grad=False, re_grad=False, buoyancy=None, buoyancy_factor=None,
                 gravity=(-9.81, 0.0), diffusion_substeps=1, advection="semi_lagrangian", correction_strength=1.0, multi_launch=False,
                 boundaries=None):
        # boundaries: "open", "periodic" or a pair (by, bx) (ops.boundaries_arg); None = the boundaries of the Domain the state given to
        # step() lives on (fluid.Domain(..., boundaries=)).  A periodic axis runs the multi-launch path with a direct solve
        # (ops.SceneMasks(boundaries=)); what is not built for periodic scenes raises there or in step(), by name.
        self._boundaries = None if boundaries is None else ops.boundaries_arg(boundaries, "KarmanFlow: boundaries")
        # multi_launch=True (opt-in): the multi-launch path on every grid with Y, X >= 16 (ops.SceneMasks(multi_launch=True)), so that
        # buoyancy, mac_cormack and "direct_scattered" serve the grids the one-workgroup kernels would take; the default picks as before
        self._multi_launch = bool(multi_launch)
        # advection="mac_cormack" (PhiFlow's advect.mac_cormack(field, velocity, dt, correction_strength)): velocity and density are advected
        # by the MacCormack scheme with the revert-to-semi-Lagrangian limiter (include/sol_hip.h, "MACCORMACK ADVECTION"), which keeps what
        # the semi-Lagrangian step smears; large grids only (step() raises SolError on a grid the one-workgroup kernels serve); composes
        # with density_grad, re_grad, buoyancy and diffusion_substeps.  The default issues the launches it always did.
        # diffusion_substeps=n (PhiFlow's diffuse(field, amount, substeps)): the velocity is diffused by n explicit substeps of alpha / n,
        # alpha = dt res^2 / Re, the boundary blend after the last one.  The single stencil is stable only while alpha <= 1/4
        # (ops.min_diffusion_substeps gives the n a run needs); grids with Y, X >= 16.
        # buoyancy=(fy, fx), a force per unit density, or PhiFlow's spelling buoyancy_factor=beta with gravity=(gy, gx): F = -gravity * beta
        # (ops.buoyancy_force).  The step's output density pushes the velocity; large grids only, like mac_cormack.
        # All three compose with each other and with density_grad and re_grad (ops.StepPhysics, built and validated once, here); the
        # defaults issue the launches they always did.
        self._physics = ops.StepPhysics.of(buoyancy, buoyancy_factor, gravity, diffusion_substeps, advection, correction_strength, "KarmanFlow")
        self._buoyancy, self._nsub, self._adv = self._physics
        # re_grad=True (opt-in): a tensor `re` given to step() that requires a gradient receives one (ops.KarmanStepFn's re mode: fit the
        # viscosity to observed frames, a loss term on Re); the default treats re as data
        self._re_grad = bool(re_grad)
        # density_grad=True (opt-in): step() keeps the density in the autograd graph (ops.KarmanStepFn's density mode: a loss on dens frames
        # differentiates with respect to the initial density and velocity); the default treats it as a passive tracer, as the reference's loss does
        self._density_grad = bool(density_grad)
        # the reference's plug point: None = this build's default ("auto": the direct solver where the grid and the
        # scene allow it, else the two-level preconditioned CG), or one of "direct" / "cg"
        # "direct_scattered" (opt-in, large grids only): the direct solve for obstacles beyond one window (precond.scattered_solver_blob)
        if pressure_solver not in (None,) + ops.PRESSURE_SOLVERS:
            raise NotImplementedError("pressure_solver must be None, 'auto', 'direct', 'cg' or 'direct_scattered': the pressure solve is "
                                      "fused into the solver step of libsol_hip.so")
        self._pressure_solver = pressure_solver or "auto"
        if make_input_divfree or not make_output_divfree:
            raise NotImplementedError("only (make_input_divfree=False, make_output_divfree=True) is on the reference path")
        self.infl = Inflow(box[5:10, 25:75])
        if obstacles is not None and active is not None:
            raise ValueError("KarmanFlow: give obstacles or an active mask, not both")
        self.active = None
        if active is not None:
            if isinstance(active, torch.Tensor):
                active = active.detach().cpu().numpy()
            self.active = (np.asarray(active, dtype=np.float64) != 0).astype(np.float64)
            if self.active.ndim != 2:
                raise ValueError("KarmanFlow: active must be a [Y, X] mask, got shape %s" % (self.active.shape,))
            self.obstacles, self.obst = None, None
        elif obstacles is not None:
            self.obstacles = [ob if isinstance(ob, Obstacle) else Obstacle(ob) for ob in obstacles]
            for ob in self.obstacles:
                if not isinstance(ob.geometry, (Sphere, Box)):
                    raise TypeError("KarmanFlow: obstacle geometries must be Sphere or Box, got %r" % (ob.geometry,))
            self.obst = None
        else:
            self.obst = Obstacle(Sphere([50, 50], 10))
            self.obstacles = [self.obst]
        self._solver = dict(cg_rtol=cg_rtol, cg_atol=cg_atol, cg_max_iter=cg_max_iter,
                            grad_pad=grad_pad, inflow_order=inflow_order)
        self._cache = {}
        self.solve_info = {}

    def scene(self, domain=None):
        """scene_record of this flow's obstacles / mask and boundaries (domain: where boundaries=None takes them from; without it open)."""
        b = ops.boundaries_name(self.periodic(domain))
        if self.active is not None:
            return scene_record(active=self.active, boundaries=b)
        return _with_boundaries({"obstacles": obstacle_spec(self.obstacles), "active": None}, b)

    def periodic(self, domain=None):
        """(py, px) this flow runs `domain` with: its own boundaries, else the domain's"""
        if self._boundaries is not None:
            return self._boundaries
        return (False, False) if domain is None else ops.boundaries_arg(getattr(domain, "boundaries", "open"), "Domain: boundaries")

    # -- constant masks of the scene for a given domain ----------------------------------
    def scene_arrays(self, domain):
        yc, xc = domain.cell_centers()
        if self.active is not None:
            if tuple(self.active.shape) != tuple(domain.resolution):
                raise ValueError("KarmanFlow: the active mask is %dx%d, the domain is %dx%d (a mask describes exactly one grid; "
                                 "use obstacles=[...] for a resolution-independent scene)" % (self.active.shape + tuple(domain.resolution)))
            active = self.active.copy()
        elif self.obst is not None:
            active = 1.0 - self.obst.geometry.value_at(yc, xc)
        else:
            solid = np.zeros(yc.shape)
            for ob in self.obstacles:
                solid = np.maximum(solid, ob.geometry.value_at(yc, xc))
            active = 1.0 - solid
        inflow = self.infl.geometry.value_at(yc, xc) * self.infl.rate
        return active, inflow

    @staticmethod
    def _digest(a):
        """content key of a boundary-condition array (shape + bytes): object identity is not one -- ids are recycled after
        garbage collection and a caller may pass a fresh but equal array every step"""
        import hashlib
        if isinstance(a, torch.Tensor):
            a = a.detach().cpu().numpy()
        a = np.ascontiguousarray(a)
        return (a.shape, str(a.dtype), hashlib.sha1(a.view(np.uint8)).hexdigest())

    def _masks(self, domain, velBCy, velBCyMask, device):
        # fast path: the same objects as last time (the training loop passes the same two arrays every step)
        last = getattr(self, "_last_masks", None)
        periodic = self.periodic(domain)
        fast = (domain.resolution, domain.box.lower, domain.box.upper, str(device), periodic)
        if last is not None and last[0] is velBCy and last[1] is velBCyMask and last[2] == fast:
            return last[3]
        key = (domain.resolution, domain.box.lower, domain.box.upper, self._digest(velBCy), self._digest(velBCyMask), str(device), self._multi_launch, periodic)
        if key not in self._cache:
            if len(self._cache) >= 8:                       # bounded: every entry holds device buffers and a solver blob
                self._cache.pop(next(iter(self._cache)))
            active, inflow = self.scene_arrays(domain)
            Y, X = domain.resolution
            bcv = np.asarray(velBCy, dtype=np.float64).reshape(-1, Y + 1, X)
            bcm = np.asarray(velBCyMask, dtype=np.float64).reshape(-1, Y + 1, X)
            if bcv.shape[0] > 1 and np.all(bcv == bcv[0:1]) and np.all(bcm == bcm[0:1]):
                bcv, bcm = bcv[0:1], bcm[0:1]
            self._cache[key] = ops.SceneMasks(active, inflow, bcv, bcm, device, pressure_solver=self._pressure_solver, multi_launch=self._multi_launch,
                                               boundaries=ops.boundaries_name(periodic))
        # (holding the two objects keeps their ids from being recycled while they serve as the fast-path key)
        self._last_masks = (velBCy, velBCyMask, fast, self._cache[key])
        return self._cache[key]

    def step(self, smoke, re, res, velBCy, velBCyMask, dt=1.0, gravity=None):
        """karman_train.py:173-185 (diffuse + BC) -> IncompressibleFlow.step."""
        domain = smoke.domain
        Y, X = domain.resolution
        B = smoke._batch_size
        dev = smoke.density.data.device
        masks = self._masks(domain, velBCy, velBCyMask, dev)
        cfg = ops.karman_cfg(B, Y, X, domain.dx[1], dt=dt, res=res, masks=masks, **self._solver)
        re_t = torch.as_tensor(re, dtype=torch.float32, device=dev).reshape(B)
        d = smoke.density.data.reshape(B, Y, X)
        vy = smoke.velocity.data[0].data.reshape(B, Y + 1, X)
        vx = smoke.velocity.data[1].data.reshape(B, Y, X + 1)
        info = {}
        self.pressure_solver_used = masks.pressure_solver        # "direct", "cg" (SceneMasks' choice for this grid and scene) or "direct_scattered"
        self._physics.require(cfg, masks, "KarmanFlow")
        if masks.large:
            # beyond the one-workgroup kernels (data generation at 256 x 128, karman.py:98-159): the multi-launch path, direct solve
            # where the scene's blob builds, else the preconditioned CG (solve_info: iterations / converged per simulation, and
            # iterations_bwd / converged_bwd after backward()); differentiable like the small path (ops.KarmanStepFn)
            n = ops.large_workspace_bytes(cfg, masks, self._physics)
            if getattr(self, "_large_ws", None) is None or self._large_ws[0] != (B, Y, X, str(dev)) or self._large_ws[1].numel() * 4 < n:
                self._large_ws = ((B, Y, X, str(dev)), torch.empty((n + 3) // 4, dtype=torch.float32, device=dev))
            d2, vy2, vx2 = ops.karman_step_large(d, vy, vx, re_t, cfg, masks, self._large_ws[1], info, density_grad=self._density_grad,
                                                 re_grad=self._re_grad, physics=self._physics)
        else:
            d2, vy2, vx2 = ops.karman_step(d, vy, vx, re_t, cfg, masks, info, density_grad=self._density_grad, re_grad=self._re_grad,
                                           physics=self._physics)
        self.solve_info = info
        return smoke.copied_with(density=d2.reshape(B, Y, X, 1),
                                 velocity=StaggeredGrid([vy2.reshape(B, Y + 1, X, 1), vx2.reshape(B, Y, X + 1, 1)],
                                                        smoke.velocity.box))


def to_feature(smokestate, ext_const_channel):
    """karman_train.py:77-86 -> [B,Y,X,3]."""
    st = smokestate.velocity.staggered_tensor()[:, :-1, :-1, 0:2]
    B = smokestate._batch_size
    re = torch.as_tensor(ext_const_channel, dtype=torch.float32, device=st.device).reshape(B, 1, 1, 1)
    return torch.cat([st, torch.ones_like(smokestate.density.data) * re], dim=-1)


def to_staggered(tensor_cen, box):
    """karman_train.py:88-90."""
    return StaggeredGrid(_lib.pad_high(tensor_cen, 1, 2), box=box)       # F.pad(tensor_cen, (0, 0, 0, 1, 0, 1)) as cat with zeros (_lib.pad_high)


def lr_schedule(epoch, current_lr):
    """karman_train.py:146-163."""
    lr = current_lr
    if epoch == 23: lr *= 0.5
    elif epoch == 21: lr *= 1e-1
    elif epoch == 16: lr *= 1e-1
    elif epoch == 11: lr *= 1e-1
    return lr
