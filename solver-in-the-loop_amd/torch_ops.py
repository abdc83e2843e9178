"""torch.library registration of the C-ABI ops: `torch.ops.sol.*` (north star: "exposed to Python
through PyTorch-ROCm custom ops with a hand-written backward for each solver op").

The ops call the wrappers of ops.py (ctypes over libsol_hip.so, raw device pointers; no torch types cross the C ABI) and carry its
hand-written adjoints (ops.KarmanStepFn, ops.BurgersStepFn, ops.Conv5x5Fn: sol_karman_step_bwd / _bwd_large, sol_burgers_step_bwd /
_bwd_large, sol_conv5x5 backward-data / -weight) under the AutogradCUDA key, so they compose with any other PyTorch op and show up in the
dispatcher (torch.ops.sol.karman_step, .conv5x5, .burgers_step, .adam_tf_step; .karman_step_dens = karman_step with a differentiable
density output, over sol_karman_density_bwd; .karman_step_re = karman_step differentiable with respect to re as well, over the _re
adjoints; .karman_step_buoy = the large-grid step with the buoyancy force (fy, fx): the density pushes the velocity and is always in the
graph; .karman_step_sub = karman_step with nsub explicit diffusion substeps, composing with the density, re and buoyancy modes;
.karman_step_adv = the large-grid step with the advection named per call (1: MacCormack with correction strength s), composing with all of them;
.karman3d_step_buoy = the same for the 3-D step, force (fy, fx, fz); .karman3d_step_sub = the 3-D step with nsub explicit diffusion
substeps, composing with its density, re and buoyancy modes; .karman3d_step_adv = the 3-D step with the advection named per call (1:
MacCormack with correction strength s), composing with all of them).  Scene constants (masks, solver blobs, the cfg struct) are not tensors: they are registered once with register_scene() and
referred to by an integer handle."""
import torch

from . import _lib, ops
from ._lib import check, ptr, stream

_SCENES = {}
_LIB = torch.library.Library("sol", "DEF")
_LIB.define("karman_step(Tensor d, Tensor vy, Tensor vx, Tensor re, int scene) -> (Tensor, Tensor, Tensor)")
_LIB.define("karman_step_dens(Tensor d, Tensor vy, Tensor vx, Tensor re, int scene) -> (Tensor, Tensor, Tensor)")
_LIB.define("karman_step_re(Tensor d, Tensor vy, Tensor vx, Tensor re, int scene, bool density=False) -> (Tensor, Tensor, Tensor)")
_LIB.define("karman_step_buoy(Tensor d, Tensor vy, Tensor vx, Tensor re, int scene, float fy, float fx, bool re_grad=False) -> (Tensor, Tensor, Tensor)")
_LIB.define("karman_step_sub(Tensor d, Tensor vy, Tensor vx, Tensor re, int scene, int nsub, bool density=False, bool re_grad=False, float fy=0.0, float fx=0.0) -> (Tensor, Tensor, Tensor)")
_LIB.define("karman_step_adv(Tensor d, Tensor vy, Tensor vx, Tensor re, int scene, int advection, float s=1.0, int nsub=1, bool density=False, bool re_grad=False, float fy=0.0, float fx=0.0) -> (Tensor, Tensor, Tensor)")
_LIB.define("karman_density_bwd(Tensor d, Tensor svy, Tensor svx, Tensor re, Tensor gd, int scene) -> (Tensor, Tensor, Tensor)")
_LIB.define("karman_step_bwd(Tensor svy, Tensor svx, Tensor re, Tensor gvy, Tensor gvx, int scene) -> (Tensor, Tensor)")
_LIB.define("karman_step_fwd_saved(Tensor d, Tensor vy, Tensor vx, Tensor re, int scene) -> (Tensor, Tensor, Tensor, Tensor, Tensor)")
_LIB.define("conv5x5(Tensor x, Tensor w, Tensor b, Tensor? residual, bool lrelu, float slope) -> Tensor")
_LIB.define("karman3d_step(Tensor d, Tensor vy, Tensor vx, Tensor vz, Tensor re, int scene) -> (Tensor, Tensor, Tensor, Tensor)")
_LIB.define("karman3d_step_dens(Tensor d, Tensor vy, Tensor vx, Tensor vz, Tensor re, int scene) -> (Tensor, Tensor, Tensor, Tensor)")
_LIB.define("karman3d_step_re(Tensor d, Tensor vy, Tensor vx, Tensor vz, Tensor re, int scene, bool density=False) -> (Tensor, Tensor, Tensor, Tensor)")
_LIB.define("karman3d_step_buoy(Tensor d, Tensor vy, Tensor vx, Tensor vz, Tensor re, int scene, float fy, float fx, float fz, bool re_grad=False) -> (Tensor, Tensor, Tensor, Tensor)")
_LIB.define("karman3d_step_sub(Tensor d, Tensor vy, Tensor vx, Tensor vz, Tensor re, int scene, int nsub, bool density=False, bool re_grad=False, float fy=0.0, float fx=0.0, float fz=0.0) -> (Tensor, Tensor, Tensor, Tensor)")
_LIB.define("karman3d_step_adv(Tensor d, Tensor vy, Tensor vx, Tensor vz, Tensor re, int scene, int advection, float s=1.0, int nsub=1, bool density=False, bool re_grad=False, float fy=0.0, float fx=0.0, float fz=0.0) -> (Tensor, Tensor, Tensor, Tensor)")
_LIB.define("karman3d_density_bwd(Tensor d, Tensor svy, Tensor svx, Tensor svz, Tensor re, Tensor gd, int scene) -> (Tensor, Tensor, Tensor, Tensor)")
_LIB.define("conv3d(Tensor x, Tensor w, Tensor b, Tensor? residual, bool lrelu, float slope) -> Tensor")
_LIB.define("burgers_step(Tensor vy, Tensor vx, Tensor? fy, Tensor? fx, float dx, float dt, float nu) -> (Tensor, Tensor)")
_LIB.define("l2_loss(Tensor vy, Tensor vx, Tensor gt_vy, Tensor gt_vx, float std_vy, float std_vx) -> Tensor")
_LIB.define("adam_tf_step(Tensor(a!) params, Tensor grads, Tensor(b!) m, Tensor(c!) v, int t, float lr, float beta1, float beta2, float eps) -> ()")


def register_scene(cfg, masks):
    """-> handle of (sol_karman_cfg, SceneMasks) for torch.ops.sol.karman_step."""
    h = len(_SCENES) + 1
    _SCENES[h] = (cfg, masks)
    return h


def _karman_fwd_saved(d, vy, vx, re, scene):
    cfg, masks = _SCENES[scene]
    outs, svy, svx = ops.karman_step_saved(d, vy, vx, re, cfg, masks)
    return (*outs, svy, svx)


def _karman_bwd(svy, svx, re, gvy, gvx, scene):
    cfg, masks = _SCENES[scene]
    return ops._step_adjoint("torch.ops.sol.karman_step_bwd", None, svy, svx, re, None, gvy, gvx, cfg, masks, ops.StepPhysics(), False, fused=True)[1:3]


def _karman_density_bwd(d, svy, svx, re, gd, scene):
    cfg, masks = _SCENES[scene]
    return ops.karman_density_bwd(d, svy, svx, re, gd, cfg, masks)


_LIB.impl("karman_step_fwd_saved", _karman_fwd_saved, "CUDA")
_LIB.impl("karman_step_bwd", _karman_bwd, "CUDA")
_LIB.impl("karman_density_bwd", _karman_density_bwd, "CUDA")


# Every differentiable step op is one mode of ops.KarmanStepFn, the hand-written forward + backward pair, under one ops.StepPhysics:
#   karman_step        the density is a passive tracer, re is data
#   karman_step_dens   opt-in: the density output is differentiable too
#   karman_step_re     opt-in: differentiable with respect to re as well (grids with Y, X >= 16); density: d_out stays in the graph
#   karman_step_buoy   the buoyant step (large grids; a force of (0, 0) is the plain step, density in the graph)
#   karman_step_sub    nsub explicit diffusion substeps (grids with Y, X >= 16), composing with density, re_grad and a force (fy, fx)
#   karman_step_adv    the advection named per call (0 semi-Lagrangian, 1 MacCormack with correction strength s; large grids),
#                      composing with all of them
def _physics(scene, who, nsub=1, fy=0.0, fx=0.0, advection=0, s=1.0, keep_zero_force=False):
    """(cfg, masks, StepPhysics) of an op's arguments, validated and checked against the scene's grid"""
    cfg, masks = _SCENES[scene]
    if advection not in (0, 1):
        raise ValueError("%s: advection must be 0 (semi_lagrangian) or 1 (mac_cormack), got %r" % (who, advection))
    ph = ops.StepPhysics.of(buoyancy=(fy, fx), diffusion_substeps=nsub, advection=ops.ADVECTIONS[advection], correction_strength=s, who=who,
                            keep_zero_force=keep_zero_force)
    ph.require(cfg, masks, who)
    return cfg, masks, ph.moving()


def _step(d, vy, vx, re, cfg, masks, ph):
    """no gradient wanted: the plain forward entry points, nothing kept"""
    with torch.no_grad():
        return (ops.karman_step_large if masks.large else ops.karman_step)(d, vy, vx, re, cfg, masks, physics=ph)


def _step_fn(d, vy, vx, re, cfg, masks, density, want_re, ph):
    if want_re:
        ops._require_staged(cfg, "re_grad")
    return ops.KarmanStepFn.apply(d, vy, vx, re, cfg, masks, None, None, density, want_re, ph)


def _want_re(re_grad, re):
    return bool(re_grad) and torch.is_grad_enabled() and re.requires_grad


def _karman_step(d, vy, vx, re, scene, density=False):
    return _step(d, vy, vx, re, *_SCENES[scene], ops.StepPhysics())


def _karman_fn(d, vy, vx, re, scene, density, want_re):
    return _step_fn(d, vy, vx, re, *_SCENES[scene], density, want_re, ops.StepPhysics())


for _op in ("karman_step", "karman_step_dens", "karman_step_re"):
    _LIB.impl(_op, _karman_step, "CUDA")
_LIB.impl("karman_step", lambda d, vy, vx, re, scene: _karman_fn(d, vy, vx, re, scene, False, False), "AutogradCUDA")
_LIB.impl("karman_step_dens", lambda d, vy, vx, re, scene: _karman_fn(d, vy, vx, re, scene, True, False), "AutogradCUDA")
_LIB.impl("karman_step_re", lambda d, vy, vx, re, scene, density=False: _karman_fn(d, vy, vx, re, scene, bool(density), True), "AutogradCUDA")


def _karman_buoy(d, vy, vx, re, scene, fy, fx, re_grad=False):
    cfg, masks = _SCENES[scene]
    with torch.no_grad():            # (a force of (0, 0) is kept: the buoyant entry point takes it)
        return ops.karman_step_large(d, vy, vx, re, cfg, masks, buoyancy=(float(fy), float(fx)))


def _karman_buoy_fn(d, vy, vx, re, scene, fy, fx, re_grad=False):
    cfg, masks, ph = _physics(scene, "torch.ops.sol.karman_step_buoy", 1, fy, fx, keep_zero_force=True)      # (a small grid is refused whatever the force)
    return _step_fn(d, vy, vx, re, cfg, masks, True, _want_re(re_grad, re), ph)


def _karman_sub(d, vy, vx, re, scene, nsub, density=False, re_grad=False, fy=0.0, fx=0.0):
    return _step(d, vy, vx, re, *_physics(scene, "torch.ops.sol.karman_step_sub", nsub, fy, fx))


def _karman_sub_fn(d, vy, vx, re, scene, nsub, density=False, re_grad=False, fy=0.0, fx=0.0):
    cfg, masks, ph = _physics(scene, "torch.ops.sol.karman_step_sub", nsub, fy, fx)
    return _step_fn(d, vy, vx, re, cfg, masks, bool(density), _want_re(re_grad, re), ph)


def _karman_adv(d, vy, vx, re, scene, advection, s=1.0, nsub=1, density=False, re_grad=False, fy=0.0, fx=0.0):
    return _step(d, vy, vx, re, *_physics(scene, "torch.ops.sol.karman_step_adv", nsub, fy, fx, advection, s))


def _karman_adv_fn(d, vy, vx, re, scene, advection, s=1.0, nsub=1, density=False, re_grad=False, fy=0.0, fx=0.0):
    cfg, masks, ph = _physics(scene, "torch.ops.sol.karman_step_adv", nsub, fy, fx, advection, s)
    return _step_fn(d, vy, vx, re, cfg, masks, bool(density), _want_re(re_grad, re), ph)


_LIB.impl("karman_step_buoy", _karman_buoy, "CUDA")
_LIB.impl("karman_step_buoy", _karman_buoy_fn, "AutogradCUDA")
_LIB.impl("karman_step_sub", _karman_sub, "CUDA")
_LIB.impl("karman_step_sub", _karman_sub_fn, "AutogradCUDA")
_LIB.impl("karman_step_adv", _karman_adv, "CUDA")
_LIB.impl("karman_step_adv", _karman_adv_fn, "AutogradCUDA")

# conv / burgers: the autograd.Functions of ops.py already are the hand-written forward + backward pairs
_LIB.impl("conv5x5", lambda x, w, b, residual, lrelu, slope: ops.Conv5x5Fn.apply(x, w, b, residual, lrelu, slope), "AutogradCUDA")


def _burgers(vy, vx, fy, fx, dx, dt, nu):
    B, Yp1, X = vy.shape
    cfg = _lib.BurgersCfg(B, Yp1 - 1, X, float(dx), float(dt))
    circ = ops.burgers_circ(Yp1 - 1, X, dt * nu, vy.device)
    if max(Yp1 - 1, X) > ops.BURGERS_LDS_MAX:       # beyond the one-workgroup kernels: the multi-launch step and its adjoint
        return ops.burgers_step_large(vy, vx, fy, fx, cfg, circ)
    return ops.burgers_step(vy, vx, fy, fx, cfg, circ)


_LIB.impl("burgers_step", _burgers, "AutogradCUDA")


def _adam(params, grads, m, v, t, lr, beta1, beta2, eps):
    check(_lib.load().sol_adam_tf_step(stream(), ptr(params), ptr(grads.contiguous()), ptr(m), ptr(v), params.numel(), int(t), float(lr),
                                       float(beta1), float(beta2), float(eps), 0.0, None, 0, None))


_LIB.impl("adam_tf_step", _adam, "CUDA")


_LIB.impl("l2_loss", lambda vy, vx, gt_vy, gt_vx, sy, sx: ops.l2_loss((vy, vx), (gt_vy, gt_vx), (sy, sx)), "AutogradCUDA")


# ---- karman-3d (BASELINE configs[4]): the step with its hand-written adjoint and Conv3D(5) with forward / backward-data / weight gradient ----
_SIMS3D = {}


def register_scene3d(sim):
    """-> handle of a karman3d.Karman3DFlow (scene + direct-solver blob + workspace) for torch.ops.sol.karman3d_step."""
    h = len(_SIMS3D) + 1
    _SIMS3D[h] = sim
    return h


# Every differentiable 3-D step op is one mode of karman3d._Karman3DStepFn under one karman3d.StepPhysics3D, as for the 2-D step (all but
# karman3d_step_sub run the registered simulator's own diffusion_substeps; the first three take no force):
#   karman3d_step        the density is a passive tracer, re is data
#   karman3d_step_dens   opt-in: the density output is differentiable too
#   karman3d_step_re    opt-in: differentiable with respect to re as well; density: d_out stays in the graph
#   karman3d_step_buoy   the buoyant step, force (fy, fx, fz), density in the graph; (0, 0, 0) is the plain step (without a gradient the
#                        force is kept as given: the _buoy entry point issues the plain launches)
#   karman3d_step_sub    nsub explicit diffusion substeps named per call, composing with density, re_grad and a force (fy, fx, fz)
#   karman3d_step_adv    the advection named per call (0 semi-Lagrangian: karman3d_step_sub's launches and bits; 1 MacCormack with
#                        correction strength s), composing with all of them
# The ops that name no advection run the registered simulator's own (Karman3DFlow.adv).
_OWN = object()


def _adv3d(op, advection, s):
    """ops.advection_arg of an op's (advection, s): None for 0, the float s for 1"""
    if advection not in (0, 1):
        raise ValueError("torch.ops.sol.%s: advection must be 0 (semi_lagrangian) or 1 (mac_cormack), got %r" % (op, advection))
    return ops.advection_arg(ops.ADVECTIONS[advection], s, "torch.ops.sol.%s: advection" % op)


def _physics3d(scene, op, nsub=None, force=None, keep_zero_force=False):
    """the StepPhysics3D of an op's arguments, validated; nsub=None: the registered simulator's own count"""
    from . import karman3d as k3
    return k3.StepPhysics3D.of(force, diffusion_substeps=_SIMS3D[scene].nsub if nsub is None else nsub, who="torch.ops.sol.%s: nsub" % op,
                               keep_zero_force=keep_zero_force)


def _karman3d_apply(scene, tensors, density, re_grad, ph, adv=_OWN):
    from . import karman3d as k3
    d, vy, vx, vz, re = (_lib.f32(t) for t in tensors)
    sim = _SIMS3D[scene]
    return k3._Karman3DStepFn.apply(sim, d, vy, vx, vz, re, bool(density), _want_re(re_grad, re), ph.moving(), sim.adv if adv is _OWN else adv)


def _karman3d_nograd(scene, tensors, ph, adv=_OWN):
    """no gradient wanted: the forward launches, nothing kept"""
    sim = _SIMS3D[scene]
    with torch.no_grad():
        return sim._forward(ph, *(_lib.f32(t) for t in tensors), adv=sim.adv if adv is _OWN else adv)[0]


def _karman3d_density_bwd(d, svy, svx, svz, re, gd, scene):
    from . import karman3d as k3
    return k3.density_bwd(_SIMS3D[scene], d, (svy, svx, svz), re, gd)


def _conv3d(x, w, b, residual, lrelu, slope):
    from . import karman3d as k3
    return k3._Conv3DFn.apply(x, w, b, residual, lrelu, slope, None)


_LIB.impl("karman3d_step", lambda d, vy, vx, vz, re, scene: _karman3d_apply(scene, (d, vy, vx, vz, re), False, False, _physics3d(scene, "karman3d_step")),
          "AutogradCUDA")
_LIB.impl("karman3d_step_dens", lambda d, vy, vx, vz, re, scene: _karman3d_apply(scene, (d, vy, vx, vz, re), True, False, _physics3d(scene, "karman3d_step_dens")),
          "AutogradCUDA")
_LIB.impl("karman3d_step_re", lambda d, vy, vx, vz, re, scene, density=False:
          _karman3d_apply(scene, (d, vy, vx, vz, re), density, True, _physics3d(scene, "karman3d_step_re")), "AutogradCUDA")
_LIB.impl("karman3d_step_buoy", lambda d, vy, vx, vz, re, scene, fy, fx, fz, re_grad=False:
          _karman3d_nograd(scene, (d, vy, vx, vz, re), _physics3d(scene, "karman3d_step_buoy", None, (fy, fx, fz), keep_zero_force=True)), "CUDA")
_LIB.impl("karman3d_step_buoy", lambda d, vy, vx, vz, re, scene, fy, fx, fz, re_grad=False:
          _karman3d_apply(scene, (d, vy, vx, vz, re), True, re_grad, _physics3d(scene, "karman3d_step_buoy", None, (fy, fx, fz))), "AutogradCUDA")
_LIB.impl("karman3d_step_sub", lambda d, vy, vx, vz, re, scene, nsub, density=False, re_grad=False, fy=0.0, fx=0.0, fz=0.0:
          _karman3d_nograd(scene, (d, vy, vx, vz, re), _physics3d(scene, "karman3d_step_sub", nsub, (fy, fx, fz))), "CUDA")
_LIB.impl("karman3d_step_sub", lambda d, vy, vx, vz, re, scene, nsub, density=False, re_grad=False, fy=0.0, fx=0.0, fz=0.0:
          _karman3d_apply(scene, (d, vy, vx, vz, re), density, re_grad, _physics3d(scene, "karman3d_step_sub", nsub, (fy, fx, fz))), "AutogradCUDA")
_LIB.impl("karman3d_step_adv", lambda d, vy, vx, vz, re, scene, advection, s=1.0, nsub=1, density=False, re_grad=False, fy=0.0, fx=0.0, fz=0.0:
          _karman3d_nograd(scene, (d, vy, vx, vz, re), _physics3d(scene, "karman3d_step_adv", nsub, (fy, fx, fz)), _adv3d("karman3d_step_adv", advection, s)), "CUDA")
_LIB.impl("karman3d_step_adv", lambda d, vy, vx, vz, re, scene, advection, s=1.0, nsub=1, density=False, re_grad=False, fy=0.0, fx=0.0, fz=0.0:
          _karman3d_apply(scene, (d, vy, vx, vz, re), density, re_grad, _physics3d(scene, "karman3d_step_adv", nsub, (fy, fx, fz)),
                          _adv3d("karman3d_step_adv", advection, s)), "AutogradCUDA")
_LIB.impl("karman3d_density_bwd", _karman3d_density_bwd, "CUDA")
_LIB.impl("conv3d", _conv3d, "AutogradCUDA")
