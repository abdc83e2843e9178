"""Fused solver-in-the-loop training step (one C call = the reference's one sess.run).

Replaces the graph built at /root/reference/karman-2d/karman_train.py:397-457 and executed
at :502: msteps x [simulator_lo.step -> CNN correction -> add], the l2 loss against the
ground-truth frames, the reverse sweep and TF-Adam.  Python only owns the device buffers;
the whole unroll is driven from C++ (sol_train_fwd_bwd) so that no per-op Python overhead
sits between the ~1000 kernel launches of a SOL-32 step.

Data parallel (new capability): one process per GPU, each rank runs the
full unroll on its shard of simulations, then ONE all-reduce(SUM) of the flat 260,354-float
gradient over RCCL (the loss is a batch SUM, karman_train.py:430, so summed shard gradients
equal the large-batch gradient) and an identical Adam update on every rank.
"""
import ctypes as C
import types

import torch

from . import _lib, ops
from ._lib import TrainCfg, check, ptr, stream
from .dist import DPStep


_CONV_PRECISION = {"split": 0, "bf16x6": 1, "fp32": 2}


def _conv_precision_code(name):
    if name is None:
        return None
    if name not in _CONV_PRECISION:
        raise ValueError("conv_precision must be one of %s or None (got %r)" % (sorted(_CONV_PRECISION), name))
    return _CONV_PRECISION[name]


def _apply_conv_precision(code):
    if code is not None:
        _lib.set_option("conv_precision", code)


class _conv_precision_scope:
    """The library's `conv_precision` option is process wide; a trainer / roll-out sets ITS value for the duration of a call
    and puts the previous one back, so objects of different precision can alternate and nothing leaks into later calls of
    the per-op API (None: leave the option alone)."""

    def __init__(self, code):
        self.code = code

    def __enter__(self):
        if self.code is not None:
            self.prev = _lib.get_option("conv_precision")
            _lib.set_option("conv_precision", self.code)

    def __exit__(self, *exc):
        if self.code is not None:
            _lib.set_option("conv_precision", self.prev)
        return False


def _refuse_large_grid(who, Y, X):
    """SolTrainer and GraphTrainer stop at the one-workgroup solver grids (ops.beyond_one_workgroup): their solver launches
    (sol_karman_step_fwd / _bwd, the fused adjoint) are built for those.  Beyond them LargeGridTrainer runs the same schedule over the
    large-grid solver pair.  Refused here, at construction, instead of in the middle of the first reverse sweep."""
    if ops.beyond_one_workgroup(Y, X):
        raise ValueError("%s: a %dx%d domain is beyond the trainers -- the 5x5 weight gradient (sol_conv5x5_bwd_weight) is built for "
                         "W <= 64 in the schedules of this class and the fused solver adjoint for at most 8192 cells; train on such a "
                         "domain with LargeGridTrainer (X a multiple of 64), differentiate single large-grid steps with "
                         "KarmanFlow.step / ops.karman_step_large" % (who, Y, X))


def _check_multi_launch(who, multi_launch, masks, Y, X):
    """multi_launch=True asks for the multi-launch solver pair on a grid the one-workgroup kernels would serve: Y, X >= 16, and masks
    (where the caller gives them) built with the same flag -- the two disagreeing is refused here, at construction.  -> bool"""
    multi_launch = bool(multi_launch)
    if multi_launch and (Y < 16 or X < 16):
        raise ValueError("%s: multi_launch=True takes grids with Y, X >= 16 (the multi-launch kernels); this one is %dx%d" % (who, Y, X))
    if masks is not None and bool(getattr(masks, "multi_launch", False)) != multi_launch:
        raise ValueError("%s: multi_launch=%r, but the masks were built with SceneMasks(multi_launch=%r); build both with the same flag"
                         % (who, multi_launch, bool(getattr(masks, "multi_launch", False))))
    return multi_launch


def _width_served(Y, X, any_width, multi_launch):
    """Whether the network's launches take rows of X cells: any width under any_width (pitched rows); a multiple of 64 on a large domain;
    under multi_launch also every width the convolutions take as it is (schedule2d.row_pitch(Y, X) == X: 16, 32, 64 ...)"""
    from .schedule2d import row_pitch
    return bool(any_width) or X % 64 == 0 or (multi_launch and row_pitch(Y, X) == X)


def _refuse_buoyancy(who, buoyancy):
    """SolTrainer and GraphTrainer run the fused one-workgroup solver kernels, which have no buoyancy term: a non-zero force is refused
    at construction (LargeGridTrainer(buoyancy=...) trains with it on a large grid).  -> None"""
    if ops.StepPhysics.of(buoyancy=buoyancy, who=who).buoyancy is not None:
        raise ValueError("%s: buoyancy=%r -- the buoyancy force is built on the multi-launch (large-grid) solver step only; this trainer "
                         "runs the fused one-workgroup kernels.  Train with it on a large grid (LargeGridTrainer)" % (who, buoyancy))
    return None


def _refuse_advection(who, advection, correction_strength=1.0):
    """SolTrainer, GraphTrainer and SolRollout run the fused one-workgroup solver kernels, which advect semi-Lagrangian: "mac_cormack" is
    refused at construction (LargeGridTrainer / LargeGridRollout take it on a large grid).  -> None"""
    if ops.StepPhysics.of(advection=advection, correction_strength=correction_strength, who=who).adv is not None:
        raise ValueError("%s: advection=%r -- the mac_cormack advection is built on the multi-launch (large-grid) solver step only; this "
                         "class runs the fused one-workgroup kernels.  Use it on a large grid (LargeGridTrainer / LargeGridRollout)"
                         % (who, advection))
    return None


def _refuse_substeps(who, diffusion_substeps, Y, X):
    """SolTrainer, GraphTrainer and SolRollout run a solver step that lives inside the library's own schedule (the fused one-workgroup
    kernels, the C-side graph): there is no place for the pre-diffusion launch.  diffusion_substeps > 1 is refused at construction
    (LargeGridTrainer / LargeGridRollout take it on a large grid; KarmanFlow.step on every grid with Y, X >= 16).  -> 1"""
    if ops.StepPhysics.of(diffusion_substeps=diffusion_substeps, who=who).nsub > 1:
        raise ValueError("%s: diffusion_substeps=%d -- diffusion substeps are built on the multi-launch (large-grid) trainers and roll-out "
                         "only; on a %dx%d grid this class runs the fused one-workgroup solver step inside the library's own schedule.  "
                         "Use LargeGridTrainer / LargeGridRollout on a large grid, or KarmanFlow(diffusion_substeps=...).step"
                         % (who, diffusion_substeps, Y, X))
    return 1


def _refuse_periodic(who, masks, use):
    """SolTrainer, GraphTrainer and SolRollout run the fused one-workgroup solver kernels, which are open on all sides: masks built with
    periodic boundaries are refused at construction.  use: the class that serves them."""
    if getattr(masks, "periodic_bits", 0):
        raise ValueError("%s: the masks were built with periodic boundaries %r -- periodic scenes run the multi-launch solver pair only; this "
                         "class runs the fused one-workgroup kernels.  Use %s (multi_launch=True on a grid the one-workgroup kernels would "
                         "serve)" % (who, ops.boundaries_name(masks.periodic), use))


CONV_PADDINGS = ("zeros", "circular")


def _conv_padding_arg(who, conv_padding, periodic=None, use=None):
    """conv_padding: "zeros" (the reference's padding='same': the default) or "circular" (the network's convolutions wrap along the
    periodic axes of the scene: NetSchedule2D(padding="circular")).  periodic: the (py, px) of the masks for a class that serves
    "circular", None for one that does not (`use` names the class that does).  Refused at construction, by name.  -> the word"""
    if conv_padding not in CONV_PADDINGS:
        raise ValueError("%s: conv_padding must be 'zeros' or 'circular' (got %r)" % (who, conv_padding))
    if conv_padding == "circular":
        if periodic is None:
            raise ValueError("%s: conv_padding='circular' pads the network's convolutions circularly along the periodic axes of a scene; this "
                             "class runs the fused one-workgroup kernels, which are open on all sides.  Use %s on masks built with periodic "
                             "boundaries" % (who, use))
        if not any(periodic):
            raise ValueError("%s: conv_padding='circular' needs a periodic axis, but the masks were built with open boundaries; build them "
                             "with boundaries='periodic' or a pair (by, bx), or keep conv_padding='zeros'" % who)
    return conv_padding


def _train_cfg(kc, msteps, net, std_v, std_re, in_std_v, out_std_v):
    """TrainCfg with its normalisation fields.  --pretf (karman_train.py:351-355,416-421): separate input / output normalisation of a
    pre-trained supervised model; 0.0 pairs stand for "as std_v"."""
    i0, i1 = (float(in_std_v[0]), float(in_std_v[1])) if in_std_v is not None else (0.0, 0.0)
    o0, o1 = (float(out_std_v[0]), float(out_std_v[1])) if out_std_v is not None else (0.0, 0.0)
    return TrainCfg(kc, msteps, float(std_v[0]), float(std_v[1]), float(std_re), float(net.slope), i0, i1, o0, o1)


class _AdamDP:
    """The optimiser / data-parallel surface of the 2-D trainers: the flat gradient with its loss slot, TF-Adam state, the per-step
    losses and the DPStep that composes fwd_bwd (the subclass's) with ONE all-reduce and apply_gradients.  A constructor calls
    _init_adam where it allocated these buffers before, then allocates its own outputs, then calls _init_dp."""

    def _init_adam(self, net, msteps, clip_grad, beta1, beta2, eps):
        dev = net.params.device
        n = net.n_params
        # gradient + one slot for the loss: the data-parallel exchange is ONE all-reduce of this buffer (dist.DPStep)
        self._flat = torch.zeros(n + 1, dtype=torch.float32, device=dev)
        self.grads = self._flat[:n]
        self.m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.v = torch.zeros(n, dtype=torch.float32, device=dev)
        self.loss_steps = torch.zeros(msteps, dtype=torch.float32, device=dev)
        self.t = 0
        self.clip_norm = 1e-3 if clip_grad else 0.0      # karman_train.py:453
        self.beta1, self.beta2, self.eps = beta1, beta2, eps
        self._offsets = (C.c_int64 * len(net.offsets))(*[int(o) for o in net.offsets])
        self.final = None
        self._want_final, self._eager = False, False

    def _init_dp(self, group, comm):
        self.scratch = torch.zeros(64, dtype=torch.float32, device=self._flat.device)
        self._dp = DPStep(self._fwd_bwd_flat, self._apply_flat, group=group, comm=comm, flat=self._flat)

    def apply_gradients(self, lr):
        """tf.compat.v1.train.AdamOptimizer(lr) update (+ optional per-tensor clip_by_norm)."""
        self.t += 1
        n = self.net.n_params
        check(self.lib.sol_adam_tf_step(stream(), ptr(self.net.params.detach()), ptr(self.grads), ptr(self.m), ptr(self.v),
                                        n, self.t, float(lr), self.beta1, self.beta2, self.eps, float(self.clip_norm),
                                        self._offsets, len(self.net.shapes), ptr(self.scratch)))

    # ---- data-parallel composition --------------------------------------------------------
    def _fwd_bwd_flat(self, *batch):
        loss = self.fwd_bwd(*batch, want_final=self._want_final, eager=self._eager)
        return loss, self.grads

    def _apply_flat(self, grads, lr):
        assert grads is self.grads
        self.apply_gradients(lr)

    def train_step(self, d0, vy0, vx0, re, gt_vy, gt_vx, lr, want_final=False, eager=False):
        """One training step on this rank's shard; returns the GLOBAL loss tensor.  want_final=True also produces
        the state after the last unrolled step in self.final = [density, vy, vx] (this is what makes the engine
        advect the passive density at all: like the TF graph of the reference, nothing that no output needs is run)."""
        self._want_final = want_final
        self._eager = eager
        return self._dp(d0, vy0, vx0, re, gt_vy, gt_vx, lr=lr)


class SolTrainer(_AdamDP):
    def __init__(self, net, masks, B, Y, X, msteps, dx, std_v, std_re, dt=1.0, res=None,
                 clip_grad=False, beta1=0.9, beta2=0.999, eps=1e-8, group=None, use_graph=True,
                 cg_rtol=1e-6, cg_atol=1e-9, cg_max_iter=2000, grad_pad="replicate", inflow_order="after",
                 conv_precision="split", comm=None, in_std_v=None, out_std_v=None, buoyancy=None, diffusion_substeps=1,
                 advection="semi_lagrangian", correction_strength=1.0, conv_padding="zeros"):
        """conv_precision: arithmetic of the 32-channel convolutions (library option `conv_precision`):
        "split" (default) fp32-equivalent fp16x3 / bf16x6 operand splits on the 16-bit matrix pipe, "bf16x6",
        or "fp32" = strict fp32 MFMA.  The option is process wide in the library; every call of this trainer sets
        it for the duration of the call (and restores the previous value), so trainers of different precision can alternate in
        one process.  None keeps whatever the option table holds
        (e.g. a SOL_CONV_NO_SB / SOL_CONV_NO_FP16 debugging override applied when the library was loaded)."""
        _refuse_large_grid("SolTrainer", Y, X)
        _refuse_buoyancy("SolTrainer", buoyancy)
        _refuse_substeps("SolTrainer", diffusion_substeps, Y, X)
        _refuse_advection("SolTrainer", advection, correction_strength)
        _refuse_periodic("SolTrainer", masks, "LargeGridTrainer")
        _conv_padding_arg("SolTrainer", conv_padding, use="LargeGridTrainer")
        _lib.require_gpu()
        self.lib = _lib.load()
        self.conv_precision = _conv_precision_code(conv_precision)
        assert net.name == "mars_moon", "the fused trainer implements model_mars_moon (the reference default)"
        self.net, self.masks = net, masks
        self.B, self.Y, self.X, self.msteps = B, Y, X, msteps
        kc = ops.karman_cfg(B, Y, X, dx, dt=dt, res=res, cg_rtol=cg_rtol, cg_atol=cg_atol,
                            cg_max_iter=cg_max_iter, grad_pad=grad_pad, inflow_order=inflow_order, masks=masks)
        self.cfg = _train_cfg(kc, msteps, net, std_v, std_re, in_std_v, out_std_v)
        dev = net.params.device
        self.device = dev
        nbytes = self.lib.sol_train_workspace_bytes(C.byref(self.cfg))
        self.workspace = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
        self.workspace_bytes = nbytes
        self._init_adam(net, msteps, clip_grad, beta1, beta2, eps)
        self.iters_fwd = torch.zeros(msteps * B, dtype=torch.int32, device=dev)
        self.iters_bwd = torch.zeros(msteps * B, dtype=torch.int32, device=dev)
        self.use_graph = use_graph
        self._graphs = {}           # want_final -> (key, handle): replayable hipGraphs of the whole fwd+bwd
        self._captures = 0          # re-captures caused by MOVED input buffers so far
        self._stage = None          # internal input buffers, used once the caller's buffers turn out not to be persistent
        self._fin = None
        self._init_dp(group, comm)

    def __del__(self):
        try:
            for _, h in self._graphs.values():
                self.lib.sol_train_graph_destroy(h)
        except Exception:
            pass

    # ---- the two halves of a step -------------------------------------------------------
    def fwd_bwd(self, d0, vy0, vx0, re, gt_vy, gt_vx, want_final=False, eager=False):
        """Inputs: d0 [B,Y,X], vy0 [B,Y+1,X], vx0 [B,Y,X+1], re [B], gt_vy [msteps,B,Y+1,X],
        gt_vx [msteps,B,Y,X+1] (fp32 CUDA, contiguous).  Fills self.grads / self.loss_steps and
        returns the scalar loss tensor (sum of per-step l2 losses / msteps, karman_train.py:436).
        The hipGraph bakes the input pointers in: pass PERSISTENT buffers (copy new data into them) for zero-copy
        replays.  Buffers that move are detected; after the third re-capture the trainer copies the inputs into
        internal staging buffers instead (one D2D copy of the batch per step, ~20 MB at C3) and keeps one graph.
        eager=True launches the kernels one by one (profiling, debugging) whatever use_graph says."""
        B, Y, X, ms = self.B, self.Y, self.X, self.msteps
        assert vy0.shape == (B, Y + 1, X) and vx0.shape == (B, Y, X + 1) and d0.shape == (B, Y, X)
        assert gt_vy.shape == (ms, B, Y + 1, X) and gt_vx.shape == (ms, B, Y, X + 1) and re.shape == (B,)
        with _conv_precision_scope(self.conv_precision):
            return self._fwd_bwd(d0, vy0, vx0, re, gt_vy, gt_vx, want_final, eager)

    def _fwd_bwd(self, d0, vy0, vx0, re, gt_vy, gt_vx, want_final, eager):
        B, Y, X, ms = self.B, self.Y, self.X, self.msteps
        if self._stage is not None and not eager:
            for dst, src in zip(self._stage, (d0, vy0, vx0, re, gt_vy, gt_vx)):
                dst.copy_(src)
            d0, vy0, vx0, re, gt_vy, gt_vx = self._stage
        fin = [None, None, None]
        if want_final:
            if self._fin is None:
                self._fin = [torch.empty_like(d0), torch.empty_like(vy0), torch.empty_like(vx0)]
            fin = self._fin
        mk = self.masks
        args = [ptr(self.net.params.detach()), ptr(d0), ptr(vy0), ptr(vx0), ptr(re), ptr(mk.active), ptr(mk.inflow),
                ptr(mk.velBCy), ptr(mk.velBCyMask), mk.bc_stride, ptr(gt_vy), ptr(gt_vx),
                ptr(self.workspace), self.workspace_bytes, ptr(self.grads), ptr(self.loss_steps),
                ptr(fin[0]), ptr(fin[1]), ptr(fin[2]), ptr(self.iters_fwd), ptr(self.iters_bwd)]
        if self.use_graph and not eager:
            # all pointers are baked into the graph: re-capture only when a buffer moved
            key = tuple(a.value if isinstance(a, C.c_void_p) else a for a in args)
            slot = bool(want_final)                      # one graph per output set: toggling want_final re-captures nothing
            cur = self._graphs.get(slot)
            if cur is None or cur[0] != key:
                if cur is not None:
                    # the caller's buffers moved (fresh tensors every step): after three such re-captures (each one is a
                    # device-wide synchronisation + ~1000 node instantiations) stage the inputs instead
                    self._captures += 1
                    if self._captures >= 3 and self._stage is None:
                        self._stage = [t.clone() for t in (d0, vy0, vx0, re, gt_vy, gt_vx)]
                        return self._fwd_bwd(d0, vy0, vx0, re, gt_vy, gt_vx, want_final, eager)
                    check(self.lib.sol_train_graph_destroy(cur[1]))
                    del self._graphs[slot]
                h = C.c_void_p()
                torch.cuda.synchronize()
                with _lib.no_gc_during_capture():
                    check(self.lib.sol_train_graph_create(C.byref(self.cfg), *args, C.byref(h)))
                self._graphs[slot] = (key, h)
            check(self.lib.sol_train_graph_launch(self._graphs[slot][1], stream()))
        else:
            check(self.lib.sol_train_fwd_bwd(C.byref(self.cfg), stream(), *args))
        self.final = fin if want_final else None
        return self.loss_steps.sum() / ms

    # ---- algorithmic traffic of the solver part ---------------------
    def solver_algorithmic_bytes(self):
        """4*(10*Nf + 9*N + 11*N*k) per forward sample-step and 4*(2*(10*Nf+9*N) + 11*N*k_bwd)
        per backward sample-step with the MEASURED CG iteration counts (k = 0 with the direct solver:
        only the stencil / advection traffic of SURVEY 8d remains)."""
        N = self.Y * self.X
        Nf = (self.Y + 1) * self.X + self.Y * (self.X + 1)
        kf = self.iters_fwd.double().sum().item()
        kb = self.iters_bwd.double().sum().item()
        nss = self.msteps * self.B
        fwd = 4.0 * ((10 * Nf + 9 * N) * nss + 11.0 * N * kf)
        bwd = 4.0 * (2 * (10 * Nf + 9 * N) * (nss - self.B) + 11.0 * N * kb)
        return fwd, bwd, kf / nss, kb / max(1, nss - self.B)


class SolRollout:
    """No-grad roll-out of solver step + CNN correction (karman_apply.py:138-158)."""

    def __init__(self, net, masks, B, Y, X, dx, std_v, std_re, dt=1.0, res=None, in_std_v=None, out_std_v=None,
                 conv_precision="split", diffusion_substeps=1, advection="semi_lagrangian", correction_strength=1.0, conv_padding="zeros",
                 **solver):
        _refuse_substeps("SolRollout", diffusion_substeps, Y, X)
        _refuse_advection("SolRollout", advection, correction_strength)
        _refuse_periodic("SolRollout", masks, "LargeGridRollout")
        _conv_padding_arg("SolRollout", conv_padding, use="LargeGridRollout")
        _lib.require_gpu()
        self.lib = _lib.load()
        self.conv_precision = _conv_precision_code(conv_precision)
        self.net, self.masks, self.B = net, masks, B
        kc = ops.karman_cfg(B, Y, X, dx, dt=dt, res=res, masks=masks, **solver)
        self.cfg = _train_cfg(kc, 1, net, std_v, std_re, in_std_v, out_std_v)
        nbytes = self.lib.sol_rollout_workspace_bytes(C.byref(self.cfg))
        self.workspace = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=net.params.device)
        self.workspace_bytes = nbytes

    def run(self, d, vy, vx, re, nsteps):
        """Advances (d, vy, vx) in place by nsteps; returns CG iterations [nsteps,B]."""
        iters = torch.zeros(nsteps * self.B, dtype=torch.int32, device=d.device)
        mk = self.masks
        with _conv_precision_scope(self.conv_precision):
            check(self.lib.sol_rollout(C.byref(self.cfg), stream(), ptr(self.net.params.detach()), ptr(d), ptr(vy), ptr(vx),
                                       ptr(re), ptr(mk.active), ptr(mk.inflow), ptr(mk.velBCy), ptr(mk.velBCyMask),
                                       mk.bc_stride, nsteps, ptr(self.workspace), self.workspace_bytes, ptr(iters)))
        return iters.reshape(nsteps, self.B)


class LargeGridRollout:
    """SolRollout's call surface for domains BEYOND the one-workgroup solver grids (ops.beyond_one_workgroup), X a multiple of 64 -- the
    reference's 256 x 128 grid: the no-grad roll-out of karman_apply.py:138-158 with a model LargeGridTrainer wrote.  Networks: mars_moon
    and mercury.  One step is three groups of library launches and nothing else: the large-grid solver step, which writes the scaled
    features itself (ops.karman_step_large(feat=...), direct or CG pressure solve as SceneMasks decided for the scene), the network's
    forward launches (NetSchedule2D(train=False); weights packed once per run) and the correction (ops.karman_correct), followed by
    one kernel copy of the new state over the old one: the state ping-pongs between two internal buffers A -> B and the copy B -> A
    closes the step, so every step reads and writes the same addresses.

    use_graph=True (direct-solve scenes, "direct" or "direct_scattered"): that step is captured once (_lib.capture_graph: kernel nodes only) and replayed nsteps times.
    On a CG scene run() is eager, so that every solve stops at convergence: a captured step would issue the launches of the WHOLE
    cg_max_iter budget per solve (converged iterations fall through; LargeGridTrainer's docstring), hundreds of launches a roll-out
    step has no use for -- use_graph=True raises there.  cg_warm_start=True (CG scenes; ignored with the direct solve): a solve starts
    from the previous step's pressure, kept in `p_guess` [B,Y,X] across steps and run() calls (zero at first; reset_guess() clears it);
    a simulation whose guess is not finite starts from zero.  After run(), `solve_info` holds "iterations" / "converged" [nsteps, B] on
    a CG scene."""

    def __init__(self, net, masks, B, Y, X, dx, std_v, std_re, dt=1.0, res=None, in_std_v=None, out_std_v=None,
                 conv_precision="split", use_graph=True, cg_warm_start=False, any_width=False, buoyancy=None, diffusion_substeps=1,
                 advection="semi_lagrangian", correction_strength=1.0, multi_launch=False, conv_padding="zeros", **solver):
        """multi_launch=True: a grid the one-workgroup roll-out would serve (Y, X >= 16), on masks built with multi_launch=True; a width
        the convolutions take as it is (schedule2d.row_pitch(Y, X) == X) runs dense, any other needs any_width=True.
        any_width=True: X need not be a multiple of 64 -- the network runs in pitched rows (NetSchedule2D(any_width=True): the features
        are copied into zero-padded rows of 64 * ceil(X / 64) pixels and the output is cropped; the solver step and the correction stay
        dense).  buoyancy=(fy, fx) (ops.buoyancy_force): the density pushes the velocity -- the solver step is the buoyant one
        (sol_karman_step_fwd_large_buoy: one launch more, captured with the rest; direct and CG scenes, warm start included).
        diffusion_substeps=n: n explicit diffusion substeps per solver step (ops.karman_step_large(diffusion_substeps=n): the
        pre-diffusion launches are part of the captured step).  advection="mac_cormack", correction_strength=s: the solver step advects
        by the MacCormack scheme (sol_karman_step_fwd_large_adv; captured with the rest).
        conv_padding="circular" (periodic masks only): the network's convolutions pad circularly along the periodic axes of the masks
        (NetSchedule2D(padding="circular"): halo buffers, any width X, the halo launches captured with the rest); "zeros" (the default)
        is the reference's padding='same' and gives the bits it always gave."""
        self.conv_padding = _conv_padding_arg("LargeGridRollout", conv_padding, tuple(getattr(masks, "periodic", (False, False))))
        ph = self.physics = ops.StepPhysics.of(buoyancy=buoyancy, diffusion_substeps=diffusion_substeps, advection=advection,
                                               correction_strength=correction_strength, who="LargeGridRollout")
        self.buoyancy, self.diffusion_substeps, self.advection = ph.buoyancy, ph.nsub, ph.advection_kw
        self.multi_launch = _check_multi_launch("LargeGridRollout", multi_launch, masks, Y, X)
        if not ops.beyond_one_workgroup(Y, X) and not self.multi_launch:
            raise ValueError("LargeGridRollout: a %dx%d domain is served by the one-workgroup roll-out -- use SolRollout (make_rollout picks); "
                             "multi_launch=True runs the multi-launch roll-out on it" % (Y, X))
        if not _width_served(Y, X, any_width or self.conv_padding == "circular", self.multi_launch):
            raise ValueError("LargeGridRollout: the convolutions of a large domain take rows of X %% 64 == 0 cells (got %dx%d); "
                             "no roll-out class serves this grid (KarmanFlow.step advances it without the network)" % (Y, X))
        # periodic masks (SceneMasks(boundaries=...)): the plain physics, a direct solve; the correction leaves the duplicate plane of a
        # periodic axis stale, so the step runs the seam sync after it (captured with the rest)
        self._periodic_bits = int(getattr(masks, "periodic_bits", 0))
        if self._periodic_bits:
            ph.require(types.SimpleNamespace(Y=Y, X=X), masks, "LargeGridRollout")
            if cg_warm_start:
                raise ValueError("LargeGridRollout: cg_warm_start=True on a periodic scene -- periodic scenes have no CG solve to warm-start "
                                 "(they run a direct solve); pass cg_warm_start=False")
        cg = masks.pressure_solver == "cg"
        if cg and use_graph:
            raise ValueError("LargeGridRollout: use_graph=True on a scene with the CG pressure solve -- the iteration count of a solve is "
                             "not known at capture time, so a captured step issues the launches of the whole cg_max_iter budget per solve; "
                             "a roll-out runs such a scene eagerly and stops every solve at convergence: pass use_graph=False")
        _lib.require_gpu()
        from .schedule2d import NetSchedule2D
        self.lib = _lib.load()
        self.conv_precision = _conv_precision_code(conv_precision)
        self.net, self.masks, self.B, self.Y, self.X = net, masks, B, Y, X
        self.cfg = ops.karman_cfg(B, Y, X, dx, dt=dt, res=res, masks=masks, **solver)
        self.pressure_solver_used = masks.pressure_solver
        self.use_graph, self._graph = bool(use_graph), None
        self.cg_warm_start = bool(cg_warm_start) and cg
        dev = self.device = net.params.device
        self._fs3 = (C.c_float * 3)(*[1.0 / float(v) for v in (list(in_std_v if in_std_v is not None else std_v) + [std_re])])
        self._so = tuple(float(v) for v in (out_std_v if out_std_v is not None else std_v))
        self.any_width = bool(any_width)
        self._sched = NetSchedule2D(net, B, Y, X, train=False, any_width=self.any_width, padding=self.conv_padding,
                                    periodic=tuple(getattr(masks, "periodic", (False, False))))
        nd, ny, nx = B * Y * X, B * (Y + 1) * X, B * Y * (X + 1)
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        views = lambda flat: (flat[:nd].view(B, Y, X), flat[nd:nd + ny].view(B, Y + 1, X), flat[nd + ny:].view(B, Y, X + 1))
        self._flat = (z(nd + ny + nx), z(nd + ny + nx))          # the state (d | vy | vx): A, the step's input and result, and B
        self._a, self._b = views(self._flat[0]), views(self._flat[1])
        self._re = torch.ones(B, dtype=torch.float32, device=dev)
        self._feat = z(B, Y, X, 4)
        self._cor = (z(B, Y + 1, X), z(B, Y, X + 1))
        self.p_guess = z(B, Y, X) if self.cg_warm_start else None
        nbytes = ops.large_workspace_bytes(self.cfg, masks, ph)
        self._ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
        self.solve_info = {}
        self._info = []

    def reset_guess(self):
        """forget the previous step's pressure: the next solve starts from zero"""
        if self.p_guess is not None:
            check(self.lib.sol_copy_words(stream(), ptr(self.p_guess), None, self.p_guess.numel()))

    def _step(self):
        info = {}
        ops.karman_step_large(*self._a, self._re, self.cfg, self.masks, self._ws, info, feat=self._feat, feat_scale=self._fs3,
                              p_guess=self.p_guess, out=self._b, physics=self.physics)
        out, _ = self._sched.forward(self._feat)
        ops.karman_correct(out, self._b[1], self._b[2], self._so, self._cor)
        if self._periodic_bits:
            ops.karman_seam_sync(self._b[1], self._b[2], self._periodic_bits)
        _lib.dcopy_(self._flat[0], self._flat[1])
        self._info.append(info)

    def run(self, d, vy, vx, re, nsteps, corr=None):
        """Advances (d, vy, vx) in place by nsteps; returns the CG iterations [nsteps, B] (zeros with the direct solve).
        corr = (cor_y [B,Y+1,X], cor_x [B,Y,X+1]): receive the correction the LAST step applied (zero on the uncorrected row / column)."""
        B, Y, X = self.B, self.Y, self.X
        assert d.shape == (B, Y, X) and vy.shape == (B, Y + 1, X) and vx.shape == (B, Y, X + 1) and re.shape == (B,)
        assert corr is None or (corr[0].shape == vy.shape and corr[1].shape == vx.shape)
        self._info = []
        with torch.no_grad(), _conv_precision_scope(self.conv_precision):
            self._sched.begin_step()                      # the weights, packed once per run
            if self.use_graph and self._graph is None and nsteps > 0:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    self._step()                          # (on the zero state of a fresh object: nothing of it is kept)
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                self._graph = _lib.capture_graph(self._step, "LargeGridRollout")
                self._info = []
            for dst, src in zip(self._a + (self._re,), (d, vy, vx, re)):
                _lib.dcopy_(dst, src)
            for _ in range(nsteps):
                if self._graph is not None:
                    self._graph.replay()
                else:
                    self._step()
            for dst, src in zip((d, vy, vx), self._a):
                _lib.dcopy_(dst, src)
            if corr is not None and nsteps > 0:
                _lib.dcopy_(corr[0], self._cor[0])
                _lib.dcopy_(corr[1], self._cor[1])
        if self.pressure_solver_used == "cg" and nsteps > 0:
            self.solve_info = {k: torch.stack([t[k] for t in self._info]) for k in ("iterations", "converged")}
            return self.solve_info["iterations"]
        return torch.zeros(nsteps, B, dtype=torch.int32, device=d.device)


def make_rollout(net, masks, B, Y, X, dx, std_v, std_re, **kw):
    """SolRollout for the one-workgroup solver grids, LargeGridRollout beyond them (use_graph / cg_warm_start / any_width belong to the latter)."""
    if ops.beyond_one_workgroup(Y, X) or kw.get("multi_launch"):
        return LargeGridRollout(net, masks, B, Y, X, dx, std_v, std_re, **kw)
    kw.pop("multi_launch", None)
    for k in ("use_graph", "cg_warm_start", "any_width"):
        kw.pop(k, None)
    ph = ops.StepPhysics.of(**{k: kw.pop(k) for k in ("buoyancy", "advection", "correction_strength") if k in kw}, who="make_rollout")
    if ph.buoyancy is not None:
        raise ValueError("make_rollout: the buoyancy force is built on the multi-launch (large-grid) solver step only; a %dx%d grid runs "
                         "the one-workgroup roll-out (SolRollout), which has no buoyancy term" % (Y, X))
    kw["diffusion_substeps"] = _refuse_substeps("make_rollout", kw.get("diffusion_substeps", 1), Y, X)
    if ph.adv is not None:
        raise ValueError("make_rollout: the mac_cormack advection is built on the multi-launch (large-grid) solver step only; a %dx%d grid "
                         "runs the one-workgroup roll-out (SolRollout), which advects semi-Lagrangian" % (Y, X))
    return SolRollout(net, masks, B, Y, X, dx, std_v, std_re, **kw)


class GraphTrainer(_AdamDP):
    """The SolTrainer call surface for networks the C++ trainer has no fused schedule for (`model_mercury`,
    karman_train.py:92-99 / `eval('model_'+...)` at :394).  The unrolled step of karman_train.py:397-457 runs as a HAND-WRITTEN
    schedule over the C ABI (`schedule="manual"`, default since round 6: _unrolled_schedule -- forward unroll keeping what the
    reverse sweep needs, reverse sweep with the weight gradients accumulated over the steps, no autograd graph) or, as the
    cross-check, COMPOSED from the differentiable HIP ops (KarmanFlow.step, to_feature, the network, to_staggered) by torch autograd
    (`schedule="autograd"`, rounds 2-5); either way captured once into a hipGraph over static buffers: a step copies the batch in
    and replays.  Same outputs as SolTrainer: the loss, `grads` (flat, Keras get_weights() order), `loss_steps`, `final` =
    [density, vy, vx] after the last step; TF-Adam with optional per-tensor clip; data parallel through the same DPStep (one SUM
    all-reduce of `grads`): the _AdamDP surface both classes derive from.  _unrolled_schedule is the only copy of the 2-D unrolled
    step; what depends on the solver sits in _schedule_setup / _solver_fwd / _solver_bwd, which LargeGridTrainer overrides."""

    def __init__(self, net, B, Y, X, msteps, std_v, std_re, res=None, clip_grad=False, beta1=0.9, beta2=0.999, eps=1e-8,
                 group=None, use_graph=True, comm=None, in_std_v=None, out_std_v=None, pressure_solver=None,
                 dx=None, dt=1.0, masks=None, cg_rtol=1e-6, cg_atol=1e-9, cg_max_iter=2000, grad_pad="replicate",
                 inflow_order="after", conv_precision="split", schedule="manual", obstacles=None, active=None,
                 buoyancy=None, diffusion_substeps=1, advection="semi_lagrangian", correction_strength=1.0, boundaries=None,
                 conv_padding="zeros"):
        """boundaries: "open" | "periodic" | (by, bx) (ops.boundaries_arg); None = those of `masks`, open without masks.  Periodic
        boundaries are LargeGridTrainer's (this class refuses them), and so is conv_padding="circular".
        dx: cell size (default 100 / X, the reference's `--len 100`); the domain is box[0:Y*dx, 0:X*dx] as the scripts
        build it (karman_train.py:363: box[0:len*2, 0:len]).  obstacles / active: the scene of KarmanFlow (default: the reference's
        sphere).  masks: optional SceneMasks of the caller -- its boundary arrays are used; its scene must be the one KarmanFlow
        derives from the domain and the obstacles (checked).  The solver options are those of SolTrainer and are forwarded to
        KarmanFlow.  schedule: "manual" | "autograd" (see the class docstring)."""
        if schedule not in ("manual", "autograd"):
            raise ValueError("schedule must be 'manual' or 'autograd'")
        self.schedule = schedule
        self._sched = None
        self._cg_fwd, self._cg_bwd = [], []       # what the solver launches of a step report (LargeGridTrainer, CG scenes)
        self._check_grid(Y, X)
        periodic = getattr(masks, "periodic", (False, False)) if boundaries is None else ops.boundaries_arg(boundaries, "trainer: boundaries")
        if masks is not None and tuple(getattr(masks, "periodic", (False, False))) != tuple(periodic):
            raise ValueError("trainer: boundaries=%r, but the masks were built with boundaries=%r; build both with the same boundaries"
                             % (boundaries, ops.boundaries_name(getattr(masks, "periodic", (False, False)))))
        self._periodic_bits = ops.periodic_bits(periodic)
        self._check_boundaries(periodic, pressure_solver)
        self._periodic = (bool(periodic[0]), bool(periodic[1]))
        self.conv_padding = self._check_conv_padding(conv_padding, self._periodic)
        ph = self.physics = self._check_physics(Y, X, buoyancy=buoyancy, diffusion_substeps=diffusion_substeps, advection=advection,
                                                correction_strength=correction_strength)
        self.buoyancy, self.diffusion_substeps, self.advection = ph.buoyancy, ph.nsub, ph.advection_kw
        if self._periodic_bits:                 # what is not built for periodic scenes is refused here, by name
            ph.require(types.SimpleNamespace(Y=Y, X=X), types.SimpleNamespace(periodic_bits=self._periodic_bits, large=True), type(self).__name__)
        from . import fluid, karman
        _lib.require_gpu()
        self.lib = _lib.load()
        self.conv_precision = _conv_precision_code(conv_precision)
        self.net, self.B, self.Y, self.X, self.msteps = net, B, Y, X, msteps
        dev = self.device = net.params.device
        dx = 100.0 / X if dx is None else float(dx)
        self.dt = float(dt)
        self.dom = fluid.Domain([Y, X], box=fluid.box[0:Y * dx, 0:X * dx])
        self.sim = karman.KarmanFlow(pressure_solver=pressure_solver, cg_rtol=cg_rtol, cg_atol=cg_atol, cg_max_iter=cg_max_iter,
                                     grad_pad=grad_pad, inflow_order=inflow_order, obstacles=obstacles, active=active,
                                     boundaries=ops.boundaries_name(periodic))
        self.res = X if res is None else res
        if masks is not None:
            import numpy as np
            active, inflow = self.sim.scene_arrays(self.dom)
            if not (np.array_equal(masks.active.reshape(Y, X).cpu().numpy(), active.astype(np.float32)) and
                    np.array_equal(masks.inflow.reshape(Y, X).cpu().numpy(), inflow.astype(np.float32))):
                raise ValueError("GraphTrainer composes KarmanFlow.step, whose scene (inflow box, obstacles) follows from the domain "
                                 "and the obstacles / active arguments; the given masks describe a different scene")
            self.bcv = masks.velBCy.reshape(-1, Y + 1, X, 1).cpu().numpy()
            self.bcm = masks.velBCyMask.reshape(-1, Y + 1, X, 1).cpu().numpy()
        else:
            self.bcv, self.bcm = karman.velocity_bc_masks(Y, X, batch_size=B)
        # (host copies: a .tolist() of a device tensor is a synchronising copy -- illegal inside a capture)
        self._std_loss_host = (float(std_v[0]), float(std_v[1]))
        self._scale_in_host = tuple(float(a) for a in (list(in_std_v if in_std_v is not None else std_v) + [std_re]))
        self._scale_out_host = tuple(float(a) for a in (out_std_v if out_std_v is not None else std_v))
        t = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
        self.scale_loss, self.scale_in, self.scale_out = t(self._std_loss_host), t(self._scale_in_host), t(self._scale_out_host)
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
        self._in = [f32(B, Y, X), f32(B, Y + 1, X), f32(B, Y, X + 1), f32(B), f32(msteps, B, Y + 1, X), f32(msteps, B, Y, X + 1)]
        self._init_adam(net, msteps, clip_grad, beta1, beta2, eps)
        self._fin = [f32(B, Y, X), f32(B, Y + 1, X), f32(B, Y, X + 1)]
        self.use_graph, self._graph = use_graph, None
        self._init_dp(group, comm)

    @staticmethod
    def _check_grid(Y, X):
        _refuse_large_grid("GraphTrainer", Y, X)

    def _check_boundaries(self, periodic, pressure_solver):
        _refuse_periodic("GraphTrainer", types.SimpleNamespace(periodic_bits=ops.periodic_bits(periodic), periodic=periodic), "LargeGridTrainer")

    @staticmethod
    def _check_conv_padding(conv_padding, periodic):
        return _conv_padding_arg("GraphTrainer", conv_padding, use="LargeGridTrainer")

    @staticmethod
    def _check_physics(Y, X, buoyancy, diffusion_substeps, advection, correction_strength):
        """-> the ops.StepPhysics of the solver pair: here the plain one, everything else refused"""
        _refuse_buoyancy("GraphTrainer", buoyancy)
        _refuse_substeps("GraphTrainer", diffusion_substeps, Y, X)
        _refuse_advection("GraphTrainer", advection, correction_strength)
        return ops.StepPhysics()

    def _unrolled(self):
        if self.schedule == "manual":
            with torch.no_grad():                   # nothing here is differentiated by torch: the reverse sweep is written out
                return self._unrolled_schedule()
        return self._unrolled_autograd()

    def _unrolled_schedule(self):
        """karman_train.py:397-457 differentiated by hand (the 2-D counterpart of karman3d.Karman3DTrainer._unrolled_schedule; train.hip does
        the same in C++ for model_mars_moon).  The ONE copy of the 2-D unrolled step: LargeGridTrainer runs it too and overrides only
        _schedule_setup / _solver_fwd / _solver_bwd.  Forward, per unrolled step i: the solver step (saves the post-diffusion velocity,
        hands back the SCALED features) -> the network's forward launches (schedule2d.NetSchedule2D) -> velocity += out_std *
        to_staggered(out) -> loss_i and d loss_i / d v_i in one pass (sol_l2_loss_fwd_bwd, gradient pre-scaled by 1 / msteps).  Reverse,
        i = n-1 .. 0: G = d loss_i / d v_i + (adjoint of step i+1 w.r.t. its input) -> d out = out_std * G at the corrected faces -> the
        network's reverse sweep (weight gradients accumulated over the steps in the layers' partial buffers) -> the solver adjoint, which
        also takes in the feature gradient / in_std.  One reduce per layer at the end."""
        d, vy, vx, re, gt_vy, gt_vx = self._in
        Y, X, ms = self.Y, self.X, self.msteps
        if self._sched is None:
            self._schedule_setup()
        sch = self._sched
        so, sl = self._scale_out_host, self._std_loss_host
        self._cg_fwd, self._cg_bwd = [], []
        sch.begin_step()
        keep, losses = [], []
        for i in range(ms):
            d2, vy2, vx2, svy, svx, feat = self._solver_fwd(d, vy, vx, re)
            out, state = sch.forward(feat)
            vy2[:, :Y].add_(out[..., 0], alpha=so[0])             # to_staggered + add (karman_train.py:88-90, 424-426): the last row / column gets no correction
            vx2[:, :, :X].add_(out[..., 1], alpha=so[1])
            if self._periodic_bits:                               # the correction left the duplicate plane stale: the loss and the next step see a consistent field
                ops.karman_seam_sync(vy2, vx2, self._periodic_bits)
            li, gi = ops.l2_loss_fwd_bwd((vy2, vx2), (gt_vy[i], gt_vx[i]), sl, gscale=1.0 / ms)
            losses.append(li.reshape(()))
            keep.append((svy, svx, state, gi))
            d, vy, vx = d2, vy2, vx2
        gin = None
        for i in range(ms - 1, -1, -1):
            svy, svx, state, G = keep[i]
            if gin is not None:
                G[0].add_(gin[0])
                G[1].add_(gin[1])
            if self._periodic_bits:                               # the seam sync's adjoint: the duplicate plane's cotangent reaches plane 0
                ops.karman_seam_fold(G[0], G[1], self._periodic_bits)
            dO = torch.stack([G[0][:, :Y] * so[0], G[1][:, :, :X] * so[1]], dim=-1)
            dfeat = sch.backward(state, dO)
            keep[i] = None
            # nothing differentiates the start state: at i == 0 the result of the small-grid solver adjoint is UNREAD (the launch is kept
            # as it always ran; LargeGridTrainer never issued it)
            if i > 0 or self._adjoint_of_first_step:
                gin = self._solver_bwd(svy, svx, re, G, dfeat)
        losses = _lib.stack0(losses)
        _lib.dcopy_(self.loss_steps, losses)
        _lib.dcopy_(self.grads, sch.end_step())
        for dst, src in zip(self._fin, (d, vy, vx)):
            _lib.dcopy_(dst, src)

    _adjoint_of_first_step = True
    _any_width = False                  # LargeGridTrainer(any_width=True): the network's launches in pitched rows (NetSchedule2D)

    def _schedule_setup(self):
        """Once, on the first run of the schedule: the network's launches, the scene's device masks, the solver configuration"""
        from .schedule2d import NetSchedule2D
        B, Y, X = self.B, self.Y, self.X
        self._sched = NetSchedule2D(self.net, B, Y, X, any_width=self._any_width, padding=self.conv_padding, periodic=self._periodic)
        self._mk = self.sim._masks(self.dom, self.bcv, self.bcm, self.device)
        self._kcfg = ops.karman_cfg(B, Y, X, self.dom.dx[1], dt=self.dt, res=self.res, masks=self._mk, **self.sim._solver)
        self._fs = [1.0 / float(v) for v in self._scale_in_host]
        self._fs3 = (C.c_float * 3)(*self._fs)

    def _solver_fwd(self, d, vy, vx, re):
        """One solver step -> (d2, vy2, vx2, saved vy, saved vx, features / in_std [B,Y,X,4]): sol_karman_step_fwd writes the features itself"""
        mk = self._mk
        d2, vy2, vx2, svy, svx = torch.empty_like(d), torch.empty_like(vy), torch.empty_like(vx), torch.empty_like(vy), torch.empty_like(vx)
        feat = torch.empty(self.B, self.Y, self.X, 4, dtype=torch.float32, device=self.device)
        check(self.lib.sol_karman_step_fwd(C.byref(self._kcfg), stream(), ptr(d), ptr(vy), ptr(vx), ptr(re), ptr(mk.active), ptr(mk.inflow),
                                           ptr(mk.velBCy), ptr(mk.velBCyMask), mk.bc_stride, ptr(d2), ptr(vy2), ptr(vx2), ptr(svy), ptr(svx),
                                           ptr(feat), self._fs3, None))
        return d2, vy2, vx2, svy, svx, feat

    def _solver_bwd(self, svy, svx, re, G, dfeat):
        """Adjoint of one solver step: cotangent G of its output velocity, dfeat of its features -> cotangent of its input velocity.
        sol_karman_step_bwd adds dfeat / in_std itself."""
        mk = self._mk
        dfeat = dfeat[..., :2].contiguous()
        oy, ox = torch.empty_like(svy), torch.empty_like(svx)
        check(self.lib.sol_karman_step_bwd(C.byref(self._kcfg), stream(), ptr(svy), ptr(svx), ptr(re), ptr(mk.active), ptr(mk.velBCyMask),
                                           mk.bc_stride, ptr(G[0]), ptr(G[1]), ptr(dfeat), self._fs3, ptr(oy), ptr(ox), None))
        return oy, ox

    def _unrolled_autograd(self):
        from . import fluid, karman
        d0, vy0, vx0, re, gt_vy, gt_vx = self._in
        B, Y, X = self.B, self.Y, self.X
        stag = lambda vy, vx: torch.stack([_lib.pad_high(vy, 2), _lib.pad_high(vx, 1)], dim=-1)     # [B,Y+1,X+1,2]
        st = fluid.Fluid(self.dom, density=d0.reshape(B, Y, X, 1), velocity=stag(vy0, vx0), batch_size=B)
        losses = []
        for i in range(self.msteps):
            st = self.sim.step(st, re=re, res=self.res, velBCy=self.bcv, velBCyMask=self.bcm, dt=self.dt)
            corr = karman.to_staggered(self.net(karman.to_feature(st, re) / self.scale_in) * self.scale_out, self.dom.box)
            st = st.copied_with(velocity=st.velocity + corr)
            # l2_loss((gt.staggered - prd.staggered) / std_v), karman_train.py:428-436, channel by channel over the padded staggered tensors.
            # One kernel per step, no torch reduction (a multi-workgroup torch .sum() puts a memset node into the captured graph: ops.L2LossFn)
            vt, gt_t = st.velocity.staggered_tensor(), stag(gt_vy[i], gt_vx[i])
            losses.append(ops.l2_loss((vt[..., 0].contiguous(), vt[..., 1].contiguous()), (gt_t[..., 0].contiguous(), gt_t[..., 1].contiguous()), self._std_loss_host))
        losses = _lib.stack0(losses)
        self.net.params.grad = None
        (losses.sum() / self.msteps).backward()
        # (kernel copies: a contiguous tensor.copy_ is a hipMemcpyAsync = a memcpy node, refused by the capture guard -- _lib.dcopy_)
        _lib.dcopy_(self.loss_steps, losses)
        _lib.dcopy_(self.grads, self.net.params.grad)
        vt = st.velocity.staggered_tensor().detach()
        _lib.dcopy_(self._fin[0], st.density.data.detach().reshape(B, Y, X))
        self._fin[1].copy_(vt[:, :, :X, 0])
        self._fin[2].copy_(vt[:, :Y, :, 1])

    def fwd_bwd(self, d0, vy0, vx0, re, gt_vy, gt_vx, want_final=False, eager=False):
        with _conv_precision_scope(self.conv_precision):
            return self._fwd_bwd(d0, vy0, vx0, re, gt_vy, gt_vx, want_final, eager)

    def _fwd_bwd(self, d0, vy0, vx0, re, gt_vy, gt_vx, want_final, eager):
        for dst, src in zip(self._in, (d0, vy0, vx0, re, gt_vy, gt_vx)):
            dst.copy_(src, non_blocking=True)
        if eager or not self.use_graph:
            self._unrolled()
        else:
            if self._graph is None:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(2):
                        self._unrolled()
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                self.net.params.grad = None
                self._graph = _lib.capture_graph(self._unrolled, "GraphTrainer")      # kernel nodes only (sol_graph_check), then instantiated
            self._graph.replay()
        self.final = self._fin if want_final else None
        return self.loss_steps.sum() / self.msteps


class LargeGridTrainer(GraphTrainer):
    """GraphTrainer's call surface (constructor keywords, fwd_bwd / train_step / apply_gradients, `grads`, `loss_steps`, `final`, data
    parallel through DPStep, use_graph) for domains BEYOND the one-workgroup solver grids (ops.beyond_one_workgroup), X a multiple of
    64 (the reference's 256 x 128 data-generation grid).  The schedule IS GraphTrainer._unrolled_schedule (forward
    unroll, correction, ops.l2_loss_fwd_bwd, reverse sweep with NetSchedule2D.backward -- weight gradients of W = 64 * tiles rows: the
    wide form of sol_conv5x5_bwd_weight --, epilogue); this class only supplies the large-grid solver pair: _solver_fwd =
    ops.karman_step_large_saved (direct, scattered direct or CG pressure solve, as SceneMasks decides for the scene and `pressure_solver`) + the scaled
    features assembled in torch, _solver_bwd = feature gradient / in_std added to the cotangent on the faces to_feature reads +
    ops.karman_step_large_bwd, _schedule_setup = their workspaces.  Networks: mars_moon and mercury.

    use_graph=True captures the step once (kernel nodes only, sol_graph_check).  With a CG scene the iteration count of a solve is not
    known at capture time: a captured step issues the launches of the WHOLE `cg_max_iter` budget per solve (converged iterations fall
    through), so choose cg_max_iter close to what the scene needs -- or run such scenes with use_graph=False, which stops at
    convergence and is fully supported.  After a step `solve_info` holds "iterations" / "converged" [msteps, B] and "iterations_bwd" /
    "converged_bwd" [msteps - 1, B] (the first unrolled step's input receives no gradient: its solver adjoint is not run) for CG scenes."""

    def __init__(self, net, B, Y, X, msteps, std_v, std_re, any_width=False, multi_launch=False, **kw):
        """multi_launch=True: a grid the one-workgroup trainers would serve (Y, X >= 16) -- the scene's masks are built with
        SceneMasks(multi_launch=True) (masks given by the caller must have been); a width the convolutions take as it is
        (schedule2d.row_pitch(Y, X) == X) runs dense, any other needs any_width=True.
        any_width=True: X need not be a multiple of 64 -- the network's forward and reverse launches run in pitched rows of
        64 * ceil(X / 64) pixels (NetSchedule2D(any_width=True): column-masked convolutions, the weight gradient at the pitch); the solver
        pair, the correction and the loss stay dense.
        buoyancy, diffusion_substeps, advection, correction_strength (keywords): the physics of the solver pair, one ops.StepPhysics
        (which describes them) built at construction and passed to ops.karman_step_saved and ops.karman_step_large_bwd(_buoy) at every
        step; the schedule is unchanged, the pre-diffusion launches are part of the (captured) schedule and the workspaces are sized
        here, so a captured step allocates nothing.  With a force _solver_fwd also keeps each step's input density and _solver_bwd =
        ops.karman_step_large_bwd_buoy (the buoyant velocity adjoint, then the density adjoint) carries g_d_in to the next (earlier)
        step as that step's g_d_out.  The loss looks at the velocity only, so the last step's g_d_out is zero; the carried gradient is
        reset at the head of every run, so a replayed graph is self-contained.
        conv_padding="circular" (keyword; periodic boundaries only): the network's convolutions pad circularly along the periodic axes
        -- forward, backward-data and weight gradient (NetSchedule2D(padding="circular"): halo buffers refreshed by sol_conv_halo,
        captured with the rest); any width X is served.  "zeros" (the default) is the reference's padding='same': the corrector then
        sees a wall at the seam, and every existing run keeps its bits."""
        # (before the base constructor: _check_grid reads it; the base constructor checks it against the boundaries)
        self._circular = _conv_padding_arg("LargeGridTrainer", kw.get("conv_padding", "zeros"), (True, True)) == "circular"
        if any_width and kw.get("schedule", "manual") == "autograd":
            raise ValueError("LargeGridTrainer: any_width=True runs the hand-written schedule only; schedule='autograd' (the composition "
                             "over ops.conv5x5) takes no pitched rows")
        if kw.get("schedule", "manual") != "manual":
            raise ValueError("LargeGridTrainer runs the hand-written schedule only (schedule='manual')")
        self._any_width = bool(any_width)       # (before the base constructor: _check_grid reads it)
        self.multi_launch = _check_multi_launch("LargeGridTrainer", multi_launch, kw.get("masks"), Y, X)
        super().__init__(net, B, Y, X, msteps, std_v, std_re, **kw)
        self.sim._multi_launch = self.multi_launch       # the KarmanFlow that builds this trainer's masks (_schedule_setup)
        self.solve_info = {}

    def _check_grid(self, Y, X):
        if not ops.beyond_one_workgroup(Y, X) and not self.multi_launch:
            raise ValueError("LargeGridTrainer: a %dx%d domain is served by the one-workgroup trainers -- use SolTrainer (mars_moon) or "
                             "GraphTrainer (make_trainer picks); multi_launch=True runs this trainer on it" % (Y, X))
        if not _width_served(Y, X, self._any_width or self._circular, self.multi_launch):
            raise ValueError("LargeGridTrainer: the convolutions of a large domain take rows of X %% 64 == 0 cells (got %dx%d)" % (Y, X))

    _adjoint_of_first_step = False

    def _check_boundaries(self, periodic, pressure_solver):
        """periodic boundaries: served (the seam sync / fold in the schedule); without a CG solve"""
        if any(periodic) and pressure_solver == "cg":
            raise ValueError("LargeGridTrainer: pressure_solver='cg' is not built for periodic boundaries; use 'auto', 'direct' or 'direct_scattered'")

    @staticmethod
    def _check_conv_padding(conv_padding, periodic):
        return _conv_padding_arg("LargeGridTrainer", conv_padding, periodic)

    @staticmethod
    def _check_physics(Y, X, **keywords):
        return ops.StepPhysics.of(who="LargeGridTrainer", **keywords)

    def _schedule_setup(self):
        super()._schedule_setup()
        cfg, mk, dev, ph = self._kcfg, self._mk, self.device, self.physics
        self._d_in, self._g_d = [], None                    # buoyant mode: the steps' input densities; the carried density gradient
        ws = lambda n: torch.empty((int(n) + 3) // 4, dtype=torch.float32, device=dev)
        if self.buoyancy is not None:
            self._ws_bwd_d = ws(ops.density_bwd_workspace_bytes(cfg, ph))
        self._ws_fwd = ws(ops.large_workspace_bytes(cfg, mk, ph, saved=True))
        self._ws_bwd = ws(ops.large_bwd_workspace_bytes(cfg, mk, ph))
        self._zplane = torch.zeros(self.B, self.Y, self.X, dtype=torch.float32, device=dev)      # the fourth (padding) input channel
        self.pressure_solver_used = mk.pressure_solver

    def _solver_fwd(self, d, vy, vx, re):
        B, Y, X, fs = self.B, self.Y, self.X, self._fs
        if not self._cg_fwd:                                  # first unrolled step of this run: one Reynolds-number plane serves them all
            self._re_plane = (re * fs[2]).reshape(B, 1, 1).expand(B, Y, X)
            self._d_in, self._g_d = [], None                  # head of a run: nothing is carried over from the previous one
        info = {}
        if self.buoyancy is not None:
            self._d_in.append(d)
        (d2, vy2, vx2), svy, svx = ops.karman_step_large_saved(d, vy, vx, re, self._kcfg, self._mk, self._ws_fwd, info, physics=self.physics)
        self._cg_fwd.append(info)
        # to_feature / in_std (karman_train.py:77-86, 413-416), padded to the four channels the first layer's kernels read
        feat = torch.stack([vy2[:, :Y] * fs[0], vx2[:, :, :X] * fs[1], self._re_plane, self._zplane], dim=-1)
        return d2, vy2, vx2, svy, svx, feat

    def _solver_bwd(self, svy, svx, re, G, dfeat):
        Y, X, fs = self.Y, self.X, self._fs
        G[0][:, :Y].add_(dfeat[..., 0], alpha=fs[0])          # feature gradient / in_std on the faces to_feature reads
        G[1][:, :, :X].add_(dfeat[..., 1], alpha=fs[1])
        info = {}
        self._cg_bwd.append(info)
        if self.buoyancy is not None:
            # the reverse sweep visits the steps last to first (the first step's adjoint is not run): the input densities come off the end
            d_in = self._d_in.pop()
            self._g_d, oy, ox = ops.karman_step_large_bwd_buoy(d_in, svy, svx, re, G[0], G[1], self._g_d, self._kcfg, self._mk, self.buoyancy,
                                                               workspace=self._ws_bwd, info=info, density_workspace=self._ws_bwd_d,
                                                               physics=self.physics)
            return oy, ox
        return ops.karman_step_large_bwd(svy, svx, re, G[0], G[1], self._kcfg, self._mk, workspace=self._ws_bwd, info=info, physics=self.physics)

    def _fwd_bwd(self, *a, **kw):
        loss = super()._fwd_bwd(*a, **kw)
        if self.pressure_solver_used == "cg":       # (the [2, B] buffers of a captured step are the graph's own: refilled by every replay)
            f, b = self._cg_fwd, self._cg_bwd[::-1]
            self.solve_info = {k: torch.stack([t[k] for t in f]) for k in ("iterations", "converged")}
            if b:
                self.solve_info.update({k: torch.stack([t[k] for t in b]) for k in ("iterations_bwd", "converged_bwd")})
        return loss


def make_trainer(net, masks, B, Y, X, msteps, dx, std_v, std_re, **kw):
    """SolTrainer (the C++ schedule: model_mars_moon), GraphTrainer (every other network) or, for a domain beyond the one-workgroup
    solver grids, LargeGridTrainer (either network)."""
    if ops.beyond_one_workgroup(Y, X) or kw.get("multi_launch"):
        return LargeGridTrainer(net, B, Y, X, msteps, std_v, std_re, dx=dx, masks=masks, **kw)
    kw.pop("multi_launch", None)
    if net.name == "mars_moon":
        # the C++ schedule takes its scene and its pressure solver from `masks` alone (obstacles / active / pressure_solver
        # describe them for GraphTrainer's KarmanFlow)
        for k in ("obstacles", "active", "pressure_solver", "any_width", "boundaries"):      # (periodic masks: SolTrainer refuses them itself)
            kw.pop(k, None)
        kw["diffusion_substeps"] = _refuse_substeps("make_trainer", kw.get("diffusion_substeps", 1), Y, X)
        _refuse_advection("make_trainer", kw.get("advection", "semi_lagrangian"), kw.get("correction_strength", 1.0))
        return SolTrainer(net, masks, B, Y, X, msteps, dx, std_v, std_re, **kw)
    kw.pop("any_width", None)           # (the one-workgroup grids: the keyword belongs to LargeGridTrainer)
    return GraphTrainer(net, B, Y, X, msteps, std_v, std_re, dx=dx, masks=masks, **kw)     # unknown keywords raise TypeError
