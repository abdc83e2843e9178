"""The one differentiable karman-2d step behind its surfaces on the GPU (pytest -m gpu): ops.karman_step / ops.karman_step_large,
torch.ops.sol.karman_step / _dens / _re and KarmanFlow.step all apply ops.KarmanStepFn, so in every mode (plain, density, re, density + re)
and under every loss (velocity, density, both) they give the same bits -- and the bits of the gradients assembled by hand from the public
adjoints on the saved velocity; each half of the adjoint runs only when its cotangent arrives, and the plain mode retains three tensors.
The same for the Burgers step (ops.BurgersStepFn behind ops.burgers_step / burgers_step_large and torch.ops.sol.burgers_step).

Grids: 32 x 16 (the smallest the staged adjoint takes; under CG the box blob is prepared on first use) and 130 x 65 (ragged 16-cell tiles,
17 095 faces: not a multiple of 256), B = 2, direct and CG solves.  Everything here is an equality of bits or of launch sets: no tolerance.
Each (grid, mode, loss, surface) runs once (run() is cached) and is shared by the tests; nothing modifies a cached result."""
import functools
import os
import sys

import pytest
import torch

from sol_amd import _lib, fluid, karman, ops, torch_ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from large2d_scenes import CG_RTOL, SCENE_SPECS, f32, masks, state, table_geometry
from re_adjoint_cases import SEED, cotangents

pytestmark = pytest.mark.gpu

GRIDS = [(32, 16, 2, "default", "direct"), (32, 16, 2, "default", "cg"), (130, 65, 2, "default", "direct"), (130, 65, 2, "two", "cg")]
MODES = {"plain": (False, False), "density": (True, False), "re": (False, True), "density_re": (True, True)}      # (density, re)
LOSSES = ("velocity", "density", "both")
SURFACES = ("ops", "torch", "flow")
STAGED = ("k_lb_", "k_l_", "pcg_")          # the staged velocity adjoint and its pressure solve (direct: k_l_*, CG: pcg_* + k_l_*)


def losses_of(mode):
    """a density-only loss needs a density output in the graph"""
    return LOSSES if MODES[mode][0] else ("velocity", "both")


@functools.lru_cache(maxsize=None)
def grid(Y, X, B, scene, solver):
    g = table_geometry(scene, Y, X)
    mk = masks(g, solver)
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk, cg_rtol=CG_RTOL)
    assert mk.large == (Y == 130) and mk.pressure_solver == solver
    return mk, cfg, state(B, Y, X, SEED, g), tuple(f32(t) for t in cotangents(Y, X, B, scene)), torch_ops.register_scene(cfg, mk)


@functools.lru_cache(maxsize=None)
def flow(scene, solver, mode):
    specs = SCENE_SPECS[scene]
    return karman.KarmanFlow(pressure_solver=solver, cg_rtol=CG_RTOL, obstacles=None if specs is None else karman.parse_obstacles(specs),
                             density_grad=MODES[mode][0], re_grad=MODES[mode][1])


def loss_of(out, w, loss):
    total = 0.0
    if loss in ("velocity", "both"):
        total = total + (out[1] * w[1]).sum() + (out[2] * w[2]).sum()
    if loss in ("density", "both"):
        total = total + (out[0] * w[0]).sum()
    return total


def step(surface, leaves, case, mode):
    Y, X, B, scene, solver = case
    mk, cfg, _, _, handle = grid(*case)
    density, re = MODES[mode]
    if surface == "ops":
        if mk.large:
            return ops.karman_step_large(*leaves, cfg, mk, density_grad=density, re_grad=re)
        return ops.karman_step(*leaves, cfg, mk, density_grad=density, re_grad=re)
    if surface == "torch":
        if re:
            return torch.ops.sol.karman_step_re(*leaves, handle, density)
        return (torch.ops.sol.karman_step_dens if density else torch.ops.sol.karman_step)(*leaves, handle)
    hd, hy, hx, hre = leaves
    dom = fluid.Domain([Y, X], box=fluid.box[0:200, 0:100])
    s = fluid.Fluid(dom, density=hd.reshape(B, Y, X, 1), batch_size=B,
                    velocity=fluid.StaggeredGrid([hy.reshape(B, Y + 1, X, 1), hx.reshape(B, Y, X + 1, 1)], dom.box))
    bcv, bcm = karman.velocity_bc_masks(Y, X, batch_size=B)
    s = flow(scene, solver, mode).step(s, re=hre, res=X, velBCy=bcv, velBCyMask=bcm)
    return s.density.data.reshape(B, Y, X), s.velocity.data[0].data.reshape(B, Y + 1, X), s.velocity.data[1].data.reshape(B, Y, X + 1)


@functools.lru_cache(maxsize=None)
def run(case, mode, loss, surface):
    """-> (outputs, (g_d, g_vy, g_vx, g_re) with None where no gradient arrived, tensors the node retained, {kernel: launches} of backward())"""
    _, _, st, w, _ = grid(*case)
    leaves = tuple(f32(t).requires_grad_(True) for t in st)
    out = step(surface, leaves, case, mode)
    node = out[1].grad_fn if surface != "flow" else None          # (the flow's outputs are reshapes of the node's)
    retained = None if node is None else len(node.saved_tensors)
    with _lib.profile() as p:
        loss_of(out, w, loss).backward()
        torch.cuda.synchronize()
    return tuple(t.detach() for t in out), tuple(t.grad for t in leaves), retained, {k.strip("()"): v[0] for k, v in p.kernels.items()}


def by_hand(case, mode, loss):
    """(g_d, g_vy, g_vx, g_re) from the public adjoints on the saved velocity: the velocity half, then the density half added onto it"""
    mk, cfg, st, w, handle = grid(*case)
    density, re = MODES[mode]
    d, vy, vx, hre = (f32(t) for t in st)
    with torch.no_grad():
        _, svy, svx = ops.karman_step_saved(d, vy, vx, hre, cfg, mk)
    od = oy = ox = g_re = None
    if loss in ("velocity", "both"):
        if re:
            oy, ox, g_re = ops.karman_step_large_bwd_re(svy, svx, hre, w[1], w[2], vy, vx, cfg, mk)
        elif mk.large:
            oy, ox = ops.karman_step_large_bwd(svy, svx, hre, w[1], w[2], cfg, mk)
        else:
            oy, ox = torch.ops.sol.karman_step_bwd(svy, svx, hre, w[1], w[2], handle)
    if density and loss in ("density", "both"):
        if re:
            od, oy, ox, g_re = ops.karman_density_bwd_re(d, svy, svx, hre, w[0], vy, vx, cfg, mk, oy, ox, g_re)
        else:
            od, oy, ox = ops.karman_density_bwd(d, svy, svx, hre, w[0], cfg, mk, oy, ox)
    torch.cuda.synchronize()
    return od, oy, ox, g_re


def same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))


# ---- 1. the surfaces agree to the bit, with each other and with the public adjoints ---------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", GRIDS, ids=lambda c: "%dx%d-%s-%s" % (c[0], c[1], c[3], c[4]))
def test_surfaces_and_the_public_adjoints_give_the_same_bits(case, mode):
    density, re = MODES[mode]
    for loss in losses_of(mode):
        what = (case, mode, loss)
        ref_out, ref_g, _, _ = run(case, mode, loss, "ops")
        assert (ref_g[0] is not None) == (density and loss != "velocity"), what        # d.grad: only a density cotangent reaches it
        assert (ref_g[3] is not None) == re, what
        assert ref_g[1] is not None and ref_g[2] is not None, what
        assert all(bool(torch.isfinite(t).all()) for t in ref_out + tuple(t for t in ref_g if t is not None)), what
        for surface in SURFACES[1:]:
            out, g, _, _ = run(case, mode, loss, surface)
            for name, a, b in zip(("d", "vy", "vx"), out, ref_out):
                assert torch.equal(a, b), (what, surface, name)
            for name, a, b in zip(("g_d", "g_vy", "g_vx", "g_re"), g, ref_g):
                assert same(a, b), (what, surface, name)
        for name, a, b in zip(("g_d", "g_vy", "g_vx", "g_re"), by_hand(case, mode, loss), ref_g):
            assert same(a, b), (what, "by hand", name)


# ---- 2. each half runs only when its cotangent arrives ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", GRIDS, ids=lambda c: "%dx%d-%s-%s" % (c[0], c[1], c[3], c[4]))
def test_each_half_of_the_adjoint_runs_only_when_its_cotangent_arrives(case, mode):
    density, re = MODES[mode]
    large = grid(*case)[0].large
    has = lambda launches, *prefixes: any(k.startswith(prefixes) for k in launches)
    for loss in losses_of(mode):
        what = (case, mode, loss)
        launches = run(case, mode, loss, "ops")[3]
        assert launches == run(case, mode, loss, "torch")[3], what
        assert launches == run(case, mode, loss, "flow")[3], what
        velocity, dens = loss != "density", density and loss != "velocity"
        assert has(launches, "k_kd_") == dens, (what, launches)
        assert has(launches, "k_re_") == re, (what, launches)
        if not velocity:          # a density-only loss: no velocity adjoint, fused or staged, and no pressure solve
            assert all(k.startswith(("k_kd_", "k_re_")) for k in launches), (what, launches)
        elif large or re:         # the staged chain with its pressure solve, and no fused adjoint
            assert has(launches, "k_lb_") and has(launches, "k_l_") and not has(launches, "k_karman_bwd"), (what, launches)
        else:                     # the fused one-workgroup adjoint, nothing from the staged chain
            assert launches.get("k_karman_bwd") == 1 and not has(launches, *STAGED), (what, launches)
            assert all(k.startswith(("k_karman_bwd", "k_kd_")) for k in launches), (what, launches)


# ---- 3. what the node retains ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GRIDS, ids=lambda c: "%dx%d-%s-%s" % (c[0], c[1], c[3], c[4]))
def test_plain_mode_retains_three_tensors_density_four_re_six(case):
    for mode, n in (("plain", 3), ("density", 4), ("re", 6), ("density_re", 6)):
        for surface in ("ops", "torch"):
            assert run(case, mode, "velocity", surface)[2] == n, (case, mode, surface)
    mk, cfg, st, _, _ = grid(*case)
    leaves = tuple(f32(t).requires_grad_(True) for t in st)
    out = step("ops", leaves, case, "plain")
    svy, svx, re = out[1].grad_fn.saved_tensors                    # (saved vy, saved vx, re), as the trainers' tools read it
    with torch.no_grad():
        _, ry, rx = ops.karman_step_saved(*leaves, cfg, mk)
    assert torch.equal(svy, ry) and torch.equal(svx, rx) and re.data_ptr() == leaves[3].data_ptr()
    assert not out[0].requires_grad and out[0].grad_fn is None


# ---- 4. Burgers ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Y,X", [(24, 20), (24, 100)])                # one workgroup; beyond BURGERS_LDS_MAX
@pytest.mark.parametrize("forcing", [False, True])
def test_burgers_surfaces_agree_and_a_missing_cotangent_is_a_zero(Y, X, forcing):
    B, dx, dt, nu = 2, 1.0, 0.1, 0.05
    large = max(Y, X) > ops.BURGERS_LDS_MAX
    cfg = _lib.BurgersCfg(B, Y, X, dx, dt)
    circ = ops.burgers_circ(Y, X, dt * nu)
    gen = torch.Generator().manual_seed(7)
    vy, vx, fy, fx, wy, wx = (f32(torch.randn(s, generator=gen)) for s in ((B, Y + 1, X), (B, Y, X + 1)) * 3)

    def run_burgers(surface, cotangent_x):
        """cotangent_x: "given" (w_x), "zero" (an explicit zero cotangent) or "missing" (vx_out stays out of the loss)"""
        leaves = tuple(t.clone().requires_grad_(True) for t in ((vy, vx, fy, fx) if forcing else (vy, vx)))
        args = leaves if forcing else leaves + (None, None)
        if surface == "ops":
            out = (ops.burgers_step_large if large else ops.burgers_step)(*args, cfg, circ)
        else:
            out = torch.ops.sol.burgers_step(*args, dx, dt, nu)
        loss = (out[0] * wy).sum()
        if cotangent_x != "missing":
            loss = loss + (out[1] * (wx if cotangent_x == "given" else torch.zeros_like(wx))).sum()
        loss.backward()
        torch.cuda.synchronize()
        return tuple(t.detach() for t in out) + tuple(t.grad for t in leaves)

    for cotangent_x in ("given", "zero", "missing"):
        a, b = run_burgers("ops", cotangent_x), run_burgers("torch", cotangent_x)
        assert all(t is not None and bool(torch.isfinite(t).all()) for t in a)
        for k, (s, t) in enumerate(zip(a, b)):
            assert torch.equal(s, t), (cotangent_x, k)
    for surface in ("ops", "torch"):
        for k, (s, t) in enumerate(zip(run_burgers(surface, "zero"), run_burgers(surface, "missing"))):
            assert torch.equal(s, t), (surface, k)
    if large:                     # nothing requires a gradient: plain tensors, nothing kept
        assert all(t.grad_fn is None and not t.requires_grad for t in ops.burgers_step_large(vy, vx, fy if forcing else None, fx if forcing else None, cfg, circ))
