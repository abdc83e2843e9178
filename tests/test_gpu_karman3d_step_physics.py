"""karman3d._step_adjoint3d on the GPU (pytest -m gpu): the gradients of Karman3DFlow.step under autograd equal, BIT FOR BIT, those of a
direct call of the chain on what the forward saved, and the library launches the same kernels (the census of _lib.profile()) -- for force
in {none, buoyancy3d_cases.FORCES[1]} x density_grad x re_grad x diffusion_substeps in {1, 3} x the cotangent sets {density, velocity,
both}, on the two smallest scenes the kernels accept: karman3d_adjoint_cases "16_comb" (B = 2, 16 x 8 x 8, direct solve; diffuse_sub
refuses less) and the wall mask of diffusion_substeps3d_cases.CG_CASE at the same shape with pressure_solver="cg".  And
through_substeps=False: no pre-diffusion launch, and the velocity result is the pre-diffusion's input of the default run.
Accuracy against the oracle is held by test_gpu_karman3d_buoyancy.py / _diffusion_substeps.py / _density_re_adjoint.py, not here."""
import functools
import itertools
import os
import sys

import pytest
import torch

import sol_oracle3d as o
from sol_amd import _lib
from sol_amd import karman3d as k3

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import buoyancy3d_cases as bc
import diffusion_substeps3d_cases as dc
from large2d_scenes import DEV, f32

pytestmark = pytest.mark.gpu

SCENES = ("16_comb", dc.CG_CASE[0])
KINDS = ("dens", "vel", "both")


@functools.lru_cache(maxsize=None)
def scene_of(name):
    wall = name == dc.CG_CASE[0]
    Y, X, Z = dc.case(name)["shape"][1:]
    g = dc.wall_geometry(Y, X, Z) if wall else o.geometry(Y, X, Z)
    return k3.Scene3D(Y, X, Z, device=DEV, active=g.active, inflow=g.inflow, pressure_solver="cg" if wall else "direct")


def sim_of(name, force, n, **kw):
    c = dc.case(name)
    return k3.Karman3DFlow(scene_of(name), c["shape"][0], dt=c["dt"], buoyancy=force, diffusion_substeps=n, cg_rtol=1e-7, **c["kw"], **kw)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(d, vy, vx, vz, re) and the cotangents (w_d, w_vy, w_vx, w_vz) on the device.  Shared, never modified."""
    d, v, re = dc.state(name)
    return tuple(f32(t) for t in (d, *v, re)), tuple(f32(t) for t in (dc.w_dens(name), *dc.w_vel(name)))


def census(p):
    return {k: v[0] for k, v in sorted(p.kernels.items())}


def same_bits(a, b):
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))


def saved_by_fwd(sim, st):
    """what the forward keeps for the adjoint: the velocity its launches read (pre-diffused under substeps) and the post-diffusion one"""
    with torch.no_grad():
        vel = k3.diffuse_sub(sim, *st[1:4], st[4], sim.nsub)
        saved = [torch.empty_like(t) for t in vel]
        sim._fwd(st[0], *vel, st[4], saved, physics=sim.physics)
    return vel, saved


@pytest.mark.parametrize("n", (1, 3))
@pytest.mark.parametrize("force", (None, bc.FORCES[1]), ids=("plain", "force"))
@pytest.mark.parametrize("name", SCENES)
def test_autograd_gradients_and_launches_are_the_direct_chains(name, force, n):
    st, w = inputs(name)
    for density, re_grad, kind in itertools.product((False, True), (False, True), KINDS):
        sim = sim_of(name, force, n, density_grad=density, re_grad=re_grad)
        in_graph = density or force is not None                     # is the density output differentiable?
        hs = [t.clone().requires_grad_(True) for t in st[:4]] + [st[4].clone().requires_grad_(re_grad)]
        out = sim.step(*hs)
        assert out[0].requires_grad == in_graph and all(t.requires_grad for t in out[1:])
        if kind == "dens" and not in_graph:
            continue                                                # the density is a passive tracer there: no cotangent can arrive
        use = [kind in ("dens", "both") and in_graph] + [kind in ("vel", "both")] * 3
        leaves = [h for h in hs if h.requires_grad]
        torch.cuda.synchronize()
        with _lib.profile() as pa:
            g = torch.autograd.grad([t for t, u in zip(out, use) if u], leaves, [c for c, u in zip(w, use) if u], allow_unused=True)
            torch.cuda.synchronize()
        got = dict(zip(("g_d", "g_vy", "g_vx", "g_vz", "g_re"), g))
        # the direct call, on what _fwd saved
        vel, saved = saved_by_fwd(sim, st)
        gd, gv = (w[0] if use[0] else None), (tuple(w[1:]) if use[1] else (None, None, None))
        torch.cuda.synchronize()
        with torch.no_grad(), _lib.profile() as pb:
            ref = k3._step_adjoint3d(sim, sim.physics, in_graph, st[0], saved, st[4], gd, gv, vel_in=vel if re_grad else None)
            torch.cuda.synchronize()
        what = (name, force, n, density, re_grad, kind)
        for (key, a), b in zip(got.items(), ref):
            assert same_bits(a, b), (what, key)
        assert len(g) == (5 if re_grad else 4) and (ref[4] is not None) == re_grad and all(t is not None for t in ref[1:4])
        assert (ref[0] is not None) == (force is not None or use[0])     # under a force a velocity-only loss yields a density gradient too
        assert census(pa) == census(pb) and sum(census(pa).values()) > 0, (what, census(pa), census(pb))


@pytest.mark.parametrize("force", (None, bc.FORCES[1]), ids=("plain", "force"))
def test_through_substeps_false_launches_no_pre_diffusion(force):
    name, n = "16_comb", 3
    st, w = inputs(name)
    sim = sim_of(name, force, n, density_grad=True, re_grad=True)
    vel, saved = saved_by_fwd(sim, st)
    runs = {}
    with torch.no_grad():
        for through in (True, False):
            torch.cuda.synchronize()
            with _lib.profile() as p:
                res = k3._step_adjoint3d(sim, sim.physics, True, st[0], saved, st[4], w[0], w[1:], vel_in=vel, through_substeps=through)
                torch.cuda.synchronize()
            runs[through] = (res, census(p))
        torch.cuda.synchronize()
        with _lib.profile() as p:
            pre = k3.diffuse_sub(sim, *runs[False][0][1:4], st[4], n)
            torch.cuda.synchronize()
    pre_census = census(p)
    assert pre_census and not set(pre_census) & set(runs[False][1])                # no pre-diffusion kernel in the False run ...
    assert {k: runs[True][1].get(k, 0) - c for k, c in runs[False][1].items()} == {k: 0 for k in runs[False][1]}
    assert {k: c for k, c in runs[True][1].items() if k not in runs[False][1]} == pre_census      # ... and exactly one pre-diffusion more in the True run
    assert all(torch.equal(a, b) for a, b in zip(pre, runs[True][0][1:4]))         # its velocity result is that pre-diffusion's input
    assert torch.equal(runs[True][0][0], runs[False][0][0]) and torch.equal(runs[True][0][4], runs[False][0][4])      # g_d and g_re (times n) either way
