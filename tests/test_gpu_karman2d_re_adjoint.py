"""Gradient of the karman-2d step with respect to the Reynolds number on the GPU (pytest -m gpu): sol_karman_step_bwd_large_re and
sol_karman_density_bwd_re (csrc/karman_re_bwd.hip) behind ops.karman_step / ops.karman_step_large(re_grad=True), KarmanFlow(re_grad=True)
and torch.ops.sol.karman_step_re, on the one-workgroup grids (32 x 16, 64 x 32: the staged adjoint instead of the fused one) and on the
smallest large grid (130 x 65: 17 095 faces, not a multiple of 256, odd rows), direct and CG solves.

Inputs, references and the bound come from re_adjoint_cases.py: |g_re - ref|_b <= TOL_GRAD S_b with S_b from the float64 oracle; the
CPU twin (test_karman2d_re_adjoint_cpu.py) pins |ref_b| >= 0.3 S_b, so the bound means at most 3.4e-4 relative.  Velocity and density
gradients: the suite's metric (large2d_scenes.check_grads, trimmed with the suite's cap; the untrimmed value is printed beside it)."""
import math
import os
import sys

import pytest
import torch

import sol_amd
from sol_amd import _lib, fluid, karman, ops, torch_ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from large2d_scenes import CG_RTOL, DEV, TOL_FIELD, TOL_GRAD, TRIM, check_grads, cotangent_at, f32, masks, rel, state, table_geometry, trimmed_rel
from re_adjoint_cases import SEED, cotangents, oracle_case

pytestmark = pytest.mark.gpu


def setup(Y, X, B, scene="default", solver="auto", grad_pad="replicate"):
    g = table_geometry(scene, Y, X)
    mk = masks(g, solver)
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk, grad_pad=grad_pad, cg_rtol=CG_RTOL)
    return g, mk, cfg, state(B, Y, X, SEED, g)


def leaves(st):
    return tuple(f32(t).requires_grad_(True) for t in st)


def step_ops(hd, hy, hx, hre, cfg, mk, info=None, **kw):
    if mk.large:
        return ops.karman_step_large(hd, hy, hx, hre, cfg, mk, info=info, **kw)
    return ops.karman_step(hd, hy, hx, hre, cfg, mk, info, **kw)


def saved(st, cfg, mk):
    """(d, vy, vx, re) on the device and the saved post-diffusion velocity of the forward step"""
    h = tuple(f32(t) for t in st)
    with torch.no_grad():
        _, svy, svx = ops.karman_step_saved(*h, cfg, mk)
    return h, svy, svx


def loss_of(out, w, path):
    loss = 0.0
    if path in ("velocity", "both"):
        loss = loss + (out[1] * f32(w[1])).sum() + (out[2] * f32(w[2])).sum()
    if path in ("density", "both"):
        loss = loss + (out[0] * f32(w[0])).sum()
    return loss


def check_g_re(got, ref, what):
    err = (got.detach().double().cpu() - ref["g_re"]).abs()
    bound = TOL_GRAD * ref["S"]
    print("%s g_re %s, oracle %s: |difference| / S %s (bound %.0e), relative %s"
          % (what, got.tolist(), ref["g_re"].tolist(), (err / ref["S"]).tolist(), TOL_GRAD, (err / ref["g_re"].abs()).tolist()))
    assert bool(torch.isfinite(got).all())
    assert bool((err <= bound).all()), (what, err.tolist(), bound.tolist())


def check_dens_grads(got, ref, what):
    for name, a, b in zip(("g_d", "g_vy", "g_vx"), got, ref):
        v, k, worst = trimmed_rel(a, b, TRIM)
        print("%s %s: rel L2 %.3e untrimmed, %.3e after leaving out %d of %d entries (largest deviation left out %.3e)"
              % (what, name, rel(a, b), v, k, b.numel(), worst))
        assert k <= int(TRIM * b.numel())
        assert v < TOL_GRAD, (what, name, v)


# ---- 1. the velocity path against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Y,X,B,scene,solver,grad_pad", [
    (32, 16, 2, "default", "direct", "replicate"),          # the smallest one-workgroup grid the staged adjoint takes
    (64, 32, 3, "default", "auto", "replicate"),            # the reference recipe's grid through the new route
    (64, 32, 3, "default", "cg", "replicate"),              # ... the box blob prepared on first use
    (130, 65, 2, "default", "direct", "replicate"),         # 17 095 faces: not a multiple of 256, odd rows
    (130, 65, 2, "two", "cg", "replicate"),
    (64, 32, 3, "default", "auto", "dirichlet0")])
def test_g_re_and_velocity_gradients_against_the_oracle(Y, X, B, scene, solver, grad_pad):
    g, mk, cfg, st = setup(Y, X, B, scene, solver, grad_pad)
    assert mk.large == (Y == 130) and mk.pressure_solver == ("cg" if solver == "cg" else "direct")
    what = "%dx%d B=%d %s %s %s" % (Y, X, B, scene, mk.pressure_solver, grad_pad)
    ref = oracle_case(Y, X, B, scene, "velocity", grad_pad)
    w = cotangents(Y, X, B, scene, grad_pad)
    hd, hy, hx, hre = leaves(st)
    info = {}
    out = step_ops(hd, hy, hx, hre, cfg, mk, info, re_grad=True)
    assert not out[0].requires_grad and out[1].requires_grad and out[2].requires_grad
    for name, a, b in zip(("d", "vy", "vx"), out, ref["out"]):
        e = rel(a, b)
        print("%s %s_out: rel L2 %.3e" % (what, name, e))
        assert e < TOL_FIELD, (what, name, e)
    loss_of(out, w, "velocity").backward()
    torch.cuda.synchronize()
    if mk.pressure_solver == "cg":
        assert bool(info["converged_bwd"].all()), info["iterations_bwd"].tolist()
    assert hd.grad is None
    check_grads((hy.grad, hx.grad), ref["g"][1:], True, what)
    check_g_re(hre.grad, ref, what)


# ---- 2. the density path, and both together --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Y,X,B", [(64, 32, 3), (130, 65, 2)])
def test_density_path_against_the_oracle_and_both_paths_accumulate(Y, X, B):
    g, mk, cfg, st = setup(Y, X, B)
    what = "%dx%d B=%d density" % (Y, X, B)
    w = cotangents(Y, X, B)
    ref = oracle_case(Y, X, B, path="density")
    hs = leaves(st)
    info = {}
    out = step_ops(*hs, cfg, mk, info, density_grad=True, re_grad=True)
    assert all(t.requires_grad for t in out)
    loss_of(out, w, "density").backward()
    torch.cuda.synchronize()
    assert "iterations_bwd" not in info and "converged_bwd" not in info       # a density-only loss runs no pressure solve
    check_dens_grads(tuple(h.grad for h in hs[:3]), ref["g"], what)
    check_g_re(hs[3].grad, ref, what)
    dens_re = hs[3].grad.clone()
    # both cotangents: the velocity result, then the density result accumulated onto it, bit for bit
    hb = leaves(st)
    loss_of(step_ops(*hb, cfg, mk, density_grad=True, re_grad=True), w, "both").backward()
    h, svy, svx = saved(st, cfg, mk)
    oy, ox, gre_v = ops.karman_step_large_bwd_re(svy, svx, h[3], f32(w[1]), f32(w[2]), h[1], h[2], cfg, mk)
    vel = tuple(t.clone() for t in (oy, ox, gre_v))
    od, oy, ox, gre = ops.karman_density_bwd_re(h[0], svy, svx, h[3], f32(w[0]), h[1], h[2], cfg, mk, oy, ox, gre_v)
    torch.cuda.synchronize()
    assert gre is gre_v and torch.equal(gre, vel[2] + dens_re)                 # ONE fp32 add of the density's part
    for name, a, b in zip(("g_d", "g_vy", "g_vx", "g_re"), tuple(t.grad for t in hb), (od, oy, ox, gre)):
        assert torch.equal(a, b), name
    # ... and the velocity part alone is what re_grad without density_grad returns
    hv = leaves(st)
    loss_of(step_ops(*hv, cfg, mk, re_grad=True), w, "velocity").backward()
    torch.cuda.synchronize()
    assert hv[0].grad is None
    for name, a, b in zip(("g_vy", "g_vx", "g_re"), tuple(t.grad for t in hv[1:]), vel):
        assert torch.equal(a, b), name
    both = oracle_case(Y, X, B, path="both")
    err = (hb[3].grad.double().cpu() - both["g_re"]).abs()
    print("%s both paths: g_re %s, oracle %s" % (what, hb[3].grad.tolist(), both["g_re"].tolist()))
    assert bool((err <= TOL_GRAD * (oracle_case(Y, X, B)["S"] + ref["S"])).all())


# ---- 3. bits ------------------------------------------------------------------------------------------------------------------------------
def both_forms(h, svy, svx, wv, wd, cfg, mk):
    """(g_vy, g_vx, g_re) of the velocity form and (g_d, g_vy, g_vx, g_re) of the density form, written"""
    v = ops.karman_step_large_bwd_re(svy, svx, h[3], wv[0], wv[1], h[1], h[2], cfg, mk)
    d = ops.karman_density_bwd_re(h[0], svy, svx, h[3], wd, h[1], h[2], cfg, mk)
    torch.cuda.synchronize()
    return v, d


def test_bits_plain_results_reproducibility_batch_rows_zero_scale_tiles_accumulate_and_poison():
    Y, X, B = 130, 65, 3
    g, mk, cfg, st = setup(Y, X, B, solver="direct")
    h, svy, svx = saved(st, cfg, mk)
    wv = tuple(f32(t) for t in cotangent_at(B, Y, X))                    # random cotangents: bit-level properties only
    gen = torch.Generator().manual_seed(5)
    wd = f32(torch.randn(B, Y, X, generator=gen, dtype=torch.float64) * torch.as_tensor(g.active))
    v, d = both_forms(h, svy, svx, wv, wd, cfg, mk)
    assert bool(torch.isfinite(v[2]).all()) and bool(torch.isfinite(d[3]).all()) and float(v[2].abs().min()) > 0 and float(d[3].abs().min()) > 0
    # the _re entry points' velocity / density gradients are the plain entry points' bits
    pv = ops.karman_step_large_bwd(svy, svx, h[3], wv[0], wv[1], cfg, mk)
    pd = ops.karman_density_bwd(h[0], svy, svx, h[3], wd, cfg, mk)
    torch.cuda.synchronize()
    for a, b in zip(v[:2] + d[:3], pv + pd):
        assert torch.equal(a, b)
    # two runs are identical
    v2, d2 = both_forms(h, svy, svx, wv, wd, cfg, mk)
    for a, b in zip(v + d, v2 + d2):
        assert torch.equal(a, b)
    # row b of the B = 3 call equals the B = 1 call
    cfg1 = ops.karman_cfg(1, Y, X, g.dx, masks=mk, cg_rtol=CG_RTOL)
    for b in range(B):
        row = lambda t: t[b:b + 1].contiguous()
        v1, d1 = both_forms(tuple(row(t) for t in h), row(svy), row(svx), (row(wv[0]), row(wv[1])), row(wd), cfg1, mk)
        assert torch.equal(v1[2], v[2][b:b + 1]) and torch.equal(d1[3], d[3][b:b + 1]), b
    # a zero cotangent gives exactly 0
    vz, dz = both_forms(h, svy, svx, (torch.zeros_like(wv[0]), torch.zeros_like(wv[1])), torch.zeros_like(wd), cfg, mk)
    assert torch.equal(vz[2], torch.zeros(B, device=DEV)) and torch.equal(dz[3], torch.zeros(B, device=DEV))
    # a cotangent scaled by 2^+-13 scales g_re exactly
    for s in (2.0 ** 13, 2.0 ** -13):
        vs, ds = both_forms(h, svy, svx, (wv[0] * s, wv[1] * s), wd * s, cfg, mk)
        assert torch.equal(vs[2], v[2] * s) and torch.equal(ds[3], d[3] * s), s
    # the scatter through LDS windows or global atomics: the same g_re
    for opt in ("k2d_adj_tile", "k2d_dens_adj_tile"):
        _lib.set_option(opt, 0)
        try:
            vt, dt = both_forms(h, svy, svx, wv, wd, cfg, mk)
        finally:
            _lib.set_option(opt, 1)
        assert torch.equal(vt[2], v[2]) and torch.equal(dt[3], d[3]), opt
    # accumulate_re = 1: one fp32 add onto what g_re holds
    acc = ops.karman_density_bwd_re(h[0], svy, svx, h[3], wd, h[1], h[2], cfg, mk, g_re=v[2].clone())[3]
    acc_v = ops.karman_step_large_bwd_re(svy, svx, h[3], wv[0], wv[1], h[1], h[2], cfg, mk, g_re=d[3].clone())[2]
    torch.cuda.synchronize()
    assert torch.equal(acc, v[2] + d[3]) and torch.equal(acc_v, d[3] + v[2])
    # a NaN in simulation 1's cotangent: g_re[1] is NaN, the others' bits are unchanged
    bad_v, bad_d = wv[0].clone(), wd.clone()
    bad_v[1, 70, 30] = float("nan")
    bad_d[1, 100, 30] = float("nan")
    vn, dn = both_forms(h, svy, svx, (bad_v, wv[1]), bad_d, cfg, mk)
    for got, clean in ((vn[2], v[2]), (dn[3], d[3])):
        assert bool(torch.isnan(got[1])) and torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])


# ---- 4. three chained steps through KarmanFlow ------------------------------------------------------------------------------------------
def flow_state(hd, hy, hx, B, Y, X):
    dom = fluid.Domain([Y, X], box=fluid.box[0:200, 0:100])
    vel = fluid.StaggeredGrid([hy.reshape(B, Y + 1, X, 1), hx.reshape(B, Y, X + 1, 1)], dom.box)
    return fluid.Fluid(dom, density=hd.reshape(B, Y, X, 1), velocity=vel, batch_size=B)


def flow_out(s, B, Y, X):
    return s.density.data.reshape(B, Y, X), s.velocity.data[0].data.reshape(B, Y + 1, X), s.velocity.data[1].data.reshape(B, Y, X + 1)


def test_three_chained_steps_through_karman_flow_against_the_oracle():
    """Bound: each step contributes at most TOL_GRAD S to g_re, |g_re| >= 0.3 S (the CPU twin's floor) and the cotangent's error grows at
    most linearly over the three steps: relative error <= 3 TOL_GRAD / 0.3 = 1e-3.  The oracle's own float32 run is at 4.6e-5."""
    Y, X, B = 64, 32, 3
    g = table_geometry("default", Y, X)
    st = state(B, Y, X, SEED, g)
    ref = oracle_case(Y, X, B, steps=3)
    w = cotangents(Y, X, B, steps=3)
    hd, hy, hx, hre = leaves(st)
    sim = karman.KarmanFlow(re_grad=True)
    bcv, bcm = karman.velocity_bc_masks(Y, X, batch_size=B)
    s = flow_state(hd, hy, hx, B, Y, X)
    for _ in range(3):
        s = sim.step(s, re=hre, res=X, velBCy=bcv, velBCyMask=bcm)
    out = flow_out(s, B, Y, X)
    for name, a, b in zip(("d", "vy", "vx"), out, ref["out"]):
        assert rel(a, b) < TOL_FIELD, (name, rel(a, b))
    loss_of(out, w, "velocity").backward()
    torch.cuda.synchronize()
    err = ((hre.grad.double().cpu() - ref["g_re"]).abs() / ref["g_re"].abs()).tolist()
    print("three steps: g_re %s, oracle %s, relative error %s (bound %.1e)" % (hre.grad.tolist(), ref["g_re"].tolist(), err, 3 * TOL_GRAD / 0.3))
    check_grads((hy.grad, hx.grad), ref["g"][1:], True, "three steps")
    assert max(err) <= 3 * TOL_GRAD / 0.3, err


# ---- 5. torch.ops.sol.karman_step_re, and the defaults ---------------------------------------------------------------------------------
@pytest.mark.parametrize("Y,X,B", [(64, 32, 3), (130, 65, 2)])
def test_torch_op_equals_the_ops_path_and_the_defaults_did_not_move(Y, X, B):
    g, mk, cfg, st = setup(Y, X, B)
    w = cotangents(Y, X, B)
    scene = torch_ops.register_scene(cfg, mk)
    for density in (False, True):
        path = "both" if density else "velocity"
        ha, hb = leaves(st), leaves(st)
        oa = step_ops(*ha, cfg, mk, density_grad=density, re_grad=True)
        ob = torch.ops.sol.karman_step_re(*hb, scene, density)
        assert ob[0].requires_grad == density and ob[1].requires_grad
        loss_of(oa, w, path).backward()
        loss_of(ob, w, path).backward()
        torch.cuda.synchronize()
        for a, b in zip(oa, ob):
            assert torch.equal(a.detach(), b.detach())
        for a, b in zip(ha, hb):
            assert (a.grad is None and b.grad is None) or torch.equal(a.grad, b.grad)
        assert ha[3].grad is not None and (ha[0].grad is not None) == density
    # the flag off: re is data, and the step's results are the same launches' bits
    hs = leaves(st)
    plain = step_ops(*hs, cfg, mk)
    with _lib.profile() as plain_launches:
        loss_of(plain, w, "velocity").backward()
        torch.cuda.synchronize()
    assert hs[3].grad is None and hs[1].grad is not None
    for a, b in zip(plain, oa):
        assert torch.equal(a.detach(), b.detach())
    hf = leaves(st)
    sim = karman.KarmanFlow()
    bcv, bcm = karman.velocity_bc_masks(Y, X, batch_size=B)
    out = flow_out(sim.step(flow_state(*hf[:3], B, Y, X), re=hf[3], res=X, velBCy=bcv, velBCyMask=bcm), B, Y, X)
    loss_of(out, w, "velocity").backward()
    torch.cuda.synchronize()
    assert hf[3].grad is None and torch.equal(hf[1].grad, hs[1].grad)
    # re_grad with an re that requires no gradient: the plain path
    hn = leaves(st[:3]) + (f32(st[3]),)
    out = step_ops(*hn, cfg, mk, re_grad=True)
    assert len(out[1].grad_fn.saved_tensors) == 3
    with _lib.profile() as p:
        loss_of(out, w, "velocity").backward()
        torch.cuda.synchronize()
    launches = {k.strip("()"): v[0] for k, v in p.kernels.items()}
    has = lambda prefix: any(k.startswith(prefix) for k in launches)
    assert launches == {k.strip("()"): v[0] for k, v in plain_launches.kernels.items()}, launches
    assert not has("k_re_") and has("k_lb_") == mk.large and has("k_karman_bwd") == (not mk.large), launches
    assert hn[3].grad is None and torch.equal(hn[1].grad, hs[1].grad) and torch.equal(hn[2].grad, hs[2].grad)


# ---- 6. identification ------------------------------------------------------------------------------------------------------------------
def test_reynolds_numbers_are_identified_from_four_frames(capsys):
    """scripts/karman_fit_re.py's loop: 64 x 32, B = 3, K = 4 frames generated by the HIP step at the true Re, start at 4 Re, Adam lr 0.2 on
    log Re, 40 iterations.  The float64 oracle running the same loop ends at Re / Re_true = 1.081 (|log| = 0.078; Adam still oscillates at
    iteration 40) with its loss at 0.010 of the first; asserted: |log| <= 0.2 (2.5 x the oracle's end point) and loss <= 0.05 x initial."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts"))
    from karman_fit_re import fit_re, flow_stepper
    Y, X, B = 64, 32, 3
    g = table_geometry("default", Y, X)
    st = state(B, Y, X, SEED, g)
    dom = fluid.Domain([Y, X], box=fluid.box[0:200, 0:100])
    step = flow_stepper(karman.KarmanFlow(re_grad=True), dom, B, Y, X, X)
    re_true = f32(st[3])
    frames = [tuple(f32(t) for t in st[:3])]
    with torch.no_grad():
        for _ in range(3):
            frames.append(step(*frames[-1], re_true))
    lines = []
    re_fit, history = fit_re(step, frames, (4.0 * re_true).tolist(), iters=40, lr=0.2, print_fn=lines.append)
    torch.cuda.synchronize()
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    logs = [abs(math.log(a / b)) for a, b in zip(re_fit.tolist(), re_true.tolist())]
    print("Re_fit / Re_true %s, |log| %s, loss %.4e -> %.4e" % ((re_fit / re_true).tolist(), logs, history[0][0], history[-1][0]))
    assert len(history) == 41 and max(logs) <= 0.2, logs
    assert history[-1][0] <= 0.05 * history[0][0], (history[0][0], history[-1][0])
