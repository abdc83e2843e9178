"""Adjoint of the karman-3d marker density and gradient with respect to the Reynolds number on the GPU (pytest -m gpu):
sol_karman3d_density_bwd(_re) (csrc/karman3d_density_bwd.hip), sol_karman3d_step_bwd_re (csrc/karman3d.hip) and the reduction
(csrc/karman3d_re_bwd.hip) behind Karman3DFlow(density_grad=True, re_grad=True).step, torch.ops.sol.karman3d_step_dens / _step_re and the
direct call karman3d.density_bwd -- against the float64 oracle's autograd, against the linearity of the density path (no oracle), bit
reproducibility (run twice, eager against captured, LDS window against global atomics), poisoning by a non-finite cotangent, and that the
defaults did not move.

Shapes: 16 x 8 x 8 with B = 2 (the minimum grid, a batch), 20 x 10 x 10 (tiles that end inside the grid, the extra face rows), 32 x 16 x 16
with departure points 2.6 cells away (targets beyond the scatter's LDS window).  Tolerances are the suite's: fields 1e-5, gradients 1e-4
relative L2 (TOL_FIELD, TOL_GRAD of test_gpu_karman3d.py); g_re relative L2 over the batch vector.  The inputs are fixed
(karman3d_adjoint_cases.py says why, test_karman3d_density_re_adjoint_cpu.py pins it): with them the oracle's own float32 run matches
float64 untrimmed, so the metric asserted on the field gradients, trimmed_rel with the suite's cap of 0.1 % of a component's entries, only
has to absorb a cell that the KERNEL's fp32 rounding decides differently; the untrimmed value is printed beside it."""
import functools
import os
import sys

import pytest
import torch

from sol_amd import _lib, torch_ops
from sol_amd import karman3d as k3

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import karman3d_adjoint_cases as kc
from large2d_scenes import DEV, TOL_FIELD, TOL_GRAD, TRIM, f32, rel, trimmed_rel

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def scene_of(shape, solver="auto"):
    _, Y, X, Z = shape
    return k3.Scene3D(Y, X, Z, device=DEV, pressure_solver=solver)


def sim_of(name, density_grad=True, re_grad=True, solver="auto", **kw):
    c = kc.case(name)
    return k3.Karman3DFlow(scene_of(c["shape"], solver), c["shape"][0], dt=c["dt"], density_grad=density_grad, re_grad=re_grad, **c["kw"], **kw)


def leaves(name, re_leaf=True):
    d, v, re = kc.state(name)
    hs = [f32(t).requires_grad_(True) for t in (d, *v)]
    return hs + [f32(re).requires_grad_(re_leaf)]


def chain(step, hs, steps=1):
    """`steps` chained calls of step(d, vy, vx, vz, re) from the leaves hs"""
    cur = hs[:4]
    for _ in range(steps):
        cur = step(*cur, hs[4])
    return cur


def backward(name, out, density=None, velocity=None):
    """the case's loss (or the given choice of cotangents) on the outputs of the last step"""
    c = kc.case(name)
    density = c["density"] if density is None else density
    velocity = c["velocity"] if velocity is None else velocity
    loss = 0.0
    if density:
        loss = loss + (out[0] * f32(kc.w_dens(name))).sum()
    if velocity:
        loss = loss + sum((a * f32(w)).sum() for a, w in zip(out[1:], kc.w_vel(name)))
    loss.backward()
    torch.cuda.synchronize()


def grads_of(hs):
    return tuple(torch.zeros_like(h) if h.grad is None else h.grad for h in hs)


def check_fields(out, ref, what):
    for n, a, b in zip(("d", "vy", "vx", "vz"), out, ref):
        e = rel(a, b)
        print("%s %s_out: rel L2 %.3e" % (what, n, e))
        assert e < TOL_FIELD, (what, n, e)


def check_grads(got, ref, what, with_re=True):
    for n, a, b in zip(kc.NAMES[:4], got, ref):
        v, k, worst = trimmed_rel(a, b, TRIM)
        print("%s %s: rel L2 %.3e untrimmed, %.3e after leaving out %d of %d entries (largest deviation left out %.3e)"
              % (what, n, rel(a, b), v, k, b.numel(), worst))
        assert k <= int(TRIM * b.numel())
        assert v < TOL_GRAD, (what, n, v)
    if with_re:
        e = rel(got[4], ref[4])
        print("%s g_re: rel L2 over the batch %.3e  (%s against %s)" % (what, e, got[4].tolist(), ref[4].tolist()))
        assert e < TOL_GRAD, (what, "g_re", e)


def forward_saved(sim, name):
    """a plain forward step of the case's state that keeps the post-diffusion velocity -> (device state, saved)"""
    d, v, re = kc.state(name)
    st = [f32(t) for t in (d, *v, re)]
    saved = [torch.empty_like(t) for t in st[1:4]]
    with torch.no_grad():
        sim._fwd(*st, saved)
    return st, saved


# ---- 1. density-only loss against the oracle, through each surface ------------------------------------------------------------------
@pytest.mark.parametrize("surface,name", [("step", "16_dens"), ("dens_op", "20_dens"), ("direct", "32_cfl"), ("step", "32_x35"), ("dens_op", "16_dens")])
def test_density_only_loss_against_the_oracle(surface, name):
    ref_out, ref_g = kc.oracle_case(name)
    sim = sim_of(name, re_grad=False)
    if surface == "direct":
        st, saved = forward_saved(sim, name)
        got = k3.density_bwd(sim, st[0], saved, st[4], f32(kc.w_dens(name)))
        torch.cuda.synchronize()
        check_grads(got, ref_g, "direct %s" % name, with_re=False)
        return
    hs = leaves(name, re_leaf=False)
    step = sim.step if surface == "step" else (lambda *a, h=torch_ops.register_scene3d(sim): torch.ops.sol.karman3d_step_dens(*a, h))
    out = chain(step, hs)
    assert all(t.requires_grad for t in out)
    check_fields(out, ref_out, "%s %s" % (surface, name))
    backward(name, out)
    check_grads(grads_of(hs[:4]), ref_g, "%s %s" % (surface, name), with_re=False)
    assert hs[4].grad is None


def test_density_only_loss_on_a_cg_scene_reports_no_backward_solve():
    name = "16_dens"
    ref_out, ref_g = kc.oracle_case(name)
    sim = sim_of(name, solver="cg", cg_rtol=1e-7)
    assert sim.cg
    hs = leaves(name)
    out = chain(sim.step, hs)
    check_fields(out, ref_out, "cg " + name)
    backward(name, out)
    assert "iterations" in sim.solve_info and "iterations_bwd" not in sim.solve_info      # no velocity adjoint, hence no pressure solve
    check_grads(grads_of(hs), ref_g, "cg " + name)
    # a velocity cotangent does run it
    hs = leaves(name)
    backward(name, chain(sim.step, hs), velocity=True)
    assert "iterations_bwd" in sim.solve_info


# ---- 2. combined density + velocity loss -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["16_comb", "20_comb"])
def test_combined_loss_against_the_oracle_and_its_two_parts(name):
    ref_out, ref_g = kc.oracle_case(name)
    sim = sim_of(name, re_grad=False)
    hs = leaves(name, re_leaf=False)
    out = chain(sim.step, hs)
    check_fields(out, ref_out, name)
    backward(name, out)
    comb = grads_of(hs[:4])
    check_grads(comb, ref_g, name, with_re=False)
    # the density-only result of the same flow
    hd = leaves(name, re_leaf=False)
    backward(name, chain(sim.step, hd), velocity=False)
    dens = grads_of(hd[:4])
    # the default path's gradient for the same velocity cotangents + the density part of an accumulate = 0 call, bit for bit
    plain_sim = sim_of(name, density_grad=False, re_grad=False)
    hv = leaves(name, re_leaf=False)
    plain = chain(plain_sim.step, hv)
    assert not plain[0].requires_grad
    backward(name, plain, density=False)
    st, saved = forward_saved(plain_sim, name)
    part = k3.density_bwd(plain_sim, st[0], saved, st[4], f32(kc.w_dens(name)))
    torch.cuda.synchronize()
    assert hv[0].grad is None
    for c in (1, 2, 3):
        assert torch.equal(comb[c], hv[c].grad + part[c]) and torch.equal(part[c], dens[c])
    assert torch.equal(comb[0], part[0]) and torch.equal(comb[0], dens[0])


# ---- 3. the step's options, two chained steps ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["16_before", "16_dirichlet", "16_two"])
def test_options_and_chained_steps_against_the_oracle(name):
    ref_out, ref_g = kc.oracle_case(name)
    sim = sim_of(name)
    hs = leaves(name)
    out = chain(sim.step, hs, kc.case(name)["steps"])
    check_fields(out, ref_out, name)
    backward(name, out)
    check_grads(grads_of(hs), ref_g, name)


# ---- 4. the gradient with respect to the Reynolds number ---------------------------------------------------------------------------
@pytest.mark.parametrize("surface,name", [("step", "16_vel"), ("re_op", "16_dens"), ("step", "16_comb"), ("re_op", "20_comb"), ("step", "16_lowre"),
                                          ("step", "32_cfl")])
def test_reynolds_gradient_against_the_oracle(surface, name):
    """velocity path alone (16_vel), density path alone (16_dens, 32_cfl), both accumulating (the others), one low-Re case"""
    c = kc.case(name)
    ref_out, ref_g = kc.oracle_case(name)
    sim = sim_of(name, density_grad=(surface == "step"))
    hs = leaves(name)
    if surface == "step":
        step = sim.step
    else:
        step = lambda *a, h=torch_ops.register_scene3d(sim): torch.ops.sol.karman3d_step_re(*a, h, c["density"])
    out = chain(step, hs)
    assert out[0].requires_grad == (surface == "step" or c["density"])
    check_fields(out, ref_out, "%s %s" % (surface, name))
    backward(name, out)
    got = grads_of(hs)
    assert hs[4].grad is not None and bool(torch.isfinite(got[4]).all()) and float(got[4].abs().min()) > 0
    check_grads(got, ref_g, "%s %s" % (surface, name))


def test_step_bwd_re_leaves_the_velocity_gradients_bit_for_bit():
    name = "16_vel"
    sim = sim_of(name)
    st, saved = forward_saved(sim, name)
    w = [f32(t) for t in kc.w_vel(name)]
    plain = sim._bwd(saved, st[4], *w)
    with_re = sim._bwd(saved, st[4], *w, vel_in=st[1:4])
    # ... and onto a buffer: one fp32 add
    base = torch.tensor([0.5, -2.0], dtype=torch.float32, device=DEV)
    acc = sim._bwd(saved, st[4], *w, vel_in=st[1:4], g_re=base.clone())
    torch.cuda.synchronize()
    assert len(plain) == 3 and len(with_re) == 4
    for a, b, c in zip(plain, with_re, acc):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(acc[3], base + with_re[3])
    assert rel(with_re[3], kc.oracle_case(name)[1][4]) < TOL_GRAD


# ---- 5. no oracle: the density gradient is the transpose of the affine density map ----------------------------------------------------
@pytest.mark.parametrize("name,dt", [("32_x35", 1.5), ("32_cfl", 4.0)])
def test_density_gradient_is_the_transpose_of_the_affine_density_map(name, dt):
    """d_out is affine in d_in at a fixed velocity: <w, step(d1) - step(d2)> = <g_d, d1 - d2>, with two forward HIP steps on the left.  At
    0.97 cells per step, and at 2.6 where the scatter's targets leave the LDS window and the domain."""
    c = kc.case(name)
    B, Y, X, Z = c["shape"]
    d, v, re = kc.state(name)
    cfl = max(float(t.abs().max()) for t in v) * dt / kc.geometry(name).dx
    assert (0.9 < cfl < 1.1) if dt == 1.5 else cfl > 2.0
    sim = k3.Karman3DFlow(scene_of(c["shape"]), B, dt=dt, density_grad=True)
    gen = torch.Generator().manual_seed(29)
    d1, d2 = f32(d), f32(torch.rand(B, Y, X, Z, generator=gen, dtype=torch.float64))
    w = f32(torch.randn(B, Y, X, Z, generator=gen, dtype=torch.float64))
    hv = [f32(t) for t in v]
    h1 = d1.clone().requires_grad_(True)
    o1 = sim.step(h1, *hv, f32(re))
    (o1[0] * w).sum().backward()
    with torch.no_grad():
        o2 = sim.step(d2, *hv, f32(re))
    torch.cuda.synchronize()
    dout = o1[0].detach().double() - o2[0].double()
    lhs = float((w.double() * dout).sum())
    rhs = float((h1.grad.double() * (d1.double() - d2.double())).sum())
    bound = 1e-5 * float(w.double().norm()) * float(dout.norm())
    print("linearity at %.2f cells per step: <w, dout> = %.9e, <g_d, din> = %.9e, difference %.3e, bound %.3e" % (cfl, lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs) > 10 * bound                    # the identity is not met by two vanishing sides
    assert abs(lhs - rhs) <= bound


# ---- 6. bit reproducibility ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["16_dens", "20_dens", "32_cfl"])
def test_bit_reproducible_twice_and_lds_window_against_global_atomics(name):
    sim = sim_of(name)
    st, saved = forward_saved(sim, name)
    hw = f32(kc.w_dens(name))
    call = lambda: k3.density_bwd(sim, st[0], saved, st[4], hw, vel_in=st[1:4])
    runs = [call() for _ in range(2)]
    torch.cuda.synchronize()
    assert len(runs[0]) == 5
    for a, b in zip(*runs):
        assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
    _lib.set_option("k3d_dens_adj_tile", 0)
    try:
        glob = call()
        torch.cuda.synchronize()
    finally:
        _lib.set_option("k3d_dens_adj_tile", 1)
    for a, b in zip(glob, runs[0]):
        assert torch.equal(a, b)
    # the plain form: the same bits without the reduction; accumulate = 1 = one fp32 add per face onto what was there
    plain = k3.density_bwd(sim, st[0], saved, st[4], hw)
    base = [torch.full_like(t, x) for t, x in zip(saved, (0.25, -3.0, 1.5))]
    acc = k3.density_bwd(sim, st[0], saved, st[4], hw, g_v=[t.clone() for t in base])
    torch.cuda.synchronize()
    assert len(plain) == 4 and all(torch.equal(a, b) for a, b in zip(plain, runs[0]))
    assert torch.equal(acc[0], plain[0]) and all(torch.equal(acc[1 + c], base[c] + plain[1 + c]) for c in range(3))


def test_eager_against_captured():
    """both adjoints with the reduction as one captured graph (kernel nodes only), replayed twice"""
    name = "20_comb"
    sim = sim_of(name)
    st, saved = forward_saved(sim, name)
    hw, wv = f32(kc.w_dens(name)), [f32(t) for t in kc.w_vel(name)]

    def both():
        gi = sim._bwd(saved, st[4], *wv, vel_in=st[1:4])
        return k3.density_bwd(sim, st[0], saved, st[4], hw, g_v=gi[:3], vel_in=st[1:4], g_re=gi[3])

    eager = both()
    torch.cuda.synchronize()
    cap = {}

    def body():
        cap["g"] = both()

    graph = _lib.capture_graph(body, "karman-3d density + Re adjoint")
    for _ in range(2):
        for t in cap["g"]:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(cap["g"], eager):
            assert torch.equal(a, b)
    # ... and the autograd surface computes the same bits
    hs = leaves(name)
    backward(name, chain(sim.step, hs))
    for a, b in zip(grads_of(hs), eager):
        assert torch.equal(a, b)


# ---- 7. a non-finite cotangent poisons its simulation only ---------------------------------------------------------------------------
def test_nonfinite_density_cotangent_poisons_its_simulation_only():
    name = "16_dens"
    sim = sim_of(name)
    st, saved = forward_saved(sim, name)
    hw = f32(kc.w_dens(name))
    clean = k3.density_bwd(sim, st[0], saved, st[4], hw, vel_in=st[1:4])
    bad = hw.clone()
    bad[1, 3, 2, 5] = float("inf")
    got = k3.density_bwd(sim, st[0], saved, st[4], bad, vel_in=st[1:4])
    # ... and added onto a finite velocity adjoint and a finite g_re
    acc = k3.density_bwd(sim, st[0], saved, st[4], bad, g_v=[torch.ones_like(t) for t in saved], vel_in=st[1:4], g_re=torch.ones(2, dtype=torch.float32, device=DEV))
    torch.cuda.synchronize()
    for res in (got, acc):
        for n, t in zip(kc.NAMES, res):
            assert bool(torch.isnan(t[1]).all()), n
    for n, a, b in zip(kc.NAMES, got, clean):
        assert torch.equal(a[0], b[0]) and bool(torch.isfinite(b).all()), n
    # through the autograd surface
    hs = leaves(name)
    out = chain(sim.step, hs)
    (out[0] * bad).sum().backward()
    torch.cuda.synchronize()
    for n, h, b in zip(kc.NAMES, hs, clean):
        assert bool(torch.isnan(h.grad[1]).all()) and torch.equal(h.grad[0], b[0]), n


# ---- 8. the defaults did not move ------------------------------------------------------------------------------------------------------
def test_defaults_keep_the_density_and_re_out_of_the_graph():
    name = "16_vel"
    plain_sim = sim_of(name, density_grad=False, re_grad=False)
    hp = leaves(name)
    plain = chain(plain_sim.step, hp)
    assert not plain[0].requires_grad and all(t.requires_grad for t in plain[1:])
    backward(name, plain)
    assert hp[0].grad is None and hp[4].grad is None
    # the flagged run's velocity part: the same outputs and velocity gradients, bit for bit
    hf = leaves(name)
    flagged = chain(sim_of(name).step, hf)
    assert all(t.requires_grad for t in flagged)
    backward(name, flagged)
    for a, b in zip(plain, flagged):
        assert torch.equal(a.detach(), b.detach())
    for c in (1, 2, 3):
        assert torch.equal(hp[c].grad, hf[c].grad)
    assert hf[4].grad is not None and hf[0].grad is None
    # torch.ops.sol.karman3d_step: as ever
    ho = leaves(name)
    op = torch.ops.sol.karman3d_step(*ho, torch_ops.register_scene3d(plain_sim))
    assert not op[0].requires_grad
    backward(name, op)
    assert ho[4].grad is None and all(torch.equal(ho[c].grad, hp[c].grad) for c in (1, 2, 3))
    # re_grad with an re that requires no gradient, nothing else either: the no-grad forward
    none = sim_of(name).step(*[t.detach() for t in hf])
    assert not any(t.requires_grad for t in none)
