"""multi_launch=True: the multi-launch karman-2d path (karman_step_large, LargeGridTrainer, LargeGridRollout) on the grids the fused
one-workgroup kernels would serve -- with it buoyancy, mac_cormack, diffusion substeps, density_grad, re_grad, any_width, the three
pressure solvers and the scripts' --multi-launch work there as they do on large grids (pytest -m gpu).

Tolerances are the project's: TOL_FIELD = 1e-5 on fields, TOL_GRAD = 1e-4 on gradients (relative L2 against the float64 references of
karman2d_multi_launch_cases, which are the oracle's step and maccormack_cases.step on the grid's geometry); MacCormack gradients in the
trimmed metric with the cap large2d_scenes.TRIM as a condition (maccormack_cases' rule); CG solves at CG_RTOL = 1e-7.  Seeds: the CPU
twin test_karman2d_multi_launch_cpu.py holds the float32 reference alone to a quarter of each tolerance at every (grid, seed) used here.
Every test here fails on a library without the keyword with a TypeError.
Measured on an MI355X (printed by the tests): fields 3.8e-8 ... 6.0e-7, gradients 1.5e-7 ... 6.0e-7 (at most 9 entries left out under
MacCormack), g_re 8.7e-7; multi-launch against the fused step 3.3e-8 ... 4.8e-7 (bound 2e-5); trainer loss 1.3e-6 / 2.1e-6, weight
gradient 1.5e-6 / 2.0e-6 (64 x 32 / 96 x 48), one Adam step 5.6e-7 of an update of 5.1e-2 (bound 1.13e-6); roll-out after four steps
d 8.0e-8, vy 7.6e-8, vx 4.6e-7; CG 27 ... 29 iterations per warm-started solve."""
import contextlib
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import sol_amd
import sol_oracle as o
from sol_amd import _lib, fluid, karman, ops, torch_ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import karman2d_multi_launch_cases as mlc
import karman2d_small_shapes as ks
from large2d_scenes import CG_RTOL, DEV, TOL_FIELD, TOL_GRAD, f32, rel

pytestmark = pytest.mark.gpu
B = mlc.B
MC = dict(advection="mac_cormack")


@contextlib.contextmanager
def option(name, value):
    old = _lib.get_option(name)
    _lib.set_option(name, value)
    try:
        yield
    finally:
        _lib.set_option(name, old)


def setup(grid, solver="auto", multi_launch=True, nb=B, **kw):
    g = o.geometry(*grid)
    mk = ops.SceneMasks(g.active, g.inflow, g.bc_mask, g.bc_mask, DEV, pressure_solver=solver, multi_launch=multi_launch)
    assert mk.large == multi_launch
    if mk.pressure_solver == "cg":
        kw.setdefault("cg_rtol", CG_RTOL)
    return g, mk, ops.karman_cfg(nb, grid[0], grid[1], g.dx, masks=mk, **kw)


def physics_kw(adv, force, n):
    kw = dict(buoyancy=force, diffusion_substeps=n)
    if adv is not None:
        kw.update(advection="mac_cormack", correction_strength=adv)
    return kw


def hip_step_and_grads(grid, mk, cfg, adv=None, force=None, n=1, kind="velocity", info=None, step=None):
    """the differentiable step on the reference's state and cotangents -> ((d, vy, vx), (g_d, g_vy, g_vx, g_re))"""
    _, _, st, (wd, wy, wx) = mlc.reference(grid, adv, force, n, kind)
    d, vy, vx, re = (f32(t) for t in st)
    leaves = [d, vy, vx, re]
    for t in leaves[:3] if kind != "re" else leaves:
        t.requires_grad_(True)
    step = step or (lambda *a: ops.karman_step_large(*a, cfg, mk, info=info, density_grad=kind == "density", re_grad=kind == "re",
                                                     **physics_kw(adv, force, n)))
    out = step(d, vy, vx, re)
    loss = (out[1] * f32(wy)).sum() + (out[2] * f32(wx)).sum()
    if wd is not None:
        loss = loss + (out[0] * f32(wd)).sum()
    loss.backward()
    torch.cuda.synchronize()
    return tuple(t.detach() for t in out), tuple(torch.zeros_like(t) if t.grad is None else t.grad for t in leaves)


def check_case(what, grid, got, adv=None, force=None, n=1, kind="velocity", trimmed=False):
    ref_out, ref_g = mlc.reference(grid, adv, force, n, kind)[:2]
    out, grads = got
    ef = [rel(a, b) for a, b in zip(out, ref_out)]
    names = ["g_vy", "g_vx"] + (["g_d"] if kind == "density" or force is not None else [])
    idx = {"g_d": 0, "g_vy": 1, "g_vx": 2}
    eg = {k: mlc.grad_error(grads[idx[k]], ref_g[idx[k]], trimmed) for k in names}
    print("%s %dx%d: fields d %.3e vy %.3e vx %.3e; gradients %s" % ((what,) + tuple(grid) + tuple(ef) + (
        ", ".join("%s %.3e (%d left out)" % (k, v[0], v[1]) for k, v in eg.items()),)))
    assert max(ef) < TOL_FIELD, (what, grid, ef)
    assert max(v[0] for v in eg.values()) < TOL_GRAD, (what, grid, eg)
    assert all(float(grads[idx[k]].abs().max()) > 0 for k in names)


# ---- 1. plain physics: against the oracle and against the fused one-workgroup step --------------------------------------------------------
@pytest.mark.parametrize("grid", mlc.PLAIN, ids=ks.sid)
@pytest.mark.parametrize("one_wg", [0, 1])
def test_plain_step_and_adjoint_against_the_oracle_and_the_fused_step(grid, one_wg):
    """the multi-launch step (GEMM chain and one-launch solve) and its staged adjoint against karman2d_small_shapes' float64 recipe; the
    fused one-workgroup step on default masks agrees within 2 TOL_FIELD"""
    g, mk, cfg = setup(grid)
    assert mk.pressure_solver == "direct" and mk.coarse_inv is None
    with option("k2d_solve_one_wg", one_wg):
        got = hip_step_and_grads(grid, mk, cfg)
    check_case("plain multi_launch (one_wg %d)" % one_wg, grid, got)
    g, fmk, fcfg = setup(grid, multi_launch=False)
    fused = hip_step_and_grads(grid, fmk, fcfg, step=lambda *a: ops.karman_step(*a, fcfg, fmk))
    e = [rel(a, b) for a, b in zip(got[0] + got[1][1:3], fused[0] + fused[1][1:3])]
    print("multi_launch against fused %dx%d: d %.3e vy %.3e vx %.3e g_vy %.3e g_vx %.3e" % (tuple(grid) + tuple(e)))
    assert max(e) < 2 * TOL_FIELD, e


# ---- 2. MacCormack, buoyancy, substeps, and all three ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,adv,force,n", mlc.MAC,
                         ids=["%s_s%s_f%s_n%d" % (ks.sid(c[0]), c[1], "0" if c[2] is None else "1", c[3]) for c in mlc.MAC])
def test_the_options_against_the_reference(grid, adv, force, n):
    g, mk, cfg = setup(grid)
    assert mk.pressure_solver == "direct"
    got = hip_step_and_grads(grid, mk, cfg, adv, force, n)
    check_case("options", grid, got, adv, force, n, trimmed=adv is not None)
    # the forward step without autograd gives the same bits, and the one-launch solve the other order of the same sums
    _, _, st, _ = mlc.reference(grid, adv, force, n)
    with torch.no_grad():
        plain = ops.karman_step_large(*(f32(t) for t in st), cfg, mk, **physics_kw(adv, force, n))
        with option("k2d_solve_one_wg", 1 - _lib.get_option("k2d_solve_one_wg")):
            other = ops.karman_step_large(*(f32(t) for t in st), cfg, mk, **physics_kw(adv, force, n))
    assert all(torch.equal(a, b) for a, b in zip(plain, got[0]))
    assert max(rel(a, b) for a, b in zip(other, got[0])) < TOL_FIELD


def test_density_grad_under_mac_cormack():
    grid = (48, 32)
    g, mk, cfg = setup(grid)
    got = hip_step_and_grads(grid, mk, cfg, 1.0, kind="density")
    check_case("density_grad", grid, got, 1.0, kind="density", trimmed=True)


def test_re_grad_under_mac_cormack():
    grid = (48, 32)
    g, mk, cfg = setup(grid)
    got = hip_step_and_grads(grid, mk, cfg, 1.0, kind="re")
    check_case("re_grad", grid, got, 1.0, kind="re", trimmed=True)
    ref = mlc.reference(grid, 1.0, None, 1, "re")[1][3]
    e = rel(got[1][3], ref)
    print("g_re: rel %.3e" % e, got[1][3].tolist(), ref.tolist())
    assert e < TOL_GRAD


# ---- 3. the CG solve and the scattered direct solve -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,solver", [((96, 32), "cg"), ((16, 64), "auto")], ids=["96x32_cg", "16x64_no_obstacle"])
def test_cg_scenes(grid, solver):
    g, mk, cfg = setup(grid, solver)
    assert mk.pressure_solver == "cg" and mk.direct is None and mk.box is not None and mk.coarse_inv is None
    info = {}
    got = hip_step_and_grads(grid, mk, cfg, info=info)
    check_case("cg", grid, got)
    for k in ("iterations", "converged", "iterations_bwd", "converged_bwd"):
        assert info[k].shape == (B,), (k, info)
    assert info["converged"].tolist() == [1] * B and info["converged_bwd"].tolist() == [1] * B
    assert min(info["iterations"].tolist()) > 0


def test_cg_warm_start_rollout_runs_eagerly():
    grid = (96, 32)
    g, mk, cfg = setup(grid, "cg")
    net = sol_amd.model_mars_moon(cin=3, cout=2, seed=0)
    ro = sol_amd.LargeGridRollout(net, mk, B, grid[0], grid[1], g.dx, (0.2, 0.2), o.STD_RE, use_graph=False, cg_warm_start=True,
                                  multi_launch=True, cg_rtol=CG_RTOL)
    st = tuple(f32(t) for t in mlc.reference(grid)[2])
    its = ro.run(*st, 3)
    torch.cuda.synchronize()
    print("cg_warm_start iterations per step:", its.tolist())
    assert ro.cg_warm_start and ro.solve_info["converged"].tolist() == [[1] * B] * 3
    assert int(its[2].max()) <= int(its[0].max()) and all(bool(torch.isfinite(t).all()) for t in st[:3])


def test_direct_scattered():
    grid = mlc.SCATTERED_GRID
    g, mk, cfg = setup(grid, "direct_scattered")
    assert mk.pressure_solver == "direct_scattered" and mk.box is None
    got = hip_step_and_grads(grid, mk, cfg)
    check_case("direct_scattered", grid, got)


# ---- 4. LargeGridTrainer(multi_launch=True) ----------------------------------------------------------------------------------------------------
def net_of(p):
    net = sol_amd.model_mars_moon(cin=3, cout=2, seed=0)
    net.set_weights([q.detach().numpy() for q in p["params"]])
    return net


@pytest.mark.parametrize("grid,nb,any_width", [((64, 32), 2, False), ((96, 48), 1, True)], ids=["64x32", "96x48_any_width"])
def test_large_grid_trainer(grid, nb, any_width):
    """mars_moon, two unrolled steps, MacCormack + buoyancy + two diffusion substeps: loss, gradient and one Adam step against the float64
    unrolled loss; the captured step equals the eager one bit for bit"""
    Y, X = grid
    ms, lr = 2, 1e-4
    p = mlc.trainer_problem(Y, X, nb, ms)
    lref, steps_ref, gref, fin_ref = mlc.trainer_reference(p)
    kw = dict(any_width=any_width, multi_launch=True, buoyancy=p["force"], diffusion_substeps=p["n"], **MC)
    args = (f32(p["d"]), f32(p["vy"]), f32(p["vx"]), f32(p["re"]), f32(torch.stack(p["gt_vy"])), f32(torch.stack(p["gt_vx"])))
    if not any_width:
        with pytest.raises(ValueError, match="multi_launch"):          # the masks and the keyword must agree
            sol_amd.LargeGridTrainer(net_of(p), nb, Y, X, ms, mlc.TRAINER_STD_V, o.STD_RE, masks=setup(grid, multi_launch=False)[1], **kw)
    else:
        with pytest.raises(ValueError, match="X % 64 == 0"):            # a width the convolutions refuse needs any_width
            sol_amd.LargeGridTrainer(net_of(p), nb, Y, X, ms, mlc.TRAINER_STD_V, o.STD_RE, **dict(kw, any_width=False))
    net = net_of(p)
    te = sol_amd.make_trainer(net, None, nb, Y, X, ms, 100.0 / X, mlc.TRAINER_STD_V, o.STD_RE, use_graph=False, **kw)
    assert isinstance(te, sol_amd.LargeGridTrainer) and te.multi_launch
    loss = float(te.fwd_bwd(*args, want_final=True))
    assert te._mk.large and te._mk.multi_launch and te.pressure_solver_used == "direct"
    e_l, e_g = abs(loss - lref) / abs(lref), rel(te.grads, gref)
    e_s = [abs(a - b) / abs(b) for a, b in zip(te.loss_steps.tolist(), steps_ref)]
    e_f = [rel(a, b) for a, b in zip(te.final, fin_ref)]
    print("LargeGridTrainer(multi_launch) %dx%d vs float64: loss %.3e, per-step %s, gradient %.3e, final state %s" % (Y, X, e_l, e_s, e_g, e_f))
    assert e_l < TOL_FIELD and max(e_s) < TOL_FIELD and e_g < TOL_GRAD and max(e_f) < TOL_FIELD, (e_l, e_s, e_g, e_f)
    g_eager, l_eager = te.grads.clone(), te.loss_steps.clone()
    w0 = net.params.detach().double().cpu().numpy()
    te.apply_gradients(lr)
    torch.cuda.synchronize()
    want = mlc.adam_reference(w0, g_eager.double().cpu().numpy(), lr)
    # bound: the new parameter is stored in fp32, half an ulp of it at most (2^-24 |w| per entry), and the update's own arithmetic
    # (moments, square root, quotient, scale: fewer than sixteen fp32 roundings, 16 x 2^-24 < 1e-6 of the update)
    got = net.params.detach().double().cpu().numpy()
    err, bound = float(np.linalg.norm(got - want)), 2.0 ** -24 * float(np.linalg.norm(w0)) + 1e-6 * float(np.linalg.norm(want - w0))
    print("one Adam step: error %.3e of an update of %.3e (bound %.3e)" % (err, float(np.linalg.norm(want - w0)), bound))
    assert err <= bound and float(np.linalg.norm(got - w0)) > 0.5 * float(np.linalg.norm(want - w0))
    tg = sol_amd.LargeGridTrainer(net_of(p), nb, Y, X, ms, mlc.TRAINER_STD_V, o.STD_RE, **kw)
    lg = float(tg.fwd_bwd(*args))
    assert tg._graph is not None
    assert lg == loss and torch.equal(tg.grads, g_eager) and torch.equal(tg.loss_steps, l_eager)
    assert float(tg.fwd_bwd(*args)) == lg and torch.equal(tg.grads, g_eager)


# ---- 5. LargeGridRollout(multi_launch=True) ----------------------------------------------------------------------------------------------------
def test_large_grid_rollout():
    """64 x 32, four steps of MacCormack step + correction against the float64 roll-out; captured equals eager bit for bit"""
    Y, X, steps = 64, 32, 4
    p = mlc.trainer_problem(Y, X, B, 2, force=None, n=1)
    ref = mlc.rollout_reference(p, steps)
    g, mk, _ = setup((Y, X))
    with pytest.raises(ValueError, match="multi_launch"):
        sol_amd.LargeGridRollout(net_of(p), setup((Y, X), multi_launch=False)[1], B, Y, X, g.dx, mlc.TRAINER_STD_V, o.STD_RE, multi_launch=True, **MC)
    runs = []
    for use_graph in (True, False):
        ro = sol_amd.make_rollout(net_of(p), mk, B, Y, X, g.dx, mlc.TRAINER_STD_V, o.STD_RE, multi_launch=True, use_graph=use_graph, **MC)
        assert isinstance(ro, sol_amd.LargeGridRollout) and ro.multi_launch
        h = tuple(f32(p[k]) for k in ("d", "vy", "vx", "re"))
        ro.run(*h, steps)
        torch.cuda.synchronize()
        assert (ro._graph is not None) == use_graph
        errs = [rel(a, b) for a, b in zip(h[:3], ref)]
        print("LargeGridRollout(multi_launch, use_graph=%s) after %d steps: d %.3e vy %.3e vx %.3e" % ((use_graph, steps) + tuple(errs)))
        assert max(errs) < TOL_FIELD, errs
        runs.append(h[:3])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ---- 6. KarmanFlow and the torch op ---------------------------------------------------------------------------------------------------------------
def test_karman_flow_and_the_torch_op_give_the_ops_bits():
    grid = (48, 32)
    Y, X = grid
    g, mk, cfg = setup(grid)
    _, _, st, (_, wy, wx) = mlc.reference(grid, 1.0)
    d, vy, vx, re = (f32(t) for t in st)
    wy, wx = f32(wy), f32(wx)
    dom = fluid.Domain([Y, X], box=fluid.box[0:Y * g.dx, 0:X * g.dx])
    bcv, bcm = karman.velocity_bc_masks(Y, X, batch_size=B)
    h = torch_ops.register_scene(cfg, mk)
    sim = karman.KarmanFlow(multi_launch=True, **MC)

    def flow(d, vy, vx):
        vel = fluid.StaggeredGrid([vy.reshape(B, Y + 1, X, 1), vx.reshape(B, Y, X + 1, 1)])
        s = sim.step(fluid.Fluid(dom, density=d.reshape(B, Y, X, 1), velocity=vel, batch_size=B), re=re, res=X, velBCy=bcv, velBCyMask=bcm)
        return s.density.data.reshape(B, Y, X), s.velocity.data[0].data.reshape(B, Y + 1, X), s.velocity.data[1].data.reshape(B, Y, X + 1)

    def run(step):
        leaves = [t.clone().requires_grad_(True) for t in (vy, vx)]
        out = step(d, *leaves)
        ((out[1] * wy).sum() + (out[2] * wx).sum()).backward()
        return tuple(t.detach() for t in out) + tuple(t.grad for t in leaves)

    a = run(lambda *t: ops.karman_step_large(*t, re, cfg, mk, **MC))
    b = run(lambda *t: torch.ops.sol.karman_step_adv(*t, re, h, 1, 1.0, 1, False))
    c = run(flow)
    torch.cuda.synchronize()
    assert sim.pressure_solver_used == "direct" and np.array_equal(g.active, mk.active.cpu().numpy().reshape(Y, X))
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z) and bool(torch.isfinite(x).all())
    # without the flag the same flow still refuses the grid
    with pytest.raises(sol_amd.SolError, match="multi-launch"):
        karman.KarmanFlow(**MC).step(fluid.Fluid(dom, density=d.reshape(B, Y, X, 1).cpu().numpy(), velocity=np.zeros((B, Y + 1, X + 1, 2), np.float32),
                                                 batch_size=B), re=re, res=X, velBCy=bcv, velBCyMask=bcm)


# ---- 7. the scripts ----------------------------------------------------------------------------------------------------------------------------
def _script(name):
    import importlib.util
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    if sdir not in sys.path:
        sys.path.insert(0, sdir)
    spec = importlib.util.spec_from_file_location("sol_script_ml_" + name, os.path.join(sdir, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_scripts_record_multi_launch_and_pick_it_up(tmp_path):
    """karman.py -r 32 --advection mac_cormack --buoyancy 0.3 --multi-launch generates 64 x 32 frames (refused without the flag) and
    records it; karman_train.py takes it from the set and records it in dataStats.pickle; karman_apply.py takes it from there"""
    gen = ["-o", str(tmp_path / "set"), "-r", "32", "-t", "7", "-s", "0", "--advection", "mac_cormack", "--buoyancy", "0.3"]
    with pytest.raises(sol_amd.SolError, match="multi-launch"):
        _script("karman").main(["-o", str(tmp_path / "refused")] + gen[2:] + ["--re", "8e5"])
    runs = [_script("karman").main(gen + ["--re", str(r), "--multi-launch"]) for r in (8.0e5, 1.6e6)]
    with open(runs[0] + "/params.pickle", "rb") as f:
        pk = pickle.load(f)
    assert pk["multi_launch"] is True and pk["advection"] == "mac_cormack" and tuple(pk["buoyancy"]) == (0.3, 0.0)
    tf = str(tmp_path / "tf")
    loss = _script("karman_train").main(["--train", str(tmp_path / "set"), "-s", "1", "-n", "2", "-b", "1", "-t", "5", "-m", "2", "-e", "1",
                                         "--lr", "1e-4", "--tf", tf, "--seed", "0"])
    assert loss is not None and np.isfinite(loss)
    with open(tf + "/dataStats.pickle", "rb") as f:
        stats = pickle.load(f)
    assert stats["multi_launch"] is True and stats["advection"] == "mac_cormack" and tuple(stats["buoyancy"]) == (0.3, 0.0)
    out = _script("karman_apply").main(["-o", str(tmp_path / "apply"), "--stats", tf + "/dataStats.pickle", "--model", tf + "/model.pt",
                                        "-r", "32", "-s", "1", "-t", "4", "--re", "8e5", "--initdH", runs[0] + "/dens_000005.npz",
                                        "--initvH", runs[0] + "/velo_000005.npz"])
    from sol_amd import scene
    frames = [scene.read_zipped_array(os.path.join(out, "velTf_%06d.npz" % i)) for i in range(4)]
    assert all(np.isfinite(f).all() for f in frames) and np.abs(frames[3] - frames[0]).max() > 0
    # (without the path from dataStats.pickle make_rollout would have refused mac_cormack and the force on this grid)
    with open(out + "/params.pickle", "rb") as f:
        assert pickle.load(f)["multi_launch"] is False           # (the flag was not given: the path came from dataStats.pickle)
