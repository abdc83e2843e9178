"""GPU tests of the karman-3d preconditioned CG pressure solve (pytest -m gpu): csrc/pcg.hip through the C ABI and
Scene3D(active=..., pressure_solver=...) against oracle/sol_oracle3d.py (float64: sparse LU on small grids, its own PCG
beyond) on the oracle's obstacles, against the direct solve where that builds, and held to properties where the oracle cannot
afford the size.  Tolerances as in test_gpu_karman3d.py: fields 1e-5, gradients 1e-4 relative L2."""
import os
import sys

import numpy as np
import pytest
import torch

import sol_oracle3d as o
from sol_amd import karman3d as k3

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_FIELD = 1e-5
TOL_GRAD = 1e-4


def rel(a, b):
    a = torch.as_tensor(np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a), dtype=torch.float64)
    b = torch.as_tensor(np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b), dtype=torch.float64)
    return float((a - b).norm() / (b.norm() + 1e-300))


def f32(t):
    return torch.as_tensor(np.asarray(t), dtype=torch.float32).to(DEV).contiguous()


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def scene(Y, X, Z, obstacle="cylinder", solver="auto"):
    g = o.geometry(Y, X, Z, obstacle=obstacle)
    return g, k3.Scene3D(Y, X, Z, device=DEV, active=g.active, inflow=g.inflow, pressure_solver=solver)


def interior_divergence(out, g):
    Y, X, Z = g.active.shape
    div = o.divergence(tuple(t.double().cpu() for t in out[1:]))
    inner = torch.zeros(Y, X, Z, dtype=torch.float64)
    inner[1:-1, 1:-1, 1:-1] = 1.0
    return float((div * inner * torch.as_tensor(g.active)).abs().max())


def assert_converged(sim, fwd=True, bwd=False):
    info = sim.solve_info
    if fwd:
        assert bool((info["converged"] == 1).all()), info
        assert int(info["iterations"].min()) >= 1, info
    if bwd:
        assert bool((info["converged_bwd"] == 1).all()), info
        assert int(info["iterations_bwd"].min()) >= 1, info


def test_cylinder_small_cg_against_oracle_and_direct():
    """32 x 16 x 16, B = 2, the extruded cylinder: the CG step against the float64 oracle (sparse LU), and against the direct solve
    on the same mask (which builds here) to fp32 round-off."""
    B, Y, X, Z = 2, 32, 16, 16
    g, sc = scene(Y, X, Z, solver="cg")
    assert sc.pressure_solver == "cg" and int(sc.direct_header[4]) == 0
    d, v = o.synthetic_state(B, Y, X, Z, 31)
    d, v = d.float().double(), tuple(c.float().double() for c in v)
    re = torch.tensor(o.RE_TRAIN[:B])
    with torch.no_grad():
        dr, vr = o.karman3d_step(d, v, re, g)
    sim = k3.Karman3DFlow(sc, B)
    out = sim.step(f32(d), f32(v[0]), f32(v[1]), f32(v[2]), f32(re))
    torch.cuda.synchronize()
    errs = [rel(a, b) for a, b in zip(out, (dr,) + tuple(vr))]
    assert max(errs) < TOL_FIELD, errs
    assert_converged(sim)
    assert sim.solve_info["iterations"].dtype == torch.int32 and sim.solve_info["iterations"].shape == (B,)
    _, sd = scene(Y, X, Z, solver="direct")
    assert sd.pressure_solver == "direct"
    outd = k3.Karman3DFlow(sd, B).step(f32(d), f32(v[0]), f32(v[1]), f32(v[2]), f32(re))
    torch.cuda.synchronize()
    errs = [rel(a, b) for a, b in zip(out, outd)]
    assert max(errs) < 2e-6, errs


@pytest.mark.timeout(900)
def test_sphere_full_size_cg_equals_direct_and_auto_is_unchanged():
    """configs[4] grid, the sphere: CG against the direct solve <= 1e-5; the default scene still picks the direct solve, and its step
    is bit-identical to an explicitly direct scene (existing behaviour is unchanged)."""
    from sol_amd import synthetic
    B, Y, X, Z = 1, 128, 64, 64
    gen = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)
    st = (torch.rand(B, Y, X, Z, generator=gen).to(DEV), (1.0 + 0.1 * rn(B, Y + 1, X, Z)).to(DEV), (0.1 * rn(B, Y, X + 1, Z)).to(DEV), (0.1 * rn(B, Y, X, Z + 1)).to(DEV))
    re = synthetic.reynolds(B).float().to(DEV)
    sc_default = k3.Scene3D(Y, X, Z, device=DEV)
    assert sc_default.pressure_solver == "direct"
    _, sc_direct = scene(Y, X, Z, "sphere", "direct")
    _, sc_cg = scene(Y, X, Z, "sphere", "cg")
    _, sc_auto = scene(Y, X, Z, "sphere", "auto")
    assert sc_auto.pressure_solver == "direct" and sc_cg.pressure_solver == "cg"
    with torch.no_grad():
        ref = k3.Karman3DFlow(sc_default, B).step(*st, re)
        dir_ = k3.Karman3DFlow(sc_direct, B).step(*st, re)
        sim = k3.Karman3DFlow(sc_cg, B)
        cg = sim.step(*st, re)
    torch.cuda.synchronize()
    for a, b in zip(ref, dir_):
        assert bool((bits(a) == bits(b)).all())
    errs = [rel(a, b) for a, b in zip(cg, ref)]
    assert max(errs) < TOL_FIELD, errs
    assert_converged(sim)


@pytest.mark.timeout(1200)
def test_cylinder_full_size_auto_picks_cg_against_oracle():
    """128 x 64 x 64 with the cylinder: the direct blob is refused (10 496 perturbed cells), "auto" runs CG; one step against the
    float64 oracle (its PCG), and the projected field is divergence free on interior active cells."""
    B, Y, X, Z = 1, 128, 64, 64
    g, sc = scene(Y, X, Z)
    assert sc.pressure_solver == "cg"
    with pytest.raises(ValueError, match="direct pressure solver does not support"):
        scene(Y, X, Z, solver="direct")
    d, v = o.synthetic_state(B, Y, X, Z, 1234)
    re = torch.tensor([o.RE_TRAIN[2]])
    with torch.no_grad():
        d1, v1 = o.karman3d_step(d, v, re, g)                     # spin-up: divergence free, consistent with the BCs
        d1, v1 = d1.float().double(), tuple(c.float().double() for c in v1)
        dr, vr = o.karman3d_step(d1, v1, re, g)
    sim = k3.Karman3DFlow(sc, B)
    out = sim.step(f32(d1), f32(v1[0]), f32(v1[1]), f32(v1[2]), f32(re))
    torch.cuda.synchronize()
    errs = [rel(a, b) for a, b in zip(out, (dr,) + tuple(vr))]
    assert max(errs) < TOL_FIELD, errs
    assert_converged(sim)
    resid = interior_divergence(out, g)
    assert resid < 2e-5, resid
    print("cylinder 128x64x64: CG iterations %d, rel errors %s, divergence residual %.2e" % (int(sim.solve_info["iterations"][0]), errs, resid))


@pytest.mark.parametrize("shape,kw", [((2, 16, 8, 8), {}), ((2, 16, 8, 8), dict(grad_pad="dirichlet0")), ((1, 32, 16, 16), {})])
def test_cylinder_cg_adjoint_against_oracle_autograd(shape, kw):
    B, Y, X, Z = shape
    g, sc = scene(Y, X, Z, solver="cg")
    d, v = o.synthetic_state(B, Y, X, Z, 13)
    v = tuple(c.float().double() for c in v)
    re = torch.tensor(o.RE_TRAIN[:B])
    gen = torch.Generator().manual_seed(3)
    w = [torch.randn(c.shape, generator=gen, dtype=torch.float64).float().double() for c in v]
    vr = tuple(c.clone().requires_grad_(True) for c in v)
    _, out = o.karman3d_step(d, vr, re, g, **kw)
    sum((a * b).sum() for a, b in zip(out, w)).backward()
    sim = k3.Karman3DFlow(sc, B, **kw)
    hv = [f32(c).requires_grad_(True) for c in v]
    hout = sim.step(f32(d), hv[0], hv[1], hv[2], f32(re))
    assert max(rel(a, b) for a, b in zip(hout[1:], out)) < TOL_FIELD
    sum((a * f32(b)).sum() for a, b in zip(hout[1:], w)).backward()
    torch.cuda.synchronize()
    errs = [rel(a.grad, b.grad) for a, b in zip(hv, vr)]
    assert max(errs) < TOL_GRAD, errs
    assert_converged(sim, fwd=True, bwd=True)


@pytest.mark.timeout(900)
def test_cylinder_full_size_cg_adjoint_by_finite_differences():
    """<J u, w> = <u, J^T w> for the CG step at 128 x 64 x 64 with the cylinder (HIP forward on both sides)."""
    from sol_amd import synthetic
    B, Y, X, Z = 1, 128, 64, 64
    _, sc = scene(Y, X, Z)
    assert sc.pressure_solver == "cg"
    sim = k3.Karman3DFlow(sc, B)
    gen = torch.Generator().manual_seed(23)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)
    st = (torch.rand(B, Y, X, Z, generator=gen).to(DEV), (1.0 + 0.1 * rn(B, Y + 1, X, Z)).to(DEV), (0.1 * rn(B, Y, X + 1, Z)).to(DEV), (0.1 * rn(B, Y, X, Z + 1)).to(DEV))
    re = synthetic.reynolds(B).float().to(DEV)
    with torch.no_grad():
        for _ in range(2):
            st = sim.step(*st, re)
    d0, v = st[0], [t.clone() for t in st[1:]]
    smooth = lambda t: torch.nn.functional.avg_pool3d(t[:, None], 5, 1, 2)[:, 0]
    u = [smooth(rn(*t.shape)).to(DEV) for t in v]
    w = [rn(*t.shape).to(DEV) for t in v]
    a = [t.clone().requires_grad_(True) for t in v]
    out = sim.step(d0, a[0], a[1], a[2], re)
    sum((o_ * w_).sum() for o_, w_ in zip(out[1:], w)).backward()
    assert_converged(sim, fwd=True, bwd=True)
    dot = lambda xs, ys: float(sum((x.double() * y.double()).sum() for x, y in zip(xs, ys)))
    rhs = dot([t.grad for t in a], u)
    res = {}
    for eps in (2e-2, 1e-2, 5e-3):
        with torch.no_grad():
            p = sim.step(d0, *[t + eps * du for t, du in zip(v, u)], re)[1:]
            m = sim.step(d0, *[t - eps * du for t, du in zip(v, u)], re)[1:]
        res[eps] = dot([x.double() - y.double() for x, y in zip(p, m)], w) / (2 * eps)
    torch.cuda.synchronize()
    scale = dot([t.grad for t in a], [t.grad for t in a]) ** 0.5 * dot(u, u) ** 0.5
    print("adjoint identity 3-D CG: <u, J^T w> = %.6e, <J u, w> by central differences %s, |u||J^T w| = %.3e" % (rhs, res, scale))
    assert min(abs(x - rhs) for x in res.values()) < 2e-3 * abs(rhs) + 2e-4 * scale, (rhs, res, scale)


@pytest.mark.parametrize("use_graph", [False, True])
def test_cylinder_trainer_sol2_against_oracle(use_graph):
    """SOL-2 at 32 x 16 x 16, B = 2, on the cylinder with the CG solve: loss and gradient against the float64 oracle, eager and
    as a replayed hipGraph (the CG launch sequence captures: no host synchronisation)."""
    import make_golden as mg
    B, Y, X, Z, ms = 2, 32, 16, 16, 2
    g, sc = scene(Y, X, Z, solver="cg")
    d, v = o.synthetic_state(B, Y, X, Z, 77)
    d, v = d.float().double(), tuple(c.float().double() for c in v)
    re = torch.tensor(o.RE_TRAIN[:B])
    gts = []
    for i in range(ms):
        _, gv = o.synthetic_state(B, Y, X, Z, 500 + i)
        gts.append(tuple(c.float().double() for c in gv))
    std_v = (0.2, 0.25, 0.3)
    params = [p.clone().requires_grad_(True) for p in mg.k3d_params()]
    loss = o.unrolled_loss(params, d, v, re, gts, g, std_v, o.STD_RE)
    loss.backward()
    gref = torch.cat([p.grad.reshape(-1) for p in params])
    net = k3.MarsMoon3D(device=DEV)
    net.set_weights([p.detach().numpy() for p in params])
    tr = k3.Karman3DTrainer(net, sc, B, ms, std_v, o.STD_RE, use_graph=use_graph)
    hl = tr.fwd_bwd(d, v[0], v[1], v[2], re, gts)
    if use_graph:
        assert tr._graph is not None
        tr._grads.zero_()
        hl = tr.fwd_bwd(d, v[0], v[1], v[2], re, gts)          # a pure replay
    torch.cuda.synchronize()
    assert abs(float(hl) - float(loss)) < 1e-5 * abs(float(loss)), (float(hl), float(loss))
    assert rel(tr.grads, gref) < TOL_GRAD, rel(tr.grads, gref)
    assert_converged(tr.sim, fwd=True, bwd=True)


@pytest.mark.timeout(1200)
def test_cylinder_full_size_trainer_replay_equals_eager():
    """SOL-2 at 128 x 64 x 64 with the cylinder (CG): the replayed graph equals the eager composition bit for bit (loss, gradient,
    final state), and two replays are bit-identical."""
    from sol_amd import synthetic
    B, Y, X, Z, ms = 1, 128, 64, 64, 2
    _, sc = scene(Y, X, Z)
    assert sc.pressure_solver == "cg"
    gen = torch.Generator().manual_seed(11)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)
    st = (torch.rand(B, Y, X, Z, generator=gen).to(DEV), (1.0 + 0.1 * rn(B, Y + 1, X, Z)).to(DEV), (0.1 * rn(B, Y, X + 1, Z)).to(DEV), (0.1 * rn(B, Y, X, Z + 1)).to(DEV))
    re = synthetic.reynolds(B).float().to(DEV)

    def make(use_graph):
        net = k3.MarsMoon3D(seed=3, device=DEV)
        w = net.get_weights()
        w[22] = w[22] * 0.01
        net.set_weights(w)
        return net, k3.Karman3DTrainer(net, sc, B, ms, (0.2, 0.2, 0.2), synthetic.STD_RE, use_graph=use_graph)

    net_g, tr_g = make(True)
    gts = []
    with torch.no_grad():
        st = tr_g.sim.step(*st, re)
        gs = (st[0], st[1] + 0.02, st[2], st[3])
        for _ in range(ms):
            gs = tr_g.sim.step(*gs, re)
            gts.append(tuple(t.clone() for t in gs[1:]))
    l1 = tr_g.fwd_bwd(*st, re, gts).clone()
    assert tr_g._graph is not None
    g1, f1 = tr_g.grads.clone(), [t.clone() for t in tr_g.final]
    tr_g._grads.zero_()
    l2 = tr_g.fwd_bwd(*st, re, gts).clone()
    torch.cuda.synchronize()
    assert bool((bits(l1) == bits(l2)).all()) and bool((bits(g1) == bits(tr_g.grads)).all()), "two replays differ"
    assert np.isfinite(float(l1)) and float(l1) > 0 and float(g1.abs().max()) > 0 and bool(torch.isfinite(g1).all())
    assert_converged(tr_g.sim, fwd=True, bwd=True)
    net_e, tr_e = make(False)
    le = tr_e.fwd_bwd(*st, re, gts)
    torch.cuda.synchronize()
    assert bool((bits(le) == bits(l1)).all()), (float(le), float(l1))
    assert bool((bits(tr_e.grads) == bits(g1)).all()), "replayed graph and eager composition give different gradients"
    for a, b in zip(tr_e.final, f1):
        assert bool((bits(a) == bits(b)).all())


def test_cylinder_cg_forward_and_adjoint_are_bit_reproducible():
    B, Y, X, Z = 1, 32, 16, 16
    _, sc = scene(Y, X, Z, solver="cg")
    d, v = o.synthetic_state(B, Y, X, Z, 41)
    re = f32(torch.tensor(o.RE_TRAIN[:B]))
    gen = torch.Generator().manual_seed(8)
    w = [f32(torch.randn(c.shape, generator=gen, dtype=torch.float64)) for c in v]
    runs = []
    for _ in range(2):
        sim = k3.Karman3DFlow(sc, B)
        hv = [f32(c).requires_grad_(True) for c in v]
        out = sim.step(f32(d), hv[0], hv[1], hv[2], re)
        sum((a * b).sum() for a, b in zip(out[1:], w)).backward()
        torch.cuda.synchronize()
        runs.append([t.detach().clone() for t in out] + [t.grad.clone() for t in hv] +
                    [sim.solve_info[k].clone() for k in ("iterations", "iterations_bwd")])
    for a, b in zip(*runs):
        assert torch.equal(bits(a) if a.dtype == torch.float32 else a, bits(b) if b.dtype == torch.float32 else b)


def test_cg_non_convergence_is_reported():
    """cg_max_iter = 1 on the cylinder: the report says not converged after one iteration, and the result (the last iterate) is finite."""
    B, Y, X, Z = 2, 32, 16, 16
    _, sc = scene(Y, X, Z, solver="cg")
    d, v = o.synthetic_state(B, Y, X, Z, 9)
    sim = k3.Karman3DFlow(sc, B, cg_max_iter=1)
    out = sim.step(f32(d), f32(v[0]), f32(v[1]), f32(v[2]), f32(torch.tensor(o.RE_TRAIN[:B])))
    torch.cuda.synchronize()
    assert sim.solve_info["converged"].tolist() == [0, 0], sim.solve_info
    assert sim.solve_info["iterations"].tolist() == [1, 1], sim.solve_info
    assert all(bool(torch.isfinite(t).all()) for t in out)
    # with the budget the report says converged, in fewer iterations than the budget
    sim2 = k3.Karman3DFlow(sc, B, cg_max_iter=300)
    sim2.step(f32(d), f32(v[0]), f32(v[1]), f32(v[2]), f32(torch.tensor(o.RE_TRAIN[:B])))
    assert_converged(sim2)
    assert int(sim2.solve_info["iterations"].max()) < 300


@pytest.mark.timeout(900)
def test_sphere_reference_resolution_forward_runs_on_cg():
    """256 x 128 x 128 (twice configs[4]), the sphere: 10 528 perturbed cells, the direct blob is refused, "auto" runs CG; two steps
    converge, the fields are finite and divergence free on interior active cells."""
    from sol_amd import synthetic
    B, Y, X, Z = 1, 256, 128, 128
    g, sc = scene(Y, X, Z, obstacle="sphere")
    assert sc.pressure_solver == "cg"
    sim = k3.Karman3DFlow(sc, B)
    gen = torch.Generator().manual_seed(2)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)
    st = (torch.rand(B, Y, X, Z, generator=gen).to(DEV), (1.0 + 0.1 * rn(B, Y + 1, X, Z)).to(DEV), (0.1 * rn(B, Y, X + 1, Z)).to(DEV), (0.1 * rn(B, Y, X, Z + 1)).to(DEV))
    re = synthetic.reynolds(B).float().to(DEV)
    with torch.no_grad():
        for _ in range(2):
            st = sim.step(*st, re)
            torch.cuda.synchronize()
            assert_converged(sim)
    assert all(bool(torch.isfinite(t).all()) for t in st)
    resid = interior_divergence(st, g)
    print("sphere 256x128x128: CG iterations %d, divergence residual %.2e" % (int(sim.solve_info["iterations"][0]), resid))
    assert resid < 2e-5, resid


def test_rollout_and_torch_op_on_a_cg_scene():
    """Karman3DRollout on the cylinder with the CG solve against the oracle's roll-out (one step: solver + network correction), and
    torch.ops.sol.karman3d_step on a CG scene equals the module-level step."""
    import make_golden as mg
    import sol_amd.torch_ops as tops
    B, Y, X, Z = 2, 32, 16, 16
    g, sc = scene(Y, X, Z, solver="cg")
    d, v = o.synthetic_state(B, Y, X, Z, 17)
    d, v = d.float().double(), tuple(c.float().double() for c in v)
    re = torch.tensor(o.RE_TRAIN[:B])
    params = mg.k3d_params()
    std_v, std_re = (0.2, 0.25, 0.3), o.STD_RE
    with torch.no_grad():
        dr, vr = o.rollout(params, d, v, re, g, std_v, std_re, 1)[-1]
    net = k3.MarsMoon3D(device=DEV)
    net.set_weights([p.numpy() for p in params])
    ro = k3.Karman3DRollout(net, sc, B, std_v, std_re)
    out = ro.run(f32(d), f32(v[0]), f32(v[1]), f32(v[2]), f32(re), 1)
    torch.cuda.synchronize()
    errs = [rel(a, b) for a, b in zip(out, (dr,) + tuple(vr))]
    assert max(errs) < TOL_FIELD, errs
    assert_converged(ro.sim)
    sim = k3.Karman3DFlow(sc, B)
    h = tops.register_scene3d(sim)
    res = []
    for use_op in (True, False):
        hv = [f32(c).requires_grad_(True) for c in v]
        o_ = torch.ops.sol.karman3d_step(f32(d), hv[0], hv[1], hv[2], f32(re), h) if use_op else sim.step(f32(d), hv[0], hv[1], hv[2], f32(re))
        (o_[1].sum() + 2 * o_[2].sum() - o_[3].sum()).backward()
        res.append(([t.detach() for t in o_], [t.grad for t in hv]))
    assert all(torch.equal(a, b) for a, b in zip(res[0][0], res[1][0]))
    assert all(torch.equal(a, b) for a, b in zip(res[0][1], res[1][1]))
    assert_converged(sim, fwd=True, bwd=True)


def test_karman3d_script_with_obstacle_mask_and_cg(tmp_path):
    """scripts/karman3d.py --obstacle-mask / --pressure-solver: frames of the cylinder scene at 16 x 8 x 8 with the CG solve."""
    import importlib.util
    import sol_amd
    from sol_amd import scene as sc_io
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    sys.path.insert(0, sdir)
    spec = importlib.util.spec_from_file_location("sol_script_karman3d_pcg", os.path.join(sdir, "karman3d.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mask = tmp_path / "cyl.npy"
    np.save(mask, o.geometry(16, 8, 8, obstacle="cylinder").active)
    outs = []
    for solver in ("cg", "direct"):
        out = mod.main(["-r", "8", "-t", "4", "--re", "1.6e5", "-o", str(tmp_path / solver), "--obstacle-mask", str(mask), "--pressure-solver", solver])
        outs.append(sc_io.read_zipped_array(out + "/velo_000003.npz"))
    assert outs[0].shape == (1, 17, 9, 9, 3) and np.isfinite(outs[0]).all()
    assert np.abs(outs[0] - outs[1]).max() < 1e-4 * np.abs(outs[1]).max()
    out = mod.main(["-r", "8", "-t", "4", "--re", "1.6e5", "-o", str(tmp_path / "sphere")])
    assert np.abs(sc_io.read_zipped_array(out + "/velo_000003.npz") - outs[0]).max() > 1e-3          # the mask acts
