"""karman-2d custom obstacles on the GPU (pytest -m gpu): the large-grid CG step (sol_karman_step_fwd_large_cg, csrc/pcg.hip) and
its solve alone against the float64 oracle with the scene's geometry, the default scene's direct path unchanged, reproducibility
(eager and captured), training / roll-out on a CG scene at 128 x 64, and the three scripts end to end with --obstacle.
Tolerances: fields 1e-5 relative L2, gradients 1e-4 (the suite's)."""
import glob
import importlib.util
import os
import pickle
import sys

import numpy as np
import pytest
import scipy.sparse.linalg as spla
import torch

import sol_amd
import sol_oracle as o
from sol_amd import fluid, karman, ops, precond

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from large2d_scenes import CG_RTOL, DEV, PLATE, TOL_FIELD, TOL_GRAD, TWO, active_of, f32, geometry, masks, rel, state

pytestmark = pytest.mark.gpu


def large_step(st, g, mk, info=None, **kw):
    d, vy, vx, re = st
    B, Y, X = d.shape
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk, **kw)
    with torch.no_grad():
        return ops.karman_step_large(f32(d), f32(vy), f32(vx), f32(re), cfg, mk, info=info)


def test_default_scene_cg_matches_direct_and_direct_is_unchanged():
    Y, X, B = 256, 128, 1
    g = o.KarmanGeometry(Y, X)
    st = state(B, Y, X, 5, g)
    m_def = ops.SceneMasks(g.active, g.inflow, g.bc_mask, g.bc_mask, DEV)
    m_auto, m_dir, m_cg = masks(g, "auto"), masks(g, "direct"), masks(g, "cg")
    assert m_def.pressure_solver == m_auto.pressure_solver == m_dir.pressure_solver == "direct" and m_cg.pressure_solver == "cg"
    out_dir = large_step(st, g, m_dir)
    for m in (m_def, m_auto):
        for a, b in zip(large_step(st, g, m), out_dir):
            assert torch.equal(a, b)
    info = {}
    out_cg = large_step(st, g, m_cg, info, cg_rtol=CG_RTOL)
    assert bool(info["converged"].all()) and int(info["iterations"].min()) >= 1
    for a, b in zip(out_cg, out_dir):
        assert rel(a, b) < TOL_FIELD, rel(a, b)
    # KarmanFlow's default scene keeps the direct path on the large grid
    dom = fluid.Domain([Y, X], box=fluid.box[0:200, 0:100])
    sim = karman.KarmanFlow()
    bcv, bcm = karman.velocity_bc_masks(Y, X, batch_size=B)
    fl = fluid.Fluid(dom, density=f32(st[0]).reshape(B, Y, X, 1), velocity=f32(o.staggered_tensor(st[1], st[2])), batch_size=B)
    with torch.no_grad():
        s2 = sim.step(fl, re=st[3].tolist(), res=X, velBCy=bcv, velBCyMask=bcm)
    assert sim.pressure_solver_used == "direct" and "converged" not in sim.solve_info
    assert torch.equal(s2.velocity.data[0].data.reshape(B, Y + 1, X), out_dir[1])


@pytest.mark.parametrize("specs", [TWO, PLATE], ids=["two_cylinders", "plate"])
def test_refused_scenes_run_cg_against_the_oracle(specs):
    Y, X, B = 256, 128, 2
    active = active_of(specs, Y, X)
    assert precond.direct_solver_blob(active, max_window=64) is None
    g = geometry(Y, X, active)
    mk = masks(g, "auto")
    assert mk.pressure_solver == "cg" and mk.direct is None
    d, vy, vx, re = state(B, Y, X, 11, g)
    hd, hy, hx = f32(d), f32(vy), f32(vx)
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk, cg_rtol=CG_RTOL)
    for _ in range(2):
        info = {}
        with torch.no_grad():
            hd, hy, hx = ops.karman_step_large(hd, hy, hx, f32(re), cfg, mk, info=info)
            d, vy, vx = o.karman_step(d, vy, vx, re, g)
        assert info["converged"].tolist() == [1] * B and int(info["iterations"].min()) >= 1, info
        for a, b in ((hd, d), (hy, vy), (hx, vx)):
            assert rel(a, b) < TOL_FIELD, rel(a, b)
        # interior cells (the box faces keep their boundary values: grad p is zero there with replicate padding)
        div = ((hy[:, 1:] - hy[:, :-1]) + (hx[:, :, 1:] - hx[:, :, :-1])).double().cpu().numpy()[:, 1:-1, 1:-1]
        inner = active[1:-1, 1:-1] != 0
        assert np.abs(div[:, inner]).max() < 1e-4 * float(hy.abs().max()), np.abs(div[:, inner]).max()


def test_pressure_solve_alone_and_the_budget_report():
    Y, X, B = 256, 128, 2
    active = active_of(TWO, Y, X)
    g = geometry(Y, X, active)
    mk = masks(g, "auto")
    _, vy, vx, _ = state(B, Y, X, 4)                     # the right-hand side the step sees: -div of an unprojected field
    rhs = -((vy[:, 1:] - vy[:, :-1]) + (vx[:, :, 1:] - vx[:, :, :-1]))
    rhs = rhs.float().double()
    lu = spla.splu((-g.pressure_matrix()).tocsc())
    ref = np.stack([lu.solve(r.numpy().ravel()).reshape(Y, X) for r in rhs])
    info = {}
    p = ops.pressure_solve_large(f32(rhs), ops.karman_cfg(B, Y, X, g.dx, masks=mk, cg_rtol=1e-7), mk, info=info)
    assert info["converged"].tolist() == [1] * B
    assert rel(p, ref) < TOL_FIELD, rel(p, ref)
    info2 = {}
    p2 = ops.pressure_solve_large(f32(rhs), ops.karman_cfg(B, Y, X, g.dx, masks=mk, cg_max_iter=2), mk, info=info2)
    assert info2["converged"].tolist() == [0] * B and info2["iterations"].tolist() == [2] * B
    assert bool(torch.isfinite(p2).all())


def test_cg_step_is_bit_reproducible_eager_and_captured():
    Y, X, B = 256, 128, 2
    active = active_of(PLATE, Y, X)
    g = geometry(Y, X, active)
    mk = masks(g, "auto")
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk, cg_max_iter=300)
    d, vy, vx, re = (f32(t) for t in state(B, Y, X, 7))
    ws = torch.empty((ops.large_workspace_bytes(cfg, mk) + 3) // 4, dtype=torch.float32, device=DEV)
    runs = []
    for _ in range(2):
        info = {}
        with torch.no_grad():
            out = ops.karman_step_large(d, vy, vx, re, cfg, mk, ws, info)
        runs.append([t.clone() for t in out] + [info["iterations"].clone(), info["converged"].clone()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert runs[0][-1].tolist() == [1] * B and int(runs[0][-2].max()) < 300
    # captured: the full budget of launches, the same bits
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    gr = torch.cuda.CUDAGraph()
    cap = {}
    with torch.cuda.stream(s), torch.no_grad():
        with torch.cuda.graph(gr, stream=s):
            out_c = ops.karman_step_large(d, vy, vx, re, cfg, mk, ws, cap)
    torch.cuda.current_stream().wait_stream(s)
    for t in list(out_c) + [cap["iterations"], cap["converged"]]:
        t.zero_()
    gr.replay()
    torch.cuda.synchronize()
    for a, b in zip(list(out_c) + [cap["iterations"], cap["converged"]], runs[0]):
        assert torch.equal(a, b)


def _custom_problem(Y, X, B, ms, active, mercury=False, seed=0):
    g = geometry(Y, X, active)
    d, vy, vx, re = state(B, Y, X, 31)
    with torch.no_grad():
        d, vy, vx = o.karman_step(d, vy, vx, re, g)           # spun up in the scene
    gts = []
    gd, gy, gx = d, vy, vx
    with torch.no_grad():
        for i in range(ms):
            gd, gy, gx = o.karman_step(gd, gy, gx, re, g)
            gts.append((gy * (1 + 0.05 * (i + 1)), gx * (1 - 0.05 * (i + 1))))
    params = [p.clone().requires_grad_(True) for p in (o.init_params_mercury(seed) if mercury else o.init_params(seed))]
    std_v = (0.2, 0.25)
    loss = o.unrolled_loss(params, d, vy, vx, re, [t[0] for t in gts], [t[1] for t in gts], g, std_v, o.STD_RE)
    loss.backward()
    args = (f32(d), f32(vy), f32(vx), f32(re), f32(torch.stack([t[0] for t in gts])), f32(torch.stack([t[1] for t in gts])))
    return g, args, params, std_v, float(loss), torch.cat([p.grad.reshape(-1) for p in params])


def test_training_and_rollout_on_a_cg_scene_at_128x64():
    Y, X, B, ms = 128, 64, 2, 2
    active = active_of(TWO, Y, X)
    # SOL-2, model_mars_moon: the C++ schedule on the scene's masks
    g, args, params, std_v, loss, gref = _custom_problem(Y, X, B, ms, active)
    mk = ops.SceneMasks(g.active, g.inflow, g.bc_mask, g.bc_mask)
    assert mk.direct is None and mk.pressure_solver == "cg"
    net = sol_amd.model_mars_moon(cin=3, cout=2, seed=0)
    net.set_weights([p.detach().numpy() for p in params])
    tr = sol_amd.make_trainer(net, mk, B, Y, X, ms, g.dx, std_v, o.STD_RE, obstacles=karman.parse_obstacles(TWO))
    assert isinstance(tr, sol_amd.SolTrainer)
    hl = float(tr.fwd_bwd(*args))
    assert abs(hl - loss) < 1e-5 * abs(loss), (hl, loss)
    assert rel(tr.grads, gref) < TOL_GRAD
    # model_mercury through GraphTrainer, both schedules, scene from the obstacle list (the caller's masks checked against it)
    g, args, params, std_v, loss, gref = _custom_problem(Y, X, B, ms, active, mercury=True, seed=1)
    for schedule in ("manual", "autograd"):
        net = sol_amd.model_mercury(cin=3, cout=2, seed=0)
        net.set_weights([p.detach().numpy() for p in params])
        tg = sol_amd.make_trainer(net, mk, B, Y, X, ms, g.dx, std_v, o.STD_RE, obstacles=karman.parse_obstacles(TWO), schedule=schedule)
        assert isinstance(tg, sol_amd.GraphTrainer)
        for _ in range(2):                                      # capture, then replay
            hl = float(tg.fwd_bwd(*args))
            assert abs(hl - loss) < 1e-5 * abs(loss), (schedule, hl, loss)
            assert rel(tg.grads, gref) < TOL_GRAD, (schedule, rel(tg.grads, gref))
    with pytest.raises(ValueError, match="different scene"):
        sol_amd.GraphTrainer(sol_amd.model_mercury(cin=3, cout=2, seed=0), B, Y, X, ms, std_v, o.STD_RE, masks=mk)
    # roll-out on the same scene
    B, n = 1, 3
    d, vy, vx, re = state(B, Y, X, 21)
    p3 = o.init_params(3)
    rd, ry, rx = d, vy, vx
    with torch.no_grad():
        for _ in range(n):
            rd, ry, rx = o.karman_step(rd, ry, rx, re, g)
            cy, cx = o.correction(p3, ry, rx, re, (0.2, 0.2), o.STD_RE)
            ry, rx = ry + cy, rx + cx
    ro = sol_amd.SolRollout(sol_amd.model_mars_moon(cin=3, cout=2, seed=3), mk, B, Y, X, g.dx, (0.2, 0.2), o.STD_RE)
    hd, hy, hx = f32(d), f32(vy), f32(vx)
    its = ro.run(hd, hy, hx, f32(re), n)
    assert int(its.min()) > 5
    assert rel(hy, ry) < TOL_FIELD and rel(hx, rx) < TOL_FIELD and rel(hd, rd) < TOL_FIELD


def test_scripts_end_to_end_with_obstacles(tmp_path):
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    sys.path.insert(0, sdir)

    def load(name):
        spec = importlib.util.spec_from_file_location("sol_script_obst_" + name, os.path.join(sdir, name + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m

    obst = sum([["--obstacle", s] for s in TWO], [])
    for re_nr in (1.6e5, 3.2e5):
        hi = load("karman").main(["-o", str(tmp_path / "hi"), "-r", "128", "-t", "7", "-s", "1", "--re", str(re_nr)] + obst)
    with open(hi + "/params.pickle", "rb") as f:
        rec = pickle.load(f)["scene"]
    assert rec == {"obstacles": TWO, "active": None}
    vel = sorted(glob.glob(hi + "/velo_0*.npz"))
    assert len(vel) == 5
    den = sorted(glob.glob(hi + "/dens_0*.npz"))
    lo = load("karman").main(["-o", str(tmp_path / "lo"), "-r", "32", "-t", "4", "-s", "0", "--initdH", den[-1], "--initvH", vel[-1],
                              "-d", "4"] + obst)
    assert len(glob.glob(lo + "/velo_0*.npz")) == 4
    # training at 64 x 32 on the down-sampled hi-res set: the scene comes from the set
    tf = str(tmp_path / "tf")
    loss = load("karman_train").main(["--train", str(tmp_path / "hi"), "-s", "4", "-n", "2", "-b", "2", "-t", "4", "-m", "2", "-e", "1",
                                      "--lr", "1e-4", "--tf", tf, "--seed", "0"])
    assert loss is not None and np.isfinite(loss)
    with open(tf + "/dataStats.pickle", "rb") as f:
        st = pickle.load(f)
    assert st["scene"] == rec and "std" in st and "ext.std" in st
    with pytest.raises(SystemExit, match="contradict"):
        load("karman_train").main(["--train", str(tmp_path / "hi"), "-s", "4", "-n", "2", "-b", "2", "-t", "4", "-m", "2", "-e", "1",
                                   "--tf", str(tmp_path / "tf2"), "--skip-ds", "--obstacle", "sphere:50,50,10"])
    out = load("karman_apply").main(["-r", "32", "-t", "3", "-o", str(tmp_path / "run"), "--stats", tf + "/dataStats.pickle",
                                     "--model", tf + "/model.pt"])
    from sol_amd import scene as sc
    last = sorted(glob.glob(out + "/velTf_0*.npz"))[-1]
    v = sc.read_zipped_array(last)
    cor = sc.read_zipped_array(last.replace("velTf", "corTf"))
    # the roll-out ran in the training scene: the uncorrected step (velTf - corTf) closes the y faces inside the SECOND cylinder
    act = active_of(TWO, 64, 32)
    inner = (act[1:, :] == 0) & (act[:-1, :] == 0)
    inner[:30] = False                                   # (rows of the first cylinder: closed in the default scene too)
    assert inner.any() and np.abs((v - cor)[0, 1:64, :32, 0][inner]).max() == 0.0
