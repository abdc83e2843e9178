"""Periodic domain boundaries of karman-2d on the device (pytest -m gpu): the multi-launch step, its pressure solve, its adjoint, the
torch op, KarmanFlow, LargeGridTrainer and LargeGridRollout on scenes with a periodic axis, against the float64 reference of
periodic_cases (periodic_step: the oracle's step with wrapped indices, a float64 solve of precond.scene_matrix(active, periodic)).

Scenes (periodic_cases.SCENES): A x periodic, empty; B x periodic, interior box (one-window blob); C x periodic, a box across the seam
(direct_scattered); D y periodic, a box across the y seam, zero velBC; E doubly periodic, empty, zero velBC, no inflow.  Shapes: 16 x 16
(multi_launch, one adjoint tile), 40 x 24 (multi_launch, ragged), 130 x 65 (natively large, odd edges).  CFL about 0.8 and 2.5, one
forward case at CFL about X + 2 (departure points wrap more than once).
Tolerances are the project's (large2d_scenes): TOL_FIELD = 1e-5 on fields, TOL_GRAD = 1e-4 on gradients, relative L2; the CPU twin
test_karman2d_periodic_cpu.py holds the float32 reference alone to them at every case used here (no case needs the trimmed metric).
Every test that passes boundaries= fails on a library without the keyword with a TypeError.
Measured on an MI355X (printed by the tests): fields d 4.3e-8 ... 9.2e-8, v_y 3.1e-8 ... 3.9e-7, v_x 2.5e-7 ... 3.8e-6 (the largest: scene
B through the fp32 one-launch solve at CFL 2.5; with fp32 sums in the GEMM chain scenes A and C reached 1.05e-5 ... 1.32e-5 in v_x at CFL
2.5 -- DESIGN 4.5-4.7 says why the solve's products accumulate in fp64 on periodic blobs); CFL 18 on 16 cells 5.3e-7; solve 7.0e-8 ...
1.4e-6; scene E max|div| 1.2e-7 ... 9.3e-7 at max|v| 1.2 ... 15.5; gradients 1.5e-7 ... 5.5e-7 untrimmed; trainer loss 1.2e-7, per-step
5.4e-8 / 2.0e-7, weight gradient 2.3e-7, final state 6.9e-7; manual schedule against the autograd composition 1.7e-7 / 1.2e-7; roll-out
after three steps d 6.6e-8, v_y 6.4e-8, v_x 8.4e-7, captured = eager bit for bit."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

import sol_amd
import sol_oracle as o
from sol_amd import _lib, fluid, karman, ops, schedule2d, torch_ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import periodic_cases as pc
from large2d_scenes import DEV, TOL_FIELD, TOL_GRAD, check_grads, f32, rel, state as open_state

pytestmark = pytest.mark.gpu
B = pc.B
sid = lambda s: "%dx%d" % s
CASE_IDS = ["%s_%s" % (n, sid(s)) for n, s in pc.CASES]


@contextlib.contextmanager
def option(name, value):
    old = _lib.get_option(name)
    _lib.set_option(name, value)
    try:
        yield
    finally:
        _lib.set_option(name, old)


def setup(name, shape):
    Y, X = shape
    g, per = pc.scene_geometry(name, Y, X), pc.periodic_of(name)
    mk = ops.SceneMasks(g.active, g.inflow, g.bc_mask, g.bc_mask, DEV, pressure_solver=pc.SCENES[name][4],
                        multi_launch=not ops.beyond_one_workgroup(Y, X), boundaries=pc.SCENES[name][0])
    assert mk.large and mk.periodic == per
    return g, per, mk, ops.karman_cfg(B, Y, X, g.dx, masks=mk)


def dup_planes(vy, vx, per):
    return ([(vy[:, -1], vy[:, 0])] if per[0] else []) + ([(vx[:, :, -1], vx[:, :, 0])] if per[1] else [])


# ---- forward -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape", pc.CASES, ids=CASE_IDS)
@pytest.mark.parametrize("cfl", pc.CFLS)
def test_forward_step(name, shape, cfl):
    g, per, mk, cfg = setup(name, shape)
    ref_out, _, st, _, reached = pc.reference(name, shape, cfl)
    d, vy, vx, re = (f32(t) for t in st)
    with torch.no_grad():
        out = ops.karman_step_large(d, vy, vx, re, cfg, mk)
        (o2, svy, svx) = ops.karman_step_saved(d, vy, vx, re, cfg, mk)
        ny, nx = vy.clone(), vx.clone()
        for dup, _ in dup_planes(ny, nx, per):
            dup.fill_(float("nan"))
        poisoned = ops.karman_step_large(d, ny, nx, re, cfg, mk)
    torch.cuda.synchronize()
    errs = [rel(a, b) for a, b in zip(out, ref_out)]
    print("scene %s %s CFL %.2f (%s): d %.3e vy %.3e vx %.3e" % ((name, sid(shape), reached, mk.pressure_solver) + tuple(errs)))
    assert max(errs) < TOL_FIELD, errs
    for a, b in dup_planes(out[1], out[2], per) + dup_planes(svy, svx, per):
        assert torch.equal(a, b)                                                # the duplicate plane equals plane 0 bit for bit
    assert all(torch.equal(a, b) for a, b in zip(out, o2))                      # the training form runs the same launches
    assert all(torch.equal(a, b) for a, b in zip(out, poisoned))                # the input's duplicate plane is never read
    if name == "E":
        uy, ux = out[1][:, :-1].double(), out[2][:, :, :-1].double()
        div = (torch.roll(uy, -1, 1) - uy) + (torch.roll(ux, -1, 2) - ux)
        vmax = max(float(uy.abs().max()), float(ux.abs().max()))
        print("scene E %s: max|div| %.3e, max|v| %.3e" % (sid(shape), float(div.abs().max()), vmax))
        assert float(div.abs().max()) < TOL_FIELD * vmax


def test_departure_points_wrap_more_than_once():
    name, shape = "A", (16, 16)
    Y, X = shape
    g, per, mk, cfg = setup(name, shape)
    st, reached = pc.state(Y, X, pc.DEFAULT_SEED, name, cfl=X + 2)
    assert reached > X + 1.5
    with torch.no_grad():
        want = pc.periodic_step(*st, g, per)
        got = ops.karman_step_large(*(f32(t) for t in st), cfg, mk)
    torch.cuda.synchronize()
    errs = [rel(a, b) for a, b in zip(got, want)]
    print("scene A 16x16 at CFL %.2f (more than one period): d %.3e vy %.3e vx %.3e" % ((reached,) + tuple(errs)))
    assert max(errs) < TOL_FIELD, errs
    assert torch.equal(got[2][:, :, -1], got[2][:, :, 0])


# ---- the pressure solve ------------------------------------------------------------------------------------------------------------------------
def solve_case(name, shape):
    Y, X = shape
    g, per, mk, cfg = setup(name, shape)
    rhs = pc.periodic_rhs(name, Y, X)
    want = torch.as_tensor(pc.solver_of(g, per)(rhs.reshape(B, -1).numpy())).reshape(B, Y, X)
    got = ops.karman_pressure_solve_large(f32(rhs), cfg, mk).double().cpu()
    torch.cuda.synchronize()
    if name == "E":
        got = got - got.mean(dim=(1, 2), keepdim=True)
        want = want - want.mean(dim=(1, 2), keepdim=True)
    return rel(got, want), mk


@pytest.mark.parametrize("name,shape", pc.CASES, ids=CASE_IDS)
def test_pressure_solve(name, shape):
    e, mk = solve_case(name, shape)
    print("solve, scene %s %s (%s, nS %d): %.3e" % (name, sid(shape), mk.pressure_solver, int(mk.direct_header[5]), e))
    assert e < TOL_FIELD
    assert mk.pressure_solver == ("direct_scattered" if name in ("C", "D") else "direct")


@pytest.mark.parametrize("one_wg", [0, 1])
def test_pressure_solve_one_window_both_forms(one_wg):
    shape = (40, 24)
    mk = setup("B", shape)[2]
    assert int(mk.direct_header[ops.DIRECT_HEADER_FLAGS]) & ops.DIRECT_ONE_WG and ops.solve_one_wg_supported(*shape, int(mk.direct_header[7]))
    with option("k2d_solve_one_wg", one_wg):
        e, _ = solve_case("B", shape)
        ref_out, _, st, _, _ = pc.reference("B", shape, 0.8)
        g, per, mk, cfg = setup("B", shape)
        with torch.no_grad():
            out = ops.karman_step_large(*(f32(t) for t in st), cfg, mk)
    torch.cuda.synchronize()
    ef = max(rel(a, b) for a, b in zip(out, ref_out))
    print("scene B 40x24, k2d_solve_one_wg = %d: solve %.3e, step %.3e" % (one_wg, e, ef))
    assert e < TOL_FIELD and ef < TOL_FIELD


# ---- adjoint -------------------------------------------------------------------------------------------------------------------------------------
def adjoint(name, shape, cfl, wy=None, wx=None):
    g, per, mk, cfg = setup(name, shape)
    _, ref_g, st, w, _ = pc.reference(name, shape, cfl)
    d, vy, vx, re = (f32(t) for t in st)
    wy, wx = f32(w[0]) if wy is None else wy, f32(w[1]) if wx is None else wx
    with torch.no_grad():
        _, svy, svx = ops.karman_step_saved(d, vy, vx, re, cfg, mk)
        got = ops.karman_step_large_bwd(svy, svx, re, wy, wx, cfg, mk)
    torch.cuda.synchronize()
    return got, ref_g, per, (svy, svx, re, cfg, mk)


@pytest.mark.parametrize("name,shape", pc.CASES, ids=CASE_IDS)
@pytest.mark.parametrize("cfl", pc.CFLS)
def test_adjoint(name, shape, cfl):
    got, ref_g, per, (svy, svx, re, cfg, mk) = adjoint(name, shape, cfl)
    check_grads(got, ref_g, (name, shape, cfl) in pc.TRIMMED, "scene %s %s CFL %.1f" % (name, sid(shape), cfl))
    for dup, _ in dup_planes(got[0], got[1], per):
        assert float(dup.abs().max()) == 0.0                                    # the input gradient's duplicate plane: exactly zero
    assert all(float(t.abs().max()) > 0 for t in got)
    # two calls, and both settings of the scatter option (one form exists for periodic scenes): identical bits
    Y, X = shape
    wy, wx = (f32(t) for t in pc.cotangent_at(B, Y, X))
    with torch.no_grad():
        again = ops.karman_step_large_bwd(svy, svx, re, wy, wx, cfg, mk)
        with option("k2d_adj_tile", 1 - _lib.get_option("k2d_adj_tile")):
            other = ops.karman_step_large_bwd(svy, svx, re, wy, wx, cfg, mk)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(got, again, other))


@pytest.mark.parametrize("name,shape", [("A", (40, 24)), ("D", (40, 24)), ("E", (16, 16)), ("E", (130, 65))], ids=lambda v: v if isinstance(v, str) else sid(v))
def test_a_cotangent_on_the_duplicate_plane_is_one_on_plane_zero(name, shape):
    Y, X = shape
    per = pc.periodic_of(name)
    wy, wx = (f32(t) for t in pc.cotangent_at(B, Y, X, seed=5))
    on_dup = (torch.zeros_like(wy), torch.zeros_like(wx))
    on_zero = (torch.zeros_like(wy), torch.zeros_like(wx))
    if per[0]:
        on_dup[0][:, -1] = wy[:, -1]
        on_zero[0][:, 0] = wy[:, -1]
    if per[1]:
        on_dup[1][:, :, -1] = wx[:, :, -1]
        on_zero[1][:, :, 0] = wx[:, :, -1]
    a = adjoint(name, shape, 0.8, *on_dup)[0]
    b = adjoint(name, shape, 0.8, *on_zero)[0]
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and all(float(x.abs().max()) > 0 for x in a)


def test_the_torch_op_and_karman_flow_give_the_direct_call_gradient():
    name, shape = "A", (40, 24)
    Y, X = shape
    g, per, mk, cfg = setup(name, shape)
    direct, ref_g, _, _ = adjoint(name, shape, 0.8)
    _, _, st, w, _ = pc.reference(name, shape, 0.8)
    d, vy, vx, re = (f32(t) for t in st)
    wy, wx = f32(w[0]), f32(w[1])
    h = torch_ops.register_scene(cfg, mk)
    dom = fluid.Domain([Y, X], box=fluid.box[0:Y * g.dx, 0:X * g.dx], boundaries=pc.SCENES[name][0])
    bcv, bcm = g.bc_mask.reshape(1, Y + 1, X, 1), g.bc_mask.reshape(1, Y + 1, X, 1)
    sim = karman.KarmanFlow(multi_launch=True, obstacles=[])                    # boundaries=None: the domain's

    def flow(d, vy, vx):
        vel = fluid.StaggeredGrid([vy.reshape(B, Y + 1, X, 1), vx.reshape(B, Y, X + 1, 1)])
        s = sim.step(fluid.Fluid(dom, density=d.reshape(B, Y, X, 1), velocity=vel, batch_size=B), re=re, res=X, velBCy=bcv, velBCyMask=bcm)
        return s.density.data.reshape(B, Y, X), s.velocity.data[0].data.reshape(B, Y + 1, X), s.velocity.data[1].data.reshape(B, Y, X + 1)

    def run(step):
        leaves = [t.clone().requires_grad_(True) for t in (vy, vx)]
        out = step(d, *leaves)
        ((out[1] * wy).sum() + (out[2] * wx).sum()).backward()
        return tuple(t.grad for t in leaves)

    a = run(lambda *t: ops.karman_step_large(*t, re, cfg, mk))
    b = run(lambda *t: torch.ops.sol.karman_step(*t, re, h))
    c = run(flow)
    torch.cuda.synchronize()
    assert sim.pressure_solver_used == "direct" and sim._masks(dom, bcv, bcm, d.device).periodic == per
    for x, y, z, w_ in zip(direct, a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z) and torch.equal(x, w_)
    check_grads(c, ref_g, False, "KarmanFlow.step(...).backward(), scene A 40x24")


# ---- the seam entries ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", [(False, True), (True, False), (True, True)], ids=["x", "y", "yx"])
def test_seam_sync_and_fold(per):
    Y, X = 17, 23
    gen = torch.Generator().manual_seed(1)
    f = torch.float32                    # (spelled out: the process's default dtype is not this test's to assume)
    vy, vx = torch.randn(B, Y + 1, X, generator=gen, dtype=f), torch.randn(B, Y, X + 1, generator=gen, dtype=f)
    sy, sx = ops.karman_seam_sync(f32(vy), f32(vx), per)
    fy, fx = ops.karman_seam_fold(f32(vy), f32(vx), ops.periodic_bits(per))
    torch.cuda.synchronize()
    wy, wx, zy, zx = vy.clone(), vx.clone(), vy.clone(), vx.clone()
    if per[0]:
        wy[:, -1] = vy[:, 0]
        zy[:, 0] = vy[:, 0] + vy[:, -1]
        zy[:, -1] = 0
    if per[1]:
        wx[:, :, -1] = vx[:, :, 0]
        zx[:, :, 0] = vx[:, :, 0] + vx[:, :, -1]
        zx[:, :, -1] = 0
    for a, b in ((sy, wy), (sx, wx), (fy, zy), (fx, zx)):
        assert torch.equal(a.cpu(), b)
    # <sync(v), w> == <v, fold(w)>, and the autograd form is the pair
    a = f32(vy).requires_grad_(True), f32(vx).requires_grad_(True)
    oy, ox = ops.SeamSyncFn.apply(*a, ops.periodic_bits(per))
    (oy.sum() * 2.0 + ox.sum() * 3.0).backward()
    torch.cuda.synchronize()
    ey, ex = torch.full_like(vy, 2.0), torch.full_like(vx, 3.0)
    if per[0]:
        ey[:, 0], ey[:, -1] = 4.0, 0.0
    if per[1]:
        ex[:, :, 0], ex[:, :, -1] = 6.0, 0.0
    assert torch.equal(a[0].grad.cpu(), ey) and torch.equal(a[1].grad.cpu(), ex) and torch.equal(oy.detach().cpu(), wy)
    with pytest.raises(sol_amd.SolError, match="periodic_bits must be a combination"):
        ops.karman_seam_sync(f32(vy), f32(vx), 1)
    same = ops.karman_seam_sync(f32(vy), f32(vx), (False, False))          # an open scene has no seam
    assert torch.equal(same[0].cpu(), vy)


# ---- trainer and roll-out: scene A at 32 x 16, msteps = 2, mars_moon ---------------------------------------------------------------------------------
def net_of(p):
    net = sol_amd.model_mars_moon(cin=3, cout=2, seed=0)
    net.set_weights([q.detach().numpy() for q in p["params"]])
    return net


def trainer_masks(p):
    g = p["g"]
    return ops.SceneMasks(g.active, g.inflow, g.bc_mask, g.bc_mask, DEV, multi_launch=True, boundaries=ops.boundaries_name(p["periodic"]))


def test_large_grid_trainer_on_a_periodic_scene():
    Y, X = pc.TRAINER_GRID
    ms = pc.TRAINER_MS
    p = pc.trainer_problem()
    lref, steps_ref, gref, fin_ref = pc.trainer_reference(p)
    args = (f32(p["d"]), f32(p["vy"]), f32(p["vx"]), f32(p["re"]), f32(torch.stack(p["gt_vy"])), f32(torch.stack(p["gt_vx"])))
    kw = dict(multi_launch=True, any_width=schedule2d.row_pitch(Y, X) != X, obstacles=[])
    te = sol_amd.make_trainer(net_of(p), trainer_masks(p), B, Y, X, ms, 100.0 / X, pc.TRAINER_STD_V, o.STD_RE, use_graph=False, **kw)
    assert isinstance(te, sol_amd.LargeGridTrainer)
    loss = float(te.fwd_bwd(*args, want_final=True))
    assert te._mk.periodic == p["periodic"] and te.pressure_solver_used == "direct"
    e_l, e_g = abs(loss - lref) / abs(lref), rel(te.grads, gref)
    e_s = [abs(a - b) / abs(b) for a, b in zip(te.loss_steps.tolist(), steps_ref)]
    e_f = [rel(a, b) for a, b in zip(te.final, fin_ref)]
    print("LargeGridTrainer, periodic x, %dx%d vs float64: loss %.3e, per-step %s, gradient %.3e, final state %s" % (Y, X, e_l, e_s, e_g, e_f))
    assert e_l < TOL_FIELD and max(e_s) < TOL_FIELD and e_g < TOL_GRAD and max(e_f) < TOL_FIELD, (e_l, e_s, e_g, e_f)
    assert torch.equal(te.final[2][:, :, -1], te.final[2][:, :, 0])            # the seam sync ran after the last correction
    g_eager, l_eager = te.grads.clone(), te.loss_steps.clone()
    # captured replay (kernel nodes only) gives the eager bits, twice
    tg = sol_amd.LargeGridTrainer(net_of(p), B, Y, X, ms, pc.TRAINER_STD_V, o.STD_RE, masks=trainer_masks(p), **kw)
    lg = float(tg.fwd_bwd(*args))
    assert tg._graph is not None
    assert lg == loss and torch.equal(tg.grads, g_eager) and torch.equal(tg.loss_steps, l_eager)
    assert float(tg.fwd_bwd(*args)) == lg and torch.equal(tg.grads, g_eager)
    # the same unrolled loss composed by autograd from the differentiable ops: KarmanFlow.step, the network, to_staggered, the seam sync
    net = net_of(p)
    g = p["g"]
    dom = fluid.Domain([Y, X], box=fluid.box[0:Y * g.dx, 0:X * g.dx], boundaries=ops.boundaries_name(p["periodic"]))
    sim = karman.KarmanFlow(multi_launch=True, obstacles=[])
    bc = g.bc_mask.reshape(1, Y + 1, X, 1)
    stag = lambda vy, vx: torch.stack([_lib.pad_high(vy, 2), _lib.pad_high(vx, 1)], dim=-1)
    si = torch.tensor(list(pc.TRAINER_STD_V) + [o.STD_RE], dtype=torch.float32, device=DEV)
    so = torch.tensor(pc.TRAINER_STD_V, dtype=torch.float32, device=DEV)
    st = fluid.Fluid(dom, density=args[0].reshape(B, Y, X, 1), velocity=stag(args[1], args[2]), batch_size=B)
    losses = []
    for i in range(ms):
        st = sim.step(st, re=args[3], res=X, velBCy=bc, velBCyMask=bc)
        corr = karman.to_staggered(net(karman.to_feature(st, args[3]) / si) * so, dom.box)
        v = st.velocity + corr
        vy, vx = ops.SeamSyncFn.apply(v.data[0].data.reshape(B, Y + 1, X), v.data[1].data.reshape(B, Y, X + 1), te._mk.periodic_bits)
        st = st.copied_with(velocity=fluid.StaggeredGrid([vy.reshape(B, Y + 1, X, 1), vx.reshape(B, Y, X + 1, 1)], dom.box))
        losses.append(ops.l2_loss((vy, vx), (args[4][i], args[5][i]), tuple(float(s) for s in pc.TRAINER_STD_V)))
    total = torch.stack([l.reshape(()) for l in losses]).sum() / ms
    net.params.grad = None
    total.backward()
    torch.cuda.synchronize()
    e_al, e_ag = abs(float(total) - loss) / abs(loss), rel(net.params.grad, g_eager)
    print("manual schedule against the autograd composition: loss %.3e, gradient %.3e" % (e_al, e_ag))
    assert e_al < TOL_FIELD and e_ag < TOL_GRAD


def test_large_grid_rollout_on_a_periodic_scene():
    Y, X = pc.TRAINER_GRID
    steps = 3
    p = pc.trainer_problem()
    ref = pc.rollout_reference(p, steps)
    mk = trainer_masks(p)
    runs = []
    for use_graph in (True, False):
        ro = sol_amd.make_rollout(net_of(p), mk, B, Y, X, p["g"].dx, pc.TRAINER_STD_V, o.STD_RE, multi_launch=True, use_graph=use_graph,
                                  any_width=schedule2d.row_pitch(Y, X) != X)
        assert isinstance(ro, sol_amd.LargeGridRollout)
        h = tuple(f32(p[k]) for k in ("d", "vy", "vx", "re"))
        ro.run(*h, steps)
        torch.cuda.synchronize()
        assert (ro._graph is not None) == use_graph
        errs = [rel(a, b) for a, b in zip(h[:3], ref)]
        print("LargeGridRollout, periodic x (use_graph=%s) after %d steps: d %.3e vy %.3e vx %.3e" % ((use_graph, steps) + tuple(errs)))
        assert max(errs) < TOL_FIELD, errs
        assert torch.equal(h[2][:, :, -1], h[2][:, :, 0])
        runs.append(h[:3])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ---- defaults: boundaries="open" spelled out is the keyword left out ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(40, 24), (130, 65)], ids=sid)
def test_open_spelled_out_gives_the_default_bits(shape):
    Y, X = shape
    g = o.geometry(Y, X)
    ml = not ops.beyond_one_workgroup(Y, X)
    res = []
    for kw in ({}, {"boundaries": "open"}, {"boundaries": ("open", "open")}):
        mk = ops.SceneMasks(g.active, g.inflow, g.bc_mask, g.bc_mask, DEV, multi_launch=ml, **kw)
        cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk)
        d, vy, vx, re = (f32(t) for t in open_state(B, Y, X, 77, g))
        wy, wx = (f32(t) for t in pc.cotangent_at(B, Y, X))
        with torch.no_grad():
            out, svy, svx = ops.karman_step_saved(d, vy, vx, re, cfg, mk)
            res.append(tuple(out) + (svy, svx) + tuple(ops.karman_step_large_bwd(svy, svx, re, wy, wx, cfg, mk)))
    torch.cuda.synchronize()
    for other in res[1:]:
        assert all(torch.equal(a, b) for a, b in zip(res[0], other))
    want = o.karman_step(*open_state(B, Y, X, 77, g), g)
    assert max(rel(a, b) for a, b in zip(res[0][:3], want)) < TOL_FIELD


# ---- refusals that need the library ----------------------------------------------------------------------------------------------------------------
def test_the_library_refuses_what_is_not_built_for_periodic_scenes():
    name, shape = "A", (40, 24)
    Y, X = shape
    g, per, mk, cfg = setup(name, shape)
    d, vy, vx, re = (f32(t) for t in pc.reference(name, shape, 0.8)[2])
    outs, head = ops._step_fwd_args(d, vy, vx, re, cfg, mk)
    for ph in (ops.StepPhysics(adv=1.0), ops.StepPhysics(buoyancy=(0.3, 0.0))):             # (past the Python checks, straight to the entry points)
        with pytest.raises(sol_amd.SolError, match="periodic scenes run the plain step only"):
            ops._fwd_large(head, cfg, mk, ph, None, None)
    with torch.no_grad():
        _, svy, svx = ops.karman_step_saved(d, vy, vx, re, cfg, mk)
    with pytest.raises(sol_amd.SolError, match="periodic scenes run the plain velocity adjoint only"):
        ops._velocity_bwd("t", svy, svx, re, vy, vx, None, cfg, mk, ops.StepPhysics(), (vy, vx, None), None, None, False)
    # a periodic box blob handed to the CG entry points is refused, not iterated on
    from sol_amd import precond
    blob = precond.box_solver_blob(Y, X, per)
    cg = ops.SceneMasks(g.active, g.inflow, g.bc_mask, g.bc_mask, DEV, pressure_solver="cg", multi_launch=True)
    cg.box, cg.box_header = torch.from_numpy(blob).to(DEV), np.ascontiguousarray(blob[:16].view(np.int32))
    with pytest.raises(sol_amd.SolError, match="CG pressure solve is not built for periodic scenes"):
        ops.karman_step_large(d, vy, vx, re, ops.karman_cfg(B, Y, X, g.dx, masks=cg), cg)
    # the Python surface, with the library loaded
    with pytest.raises(sol_amd.SolError, match="density_grad is not built for periodic"):
        ops.karman_step_large(d, vy.clone().requires_grad_(True), vx, re, cfg, mk, density_grad=True)
    with pytest.raises(sol_amd.SolError, match="a buoyancy force is not built for periodic"):
        karman.KarmanFlow(multi_launch=True, obstacles=[], buoyancy=(0.3, 0.0), boundaries=pc.SCENES[name][0]).step(
            fluid.Fluid(fluid.Domain([Y, X], box=fluid.box[0:Y * g.dx, 0:X * g.dx]), density=d.reshape(B, Y, X, 1),
                        velocity=np.zeros((B, Y + 1, X + 1, 2), np.float32), batch_size=B),
            re=re, res=X, velBCy=g.bc_mask.reshape(1, Y + 1, X, 1), velBCyMask=g.bc_mask.reshape(1, Y + 1, X, 1))
    torch.cuda.synchronize()


# ---- the scripts ---------------------------------------------------------------------------------------------------------------------------------
def _script(name):
    import importlib.util
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    if sdir not in sys.path:
        sys.path.insert(0, sdir)
    spec = importlib.util.spec_from_file_location("sol_script_periodic_" + name, os.path.join(sdir, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_scripts_record_the_boundaries_and_pick_them_up(tmp_path):
    """karman.py -r 32 --multi-launch --boundaries periodic-x generates 64 x 32 frames with equal seam planes and records the boundaries
    (refused without --multi-launch); karman_train.py takes them from the set and records them in dataStats.pickle; karman_apply.py
    takes them from there; karman_fit_re.py refuses the set by name (re_grad)"""
    import pickle
    from sol_amd import scene
    gen = ["-o", str(tmp_path / "set"), "-r", "32", "-t", "7", "-s", "0", "--boundaries", "periodic-x"]
    with pytest.raises(ValueError, match="multi_launch=True"):
        _script("karman").main(["-o", str(tmp_path / "refused")] + gen[2:] + ["--re", "8e5"])
    runs = [_script("karman").main(gen + ["--re", str(r), "--multi-launch"]) for r in (8.0e5, 1.6e6)]
    with open(runs[0] + "/params.pickle", "rb") as f:
        pk = pickle.load(f)
    assert pk["boundaries"] == "periodic-x" and tuple(pk["scene"]["boundaries"]) == ("open", "periodic") and pk["multi_launch"] is True
    v = scene.read_zipped_array(os.path.join(runs[0], "velo_000005.npz"))
    assert np.isfinite(v).all() and np.array_equal(v[:, :-1, -1, 1], v[:, :-1, 0, 1])          # v_x: the duplicate plane is plane 0
    tf = str(tmp_path / "tf")
    loss = _script("karman_train").main(["--train", str(tmp_path / "set"), "-s", "1", "-n", "2", "-b", "1", "-t", "5", "-m", "2", "-e", "1",
                                         "--lr", "1e-4", "--tf", tf, "--seed", "0"])
    assert loss is not None and np.isfinite(loss)
    with open(tf + "/dataStats.pickle", "rb") as f:
        stats = pickle.load(f)
    assert stats["boundaries"] == "periodic-x" and tuple(stats["scene"]["boundaries"]) == ("open", "periodic")
    out = _script("karman_apply").main(["-o", str(tmp_path / "apply"), "--stats", tf + "/dataStats.pickle", "--model", tf + "/model.pt",
                                        "-r", "32", "-s", "1", "-t", "4", "--re", "8e5", "--initdH", runs[0] + "/dens_000005.npz",
                                        "--initvH", runs[0] + "/velo_000005.npz"])
    frames = [scene.read_zipped_array(os.path.join(out, "velTf_%06d.npz" % i)) for i in range(4)]
    assert all(np.isfinite(f).all() for f in frames) and np.abs(frames[3] - frames[0]).max() > 0
    assert np.array_equal(frames[3][:, :-1, -1, 1], frames[3][:, :-1, 0, 1])                   # the roll-out's seam sync
    with pytest.raises(sol_amd.SolError, match="re_grad is not built for periodic"):
        _script("karman_fit_re").main(["--input", runs[0], "-k", "3", "--iters", "1"])
