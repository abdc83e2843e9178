"""The one-workgroup karman-2d step (csrc/karman_step.hip: k_karman_fwd / k_karman_bwd<CPT, SOLVER>, fd_solve_small, the density chain) at
every kind of grid check_cfg accepts (pytest -m gpu).  The rest of the suite runs these kernels at 16 x 8, 32 x 16, 64 x 32 and 128 x 64
only; the table in karman2d_small_shapes.py lists the grids that reach the other paths and says what each is there for, and
test_karman2d_small_shapes_cpu.py pins those claims and the refusals without a device.

Tolerances are the suite's: fields 1e-5, gradients 1e-4 relative L2, UNTRIMMED, against the float64 oracle and its autograd.  They bind
the kernel: at every row's state the float32 oracle alone stays within a quarter of each (karman2d_small_shapes.ORACLE_ALONE, pinned by
the CPU twin).  Every figure is printed before it is asserted."""
import os
import sys

import pytest
import torch

import sol_amd
import sol_oracle as o
from sol_amd import _lib, ops, trainer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import density_adjoint_cases as dac
import diffusion_substeps_cases as dc
import karman2d_small_shapes as ks
import re_adjoint_cases as rac
from karman2d_small_shapes import B, CG_RTOL, DEV, TOL_FIELD, TOL_GRAD, cotangent_at, f32, rel
from large2d_scenes import masks, state

pytestmark = pytest.mark.gpu
CG_MAX_ITER = 2000
CASES = [(c, s) for c in ks.ROWS for s in (("cg", "direct") if ks.ROWS[c][5] is not None else ("cg",))]


class forced_cpt:
    """sol_set_option("cpt", v) for the duration of a block"""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        _lib.set_option("cpt", self.v)

    def __exit__(self, *exc):
        _lib.set_option("cpt", 0)


def setup(c, solver, **kw):
    g = ks.geometry(c)
    mk = masks(g, solver)
    assert not mk.large and mk.pressure_solver == solver
    return g, mk, ops.karman_cfg(B, *c, g.dx, masks=mk, cg_rtol=CG_RTOL, cg_max_iter=CG_MAX_ITER, **kw)


def run_case(c, solver, what, grad_pad="replicate", inflow_order="after"):
    """one step and its adjoint through ops.karman_step + backward() against ks.reference -> info"""
    g, mk, cfg = setup(c, solver, grad_pad=grad_pad, inflow_order=inflow_order)
    ref_out, ref_g = ks.reference(c, grad_pad, inflow_order)
    d, vy, vx, re = ks.row_state(c)
    wy, wx = cotangent_at(B, *c)
    hy, hx = f32(vy).requires_grad_(True), f32(vx).requires_grad_(True)
    info = {}
    out = ops.karman_step(f32(d), hy, hx, f32(re), cfg, mk, info)
    ((out[1] * f32(wy)).sum() + (out[2] * f32(wx)).sum()).backward()
    torch.cuda.synchronize()
    fe = [rel(a, b) for a, b in zip(out, ref_out)]
    ge = [rel(a, b) for a, b in zip((hy.grad, hx.grad), ref_g)]
    its = (info["iterations"].tolist(), info["iterations_bwd"].tolist())
    print("%s %s %s: fields d %.2e vy %.2e vx %.2e, gradients g_vy %.2e g_vx %.2e, iterations fwd %s bwd %s"
          % (ks.sid(c), solver, what, *fe, *ge, *its))
    assert max(fe) < TOL_FIELD, (what, fe)
    assert max(ge) < TOL_GRAD, (what, ge)
    for it in its[0] + its[1]:
        assert it == 0 if solver == "direct" else 5 < it < CG_MAX_ITER, (what, its)
    return out


@pytest.fixture(scope="module", autouse=True)
def _library():
    sol_amd.load()
    assert torch.cuda.is_available() and _lib.get_option("cpt") == 0
    yield
    _lib.set_option("cpt", 0)


# ---- 1. forward and adjoint against the oracle, every row, every solver the row admits -------------------------------------------------
@pytest.mark.parametrize("c,solver", CASES, ids=["%s-%s" % (ks.sid(c), s) for c, s in CASES])
def test_step_and_adjoint_against_the_oracle(c, solver):
    run_case(c, solver, "default strip height (cpt %d)" % ks.ROWS[c][2 if solver == "direct" else 1])


@pytest.mark.parametrize("c", [(24, 16), (32, 64)], ids=ks.sid)
def test_dirichlet_gradient_padding_and_inflow_before(c):
    for solver in ("cg", "direct") if ks.ROWS[c][5] is not None else ("cg",):
        run_case(c, solver, "dirichlet0 / before", "dirichlet0", "before")


def test_a_scene_without_obstacle_is_cg_under_auto_and_direct_raises():
    g = ks.geometry((16, 64))
    assert masks(g, "auto").pressure_solver == "cg" and masks(g, "auto").direct is None
    with pytest.raises(ValueError, match="does not support this scene"):
        masks(g, "direct")


# ---- 2. both strip heights ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", ks.BOTH_CPT, ids=ks.sid)
@pytest.mark.parametrize("cpt", [8, 16])
def test_both_strip_heights_cg(c, cpt):
    with forced_cpt(cpt):
        run_case(c, "cg", "forced cpt %d" % cpt)


@pytest.mark.parametrize("c", ks.DIRECT_CPT16, ids=ks.sid)
def test_direct_solve_with_16_cell_strips(c):
    """fd_solve_small<16>: the direct small-grid solve under a forced strip height of 16 (its default is 8; only sol_set_option("cpt", 16)
    / SOL_CPT=16 reaches these instantiations).

    This test found a wrong adjoint: with k_karman_bwd<16, 2> holding both direct solvers, the forward met the oracle (fields 4e-8 ..
    3e-7, bit for bit the cpt-8 result) while the adjoint read g_vy / g_vx 1.16e-2 / 1.51e-2 at 48 x 32 and 4.21e-3 / 3.90e-3 at
    112 x 16 (0.2 .. 3 % on every small direct grid), where cpt 8 and CG at cpt 16 read 2e-7 .. 7e-7.  The kernel was mis-scheduled by the
    compiler's experimental scheduler strategy, not wrong in source (karman_step.hip, above karman_bwd_body); the kernels that run
    fd_solve_small are now built without that strategy (karman_step_small.hip).  Every row with a blob runs here."""
    with forced_cpt(16):
        run_case(c, "direct", "forced cpt 16")


# ---- 3. properties -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", list(ks.ROWS), ids=ks.sid)
def test_properties_batch_rows_repeat_inflow_and_closed_faces(c):
    g = ks.geometry(c)
    mk = masks(g, "auto")
    Y, X = c
    d, vy, vx, re = (f32(t) for t in ks.row_state(c, 3))
    step = lambda nb, *a: ops.karman_step(*a, ops.karman_cfg(nb, Y, X, g.dx, masks=mk, cg_rtol=CG_RTOL), mk)
    with torch.no_grad():
        full = step(3, d, vy, vx, re)
        again = step(3, d, vy, vx, re)
        rows = [step(1, d[b:b + 1].contiguous(), vy[b:b + 1].contiguous(), vx[b:b + 1].contiguous(), re[b:b + 1].contiguous()) for b in range(3)]
        zero = step(3, torch.zeros_like(d), vy, vx, re)
    torch.cuda.synchronize()
    for k in range(3):
        assert torch.equal(full[k], again[k]), "a second run differs"
        assert torch.equal(full[k], torch.cat([r[k] for r in rows])), "B = 3 differs from three B = 1 calls"
    assert bool(((d - d[0:1]).abs().amax(dim=(1, 2))[1:] > 0).all())          # the three simulations are different states
    assert torch.equal(zero[0], f32(g.inflow).expand(3, Y, X))               # dt = 1: density of a zero field is the inflow mask
    my, mx = f32(g.my), f32(g.mx)
    assert bool((full[1][:, my == 0] == 0).all()) and bool((full[2][:, mx == 0] == 0).all())      # faces closed by the obstacle
    if g.obstacle.any():
        assert int((my == 0).sum()) > 0 and int((mx == 0).sum()) > 0


# ---- 4. the opt-in features on non-2:1 grids ---------------------------------------------------------------------------------------------
def check_grads(names, got, ref, what):
    for name, a, b in zip(names, got, ref):
        e = rel(a, b)
        print("%s %s: rel L2 %.3e" % (what, name, e))
        assert e < TOL_GRAD, (what, name, e)


@pytest.mark.parametrize("c", ks.FEATURE_ROWS, ids=ks.sid)
@pytest.mark.parametrize("solver", ["direct", "cg"])
def test_density_gradient(c, solver):
    """density_grad=True (the staged density adjoint, csrc/karman_density_bwd.hip) with density and velocity cotangents together"""
    Y, X = c
    g = dac.scene(Y, X)
    mk = masks(g, solver)
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk, cg_rtol=CG_RTOL)
    ref_out, ref_g = dac.oracle_case(Y, X, B, with_velocity=True)
    st = state(B, Y, X, dac.SEED, g)
    hs = [f32(t).requires_grad_(True) for t in st[:3]]
    out = ops.karman_step(*hs, f32(st[3]), cfg, mk, density_grad=True)
    wy, wx = cotangent_at(B, Y, X)
    ((out[0] * f32(dac.w_dens(B, Y, X, g))).sum() + (out[1] * f32(wy)).sum() + (out[2] * f32(wx)).sum()).backward()
    torch.cuda.synchronize()
    what = "%s %s density_grad" % (ks.sid(c), solver)
    fe = [rel(a, b) for a, b in zip(out, ref_out)]
    print(what, "fields", fe)
    assert max(fe) < TOL_FIELD
    check_grads(("g_d", "g_vy", "g_vx"), [h.grad for h in hs], ref_g, what)


@pytest.mark.parametrize("c", ks.FEATURE_ROWS, ids=ks.sid)
@pytest.mark.parametrize("solver", ["direct", "cg"])
def test_reynolds_gradient(c, solver):
    """re_grad=True: the staged adjoint (sol_karman_step_bwd_large_re) on a one-workgroup grid, SceneMasks.staged_box() with CG"""
    Y, X = c
    g = rac.table_geometry("default", Y, X)
    mk = masks(g, solver)
    cfg = ops.karman_cfg(B, Y, X, g.dx, masks=mk, cg_rtol=CG_RTOL)
    ref = rac.oracle_case(Y, X, B)
    w = rac.cotangents(Y, X, B)
    hd, hy, hx, hre = (f32(t).requires_grad_(True) for t in state(B, Y, X, rac.SEED, g))
    info = {}
    out = ops.karman_step(hd, hy, hx, hre, cfg, mk, info, re_grad=True)
    ((out[1] * f32(w[1])).sum() + (out[2] * f32(w[2])).sum()).backward()
    torch.cuda.synchronize()
    what = "%s %s re_grad" % (ks.sid(c), solver)
    fe = [rel(a, b) for a, b in zip(out, ref["out"])]
    print(what, "fields", fe)
    assert max(fe) < TOL_FIELD
    if solver == "cg":
        assert bool(info["converged_bwd"].all()), info["iterations_bwd"].tolist()
    check_grads(("g_vy", "g_vx"), (hy.grad, hx.grad), ref["g"][1:], what)
    err = (hre.grad.double().cpu() - ref["g_re"]).abs()
    print("%s g_re %s, oracle %s, |difference| / S %s" % (what, hre.grad.tolist(), ref["g_re"].tolist(), (err / ref["S"]).tolist()))
    assert bool((err <= TOL_GRAD * ref["S"]).all())          # the bound of re_adjoint_cases.py


@pytest.mark.parametrize("c", ks.FEATURE_ROWS, ids=ks.sid)
def test_three_diffusion_substeps(c):
    Y, X = c
    n = dc.SMALL_N
    g, st = dc.small_state(Y, X)
    mk = masks(g)
    cfg = ops.karman_cfg(dc.B, Y, X, g.dx, masks=mk, cg_rtol=CG_RTOL)
    wy, wx = (f32(t) for t in dc.small_cotangents(Y, X))
    for re_grad in (False, True):
        ref_out, ref_g = dc.small_reference(Y, X, n, re_grad)
        d, vy, vx, re = (f32(t) for t in st)
        leaves = [t.requires_grad_(True) for t in ((vy, vx, re) if re_grad else (vy, vx))]
        out = ops.karman_step(d, vy, vx, re, cfg, mk, re_grad=re_grad, diffusion_substeps=n)
        ((out[1] * wy).sum() + (out[2] * wx).sum()).backward()
        torch.cuda.synchronize()
        what = "%s n=%d re_grad=%s" % (ks.sid(c), n, re_grad)
        fe = [rel(a, b) for a, b in zip(out, ref_out)]
        print(what, "fields", fe)
        assert max(fe) < TOL_FIELD
        check_grads(("g_vy", "g_vx", "g_re")[:len(leaves)], [t.grad for t in leaves], ref_g, what)


# ---- 5. training and roll-out --------------------------------------------------------------------------------------------------------------
def oracle_problem(Y, X, ms):
    g = o.geometry(Y, X)
    d, vy, vx = o.synthetic_state(B, Y, X, 1234)
    re = torch.tensor(o.RE_TRAIN[:B], dtype=torch.float64)
    gts = [o.synthetic_state(B, Y, X, 4321 + i, project_it=False) for i in range(ms)]
    params = [p.clone().requires_grad_(True) for p in o.init_params(0)]
    std_v = (0.2, 0.25)
    loss = o.unrolled_loss(params, d, vy, vx, re, [s[1] for s in gts], [s[2] for s in gts], g, std_v, o.STD_RE)
    loss.backward()
    return g, d, vy, vx, re, gts, params, std_v, loss


@pytest.mark.parametrize("c", ks.FEATURE_ROWS, ids=ks.sid)
def test_one_training_step(c):
    """make_trainer with mars_moon on a non-2:1 grid: SolTrainer (the C++ schedule), direct solve, and -- the fused adjoint +
    weight-gradient launch exists at 64 x 32 and 128 x 64 only -- the plain k_karman_bwd beside separate weight-gradient launches"""
    Y, X = c
    ms = 2
    g, d, vy, vx, re, gts, params, std_v, loss = oracle_problem(Y, X, ms)
    mk = masks(g)
    net = sol_amd.model_mars_moon(cin=3, cout=2, seed=0)
    net.set_weights([p.detach().numpy() for p in params])
    tr = trainer.make_trainer(net, mk, B, Y, X, ms, g.dx, std_v, o.STD_RE)
    assert type(tr).__name__ == "SolTrainer" and mk.pressure_solver == "direct"
    args = (f32(d), f32(vy), f32(vx), f32(re), f32(torch.stack([s[1] for s in gts])), f32(torch.stack([s[2] for s in gts])))
    with _lib.profile() as p:
        hl = tr.fwd_bwd(*args, eager=True)
        torch.cuda.synchronize()
    names = {k.strip("()"): v[0] for k, v in p.kernels.items()}
    gref = torch.cat([q.grad.reshape(-1) for q in params])
    le, ge = abs(float(hl) - float(loss)) / abs(float(loss)), rel(tr.grads, gref)
    print("%s training step: loss %.6f (oracle %.6f, rel %.2e), gradient rel L2 %.2e, kernels %s" % (ks.sid(c), float(hl), float(loss), le, ge, sorted(names)))
    assert le < 1e-5 and ge < TOL_GRAD
    assert names.get("k_karman_fwd") == ms and names.get("k_karman_bwd") == ms - 1, names           # the unfused adjoint
    assert "k_karman_bwd_bww_small" not in names and "k_karman_bwd_bww" not in names, names


def test_three_step_rollout():
    Y, X, n = 32, 64, 3
    g, d, vy, vx, re, gts, params, std_v, _ = oracle_problem(Y, X, 1)
    mk = masks(g)
    net = sol_amd.model_mars_moon(cin=3, cout=2, seed=0)
    net.set_weights([p.detach().numpy() for p in params])
    ro = trainer.make_rollout(net, mk, B, Y, X, g.dx, std_v, o.STD_RE)
    assert type(ro).__name__ == "SolRollout"
    hd, hy, hx = f32(d), f32(vy), f32(vx)
    its = ro.run(hd, hy, hx, f32(re), n)
    torch.cuda.synchronize()
    with torch.no_grad():
        rd, ry, rx = d, vy, vx
        for _ in range(n):
            rd, ry, rx = o.karman_step(rd, ry, rx, re, g)
            cy, cx = o.correction([p.detach() for p in params], ry, rx, re, std_v, o.STD_RE)
            ry, rx = ry + cy, rx + cx
    fe = [rel(hd, rd), rel(hy, ry), rel(hx, rx)]
    print("32x64 roll-out of %d steps: fields %s, iterations %s" % (n, fe, its.tolist()))
    assert its.shape == (n, B) and int(its.max()) == 0
    assert max(fe) < TOL_FIELD
