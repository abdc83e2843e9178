"""Periodic domain boundaries of karman-2d, the part that needs no device: the float64 reference of the GPU tests
(periodic_cases.periodic_step) tied to the oracle, the Hartley tables, every solver blob through its float64 reference against the dense
solve of precond.scene_matrix(active, periodic), the default blobs unchanged, translation equivariance of the reference, the gradient
cases of test_gpu_karman2d_periodic.py measured in float32 against float64, argument handling and the refusals.

Figures measured here (float32 reference against float64 reference, seed 77 throughout; printed by the tests): fields 2.3e-7 ... 2.2e-6,
gradients 1.3e-7 ... 2.8e-7 untrimmed at every case (periodic_cases.TRIMMED is empty: no case needs the trimmed metric; at most 17 of 17030
entries would be left out under its cap); the CFL 18 case 5.2e-7; trainer loss / final state 6.9e-7, weight gradient 3.3e-7, roll-out
after three steps 8.3e-7; every blob through its float64 reference against the dense solve 1.1e-15 ... 2.1e-14 (bound 1e-9)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import sol_oracle as o
from sol_amd import _lib, fluid, karman, ops, precond, trainer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import periodic_cases as pc
from large2d_scenes import TOL_FIELD, TOL_GRAD, TRIM, rel, state, trimmed_rel

OP, PE = "open", "periodic"
BLOB_SHAPES = [(16, 16), (24, 16), (20, 17), (40, 24)]
sid = lambda s: "%dx%d" % s


def masks_of(g, **kw):
    return ops.SceneMasks(g.active, g.inflow, g.bc_mask, g.bc_mask, "cpu", **kw)


# ---- the reference is the oracle's step where nothing is periodic ---------------------------------------------------------------------------
def test_the_reference_with_open_axes_is_the_oracle_step():
    g = o.geometry(32, 16)
    st = state(2, 32, 16, 77, g)
    for kw in ({}, {"grad_pad": "dirichlet0"}, {"inflow_order": "before"}):
        want = o.karman_step(*st, g, **kw)
        got = pc.periodic_step(*st, g, (False, False), **kw)
        for a, b in zip(got, want):
            assert float((a - b).abs().max()) < 1e-12, kw


# ---- Hartley tables ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 17, 24, 65])
def test_hartley_matrix_is_symmetric_involutory_and_diagonalises_the_periodic_second_difference(n):
    H = precond.hartley_matrix(n)
    assert np.abs(H - H.T).max() < 1e-12 and np.abs(H @ H - np.eye(n)).max() < 1e-12
    T = 2 * np.eye(n) - np.roll(np.eye(n), 1, 0) - np.roll(np.eye(n), -1, 0)
    lam = 2 - 2 * np.cos(2 * np.pi * np.arange(n) / n)
    assert np.abs(H @ T @ H - np.diag(lam)).max() < 1e-12


# ---- solver blobs -----------------------------------------------------------------------------------------------------------------------------
def dense_solve(active, per, b):
    M = precond.scene_matrix(active, per)
    Bn = b.shape[0]
    r = b.reshape(Bn, -1).T
    if all(per):
        x = np.linalg.lstsq(M, r - r.mean(0, keepdims=True), rcond=None)[0]
        x = x - x.mean(0, keepdims=True)
    else:
        x = np.linalg.solve(M, r)
    return x.T.reshape(b.shape)


def relerr(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


BLOB_CASES = [(bnd, kind) for bnd in ((OP, PE), (PE, OP)) for kind in ("none", "interior", "seam")] + [((PE, PE), "none")]


@pytest.mark.parametrize("shape", BLOB_SHAPES, ids=sid)
@pytest.mark.parametrize("bnd,kind", BLOB_CASES, ids=lambda v: v if isinstance(v, str) else "%s_%s" % v)
def test_every_blob_solves_the_periodic_scene_matrix(shape, bnd, kind):
    Y, X = shape
    per = ops.boundaries_arg(bnd)
    active = pc.scene_active({"seam": "seam_x" if per[1] else "seam_y"}.get(kind, kind), Y, X)
    b = pc.field_rhs(active, per, Y, X).numpy()
    want = dense_solve(active, per, b)
    f64 = np.float64
    blobs = {}
    if kind == "none":
        assert precond._perturbation(active, per) == {}
        blobs["box"] = (precond.box_solver_blob(Y, X, per, dtype=f64), precond.box_solve_reference)
        blobs["empty periodic direct"] = (precond.direct_solver_blob(active, 64, per, dtype=f64), precond.direct_solve_reference)
        assert precond.scattered_solver_blob(active, periodic=per) is None
        dev = precond.direct_solver_blob(active, 64, per)               # the device blob: the box blob, nS = 0, the axes in word 8
        assert np.array_equal(dev.view(np.uint32), precond.box_solver_blob(Y, X, per).view(np.uint32))
        hdr = dev[:16].view(np.int32)
        assert tuple(hdr[:8]) == (precond.FD_MAGIC, Y, X, 0, 0, 0, 0, 0) and hdr[8] == ops.periodic_bits(per)
    elif kind == "interior":
        blobs["one window"] = (precond.direct_solver_blob(active, 64, per, dtype=f64), precond.direct_solve_reference)
        blobs["scattered"] = (precond.scattered_solver_blob(active, f64, per), precond.scattered_solve_reference)
        assert precond.direct_solver_blob(active, 64, per)[:16].view(np.int32)[8] == ops.periodic_bits(per)
    else:
        # across the seam the support set spans the whole axis: the window form takes it only where a window covers that axis
        n = X if per[1] else Y
        one = precond.direct_solver_blob(active, 64, per, dtype=f64)
        assert (one is None) == (n not in (16, 32, 64)), (n, one is None)
        if one is not None:
            blobs["one window (whole axis)"] = (one, precond.direct_solve_reference)
        blobs["scattered"] = (precond.scattered_solver_blob(active, f64, per), precond.scattered_solve_reference)
        hdr = precond.scattered_solver_blob(active, periodic=per)[:16].view(np.int32)
        assert hdr[0] == precond.FDS_MAGIC and hdr[9] == ops.periodic_bits(per)
    for name, (blob, ref) in blobs.items():
        assert blob is not None, name
        assert precond.blob_periodic(blob) == per
        got = np.stack([ref(blob, b[i]) for i in range(b.shape[0])])
        e = relerr(got, want)
        print("%s %s %s %s: %.3e" % (sid(shape), bnd, kind, name, e))
        assert e < 1e-9, (name, e)


def test_a_doubly_periodic_obstacle_is_refused():
    active = pc.scene_active("interior", 16, 16)
    for fn in (lambda: precond.direct_solver_blob(active, 64, (True, True)), lambda: precond.scattered_solver_blob(active, periodic=(True, True))):
        with pytest.raises(ValueError, match="doubly periodic scene must be empty"):
            fn()
    g = pc.geometry(16, 16, active)
    with pytest.raises(ValueError, match="doubly periodic scene must be empty"):
        masks_of(g, multi_launch=True, boundaries="periodic")


def test_default_blobs_do_not_move():
    for Y, X in ((48, 32), (130, 65)):
        act = np.asarray(o.geometry(Y, X).active)
        eq = lambda a, b: np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert eq(precond.direct_solver_blob(act, 64), precond.direct_solver_blob(act, 64, periodic=(False, False)))
        assert eq(precond.box_solver_blob(Y, X), precond.box_solver_blob(Y, X, periodic=(False, False)))
        assert eq(precond.scattered_solver_blob(act), precond.scattered_solver_blob(act, periodic=(False, False)))
        assert np.array_equal(precond.scene_matrix(act), precond.scene_matrix(act, (False, False))) if Y == 48 else True
        assert precond._perturbation(act) == precond._perturbation(act, (False, False))
        # the open expressions, bit for bit: the tables are the sine transform's and every flag word is zero
        blob = precond.direct_solver_blob(act, 64)
        assert blob[:16].view(np.int32)[8] == 0 and precond.scattered_solver_blob(act)[:16].view(np.int32)[9] == 0
        assert np.array_equal(blob[16:16 + Y * Y], precond.dst_matrix(Y).astype(np.float32).ravel())
    assert precond.direct_solver_blob(np.ones((32, 32)), 64) is None            # an empty OPEN scene still has no direct blob
    g = o.geometry(64, 32)
    a, b = masks_of(g, multi_launch=True), masks_of(g, multi_launch=True, boundaries="open")
    assert a.periodic == b.periodic == (False, False) and a.periodic_bits == 0
    assert np.array_equal(a.direct.numpy().view(np.uint32), b.direct.numpy().view(np.uint32)) and np.array_equal(a.direct_header, b.direct_header)


# ---- translation equivariance of the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape", [("A0", (24, 16)), ("E", (16, 16))])
def test_the_reference_commutes_with_a_roll_along_a_periodic_axis(name, shape):
    Y, X = shape
    g, per = pc.scene_geometry(name, Y, X), pc.periodic_of(name)
    (d, vy, vx, re), _ = pc.state(Y, X, 77, name, cfl=2.5)
    sh = (5 if per[0] else 0, 5 if per[1] else 0)
    roll = lambda t: torch.roll(t, sh, (1, 2))
    uy, ux = pc.unique(vy, vx, per)
    ry, rx = pc.with_duplicates(roll(uy), roll(ux), per)
    out = pc.periodic_step(d, vy, vx, re, g, per)
    out_r = pc.periodic_step(roll(d), ry, rx, re, g, per)
    assert float((roll(out[0]) - out_r[0]).abs().max()) < 1e-12
    for a, b in zip(pc.unique(out[1], out[2], per), pc.unique(out_r[1], out_r[2], per)):
        assert float((roll(a) - b).abs().max()) < 1e-12
    # and the duplicate planes of the output equal plane 0; a NaN in the input's changes nothing
    if per[0]:
        assert torch.equal(out[1][:, -1], out[1][:, 0])
    if per[1]:
        assert torch.equal(out[2][:, :, -1], out[2][:, :, 0])
    ny, nx = vy.clone(), vx.clone()
    if per[0]:
        ny[:, -1] = float("nan")
    if per[1]:
        nx[:, :, -1] = float("nan")
    for a, b in zip(pc.periodic_step(d, ny, nx, re, g, per), out):
        assert torch.equal(a, b)


def test_the_doubly_periodic_reference_is_divergence_free():
    Y, X = 16, 16
    out = pc.reference("E", (Y, X), 2.5)[0]
    uy, ux = pc.unique(out[1], out[2], (True, True))
    div = (torch.roll(uy, -1, 1) - uy) + (torch.roll(ux, -1, 2) - ux)
    assert float(div.abs().max()) < 1e-12 * max(float(uy.abs().max()), float(ux.abs().max()), 1.0)


# ---- the GPU tests' gradient cases, float32 against float64 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape", pc.CASES, ids=lambda v: v if isinstance(v, str) else sid(v))
@pytest.mark.parametrize("cfl", pc.CFLS)
def test_the_gradient_cases_in_float32_hold_the_tolerances(name, shape, cfl):
    assert TRIM == 1e-3 and TOL_GRAD == 1e-4 and TOL_FIELD == 1e-5
    o64, g64 = pc.reference(name, shape, cfl)[:2]
    o32, g32 = pc.reference(name, shape, cfl, torch.float32)[:2]
    ef = max(rel(a, b) for a, b in zip(o32, o64))
    trimmed = (name, shape, cfl) in pc.TRIMMED
    worst = 0.0
    for a, b in zip(g32, g64):
        full = rel(a, b)
        v, k, _ = trimmed_rel(a, b)
        print("float32 against float64, scene %s %s cfl %.1f seed %d: fields %.3e, gradient %.3e untrimmed, %.3e with %d of %d left out"
              % (name, sid(shape), cfl, pc.seed_of(name, shape, cfl), ef, full, v, k, b.numel()))
        assert k <= int(TRIM * b.numel())
        worst = max(worst, v if trimmed else full)
        if not trimmed:
            assert full < TOL_GRAD, "list the case in periodic_cases.TRIMMED or change its seed"
    assert ef < TOL_FIELD and worst < TOL_GRAD


def test_the_wrap_twice_case_reaches_its_cfl():
    X = 16
    (d, vy, vx, re), reached = pc.state(16, X, 77, "A", cfl=X + 2)
    assert X + 1.5 < reached < X + 2.5
    o64 = pc.periodic_step(d, vy, vx, re, pc.scene_geometry("A", 16, X), pc.periodic_of("A"))
    o32 = pc.periodic_step(d.float(), vy.float(), vx.float(), re.float(), pc.scene_geometry("A", 16, X), pc.periodic_of("A"))
    e = max(rel(a, b) for a, b in zip(o32, o64))
    print("wrap-twice case, float32 against float64: %.3e at CFL %.2f" % (e, reached))
    assert e < TOL_FIELD


def test_the_trainer_and_rollout_references_in_float32_hold_the_tolerances():
    p = pc.trainer_problem()
    l64, s64, g64, f64 = pc.trainer_reference(p)
    l32, s32, g32, f32 = pc.trainer_reference(p, torch.float32)
    ef = max([abs(l32 - l64) / abs(l64)] + [abs(a - b) / abs(b) for a, b in zip(s32, s64)] + [rel(a, b) for a, b in zip(f32, f64)])
    eg = rel(g32, g64)
    er = max(rel(a, b) for a, b in zip(pc.rollout_reference(p, 3, torch.float32), pc.rollout_reference(p, 3)))
    print("trainer reference float32 against float64: loss / final state %.3e, weight gradient %.3e; roll-out after three steps %.3e" % (ef, eg, er))
    assert ef < TOL_FIELD and eg < TOL_GRAD and er < TOL_FIELD
    # the seam sync is part of the composed reference: the final state's duplicate plane equals plane 0
    assert torch.equal(f64[2][:, :, -1], f64[2][:, :, 0])


# ---- argument handling -------------------------------------------------------------------------------------------------------------------------
def test_boundaries_arg():
    assert ops.boundaries_arg("open") == (False, False) and ops.boundaries_arg("periodic") == (True, True)
    assert ops.boundaries_arg(("open", "periodic")) == (False, True) and ops.boundaries_arg(["periodic", "open"]) == (True, False)
    assert ops.boundaries_arg(fluid.PERIODIC) == (True, True) and ops.boundaries_arg((fluid.OPEN, fluid.PERIODIC)) == (False, True)
    assert ops.boundaries_name((False, True)) == ("open", "periodic") and ops.periodic_bits((True, False)) == 2 and ops.periodic_bits((False, True)) == 4
    for bad in ("closed", None, 1, ("open",), ("open", "periodic", "open"), ("open", "wall"), (True, False)):
        with pytest.raises(ValueError, match="must be 'open', 'periodic' or a pair"):
            ops.boundaries_arg(bad)


def test_scene_masks_carry_the_boundaries_and_pick_a_direct_blob():
    Y, X = 40, 24
    for name in ("A", "B", "C", "D", "E"):
        g, per = pc.scene_geometry(name, Y, X), pc.periodic_of(name)
        mk = masks_of(g, multi_launch=True, boundaries=pc.SCENES[name][0], pressure_solver=pc.SCENES[name][4])
        assert mk.periodic == per and mk.periodic_bits == ops.periodic_bits(per) and mk.large and mk.box is None and mk.direct is not None
        assert precond.blob_periodic(mk.direct_header) == per == precond.blob_periodic(mk.direct.numpy())
        want = "direct_scattered" if name in ("C", "D") else "direct"
        assert mk.pressure_solver == want, (name, mk.pressure_solver)
        assert (int(mk.direct_header[5]) == 0) == (name in ("A", "E"))
    # "auto" falls through to the scattered blob where the window refuses (an obstacle across the seam)
    g = pc.scene_geometry("C", Y, X)
    assert masks_of(g, multi_launch=True, boundaries=("open", "periodic")).pressure_solver == "direct_scattered"
    with pytest.raises(ValueError, match="no direct pressure solver takes this periodic scene"):
        masks_of(g, multi_launch=True, boundaries=("open", "periodic"), pressure_solver="direct")


def test_refusals_that_need_no_device():
    Y, X = 40, 24
    g = pc.scene_geometry("A", Y, X)
    bnd = ("open", "periodic")
    with pytest.raises(ValueError, match="pass multi_launch=True"):
        masks_of(g, boundaries=bnd)
    with pytest.raises(ValueError, match="pressure_solver='cg' is not built for periodic boundaries"):
        masks_of(g, multi_launch=True, boundaries=bnd, pressure_solver="cg")
    mk = masks_of(g, multi_launch=True, boundaries=bnd)
    cfg = ops.karman_cfg(2, Y, X, g.dx, masks=mk)
    for kw, what in ((dict(buoyancy=(0.3, 0.0)), "a buoyancy force is not built for periodic"),
                     (dict(advection="mac_cormack"), "advection='mac_cormack' is not built for periodic"),
                     (dict(diffusion_substeps=2), "diffusion_substeps > 1 is not built for periodic")):
        with pytest.raises(_lib.SolError, match=what):
            ops.StepPhysics.of(**kw).require(cfg, mk, "t")
        z = torch.zeros
        with pytest.raises(_lib.SolError, match=what):
            ops.karman_step_large(z(2, Y, X), z(2, Y + 1, X), z(2, Y, X + 1), torch.ones(2), cfg, mk, **kw)
        with pytest.raises(_lib.SolError, match=what):
            ops.karman_step_saved(z(2, Y, X), z(2, Y + 1, X), z(2, Y, X + 1), torch.ones(2), cfg, mk, **kw)
        net = types.SimpleNamespace(name="mars_moon")
        with pytest.raises((_lib.SolError, ValueError), match=what):
            trainer.LargeGridTrainer(net, 2, Y, X, 2, (1.0, 1.0), 1.0, multi_launch=True, any_width=True, masks=mk, **kw)
        with pytest.raises((_lib.SolError, ValueError), match=what):
            trainer.LargeGridRollout(net, mk, 2, Y, X, g.dx, (1.0, 1.0), 1.0, multi_launch=True, any_width=True, **kw)
    ops.StepPhysics.of(buoyancy=(0.0, 0.0)).require(cfg, mk, "t")            # a zero force is the plain step
    z = torch.zeros
    with pytest.raises(_lib.SolError, match="density_grad is not built for periodic"):
        ops.karman_step_large(z(2, Y, X), z(2, Y + 1, X), z(2, Y, X + 1), torch.ones(2), cfg, mk, density_grad=True)
    with pytest.raises(_lib.SolError, match="re_grad is not built for periodic"):
        ops.karman_step_large(z(2, Y, X), z(2, Y + 1, X), z(2, Y, X + 1), torch.ones(2), cfg, mk, re_grad=True)
    with pytest.raises(_lib.SolError, match="re_grad is not built for periodic"):
        ops.karman_step_large_bwd_re(z(2, Y + 1, X), z(2, Y, X + 1), torch.ones(2), z(2, Y + 1, X), z(2, Y, X + 1), z(2, Y + 1, X), z(2, Y, X + 1), cfg, mk)
    for fn in (ops.karman_advect, ops.karman_advect_bwd):
        with pytest.raises(_lib.SolError, match="the advection stage alone is not built for periodic"):
            fn(*([None] * 6 + ([None] * 3 if fn is ops.karman_advect_bwd else [])), boundaries=bnd)
    std = (1.0, 1.0)
    with pytest.raises(ValueError, match="SolTrainer: the masks were built with periodic boundaries"):
        trainer.SolTrainer(None, mk, 2, Y, X, 2, g.dx, std, 1.0)
    with pytest.raises(ValueError, match="SolRollout: the masks were built with periodic boundaries"):
        trainer.SolRollout(None, mk, 2, Y, X, g.dx, std, 1.0)
    with pytest.raises(ValueError, match="GraphTrainer: the masks were built with periodic boundaries"):
        trainer.GraphTrainer(None, 2, Y, X, 2, std, 1.0, masks=mk)
    with pytest.raises(ValueError, match="GraphTrainer: the masks were built with periodic boundaries"):
        trainer.GraphTrainer(None, 2, Y, X, 2, std, 1.0, boundaries=bnd)
    with pytest.raises(ValueError, match="but the masks were built with boundaries"):
        trainer.LargeGridTrainer(None, 2, Y, X, 2, std, 1.0, multi_launch=True, any_width=True, masks=mk, boundaries="open")
    with pytest.raises(ValueError, match="pressure_solver='cg' is not built for periodic"):
        trainer.LargeGridTrainer(None, 2, Y, X, 2, std, 1.0, multi_launch=True, any_width=True, masks=mk, pressure_solver="cg")
    with pytest.raises(ValueError, match="cg_warm_start=True on a periodic scene"):
        trainer.LargeGridRollout(None, mk, 2, Y, X, g.dx, std, 1.0, multi_launch=True, any_width=True, cg_warm_start=True)


def test_karman_flow_follows_the_domain_and_the_records_carry_the_boundaries():
    Y, X = 48, 32
    bcv, bcm = karman.velocity_bc_masks(Y, X, batch_size=1)
    box = fluid.box[0:150, 0:100]
    dom = fluid.Domain([Y, X], box=box, boundaries=(fluid.OPEN, fluid.PERIODIC))
    sim = karman.KarmanFlow(multi_launch=True, obstacles=[])
    mk = sim._masks(dom, bcv, bcm, "cpu")
    assert mk.periodic == (False, True) and mk.pressure_solver == "direct" and sim.periodic(dom) == (False, True)
    assert not karman.KarmanFlow(multi_launch=True, obstacles=[])._masks(fluid.Domain([Y, X], box=box), bcv, bcm, "cpu").periodic_bits
    # the simulator's own boundaries go before the domain's; a domain that used to run open without a word now raises where not built
    assert karman.KarmanFlow(multi_launch=True, obstacles=[], boundaries="open")._masks(dom, bcv, bcm, "cpu").periodic_bits == 0
    with pytest.raises(ValueError, match="pass multi_launch=True"):
        karman.KarmanFlow(obstacles=[])._masks(dom, bcv, bcm, "cpu")
    with pytest.raises(ValueError, match="must be 'open', 'periodic' or a pair"):
        karman.KarmanFlow(boundaries="wall")
    rec = karman.scene_record(["box:70:73,20:80"], boundaries=("open", "periodic"))
    assert rec["boundaries"] == ("open", "periodic") and "boundaries y open, x periodic" in karman.describe_scene(rec)
    plain = karman.scene_record(["box:70:73,20:80"])
    assert "boundaries" not in plain and "boundaries" not in karman.scene_record(["box:70:73,20:80"], boundaries="open")
    assert karman.record_boundaries(plain) == ("open", "open") and "boundaries" not in karman.describe_scene(plain)
    assert not karman.scenes_equal(rec, plain) and karman.scenes_equal(rec, dict(rec)) and karman.scenes_equal(plain, dict(plain))
    assert karman.KarmanFlow(obstacles=[], boundaries=("open", "periodic")).scene()["boundaries"] == ("open", "periodic")
    assert sim.scene(dom)["boundaries"] == ("open", "periodic") and "boundaries" not in sim.scene()


def test_the_library_exports_the_seam_entries_and_keeps_its_abi():
    lib = _lib.load()
    assert lib.sol_version() == _lib.ABI_VERSION == 216          # additions only: the ABI number stays
    for name in ("sol_karman_seam_sync", "sol_karman_seam_fold"):
        assert name in _lib.declared_symbols() and hasattr(lib, name)
