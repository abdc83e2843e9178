"""multi_launch=True on the one-workgroup grids, the part that needs no device: the host rules of SceneMasks(multi_launch=True) and of the
one-launch solve, the refusals that stay without the flag, and the float64 references of the GPU tests (test_gpu_karman2d_solve_one_wg.py,
test_gpu_karman2d_multi_launch.py) measured in float32 against float64 at every (grid, seed) those tests use.

The seed rule is karman2d_small_shapes.SEEDS': the first seed of (77, 11, 5, 7, 13) at which the float32 reference agrees with the
float64 reference to a quarter of TOL_FIELD / TOL_GRAD, so that a GPU failure is the kernel's.  Measured at the seeds chosen (all 77):
fields 4.3e-7 ... 9.3e-7, gradients 1.2e-6 ... 5.3e-6 (MacCormack cases in the trimmed metric, cap large2d_scenes.TRIM as a condition),
g_re 1.6e-6; the trainer problems loss 1.4e-6 / 5.8e-7 and weight gradient 1.6e-6 / 7.4e-7 (64 x 32 / 96 x 48), the roll-out 6.8e-7.
(Trainer seed 11, the MacCormack suite's, misses at 64 x 32: 9.1e-5 in the second step's loss.)"""
import os
import sys
import types

import numpy as np
import pytest
import torch

import sol_oracle as o
from sol_amd import _lib, ops, precond, schedule2d, trainer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import karman2d_multi_launch_cases as mlc
import karman2d_small_shapes as ks
from large2d_scenes import TOL_FIELD, TOL_GRAD, TRIM, rel

GRIDS = sorted({c[:2] for c in mlc.SOLVE_CASES.values()} | set(mlc.PLAIN) | set(mlc.CG_GRIDS) | {c[0] for c in mlc.MAC})


def masks_of(g, **kw):
    return ops.SceneMasks(g.active, g.inflow, g.bc_mask, g.bc_mask, "cpu", **kw)


# ---- host rules ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS, ids=ks.sid)
def test_multi_launch_sets_large_and_everything_that_follows(grid):
    Y, X = grid
    assert not ops.beyond_one_workgroup(Y, X)
    g = o.geometry(Y, X)
    mk = masks_of(g, multi_launch=True)
    assert mk.large and mk.multi_launch and mk.coarse_inv is None
    blob = precond.direct_solver_blob(np.asarray(g.active), 64)
    if blob is None:
        assert grid == (16, 64) and mk.pressure_solver == "cg" and mk.direct is None and mk.box is not None
    else:
        assert mk.pressure_solver == "direct" and mk.box is None and np.array_equal(mk.direct.numpy().view(np.int32), blob.view(np.int32))      # the device blob keeps word 8 zero
        hdr = mk.direct_header
        assert np.array_equal(hdr[:8], blob[:8].view(np.int32)) and int(hdr[ops.DIRECT_HEADER_FLAGS]) == ops.DIRECT_ONE_WG
        assert int(blob[:16].view(np.int32)[ops.DIRECT_HEADER_FLAGS]) == 0
    cg = masks_of(g, multi_launch=True, pressure_solver="cg")
    assert cg.large and cg.pressure_solver == "cg" and cg.direct is None and cg.box is not None and cg.coarse_inv is None
    if blob is not None:
        sc = masks_of(g, multi_launch=True, pressure_solver="direct_scattered")
        assert sc.pressure_solver == "direct_scattered" and int(sc.direct_header[0]) == precond.FDS_MAGIC
    if ks.check_cfg(Y, X) is None:               # a grid the one-workgroup entry takes: the default picks what it picked
        d = masks_of(g)
        assert not d.large and not d.multi_launch
        assert d.direct_header is None or int(d.direct_header[ops.DIRECT_HEADER_FLAGS]) == 0


@pytest.mark.parametrize("case", list(mlc.SOLVE_CASES))
def test_the_solve_table_reaches_what_it_says(case):
    Y, X = mlc.SOLVE_CASES[case][:2]
    g = mlc.solve_geometry(case)
    hdr = precond.direct_solver_blob(np.asarray(g.active), 64)[:16].view(np.int32)
    assert tuple(int(v) for v in hdr[3:8]) == mlc.SOLVE_WINDOWS[case]
    wy0, wx0, nS, SP, win = mlc.SOLVE_WINDOWS[case]
    assert mlc.one_wg_supported(Y, X, win) and SP % 64 == 0 and nS <= SP <= 4096
    if case == "16x16":
        assert (win, wy0, wx0) == (16, 0, 0)
    if case == "32x64":
        assert SP == 128 and Y < X
    if case == "128x64_two_boxes":
        assert win == 64 and Y * X == 8192
    if case in ("40x24", "96x48"):
        assert ks.check_cfg(Y, X) is not None and schedule2d.row_pitch(Y, X) != X      # no entry took the grid; its width needs any_width
    if case == "512x16":
        assert Y == 8192 // 16


def test_one_wg_supported_equals_its_replica():
    lib = _lib.load()
    for Y in list(range(8, 140)) + [256, 511, 512, 513, 520]:
        for X in list(range(8, 70)) + [128]:
            for win in (0, 8, 16, 32, 64, 128):
                assert bool(lib.sol_karman_solve_one_wg_supported(Y, X, win)) == mlc.one_wg_supported(Y, X, win), (Y, X, win)
    assert ops.solve_one_wg_supported(128, 64, 64) and not ops.solve_one_wg_supported(136, 64, 16) and not ops.solve_one_wg_supported(64, 65, 16)
    assert _lib.get_option("k2d_solve_one_wg") in (0, 1)
    assert "sol_karman_solve_one_wg_supported" in _lib.declared_symbols()


def test_multi_launch_below_16_cells_is_refused():
    g = o.geometry(16, 8)
    with pytest.raises(ValueError, match="multi_launch=True takes grids with Y, X >= 16"):
        masks_of(g, multi_launch=True)
    with pytest.raises(ValueError, match="multi_launch=True takes grids with Y, X >= 16"):
        trainer._check_multi_launch("LargeGridTrainer", True, None, 16, 8)


# ---- the refusals stay ----------------------------------------------------------------------------------------------------------------------------
def test_without_the_flag_every_refusal_still_raises():
    Y, X = 64, 32
    g = o.geometry(Y, X)
    mk = masks_of(g)
    cfg = ops.karman_cfg(2, Y, X, g.dx)
    with pytest.raises(_lib.SolError, match="the buoyancy force is built on the multi-launch"):
        ops.StepPhysics.of(buoyancy=(0.3, 0.0)).require(cfg, mk, "t")
    with pytest.raises(_lib.SolError, match="the mac_cormack advection is built on the multi-launch"):
        ops.StepPhysics.of(advection="mac_cormack").require(cfg, mk, "t")
    ml = masks_of(g, multi_launch=True)
    ops.StepPhysics.of(buoyancy=(0.3, 0.0), advection="mac_cormack", diffusion_substeps=3).require(cfg, ml, "t")      # with it: served
    with pytest.raises(ValueError, match="pressure_solver='direct_scattered' serves the large-grid path only"):
        masks_of(g, pressure_solver="direct_scattered")
    std = (1.0, 1.0)
    for kw, what in ((dict(buoyancy=(0.3, 0.0)), "buoyancy"), (dict(advection="mac_cormack"), "advection='mac_cormack'"),
                     (dict(diffusion_substeps=3), "diffusion_substeps=3")):
        with pytest.raises(ValueError, match=what):
            trainer.SolTrainer(None, None, 2, Y, X, 2, 100.0 / X, std, 1.0, **kw)
        with pytest.raises(ValueError, match=what):
            trainer.GraphTrainer(None, 2, Y, X, 2, std, 1.0, **kw)
        net = types.SimpleNamespace(name="mars_moon")
        with pytest.raises(ValueError):
            trainer.make_trainer(net, mk, 2, Y, X, 2, 100.0 / X, std, 1.0, **kw)
        with pytest.raises(ValueError):
            trainer.make_rollout(net, mk, 2, Y, X, 100.0 / X, std, 1.0, **kw)
    with pytest.raises(ValueError, match="SolRollout"):
        trainer.SolRollout(None, mk, 2, Y, X, 100.0 / X, std, 1.0, advection="mac_cormack")
    with pytest.raises(ValueError, match="is served by the one-workgroup trainers"):
        trainer.LargeGridTrainer(None, 2, Y, X, 2, std, 1.0)
    with pytest.raises(ValueError, match="is served by the one-workgroup roll-out"):
        trainer.LargeGridRollout(None, mk, 2, Y, X, 100.0 / X, std, 1.0)
    for c in ((96, 48), (96, 24)):                      # the one-workgroup entry refuses these widths; the README said so
        assert ks.check_cfg(*c) == "X must be 8, 16, 32 or 64" and not ops.beyond_one_workgroup(*c)


def test_the_flag_and_the_masks_must_agree_and_the_width_rule():
    g = o.geometry(64, 32)
    mk, ml = masks_of(g), masks_of(g, multi_launch=True)
    assert trainer._check_multi_launch("t", True, ml, 64, 32) is True and trainer._check_multi_launch("t", False, mk, 64, 32) is False
    assert trainer._check_multi_launch("t", True, None, 64, 32) is True
    with pytest.raises(ValueError, match="multi_launch=True, but the masks were built with SceneMasks\\(multi_launch=False\\)"):
        trainer._check_multi_launch("t", True, mk, 64, 32)
    with pytest.raises(ValueError, match="multi_launch=False, but the masks were built with SceneMasks\\(multi_launch=True\\)"):
        trainer.LargeGridRollout(None, ml, 2, 64, 32, 100.0 / 32, (1.0, 1.0), 1.0)
    with pytest.raises(ValueError, match="multi_launch=True, but the masks"):
        trainer.LargeGridTrainer(None, 2, 64, 32, 2, (1.0, 1.0), 1.0, multi_launch=True, masks=mk)
    # a width the convolutions take as it is runs dense; any other needs any_width, as on large grids
    for (Y, X), dense in (((64, 32), True), ((48, 32), True), ((16, 16), True), ((128, 64), True), ((96, 48), False), ((40, 24), False)):
        assert (schedule2d.row_pitch(Y, X) == X) == dense
        assert trainer._width_served(Y, X, False, True) == dense and trainer._width_served(Y, X, True, True)
        assert trainer._width_served(Y, X, False, False) == (X % 64 == 0)
    with pytest.raises(ValueError, match="X % 64 == 0"):
        trainer.LargeGridTrainer(None, 1, 96, 48, 2, (1.0, 1.0), 1.0, multi_launch=True)


def test_karman_flow_passes_the_flag_on_and_keys_its_cache_on_it():
    from sol_amd import fluid, karman
    Y, X = 48, 32
    dom = fluid.Domain([Y, X], box=fluid.box[0:150, 0:100])
    bcv, bcm = karman.velocity_bc_masks(Y, X, batch_size=1)
    sim = karman.KarmanFlow(multi_launch=True)
    a = sim._masks(dom, bcv, bcm, "cpu")
    assert a.large and a.multi_launch
    sim._multi_launch = False
    sim._last_masks = None
    b = sim._masks(dom, bcv, bcm, "cpu")
    assert not b.large and b is not a and len(sim._cache) == 2
    assert not karman.KarmanFlow()._masks(dom, bcv, bcm, "cpu").large


# ---- the references alone: float32 against float64 at the seeds the GPU tests use -----------------------------------------------------------------
def alone(key, seed):
    grid, adv, force, n = key[:4]
    kind = key[4] if len(key) > 4 else "velocity"
    o64, g64 = mlc.reference(grid, adv, force, n, kind, seed)[:2]
    o32, g32 = mlc.reference(grid, adv, force, n, kind, seed, torch.float32)[:2]
    ef = max(rel(a, b) for a, b in zip(o32, o64))
    which = [1, 2] + ([0] if kind == "density" or force is not None else [])
    eg = max(mlc.grad_error(g32[i], g64[i], adv is not None)[0] for i in which)          # (grad_error holds the trimmed metric to its cap TRIM)
    if kind == "re":
        eg = max(eg, rel(g32[3], g64[3]))
    return ef, eg


@pytest.mark.parametrize("key", list(mlc.SEEDS), ids=lambda k: "%s_%s" % (ks.sid(k[0]), "_".join(str(v) for v in k[1:])))
def test_the_step_references_in_float32_hold_a_quarter_of_the_tolerances(key):
    seed = mlc.SEEDS[key]
    assert seed in mlc.CANDIDATES and TRIM == 1e-3
    for s in mlc.CANDIDATES[:mlc.CANDIDATES.index(seed)]:            # the FIRST seed that does
        ef, eg = alone(key, s)
        assert not (ef < TOL_FIELD / 4 and eg < TOL_GRAD / 4), (key, s)
    ef, eg = alone(key, seed)
    print("float32 against float64, %s seed %d: fields %.3e, gradients %.3e" % (key, seed, ef, eg))
    assert ef < TOL_FIELD / 4 and eg < TOL_GRAD / 4, (key, ef, eg)


def trainer_alone(Y, X, nb, seed):
    p = mlc.trainer_problem(Y, X, nb, seed=seed)
    l64, s64, g64, f64 = mlc.trainer_reference(p)
    l32, s32, g32, f32 = mlc.trainer_reference(p, torch.float32)
    return (max([abs(l32 - l64) / abs(l64)] + [abs(a - b) / abs(b) for a, b in zip(s32, s64)] + [rel(a, b) for a, b in zip(f32, f64)]), rel(g32, g64))


@pytest.mark.parametrize("grid,nb", mlc.TRAINER_CASES, ids=["64x32", "96x48"])
def test_the_trainer_reference_in_float32_holds_a_quarter_of_the_tolerances(grid, nb):
    seed = mlc.TRAINER_SEED
    for s in mlc.CANDIDATES[:mlc.CANDIDATES.index(seed)]:
        ef, eg = trainer_alone(*grid, nb, s)
        assert not (ef < TOL_FIELD / 4 and eg < TOL_GRAD / 4), (grid, s)
    ef, eg = trainer_alone(*grid, nb, seed)
    print("trainer reference float32 against float64, %s: loss / final state %.3e, weight gradient %.3e" % (grid, ef, eg))
    assert ef < TOL_FIELD / 4 and eg < TOL_GRAD / 4


def test_the_rollout_reference_in_float32_holds_a_quarter_of_the_tolerance():
    p = mlc.trainer_problem(64, 32, mlc.B, force=None, n=1)
    e = max(rel(a, b) for a, b in zip(mlc.rollout_reference(p, 4, torch.float32), mlc.rollout_reference(p, 4)))
    print("roll-out reference float32 against float64 after four steps: %.3e" % e)
    assert e < TOL_FIELD / 4
