"""CPU twin of test_gpu_karman2d_small_shapes.py (no device): the shape table's path claims against replicas of the host rules of
csrc/karman_step.hip, the replicas against the library (sol_karman_step_fwd validates its cfg before it looks at a pointer, so a call
with NULL arrays launches nothing and reports the first rule the grid breaks), the refusals, the one rule of check_cfg's direct branch and
sol_karman_direct_supported, what the Python routing does with a grid the one-workgroup entry refuses, and that the float32 oracle alone
stays within a quarter of each tolerance at every row's state -- the condition under which TOL_FIELD / TOL_GRAD are a bound on the kernel
and not on the reference."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import sol_amd
import sol_oracle as o
from sol_amd import ops, precond

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import karman2d_small_shapes as ks
from karman2d_small_shapes import TOL_FIELD, TOL_GRAD, rel

ACCEPTED = "NULL pointer"        # the message of a cfg that passed check_cfg (the arrays are NULL)
FAKE_BLOB = 16                   # check_cfg never dereferences cfg.direct


@pytest.fixture(scope="module")
def lib():
    return sol_amd.load()


def verdict(lib, Y, X, direct=False, entry="fwd"):
    """(return code, message) of the one-workgroup entry on a cfg with NULL arrays"""
    cfg = ops.karman_cfg(1, Y, X, 100.0 / X)
    if direct:
        cfg.direct, cfg.direct_n = FAKE_BLOB, 8 * 512 * 32
    if entry == "fwd":
        rc = lib.sol_karman_step_fwd(C.byref(cfg), None, *([None] * 8), 0, *([None] * 6), None, None)
    else:
        rc = lib.sol_karman_step_bwd(C.byref(cfg), None, *([None] * 5), 0, *([None] * 3), None, *([None] * 3))
    return rc, lib.sol_last_error().decode()


def test_oracle_geometry_on_any_grid_keeps_the_reference_grids():
    """dx = length / X on every grid, the masks keep their physical definitions, and a (2r, r) grid is what it was"""
    for c in ks.ROWS:
        g = o.KarmanGeometry(*c)
        assert g.dx == 100.0 / c[1] and g.active.shape == c and g.my.shape == (c[0] + 1, c[1]) and g.mx.shape == (c[0], c[1] + 1)
        yc, xc = np.meshgrid((np.arange(c[0]) + 0.5) * g.dx, (np.arange(c[1]) + 0.5) * g.dx, indexing="ij")
        assert np.array_equal(g.obstacle, ((yc - 50.0) ** 2 + (xc - 50.0) ** 2 <= 100.0).astype(np.float64))
        assert np.array_equal(g.inflow, ((yc >= 5.0) & (yc <= 10.0) & (xc >= 25.0) & (xc <= 75.0)).astype(np.float64))
    assert int(o.geometry(16, 64).obstacle.sum()) == 0                      # the domain ends at y = 25: no obstacle
    assert int(o.geometry(32, 64).obstacle.sum()) == 62 and o.geometry(32, 64).obstacle[-1].any()      # cut by the top wall
    assert int(o.geometry(8, 8).obstacle.sum()) == 4
    assert int(o.geometry(64, 32).obstacle.sum()) == 32 and int(o.geometry(128, 64).obstacle.sum()) == 124


def test_table_figures_follow_from_the_host_rules():
    for c, (_, cpt_cg, cpt_direct, threads, lds, blob) in ks.ROWS.items():
        assert ks.check_cfg(*c) is None, c
        assert ks.pick_cpt(*c) == cpt_cg and ks.threads_of(*c, cpt_cg) == threads and ks.lds_bytes(*c, cpt_cg) == lds, c
        assert lds <= ks.LDS_LIMIT
        if cpt_direct is not None:
            assert blob is not None and ks.direct_supported(*c) and ks.pick_cpt(*c, direct=True) == cpt_direct and ks.check_cfg(*c, True) is None
        else:
            assert blob is None
    # the path claims
    owners = lambda c, cpt: (c[0] // cpt) * c[1]
    assert owners((8, 8), 8) == 8 and owners((24, 8), 8) == 24 and owners((16, 16), 16) == 16              # fewer owners than a wave
    for c in ((24, 16), (40, 32), (120, 64)):
        assert c[0] % 16 and c[1] >= 16 and ks.pick_cpt(*c) == 8                                          # <8, 0> at X >= 16
    assert ks.threads_of(120, 64, 8) == 960 and ks.check_cfg(136, 64) == "exceeds one workgroup"                # 128 x 64 is cpt 16; 136 x 64 would be 1088 threads
    assert ks.threads_of(256, 32, 16) == ks.threads_of(512, 16, 16) == 512
    assert ks.check_cfg(272, 32) is not None and ks.check_cfg(528, 16) is not None                        # the next grids up are refused
    assert ks.BOTH_CPT == ks.both_cpt_rows() and len(ks.BOTH_CPT) == 11                                   # every row that admits both, none left out
    assert ks.threads_of(256, 32, 8) == ks.threads_of(512, 16, 8) == 1024 and ks.lds_bytes(256, 32, 8) == 161296 and ks.lds_bytes(512, 16, 8) == 162704
    assert ks.DIRECT_CPT16 == ks.DIRECT_ROWS
    for c in ks.BOTH_CPT:
        assert all(ks.check_cfg(*c, forced=f) is None for f in (8, 16)), c
    for c in ks.DIRECT_CPT16:
        assert ks.pick_cpt(*c, direct=True, forced=16) == 16 and ks.check_cfg(*c, True, forced=16) is None
    assert all(c in ks.ROWS for c in ks.BOTH_CPT + ks.DIRECT_CPT16 + ks.FEATURE_ROWS)
    assert ks.fd_small_floats(32, 64) > 0 and ks.ROWS[(32, 64)][5][3] == 128 > 64                         # K' does not fit the LDS slot
    for c in ((96, 32), (256, 32), (512, 16)):
        assert c[0] * c[1] > 2048 and not ks.direct_supported(*c)


def test_blob_headers_of_the_table(lib):
    for c, row in ks.ROWS.items():
        g = ks.geometry(c)
        if min(c) < 16:
            assert lib.sol_karman_direct_supported(*c) == 0 and row[5] is None
            continue
        blob = precond.direct_solver_blob(g.active, max_window=16)
        hdr = None if blob is None else tuple(int(v) for v in blob[:16].view(np.int32)[3:8])
        if lib.sol_karman_direct_supported(*c):
            assert hdr == row[5], (c, hdr)
        else:
            assert row[5] is None and row[2] is None            # a blob may exist (24 x 16: it does); the solver does not take the grid
    assert precond.direct_solver_blob(ks.geometry((16, 64)).active, max_window=16) is None
    assert lib.sol_karman_direct_supported(16, 64) == 1        # ... the grid is fine, the scene has nothing to correct


def test_replicas_agree_with_the_library_on_every_grid(lib):
    """check_cfg's verdict and sol_karman_direct_supported for all Y <= 256 (and the taller grids of the table), X <= 64, with and
    without a direct blob: the replica names the rule the library's message names.  With it: check_cfg's direct branch and the predicate
    are ONE rule -- on a grid the entry takes with CG, it takes a blob exactly where sol_karman_direct_supported says so."""
    grids = [(Y, X) for Y in range(1, 257) for X in range(1, 65)] + [(Y, X) for Y in (264, 272, 512, 520, 528, 1024) for X in (8, 16, 32, 64)]
    n_direct = 0
    for Y, X in grids:
        assert lib.sol_karman_direct_supported(Y, X) == int(ks.direct_supported(Y, X)), (Y, X)
        verdicts = {}
        for direct in (False, True):
            rc, msg = verdict(lib, Y, X, direct)
            want = ks.check_cfg(Y, X, direct)
            assert rc == -1 and (ACCEPTED if want is None else want) in msg, (Y, X, direct, msg, want)
            verdicts[direct] = ACCEPTED in msg
        if verdicts[False]:
            assert verdicts[True] == bool(lib.sol_karman_direct_supported(Y, X)), (Y, X)
            n_direct += verdicts[True]
        else:
            assert not verdicts[True], (Y, X)
    # 128 x 64 is fd_solve's grid (the host asks for both extents); no blob is taken at Y == 128 with another width
    for X in range(1, 65):
        if X != 64:
            assert lib.sol_karman_direct_supported(128, X) == 0 and ACCEPTED not in verdict(lib, 128, X, True)[1], X
    assert n_direct == sum(1 for Y, X in grids if ks.check_cfg(Y, X) is None and ks.check_cfg(Y, X, True) is None) == 14      # 7 at X = 16, 4 at X = 32, 2 at X = 64, and 128 x 64


@pytest.mark.parametrize("c", list(ks.REFUSED), ids=ks.sid)
def test_refused_grids_return_an_error_and_a_message(lib, c):
    for entry in ("fwd", "bwd"):
        for direct in (False, True):
            rc, msg = verdict(lib, *c, direct, entry)
            assert rc == -1 and ks.REFUSED[c] in msg and ("%dx%d" % c in msg or "(got %d)" % c[0] in msg or "(got %d)" % c[1] in msg), (c, entry, direct, msg)


@pytest.mark.parametrize("c", ks.DIRECT_REFUSED, ids=ks.sid)
def test_a_direct_blob_is_refused_where_the_solver_is_not_built(lib, c):
    assert verdict(lib, *c)[1].endswith(ACCEPTED + " argument")                  # the grid itself is fine
    for entry in ("fwd", "bwd"):
        rc, msg = verdict(lib, *c, True, entry)
        assert rc == -1 and "the direct pressure solver is built for 128x64" in msg and "%dx%d" % c in msg, (c, msg)


def test_python_routing_of_grids_the_one_workgroup_entry_refuses():
    """ops.beyond_one_workgroup is `more than 8192 cells or X > 64`; check_cfg is stricter (X in {8, 16, 32, 64}, Y % 8 == 0, the thread
    and LDS limits).  A grid between the two -- 96 x 48, 1024 x 8 -- is NOT routed to the large-grid path: SceneMasks calls it small, the
    one-workgroup entry refuses it with check_cfg's message, and the large-grid classes refuse it as "not beyond".  (136 x 64 and 144 x 64
    have more than 8192 cells and do run the large-grid path.)  Pinned here as it
    stands (the README's grid list says the same); widening beyond_one_workgroup is left to a change of its own."""
    from sol_amd import trainer
    for c in ((96, 48), (1024, 8), (20, 8), (96, 24)):
        assert not ops.beyond_one_workgroup(*c) and ks.check_cfg(*c) is not None
    for c in ks.ROWS:
        assert not ops.beyond_one_workgroup(*c)
    assert ops.beyond_one_workgroup(144, 72) and ops.beyond_one_workgroup(130, 65)
    assert ops.beyond_one_workgroup(136, 64) and ops.beyond_one_workgroup(144, 64)      # more than 8192 cells: these run the large-grid path
    net = sol_amd.model_mars_moon(cin=3, cout=2, seed=0, device="cpu")
    with pytest.raises(ValueError, match="96x48"):
        trainer.LargeGridTrainer(net, 1, 96, 48, 2, (0.2, 0.2), 1.0, dx=100.0 / 48, masks=None, any_width=True)
    with pytest.raises(ValueError, match="96x48"):
        trainer.LargeGridRollout(net, None, 1, 96, 48, 100.0 / 48, (0.2, 0.2), 1.0, any_width=True)


@pytest.mark.parametrize("c", list(ks.ROWS), ids=ks.sid)
def test_float32_oracle_alone_is_within_a_quarter_of_each_tolerance(c):
    """untrimmed, at the row's state and cotangent; the measured figures are recorded in karman2d_small_shapes.ORACLE_ALONE"""
    r64, r32 = ks.reference(c), ks.reference(c, dtype=torch.float32)
    fe = max(rel(a, b) for a, b in zip(r32[0], r64[0]))
    ge = max(rel(a, b) for a, b in zip(r32[1], r64[1]))
    print("%s seed %d: float32 oracle against float64 oracle: fields %.2e, gradients %.2e" % (ks.sid(c), ks.SEEDS[c], fe, ge))
    assert fe <= TOL_FIELD / 4 and ge <= TOL_GRAD / 4, (c, fe, ge)
    rec = ks.ORACLE_ALONE[c]
    assert 0.5 * rec[0] <= fe <= 2.0 * rec[0] and 0.5 * rec[1] <= ge <= 2.0 * rec[1], (c, fe, ge, rec)       # the record is what was measured


@pytest.mark.parametrize("c", [(24, 16), (32, 64)], ids=ks.sid)
def test_float32_oracle_alone_dirichlet_before(c):
    r64 = ks.reference(c, "dirichlet0", "before")
    r32 = ks.reference(c, "dirichlet0", "before", torch.float32)
    assert max(rel(a, b) for a, b in zip(r32[0], r64[0])) <= TOL_FIELD / 4
    assert max(rel(a, b) for a, b in zip(r32[1], r64[1])) <= TOL_GRAD / 4
