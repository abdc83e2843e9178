"""The ragged-shape table of the large-grid karman-2d tests, CPU side (no GPU needed): every cell of large2d_scenes.WINDOWS names the
window edge (16 / 32 / 64) and the window origin -- clamped to the domain edge for the obstacles that touch it -- that
precond.direct_solver_blob(active, max_window=64) picks there, so that each case of test_gpu_karman2d_large_shapes.py demonstrably
reaches the window or clamp it is listed for.  Pinned here: the header words {Y, X, wy0, wx0, nS, SP, win}, the refusals, and the
agreement of the float64 restatements (precond.direct_solve_reference, precond.scattered_solve_reference) with a sparse LU of the
scene matrix, for the one-window blob and for the scattered blob of every cell.

Bounds (those of test_scattered_direct_cpu.py's LU comparison): 1e-5 relative L2 on the fluid cells for a float32 blob (measured
5.4e-8 ... 8.8e-7 over the 18 cells, both blobs), 1e-9 for the unrounded float64 scattered blob (measured <= 1e-12)."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from sol_amd import precond

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from large2d_scenes import SCENE_SPECS, SHAPES, WINDOWS, step_like_rhs, table_geometry
from test_scattered_direct_cpu import sparse_matrix

CELLS = [(name, Y, X) for Y, X in SHAPES for name in SCENE_SPECS]


@pytest.fixture(scope="module", params=CELLS, ids=["%s_%dx%d" % c for c in CELLS])
def cell(request):
    name, Y, X = request.param
    active = table_geometry(name, Y, X).active
    lu = spla.splu(sparse_matrix(active))
    b = step_like_rhs(1, Y, X)[0].numpy()
    ref = lu.solve(b.ravel()).reshape(Y, X)
    fluid_cells = active != 0
    err = lambda x: float(np.linalg.norm((x - ref)[fluid_cells]) / np.linalg.norm(ref[fluid_cells]))
    return name, Y, X, active, b, err


def test_table_is_complete_and_names_every_window_and_a_clamp():
    assert set(WINDOWS) == {(name, Y) for name, Y, _ in CELLS} and all(Y == 2 * X for Y, X in SHAPES)
    wins = {w[4] for w in WINDOWS.values() if w is not None}
    assert wins == {16, 32, 64}
    # a window clamped in both axes, and one clamped in y alone
    assert WINDOWS[("corner", 130)][:2] == (130 - 16, 65 - 16) and WINDOWS[("top_edge", 130)][0] == 130 - 16
    # the ragged sizes: tiles of 16 (adjoint) and 64 (GEMM)
    assert (130 % 16, 65 % 16) == (2, 1) and (144 % 16, 72 % 16, 144 % 64, 72 % 64) == (0, 8, 16, 8) and (80 % 16, 80 % 64) == (0, 16)


def test_one_window_blob_header_and_reference_against_sparse_lu(cell):
    name, Y, X, active, b, err = cell
    blob = precond.direct_solver_blob(active, max_window=64)
    want = WINDOWS[(name, Y)]
    if want is None:
        assert blob is None                                  # two cylinders span more than 64 rows at 144 x 72 and beyond
        return
    hdr = blob[:16].view(np.int32)
    assert hdr[0] == precond.FD_MAGIC and (int(hdr[1]), int(hdr[2])) == (Y, X)
    assert tuple(int(v) for v in hdr[3:8]) == want, (name, Y, X, hdr[3:8].tolist())
    wy0, wx0, nS, SP, win = want
    assert 0 <= wy0 <= Y - win and 0 <= wx0 <= X - win and nS <= SP < nS + 64 and SP % 64 == 0
    # every support cell lies inside the window the header names (a clamp that moved the window off the support would lose cells)
    S = np.array(sorted({r for r, _ in precond._perturbation(active)}))
    js, is_ = S // X, S % X
    assert len(S) == nS and wy0 <= js.min() and js.max() < wy0 + win and wx0 <= is_.min() and is_.max() < wx0 + win
    sidx = blob[16 + Y * Y + X * X + X * Y + SP * SP:][:SP].view(np.int32)
    np.testing.assert_array_equal(sidx[:nS], (js - wy0) * win + (is_ - wx0))
    assert np.all(sidx[nS:] == -1)
    e = err(precond.direct_solve_reference(blob, b))
    print("%s %dx%d one-window blob (win %d at %d, %d): %.3e against sparse LU" % (name, Y, X, win, wy0, wx0, e))
    assert e < 1e-5, e


def test_scattered_blob_builds_and_reference_against_sparse_lu(cell):
    name, Y, X, active, b, err = cell
    blob = precond.scattered_solver_blob(active)
    assert blob is not None and blob.dtype == np.float32
    s = precond.scattered_sections(blob)
    assert (s["Y"], s["X"]) == (Y, X) and s["SP"] % 64 == 0 and s["nS"] <= s["SP"] < s["nS"] + 64
    if WINDOWS[(name, Y)] is not None:
        assert s["nS"] == WINDOWS[(name, Y)][2]              # the same support set as the one-window blob
    e64 = err(precond.scattered_solve_reference(precond.scattered_solver_blob(active, dtype=np.float64), b))
    e32 = err(precond.scattered_solve_reference(blob, b))
    print("%s %dx%d scattered blob (nR %d, nC %d, nS %d): float64 blob %.3e, float32 blob %.3e against sparse LU"
          % (name, Y, X, s["nR"], s["nC"], s["nS"], e64, e32))
    assert e64 < 1e-9, e64
    assert e32 < 1e-5, e32
