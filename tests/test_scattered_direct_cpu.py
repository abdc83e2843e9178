"""The scattered direct pressure solver, CPU side (no GPU needed): precond.scattered_solver_blob on the scenes the one-window blob
refuses, its float64 restatement against a sparse LU of the scene matrix, the refusals, agreement with the one-window solver where
both build, the untouched one-window blob, and the new C entry points.

Bounds: 1e-9 relative L2 on the fluid cells against the sparse LU for the restatement on the unrounded (dtype=np.float64) blob
(measured 1e-13), 1e-5 (the GPU tests' field tolerance) on the device's float32 blob, whose rounded matrices are part of the solver;
1e-10 between the two restatements on the default sphere.
The one-window blob is guarded twice: the text of the functions that build it is the parent's (sha256: same code, same inputs, same
bytes on a given numpy / BLAS), and their output agrees with the parent's output stored under tests/golden/ to float32 rounding
(integer sections exactly) -- a byte comparison of LAPACK results across CPU models would test the BLAS kernel selection, not this code."""
import ctypes as C
import hashlib
import inspect
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import sol_oracle as o
import sol_amd
from sol_amd import _lib, fluid, karman, ops, precond

TWO = ["sphere:50,50,10", "sphere:120,50,10"]
PLATE = ["box:70:73,20:80"]
FAKE = C.c_void_p(4096)          # never dereferenced: every case below fails validation first


def active_of(specs, Y, X):
    dom = fluid.Domain([Y, X], box=fluid.box[0:200, 0:100])
    return karman.KarmanFlow(obstacles=karman.parse_obstacles(specs)).scene_arrays(dom)[0]


def two_boxes(Y, X):
    a = np.ones((Y, X))
    a[20:27, 11:20] = 0.0
    a[50:61, 40:53] = 0.0
    return a


def sparse_matrix(active):
    """M = -A of the scene as a sparse matrix (the stencil of precond.scene_matrix)"""
    act = (np.asarray(active) != 0).astype(np.float64)
    Y, X = act.shape
    acc = np.pad(act, 1, mode="edge")
    diag = np.maximum(acc[0:Y, 1:X + 1] + acc[2:Y + 2, 1:X + 1] + acc[1:Y + 1, 0:X] + acc[1:Y + 1, 2:X + 2], 1.0)
    idx = np.arange(Y * X).reshape(Y, X)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [diag.ravel()]
    for sj, si in ((1, 0), (0, 1)):
        a = (act[0:Y - sj, 0:X - si] * act[sj:Y, si:X]).ravel()
        r, c = idx[0:Y - sj, 0:X - si].ravel(), idx[sj:Y, si:X].ravel()
        rows += [r, c]; cols += [c, r]; vals += [-a, -a]
    return sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(Y * X, Y * X))


def step_like_rhs(Y, X, seed):
    _, vy, vx = o.synthetic_state(1, Y, X, seed, project_it=False)
    return (-((vy[:, 1:] - vy[:, :-1]) + (vx[:, :, 1:] - vx[:, :, :-1])))[0].numpy().astype(np.float64)


SCENES = {"two": (256, 128, lambda: active_of(TWO, 256, 128), (1188, 55, 28)),
          "plate": (256, 128, lambda: active_of(PLATE, 256, 128), (386, 5, 78)),
          "two_boxes_96x72": (96, 72, lambda: two_boxes(96, 72), None)}


@pytest.fixture(scope="module", params=list(SCENES))
def scene(request):
    Y, X, mk, sizes = SCENES[request.param]
    active = mk()
    return request.param, Y, X, active, sizes, precond.scattered_solver_blob(active)


def test_blob_header_and_sections_are_consistent(scene):
    name, Y, X, active, sizes, blob = scene
    assert blob is not None and blob.dtype == np.float32
    s = precond.scattered_sections(blob)
    hdr = blob[:16].view(np.int32)
    assert hdr[0] == precond.FDS_MAGIC != precond.FD_MAGIC and (s["Y"], s["X"]) == (Y, X) and not hdr[9:].any()
    assert s["words"] == blob.size
    if sizes is not None:
        assert (s["nS"], s["nR"], s["nC"]) == sizes
    assert s["SP"] % 64 == 0 and s["nS"] <= s["SP"] < s["nS"] + 64 and s["SP"] <= 4096
    assert s["RP"] % 4 == 0 and s["nR"] <= s["RP"] < s["nR"] + 4 and s["CP"] % 4 == 0 and s["nC"] <= s["CP"] < s["nC"] + 4
    # K'^T starts on a 16-byte boundary of the blob
    assert (16 + precond._pad4(Y * Y + X * X + X * Y)) % 4 == 0
    rows, cols, sidx = s["rows"], s["cols"], s["sidx"]
    assert np.all(np.diff(rows[:s["nR"]]) > 0) and np.all(rows[s["nR"]:] == -1) and rows[:s["nR"]].min() >= 0 and rows[:s["nR"]].max() < Y
    assert np.all(np.diff(cols[:s["nC"]]) > 0) and np.all(cols[s["nC"]:] == -1) and cols[:s["nC"]].min() >= 0 and cols[:s["nC"]].max() < X
    assert np.all(sidx[s["nS"]:] == -1) and np.all(np.diff(sidx[:s["nS"]]) > 0) and sidx[0] >= 0 and sidx[s["nS"] - 1] < s["RP"] * s["CP"]
    # the slot index names the support cells: solid cells and their neighbours, i.e. the rows of M that differ from the empty box's
    cells = rows[sidx[:s["nS"]] // s["CP"]] * X + cols[sidx[:s["nS"]] % s["CP"]]
    support = np.array(sorted({r for r, _ in precond._perturbation(active)}))
    np.testing.assert_array_equal(cells, support)
    # gathered slabs, zero in the padding
    np.testing.assert_array_equal(s["QyR"][:s["nR"]], s["Qy"][rows[:s["nR"]]])
    np.testing.assert_array_equal(s["QxC"][:, :s["nC"]], s["Qx"][:, cols[:s["nC"]]])
    np.testing.assert_array_equal(s["QyRt"], s["QyR"].T)
    np.testing.assert_array_equal(s["QxCr"], s["QxC"].T)
    assert not s["QyR"][s["nR"]:].any() and not s["QxC"][:, s["nC"]:].any()
    assert not s["KpT"][s["nS"]:].any() and not s["KpT"][:, s["nS"]:].any()


def test_reference_solves_the_scene_against_sparse_lu(scene):
    name, Y, X, active, _, blob = scene
    lu = spla.splu(sparse_matrix(active))
    b = step_like_rhs(Y, X, 4)
    ref = lu.solve(b.ravel()).reshape(Y, X)
    fluid_cells = active != 0
    err = lambda x: np.linalg.norm((x - ref)[fluid_cells]) / np.linalg.norm(ref[fluid_cells])
    # the algorithm alone, on the unrounded blob: 1e-9 (measured 1e-13)
    blob64 = precond.scattered_solver_blob(active, dtype=np.float64)
    assert blob64.dtype == np.float64 and blob64.size == blob.size
    np.testing.assert_array_equal(blob64[16:16 + Y * Y].astype(np.float32), blob[16:16 + Y * Y])      # the same words, unrounded
    e64 = err(precond.scattered_solve_reference(blob64, b))
    # the device's float32 blob: the same algorithm with matrices rounded to 2^-24 relative, conditioning ~1e4 / step-like rhs: the
    # field tolerance of the GPU tests (1e-5; the issue's float32 restatement measures 3e-6)
    e32 = err(precond.scattered_solve_reference(blob, b))
    print("%s: float64 blob %.3e, float32 blob %.3e" % (name, e64, e32))
    assert e64 < 1e-9, e64
    assert e32 < 1e-5, e32


def test_refusals():
    assert precond.scattered_solver_blob(np.ones((96, 72))) is None                     # the empty box: no perturbation
    many = np.ones((256, 128))
    many[8:248:4, 8:120:4] = 0.0                                                        # 60 x 28 single solid cells, five support cells each
    assert len({r for r, _ in precond._perturbation(many)}) > 4096
    assert precond.scattered_solver_blob(many) is None


def test_equals_the_one_window_solver_on_the_default_sphere():
    Y, X = 128, 64
    active = o.geometry(Y, X).active
    one, sc = precond.direct_solver_blob(active), precond.scattered_solver_blob(active)
    assert one is not None and sc is not None
    assert int(one[:16].view(np.int32)[5]) == precond.scattered_sections(sc)["nS"] == 164
    b = step_like_rhs(Y, X, 4)
    x1, x2 = precond.direct_solve_reference(one, b), precond.scattered_solve_reference(sc, b)
    e = np.linalg.norm(x1 - x2) / np.linalg.norm(x1)
    print("scattered against one-window restatement: %.3e" % e)
    assert e < 1e-10, e


PARENT_SOURCE_SHA256 = {
    "dst_matrix": "e58f17fa69ec6da3ec0ae52299a14d97342df1b48801c49b969aa4dc35cccc10",
    "_perturbation": "32731f8954ac0c122f8eadf8e36816bfce35427e1194db2a0ec2639609f20364",
    "direct_solver_blob": "3152645bf92e22a13a814a2e4992cac17b23e5dc0068a6a9238e2d9e0dddc449",
    "direct_solve_reference": "bc9e268ee918bc7f799e83eb7e502e2dd9e7cffb028c547e2c9d28d957f1be53",
    "box_solver_blob": "92104325f7db0c90e66a8ca9a311c34ffabcd196b7f8ed3c5e00fc131bc136c7",
}


def test_one_window_blob_is_the_parents(golden_dir):
    for fn, sha in PARENT_SOURCE_SHA256.items():
        assert hashlib.sha256(inspect.getsource(getattr(precond, fn)).encode()).hexdigest() == sha, "precond.%s changed" % fn
    assert precond.FD_MAGIC == 0x46443032 and precond.FD_HEADER == 16
    z = np.load(os.path.join(golden_dir, "direct_blob_default_sphere.npz"))
    blob = precond.direct_solver_blob(o.geometry(128, 64).active)
    gold = z["blob_128x64"]
    assert blob.shape == gold.shape and blob.dtype == gold.dtype
    Y, X, SP = 128, 64, 192
    k0 = 16 + Y * Y + X * X + X * Y
    i0 = k0 + SP * SP
    np.testing.assert_array_equal(blob[:16].view(np.int32), gold[:16].view(np.int32))
    np.testing.assert_array_equal(blob[i0:i0 + SP].view(np.int32), gold[i0:i0 + SP].view(np.int32))
    print("one-window blob 128x64 byte-identical to the parent's: %s" % np.array_equal(blob.view(np.int32), gold.view(np.int32)))
    # float sections: float32 roundings of float64 results that may differ in their last bits between BLAS kernels
    for lo, hi in ((16, k0), (i0 + SP, blob.size)):
        np.testing.assert_allclose(blob[lo:hi], gold[lo:hi], rtol=0, atol=2 ** -23)                      # |Q| <= 1, 1/lam <= 1 / lam_min ...
    np.testing.assert_allclose(blob[k0:i0], gold[k0:i0], rtol=1e-6, atol=1e-6 * float(np.abs(gold[k0:i0]).max()))
    big = precond.direct_solver_blob(o.geometry(256, 128).active, max_window=64)
    assert big.size == int(z["words_256x128"])
    np.testing.assert_array_equal(big[:16].view(np.int32), z["header_256x128"])
    Y, X, SP = 256, 128, int(z["header_256x128"][6])
    k0 = 16 + Y * Y + X * X + X * Y
    KpT = big[k0:k0 + SP * SP].reshape(SP, SP)
    np.testing.assert_array_equal(big[k0 + SP * SP:k0 + SP * SP + SP].view(np.int32), z["sidx_256x128"])
    scale = float(np.abs(z["kpt_diag_256x128"]).max())
    np.testing.assert_allclose(np.diag(KpT), z["kpt_diag_256x128"], rtol=1e-6, atol=1e-6 * scale)
    np.testing.assert_allclose(KpT[0], z["kpt_row0_256x128"], rtol=1e-6, atol=1e-6 * scale)
    # the scenes the one-window blob refuses stay refused
    assert precond.direct_solver_blob(active_of(TWO, 256, 128), max_window=64) is None


def test_new_entry_points_are_declared_exported_and_check_their_arguments():
    lib = sol_amd.load()
    assert lib.sol_version() == 216 == _lib.ABI_VERSION
    decl = sol_amd.declared_symbols()
    new = ("sol_karman_step_large_workspace_bytes_for", "sol_karman_step_bwd_large_workspace_bytes_for", "sol_karman_pressure_solve_large_direct")
    for name in new:
        assert name in decl and name in _lib._SIGS and hasattr(lib, name), name
    B, Y, X = 2, 256, 128
    cfg = ops.karman_cfg(B, Y, X, 100.0 / X)
    old = lib.sol_karman_step_large_workspace_bytes(C.byref(cfg))
    assert old == 4 * (B * ((Y + 1) * X + Y * (X + 1)) + B * (3 * Y * X + 2 * Y * 64 + 2 * 64 * 64) + 256)        # what it returned before
    hp = lambda h: h.ctypes.data_as(C.c_void_p)
    fd = np.zeros(16, dtype=np.int32); fd[:8] = [precond.FD_MAGIC, Y, X, 50, 50, 600, 640, 32]
    assert lib.sol_karman_step_large_workspace_bytes_for(C.byref(cfg), None) == old
    assert lib.sol_karman_step_large_workspace_bytes_for(C.byref(cfg), hp(fd)) == old
    sc = np.zeros(16, dtype=np.int32); sc[:9] = [precond.FDS_MAGIC, Y, X, 59, 74, 1194, 1216, 60, 76]
    want = 4 * (B * ((Y + 1) * X + Y * (X + 1)) + B * (3 * Y * X + 2 * Y * 76 + 2 * 60 * 76) + 256)
    assert lib.sol_karman_step_large_workspace_bytes_for(C.byref(cfg), hp(sc)) == want
    # the adjoint's size follows the header in the same way (cfg.direct set selects the direct layout)
    cfg.direct, cfg.direct_n = 4096, 16
    b_old = lib.sol_karman_step_bwd_large_workspace_bytes(C.byref(cfg))
    assert lib.sol_karman_step_bwd_large_workspace_bytes_for(C.byref(cfg), hp(fd)) == b_old
    assert lib.sol_karman_step_bwd_large_workspace_bytes_for(C.byref(cfg), hp(sc)) - b_old == 4 * B * (2 * Y * 76 + 2 * 60 * 76 - 2 * Y * 64 - 2 * 64 * 64)
    # argument checks of the solve alone, all before any launch
    f = lib.sol_karman_pressure_solve_large_direct
    assert f(C.byref(cfg), None, None, FAKE, hp(sc), FAKE, 1 << 30) == -1 and b"NULL" in lib.sol_last_error()
    assert f(C.byref(cfg), None, FAKE, FAKE, hp(sc), FAKE, 1 << 30) == -1 and b"alias" in lib.sol_last_error()
    other = C.c_void_p(8192)
    assert f(C.byref(cfg), None, FAKE, other, hp(sc), FAKE, 1 << 30) == -1 and b"direct_n" in lib.sol_last_error()      # 16 words cannot hold this blob
    cfg.direct_n = 1 << 30
    assert f(C.byref(cfg), None, FAKE, other, hp(sc), FAKE, 16) == -1 and b"workspace too small" in lib.sol_last_error()
    bad = sc.copy(); bad[6] = 1200                                      # SP not a multiple of the kernel's tile
    assert f(C.byref(cfg), None, FAKE, other, hp(bad), FAKE, 1 << 30) == -1 and b"inconsistent" in lib.sol_last_error()
    bad = sc.copy(); bad[1] = 128
    assert f(C.byref(cfg), None, FAKE, other, hp(bad), FAKE, 1 << 30) == -1 and b"grid" in lib.sol_last_error()
    unk = sc.copy(); unk[0] = 0x12345678
    assert f(C.byref(cfg), None, FAKE, other, hp(unk), FAKE, 1 << 30) == -1 and b"first 16 words" in lib.sol_last_error()


def test_python_surface_names_the_solver():
    assert ops.PRESSURE_SOLVERS == ("auto", "direct", "cg", "direct_scattered")
    assert ops.is_direct("direct") and ops.is_direct("direct_scattered") and not ops.is_direct("cg")
    karman.KarmanFlow(pressure_solver="direct_scattered")
    with pytest.raises(NotImplementedError, match="direct_scattered"):
        karman.KarmanFlow(pressure_solver="multigrid")
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    sys.path.insert(0, sdir)
    import argparse
    import _common
    p = argparse.ArgumentParser()
    _common.add_scene_args(p, warm_start=True)
    assert p.parse_args(["--pressure-solver", "direct_scattered"]).pressure_solver == "direct_scattered"
