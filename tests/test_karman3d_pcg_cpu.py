"""karman-3d preconditioned CG pressure solve, CPU side: the extended sol_karman3d_cfg mirror matches the library, the CG solve
asks for its own workspace, and the entry points reject bad solver fields and mismatched blobs with a message before any launch
(no GPU needed).  Scene3D's solver choice is host logic too, but it uploads to the device: tests/test_gpu_karman3d_pcg.py."""
import ctypes as C

import numpy as np
import pytest

import sol_oracle3d as o
import sol_amd
from sol_amd import _lib, precond3d as p3

FAKE = C.c_void_p(4096)          # never dereferenced: every case below fails validation first


@pytest.fixture(scope="module")
def lib():
    return sol_amd.load()


def cfg3d(Y=32, X=16, Z=16, B=2, hdr=None, **kw):
    nS, SP = (0, 0) if hdr is None else (int(hdr[4]), int(hdr[5]))
    words = 16 + Y * Y + X * X + Z * Z + Y * X * Z + SP * SP + SP
    c = _lib.Karman3DCfg(B, Y, X, Z, 100.0 / X, 1.0, float(X), 0, 0, words, FAKE.value)
    c.pressure_solver, c.cg_max_iter, c.cg_rtol, c.cg_atol = 1, 100, 1e-6, 1e-9
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def header(Y=32, X=16, Z=16, nS=0, SP=0):
    h = np.zeros(16, dtype=np.int32)
    h[:6] = [p3.FD3_MAGIC, Y, X, Z, nS, SP]
    return h


def fwd(lib, c, hdr, ws_bytes=1 << 40):
    return lib.sol_karman3d_step_fwd(C.byref(c), None, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 0,
                                     FAKE, FAKE, FAKE, FAKE, None, None, None, None, None,
                                     hdr.ctypes.data_as(C.c_void_p), FAKE, ws_bytes)


def bwd(lib, c, hdr, ws_bytes=1 << 40):
    return lib.sol_karman3d_step_bwd(C.byref(c), None, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 0, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE,
                                     hdr.ctypes.data_as(C.c_void_p), FAKE, ws_bytes)


def test_extended_cfg_mirror_matches_the_library(lib):
    assert lib.sol_version() == _lib.ABI_VERSION == 216
    c = cfg3d()
    assert lib.sol_abi_size_karman3d() == C.sizeof(c)
    names = [f[0] for f in _lib.Karman3DCfg._fields_]
    assert names[-5:] == ["pressure_solver", "cg_max_iter", "cg_rtol", "cg_atol", "cg_info"]
    # the 11-argument positional form still constructs the struct, with an all-zero (= direct solve) tail
    old = _lib.Karman3DCfg(2, 128, 64, 64, 1.5625, 1.0, 64.0, 0, 0, 0, None)
    assert (old.pressure_solver, old.cg_max_iter, old.cg_rtol, old.cg_atol, old.cg_info) == (0, 0, 0.0, 0.0, None)


def test_cg_workspace_is_larger_than_the_direct_one(lib):
    for (B, Y, X, Z) in ((2, 32, 16, 16), (1, 128, 64, 64), (1, 256, 128, 128)):
        d = cfg3d(Y, X, Z, B, pressure_solver=0)
        g = cfg3d(Y, X, Z, B)
        nd, ng = lib.sol_karman3d_step_workspace_bytes(C.byref(d)), lib.sol_karman3d_step_workspace_bytes(C.byref(g))
        bd, bg = lib.sol_karman3d_step_bwd_workspace_bytes(C.byref(d)), lib.sol_karman3d_step_bwd_workspace_bytes(C.byref(g))
        cells = B * Y * X * Z * 4
        assert ng - nd >= 4 * cells and bg - bd >= 4 * cells            # x, two p buffers, q (+ the fp64 slabs)
        assert ng - nd < 4 * cells + (1 << 20)


@pytest.mark.parametrize("entry", [fwd, bwd])
def test_bad_solver_fields_are_rejected_before_any_launch(lib, entry):
    h0 = header()
    cases = [(dict(pressure_solver=2), b"pressure_solver must be 0"),
             (dict(pressure_solver=-1), b"pressure_solver must be 0"),
             (dict(cg_max_iter=0), b"cg_max_iter must be >= 1"),
             (dict(cg_rtol=0.0), b"cg_rtol must be > 0"),
             (dict(cg_rtol=-1e-6), b"cg_rtol must be > 0"),
             (dict(cg_atol=-1.0), b"cg_atol must be >= 0"),
             (dict(cg_rtol=float("nan")), b"cg_rtol must be > 0")]
    for kw, msg in cases:
        rc = entry(lib, cfg3d(**kw), h0)
        assert rc == -1, kw
        assert msg in lib.sol_last_error(), (kw, lib.sol_last_error())
    # a capacitance blob (nS > 0) is refused by the CG solve ...
    hs = header(nS=32, SP=64)
    rc = entry(lib, cfg3d(hdr=hs), hs)
    assert rc == -1 and b"needs the blob without capacitance part" in lib.sol_last_error()
    # ... a grid mismatch by both
    rc = entry(lib, cfg3d(), header(Y=64))
    assert rc == -1 and b"grid" in lib.sol_last_error()
    # valid cfgs get past the solver checks (and stop at the workspace size, still before any launch): the direct solve keeps
    # accepting both blobs (nS = 0 is the empty box), the CG fields are not checked for it (the all-zero tail of older callers)
    for c, h in ((cfg3d(), h0), (cfg3d(pressure_solver=0), h0), (cfg3d(hdr=hs, pressure_solver=0), hs),
                 (cfg3d(pressure_solver=0, cg_max_iter=0, cg_rtol=0.0, cg_atol=0.0), h0)):
        rc = entry(lib, c, h, ws_bytes=0)
        assert rc == -1 and b"workspace too small" in lib.sol_last_error(), lib.sol_last_error()


def test_cg_preconditioner_blob_is_the_empty_box_for_every_oracle_obstacle():
    """The CG scene's blob is direct_solver_blob3d(np.ones_like(active)): no capacitance part, whatever the obstacle; the
    direct blob refuses the cylinder at 128 x 64 x 64 (the case the CG solve exists for) and builds the sphere."""
    for ob in ("sphere", "cylinder"):
        g = o.geometry(32, 16, 16, obstacle=ob)
        blob = p3.direct_solver_blob3d(np.ones_like(g.active))
        assert tuple(blob[:16].view(np.int32)[1:6]) == (32, 16, 16, 0, 0)
        assert p3.direct_solver_blob3d(g.active) is not None
    assert p3.direct_solver_blob3d(o.geometry(128, 64, 64, obstacle="cylinder").active) is None
