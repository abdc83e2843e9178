"""karman-2d custom obstacles and the large-grid CG pressure solve, CPU side (no GPU needed): the obstacle specs of the scripts,
KarmanFlow's masks for obstacles / an active mask, the empty-box blob, a float64 restatement of the device PCG against a sparse
direct solve, and the new C entry points' bindings and argument checks (rejected before any launch)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import sol_oracle as o
import sol_amd
from sol_amd import _lib, fluid, karman, precond

FAKE = C.c_void_p(4096)          # never dereferenced: every case below fails validation first


def domain(Y, X):
    return fluid.Domain([Y, X], box=fluid.box[0:200, 0:100])


def centres(Y, X):
    dx = 100.0 / X
    return np.meshgrid((np.arange(Y) + 0.5) * dx, (np.arange(X) + 0.5) * dx, indexing="ij")


# ---- obstacle specs ---------------------------------------------------------------------------------------------------
def test_parse_obstacles_round_trip():
    specs = ["sphere:50,50,10", "sphere:120,50,10", "box:70:73,20:80", "sphere:12.5,30.25,3.5"]
    obs = karman.parse_obstacles(specs)
    assert [type(ob.geometry).__name__ for ob in obs] == ["Sphere", "Sphere", "Box", "Sphere"]
    assert karman.obstacle_spec(obs) == specs
    assert karman.obstacle_spec(karman.parse_obstacles(karman.obstacle_spec(obs))) == specs
    b = obs[2].geometry
    assert b.lower == (70.0, 20.0) and b.upper == (73.0, 80.0)
    assert karman.parse_obstacles("none") == [] and karman.parse_obstacles(["None"]) == []
    assert karman.obstacle_spec(karman.parse_obstacles(" Sphere:1,2,3 ")) == ["sphere:1,2,3"]
    assert sol_amd.parse_obstacles is karman.parse_obstacles


@pytest.mark.parametrize("bad", ["sphere:50,50", "sphere:50,50,0", "sphere:a,b,c", "box:70:73", "box:73:70,20:80",
                                 "box:1:2:3,4:5", "cylinder:1,2,3", "", "sphere"])
def test_parse_obstacles_rejects_malformed_specs(bad):
    with pytest.raises(ValueError, match="bad obstacle spec"):
        karman.parse_obstacles([bad])


def test_none_cannot_be_combined():
    with pytest.raises(ValueError, match="'none' cannot be combined"):
        karman.parse_obstacles(["none", "sphere:50,50,10"])


# ---- KarmanFlow masks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Y,X", [(64, 32), (128, 64), (256, 128)])
def test_obstacle_masks_match_a_hand_computation(Y, X):
    yc, xc = centres(Y, X)
    first = (yc - 50) ** 2 + (xc - 50) ** 2 <= 100
    second = (yc - 120) ** 2 + (xc - 50) ** 2 <= 100
    plate = (yc >= 70) & (yc <= 73) & (xc >= 20) & (xc <= 80)
    assert plate.any() and second.any()
    for specs, solid in ((["sphere:50,50,10", "sphere:120,50,10"], first | second), (["box:70:73,20:80"], plate),
                         (["sphere:50,50,10", "box:70:73,20:80"], first | plate)):
        active, inflow = karman.KarmanFlow(obstacles=karman.parse_obstacles(specs)).scene_arrays(domain(Y, X))
        np.testing.assert_array_equal(active, 1.0 - solid.astype(np.float64))
        np.testing.assert_array_equal(inflow, o.KarmanGeometry(Y, X).inflow)
    active, _ = karman.KarmanFlow(obstacles=[]).scene_arrays(domain(Y, X))
    assert np.all(active == 1.0)


def test_default_scene_is_unchanged():
    for Y, X in ((64, 32), (128, 64), (256, 128)):
        g = o.geometry(Y, X)
        f = karman.KarmanFlow()
        active, inflow = f.scene_arrays(domain(Y, X))
        np.testing.assert_array_equal(active, g.active)
        np.testing.assert_array_equal(inflow, g.inflow)
        assert isinstance(f.obst.geometry, fluid.Sphere) and f.obst.geometry.center == (50.0, 50.0) and f.obst.geometry.radius == 10.0
        assert f.scene() == {"obstacles": ["sphere:50,50,10"], "active": None}
        # the same sphere spelled as an obstacle list gives the same mask
        a2, _ = karman.KarmanFlow(obstacles=karman.parse_obstacles("sphere:50,50,10")).scene_arrays(domain(Y, X))
        np.testing.assert_array_equal(a2, g.active)


def test_active_mask_is_for_one_grid():
    m = np.ones((64, 32))
    m[20:24, 10:20] = 0
    f = karman.KarmanFlow(active=m)
    a, _ = f.scene_arrays(domain(64, 32))
    np.testing.assert_array_equal(a, m)
    with pytest.raises(ValueError, match="exactly one grid"):
        f.scene_arrays(domain(128, 64))
    with pytest.raises(ValueError, match="not both"):
        karman.KarmanFlow(obstacles=[], active=m)
    rec = f.scene()
    assert rec["obstacles"] is None and rec["active"].dtype == np.float32
    assert karman.scenes_equal(rec, karman.scene_record(active=m))
    assert not karman.scenes_equal(rec, karman.scene_record())
    assert karman.scenes_equal(karman.scene_record(obstacles=["sphere:50,50,10"]), karman.scene_record())


# ---- empty-box blob and the PCG restatement ---------------------------------------------------------------------------
def test_box_solver_blob_layout():
    Y, X = 32, 16
    blob = precond.box_solver_blob(Y, X)
    hdr = blob[:16].view(np.int32)
    assert hdr[0] == precond.FD_MAGIC and tuple(hdr[1:8]) == (Y, X, 0, 0, 0, 0, 0) and not hdr[8:].any()
    assert blob.dtype == np.float32 and blob.size == 16 + Y * Y + X * X + X * Y
    o_ = 16
    np.testing.assert_allclose(blob[o_:o_ + Y * Y].reshape(Y, Y), precond.dst_matrix(Y), atol=1e-7)
    o_ += Y * Y
    np.testing.assert_allclose(blob[o_:o_ + X * X].reshape(X, X), precond.dst_matrix(X), atol=1e-7)
    # G = M_r^-1 of the empty box
    b = np.random.default_rng(0).standard_normal((Y, X))
    M = precond.scene_matrix(np.ones((Y, X)))
    np.testing.assert_allclose(precond.box_solve_reference(blob, b).ravel(), np.linalg.solve(M, b.ravel()), rtol=1e-5, atol=1e-6)
    # the direct blob of the default scene keeps its layout (same leading sections)
    d = precond.direct_solver_blob(o.geometry(64, 32).active)
    np.testing.assert_array_equal(d[16:16 + 64 * 64 + 32 * 32 + 32 * 64], precond.box_solver_blob(64, 32)[16:])


def test_pcg_restatement_converges_to_the_sparse_solve():
    Y, X = 64, 32
    active, _ = karman.KarmanFlow(obstacles=karman.parse_obstacles(["sphere:50,50,10", "sphere:120,50,10", "box:150:160,20:80"])
                                  ).scene_arrays(domain(Y, X))
    assert precond.direct_solver_blob(active) is None          # not one 16 x 16 window: the scene the CG path exists for
    rng = np.random.default_rng(3)
    b = rng.standard_normal((Y, X))
    x, its, conv = precond.pcg_reference(active, precond.box_solver_blob(Y, X), b, rtol=1e-10, atol=0.0)
    ref = spla.spsolve(sp.csc_matrix(precond.scene_matrix(active)), b.ravel())
    assert conv and 1 < its < 200, its
    np.testing.assert_allclose(x.ravel(), ref, rtol=1e-7, atol=1e-7 * np.abs(ref).max())
    # the same system as the oracle's pressure matrix (A = -M) of the custom geometry
    g = o.KarmanGeometry(Y, X)
    g.obstacle = 1.0 - active
    g.active = active
    acc = np.pad(active, 1, mode="edge")
    g.diag = np.minimum(-(acc[0:Y, 1:X + 1] + acc[2:Y + 2, 1:X + 1] + acc[1:Y + 1, 0:X] + acc[1:Y + 1, 2:X + 2]), -1.0)
    np.testing.assert_allclose(-g.pressure_matrix().toarray(), precond.scene_matrix(active))
    # a budget too small: reported, not converged
    _, its2, conv2 = precond.pcg_reference(active, precond.box_solver_blob(Y, X), b, rtol=1e-10, atol=0.0, max_iter=2)
    assert its2 == 2 and not conv2


# ---- C ABI ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return sol_amd.load()


NEW = ("sol_karman_step_large_cg_workspace_bytes", "sol_karman_step_fwd_large_cg", "sol_karman_pressure_solve_large")


def test_new_symbols_are_declared_exported_and_bound(lib):
    assert lib.sol_version() == _lib.ABI_VERSION == 216
    decl = _lib.declared_symbols()
    for name in NEW:
        assert name in decl and name in _lib._SIGS and hasattr(lib, name)


def cfg2d(Y=256, X=128, B=2, **kw):
    c = _lib.KarmanCfg(B, Y, X, 100.0 / X, 1.0, float(X), 1e-6, 1e-9, 2000, 0, 0, 0, None, 0, None)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def header(Y=256, X=128, nS=0, SP=0):
    h = np.zeros(16, dtype=np.int32)
    h[:7] = [precond.FD_MAGIC, Y, X, 0, 0, nS, SP]
    return h


def step(lib, c, hdr, ws=1 << 40, info=FAKE, blob=FAKE, vy_out=C.c_void_p(16384), d_out=None):
    return lib.sol_karman_step_fwd_large_cg(C.byref(c), None, None, FAKE, C.c_void_p(8192), FAKE, FAKE, None, FAKE, FAKE, 0,
                                            d_out, vy_out, C.c_void_p(12288), None, None, blob,
                                            None if hdr is None else hdr.ctypes.data_as(C.c_void_p), info, FAKE, ws)


def solve(lib, c, hdr, ws=1 << 40, info=FAKE, rhs=C.c_void_p(8192), p=C.c_void_p(12288), blob=FAKE):
    return lib.sol_karman_pressure_solve_large(C.byref(c), None, FAKE, rhs, p, blob,
                                               None if hdr is None else hdr.ctypes.data_as(C.c_void_p), info, FAKE, ws)


def test_workspace_covers_the_cg_vectors(lib):
    for B, Y, X in ((1, 256, 128), (2, 256, 128), (3, 128, 64)):
        n = lib.sol_karman_step_large_cg_workspace_bytes(C.byref(cfg2d(Y, X, B)))
        assert n >= 4 * B * Y * X * 10 and n < 4 * B * Y * X * 11 + (1 << 20)
    assert lib.sol_karman_step_large_cg_workspace_bytes(None) == 0


@pytest.mark.parametrize("entry", [step, solve])
def test_validation_messages(lib, entry):
    h0 = header()
    cases = [(dict(c=cfg2d(cg_max_iter=0)), b"cg_max_iter must be >= 1"),
             (dict(c=cfg2d(cg_rtol=-1e-6)), b"must be >= 0 and finite"),
             (dict(c=cfg2d(cg_atol=-1.0)), b"must be >= 0 and finite"),
             (dict(c=cfg2d(cg_rtol=float("nan"))), b"must be >= 0 and finite"),
             (dict(c=cfg2d(cg_rtol=0.0, cg_atol=0.0)), b"both zero"),
             (dict(hdr=header(Y=128)), b"the box blob is for a 128x128 grid"),
             (dict(hdr=header(nS=32, SP=64)), b"needs the empty-box blob"),
             (dict(hdr=np.zeros(16, dtype=np.int32)), b"first 16 words of the blob"),
             (dict(hdr=None), b"NULL pointer"),
             (dict(info=None), b"NULL pointer"),
             (dict(blob=None), b"NULL pointer"),
             (dict(ws=0), b"workspace too small"),
             (dict(c=cfg2d(B=0)), b"B in [1, 65535]")]
    for kw, msg in cases:
        c = kw.pop("c", cfg2d())
        hdr = kw.pop("hdr", h0)
        rc = entry(lib, c, hdr, **kw)
        assert rc == -1, (kw, msg)
        assert msg in lib.sol_last_error(), (kw, msg, lib.sol_last_error())


def test_aliasing_is_rejected(lib):
    h0 = header()
    assert step(lib, cfg2d(), h0, vy_out=FAKE) == -1 and b"alias" in lib.sol_last_error()
    assert step(lib, cfg2d(), h0, vy_out=C.c_void_p(4096 * 5), info=C.c_void_p(8192)) == -1 and b"alias" in lib.sol_last_error()
    assert solve(lib, cfg2d(), h0, p=C.c_void_p(8192)) == -1 and b"alias" in lib.sol_last_error()
    assert solve(lib, cfg2d(), h0, p=FAKE) == -1 and b"alias" in lib.sol_last_error()
