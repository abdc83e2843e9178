"""karman-3d direct pressure solve for obstacles extruded along z, CPU side: precond3d.extruded_solver_blob3d and its float64
restatement against a sparse LU of the oracle's pressure matrix, the blob's sizes against the dense blob's table, its refusals, the
untouched dense blob, the scene helpers, and the library's check of an extruded header (no GPU needed: every call fails validation
before any launch).  The device side: tests/test_gpu_karman3d_extruded.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import sol_oracle3d as o
import sol_amd
from sol_amd import _lib, karman3d as k3, precond3d as p3

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import karman3d_shapes as ks
from karman3d_shapes import sid

LU_CELLS = [(16, 9, 9), (22, 10, 12), (24, 12, 72), (32, 32, 32)]
FAKE = C.c_void_p(4096)          # never dereferenced: every library case below fails validation first


def cylinder(cell):
    return ks.geometry(cell, "cylinder")


def header_of(blob):
    return [int(v) for v in blob[:16].view(np.int32)[:6]]


@pytest.mark.parametrize("cell", LU_CELLS, ids=sid)
def test_extruded_blob_solves_the_oracle_system(cell):
    """extruded_solve_reference3d on the blob against a sparse LU of -geometry(cell, "cylinder").pressure_matrix(), for the right-hand sides
    the step's solve sees (no divergence inside the obstacle) and white ones (non-zero inside it).  Bound: the dense blob's in
    test_karman3d_cpu.py, max |x - p| < 1e-6 max |p| (fp32 storage of the blob).
    Measured: 1.0e-7 ... 7.9e-7 (the largest at 32 x 32 x 32)."""
    g = cylinder(cell)
    blob = p3.extruded_solver_blob3d(g.active)
    Y, X, Z = cell
    magic, hy, hx, hz, nS2, SP2 = header_of(blob)
    assert magic == p3.FD3E_MAGIC and (hy, hx, hz) == cell and 0 < nS2 <= SP2 and SP2 % 32 == 0 and SP2 - nS2 < 32
    assert blob.dtype == np.float32 and blob.size == 16 + Y * Y + X * X + Z * Z + Y * X * Z + Z * SP2 * SP2 + SP2
    # Qy, Qx, Qz and invlam stand where the dense blob has them: the empty-box solve and the CG preconditioner read either
    head = 16 + Y * Y + X * X + Z * Z + Y * X * Z
    assert np.array_equal(blob[16:head], p3.direct_solver_blob3d(np.ones(cell))[16:head])
    sidx2 = blob[-SP2:].view(np.int32)
    assert np.all(sidx2[nS2:] == -1) and np.all(np.diff(sidx2[:nS2]) > 0) and sidx2[0] >= 0 and sidx2[nS2 - 1] < Y * X
    lu = spla.splu((-g.pressure_matrix()).astype(np.float64).tocsc())
    for name, rhs in (("step-like", ks.step_like_rhs(2, cell).numpy() * g.active), ("white", ks.white_rhs(2, cell).numpy())):
        for b in rhs:
            x = p3.extruded_solve_reference3d(blob, b)
            p = lu.solve(b.ravel()).reshape(cell)
            e = np.abs(x - p).max() / np.abs(p).max()
            print("%s %s: max error %.3e of max |p|" % (sid(cell), name, e))
            assert e < 1e-6


def test_in_plane_set_times_z_is_the_dense_set():
    """nS2 Z equals the dense blob's nS (karman3d_shapes.BLOBS) on the cylinder of every cell of the table: the dense set is the in-plane
    set in every layer.  At 128 x 64 x 64: nS2 = 164, SP2 = 192"""
    for cell in ks.CELLS:
        g = cylinder(cell)
        S2 = p3._perturbation2d(g.active[:, :, 0])[0]
        assert len(S2) * cell[2] == ks.BLOBS[(cell, "cylinder")][0], cell
        assert p3.extruded_solver_refusal3d(g.active) is None
    blob = p3.extruded_solver_blob3d(o.geometry(128, 64, 64, obstacle="cylinder").active)
    assert header_of(blob) == [p3.FD3E_MAGIC, 128, 64, 64, 164, 192]
    assert blob.size == 16 + 128 * 128 + 2 * 64 * 64 + 128 * 64 * 64 + 64 * 192 * 192 + 192


@pytest.mark.parametrize("cell", [(22, 10, 12), (48, 24, 8)], ids=sid)
def test_extruded_reference_agrees_with_the_dense_one(cell):
    """the same cylinder through the dense blob (direct_solve_reference3d) and the extruded one: two float32 roundings of one solution
    (each within 1e-6 of it in the test above, so within 2e-6 of each other).  Measured: 1.1e-7, 1.4e-7"""
    g = cylinder(cell)
    dense, ext = p3.direct_solver_blob3d(g.active), p3.extruded_solver_blob3d(g.active)
    assert header_of(dense)[4:] == list(ks.BLOBS[(cell, "cylinder")])
    for b in ks.white_rhs(2, cell).numpy():
        xd, xe = p3.direct_solve_reference3d(dense, b), p3.extruded_solve_reference3d(ext, b)
        e = np.abs(xd - xe).max() / np.abs(xd).max()
        print("%s dense against extruded: %.3e" % (sid(cell), e))
        assert e < 2e-6


def test_refusals_each_with_its_message():
    cell = (22, 10, 12)
    cases = []
    cases.append((ks.geometry(cell, "sphere").active, "depends on z"))
    a = cylinder(cell).active.copy()
    j, i = np.argwhere(a[:, :, 0] == 0)[0]
    a[j, i, 5] = 1.0                                        # one cell changed at one k
    cases.append((a, "depends on z"))
    cases.append((np.ones(cell), "no obstacle"))
    big = np.ones((64, 64))
    big[::2, ::2] = 0.0                                     # 1024 solid cells, every cell of the plane perturbed: beyond SP2 = 1024
    cases.append((k3.extrude_mask(big, 8), "size cap"))
    wide = np.ones((44, 44))
    wide[4:40:2, 4:40:2] = 0.0                              # nS2 = 37^2 - 19^2 = 1008: SP2 = 1024 fits, Z SP2^2 = 72 * 2^20 does not
    assert len(p3._perturbation2d(wide)[0]) == 1008
    cases.append((k3.extrude_mask(wide, 72), "size cap"))
    assert p3.extruded_solver_refusal3d(k3.extrude_mask(wide, 64)) is None      # ... and 64 * 2^20 = 2^26 does
    cases.append((k3.extrude_mask(cylinder(cell).active[:, :, 0], 129), "Z = 129"))
    for act, msg in cases:
        why = []
        assert p3.extruded_solver_blob3d(act, why) is None
        assert len(why) == 1 and msg in why[0], (msg, why)
        assert msg in p3.extruded_solver_refusal3d(act)
        assert p3.extruded_solver_blob3d(act) is None       # without the list: None, nothing raised
    # Z = 128 is accepted (the header alone: the blob of this tiny plane builds in a moment)
    blob = p3.extruded_solver_blob3d(k3.extrude_mask(cylinder((16, 9, 9)).active[:, :, 0], 128))
    assert header_of(blob)[3:] == [128, 5, 32]


# sha256 of inspect.getsource of what builds and restates the dense blob, on the commit before "direct_extruded"
PARENT_SOURCE_SHA256 = {
    "direct_solver_blob3d": "33edcbae147f566c6498f3f1acff627920decd47de6093ebf97315c378c1a232",
    "_perturbation3d": "b068b241e49fe31af867c2c724c4e4550117da1f05ed5bf43a76e9718f99728e",
    "_green_on_window": "023317c8d364aa60a6797bc19950794907356a4e0ba48cbc39a6ca2b07900255",
    "_accessible_diag": "39e8223ab18dc1b1652d71d219267a1d78badfed3f4216bbf097d3c63385c148",
    "rect_eigenvalues": "9e73c10c3036a22c20031cfc5b0ec2d754f25ef2f40f354c15a655c2716c8b52",
    "direct_solve_reference3d": "6635322137cdbf7129990a6fac3d46eb5c1d17ad4445a4c997405b30e21cd15e",
}


def test_the_dense_blob_is_what_it_was():
    """"auto", "direct" and "cg" build their blobs with direct_solver_blob3d alone: its headers and sizes on the sphere and the cylinder at
    22 x 10 x 12 are the table's, the source of every function it runs is the parent commit's (as test_scattered_direct_cpu.py holds the 2-D blob), and it
    still refuses the cylinder at 128 x 64 x 64: "auto" sends that scene to CG as it did"""
    import hashlib
    import inspect
    for fn, sha in PARENT_SOURCE_SHA256.items():
        assert hashlib.sha256(inspect.getsource(getattr(p3, fn)).encode()).hexdigest() == sha, "precond3d.%s changed" % fn
    assert p3.FD3_MAGIC == 0x46443333 and p3.FD3_HEADER == 16 and p3.FD3_MAX_S == 8192
    cell = (22, 10, 12)
    Y, X, Z = cell
    for ob in ("sphere", "cylinder"):
        blob = p3.direct_solver_blob3d(ks.geometry(cell, ob).active)
        nS, SP = ks.BLOBS[(cell, ob)]
        assert header_of(blob) == [p3.FD3_MAGIC, Y, X, Z, nS, SP]
        assert blob.size == 16 + Y * Y + X * X + Z * Z + Y * X * Z + SP * SP + SP
    assert p3.direct_solver_blob3d(o.geometry(128, 64, 64, obstacle="cylinder").active) is None
    assert k3.PRESSURE_SOLVERS3D == ("auto", "direct", "cg", "direct_extruded")


def test_cylinder_arrays_equal_the_oracle_geometry():
    for cell in ((32, 16, 16), (128, 64, 64), (22, 10, 12)):
        g = o.geometry(*cell, obstacle="cylinder")
        active, inflow = k3.cylinder_arrays3d(*cell)
        assert active.dtype == np.float64 and np.array_equal(active, g.active) and np.array_equal(inflow, g.inflow)
    with pytest.raises(NotImplementedError):
        k3.scene_arrays3d(32, 16, 16, obstacle="cylinder")


def test_extrude_mask_round_trip():
    rng = np.random.default_rng(3)
    m = (rng.random((7, 5)) < 0.5).astype(np.float32)
    e = k3.extrude_mask(m, 4)
    assert e.shape == (7, 5, 4) and e.dtype == np.float64 and e.flags["C_CONTIGUOUS"] and e.flags["WRITEABLE"]
    assert all(np.array_equal(e[:, :, k], m) for k in range(4))
    assert np.array_equal(k3.extrude_mask(e[:, :, 0], 4), e)
    for bad in ((np.ones(3), 4), (np.ones((3, 3, 3)), 4), (m, 0), (m, 2.0)):
        with pytest.raises(ValueError, match="extrude_mask"):
            k3.extrude_mask(*bad)


# ---- the library's check of an extruded header ---------------------------------------------------------------------------------------
def ext_words(Y, X, Z, SP2):
    return 16 + Y * Y + X * X + Z * Z + Y * X * Z + Z * SP2 * SP2 + SP2


def ext_header(Y=32, X=16, Z=16, nS2=20, SP2=32):
    h = np.zeros(16, dtype=np.int32)
    h[:6] = [p3.FD3E_MAGIC, Y, X, Z, nS2, SP2]
    return h


def ext_cfg(h, words=None, solver=0):
    Y, X, Z = (int(v) for v in h[1:4])
    c = _lib.Karman3DCfg(2, Y, X, Z, 100.0 / X, 1.0, float(X), 0, 0, ext_words(Y, X, Z, int(h[5])) if words is None else words, FAKE.value)
    c.pressure_solver, c.cg_max_iter, c.cg_rtol, c.cg_atol = solver, 100, 1e-6, 1e-9
    return c


def fwd(lib, c, hdr, ws_bytes=1 << 40):
    return lib.sol_karman3d_step_fwd(C.byref(c), None, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 0,
                                     FAKE, FAKE, FAKE, FAKE, None, None, None, None, None,
                                     hdr.ctypes.data_as(C.c_void_p), FAKE, ws_bytes)


def bwd(lib, c, hdr, ws_bytes=1 << 40):
    return lib.sol_karman3d_step_bwd(C.byref(c), None, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 0, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE,
                                     hdr.ctypes.data_as(C.c_void_p), FAKE, ws_bytes)


@pytest.mark.parametrize("entry", [fwd, bwd])
def test_library_checks_an_extruded_header_before_any_launch(entry):
    lib = sol_amd.load()
    good = ext_header()
    bad = [(ext_header(SP2=48), None, b"extruded direct-solver blob header is inconsistent (nS2 20, SP2 48"),      # not a multiple of 32
           (ext_header(nS2=40), None, b"header is inconsistent (nS2 40, SP2 32"),                                  # more cells than columns
           (ext_header(nS2=0), None, b"header is inconsistent (nS2 0"),                                            # no obstacle: the dense blob's scene
           (ext_header(SP2=1056, nS2=1040), None, b"header is inconsistent"),                                      # beyond 1024 (and beyond Y X)
           (ext_header(Y=8, X=8, Z=16, SP2=96, nS2=60), None, b"header is inconsistent"),                          # beyond Y X = 64: the scratch
           (ext_header(Y=16, X=8, Z=130), None, b"header is inconsistent"),                                        # Z beyond 128
           (good, ext_words(32, 16, 16, 32) - 1, b"extruded direct-solver blob has"),                              # word count
           (good, 16 + 32 * 32 + 2 * 16 * 16 + 32 * 16 * 16 + 32 * 32 + 32, b"extruded direct-solver blob has")]   # the dense blob's count
    for h, words, msg in bad:
        rc = entry(lib, ext_cfg(h, words), h)
        assert rc == -1 and msg in lib.sol_last_error(), (h[:6].tolist(), words, lib.sol_last_error())
    # a grid mismatch, and the CG solve on a blob with a capacitance part, are refused as they are for the dense blob
    rc = entry(lib, ext_cfg(ext_header()), ext_header(Y=64))
    assert rc == -1 and b"grid" in lib.sol_last_error()
    rc = entry(lib, ext_cfg(good, solver=1), good)
    assert rc == -1 and b"needs the blob without capacitance part" in lib.sol_last_error()
    # an unknown magic keeps its message
    h = ext_header()
    h[0] = 0x46443346
    rc = entry(lib, ext_cfg(h), h)
    assert rc == -1 and b"direct_header_host must be the first 16 words" in lib.sol_last_error()
    # a consistent header passes the check and stops at the workspace size, still before any launch; Z = 128 and SP2 = 1024 are taken
    for h in (good, ext_header(Y=16, X=8, Z=128, nS2=5, SP2=32), ext_header(Y=64, X=64, Z=64, nS2=1000, SP2=1024)):
        rc = entry(lib, ext_cfg(h), h, ws_bytes=0)
        assert rc == -1 and b"workspace too small" in lib.sol_last_error(), lib.sol_last_error()


def test_the_scripts_obstacle_flag_parses_records_and_agrees():
    """scripts/karman3d.py --obstacle sphere|cylinder and --pressure-solver direct_extruded: recorded in the parameters (what params.pickle
    holds) as "obstacle", and a model's record wins.  parse_params and apply_model_record touch no device."""
    import importlib.util
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    sys.path.insert(0, sdir)
    spec = importlib.util.spec_from_file_location("sol_script_karman3d_extruded", os.path.join(sdir, "karman3d.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rec = lambda *a, model_record=None: mod.apply_model_record(mod.parse_params(list(a)), model_record)["obstacle"]
    assert mod.parse_params([])["obstacle"] is None and rec() == "sphere" and rec("--obstacle", "cylinder") == "cylinder"
    assert mod.parse_params(["--pressure-solver", "direct_extruded"])["pressure_solver"] == "direct_extruded"
    with pytest.raises(SystemExit):
        mod.parse_params(["--obstacle", "cube"])
    with pytest.raises(SystemExit):
        mod.parse_params(["--obstacle", "cylinder", "--obstacle-mask", "m.npy"])
    model = {"obstacle": "cylinder", "buoyancy": None}
    assert rec("--model", "m.pt", model_record=model) == "cylinder" and rec("--model", "m.pt", "--obstacle", "cylinder", model_record=model) == "cylinder"
    with pytest.raises(SystemExit, match="--obstacle sphere contradicts"):
        rec("--model", "m.pt", "--obstacle", "sphere", model_record=model)
    assert rec("--model", "m.pt", model_record={"buoyancy": None}) == "sphere"                        # no record: the sphere
    assert rec("--model", "m.pt", "--obstacle", "cylinder", model_record={"buoyancy": None}) == "cylinder"
