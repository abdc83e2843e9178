"""Host side of the z-periodic karman-3d step (no GPU): the float64 reference of periodic3d_cases.py tied to the committed oracles, the
periodic blobs of precond3d against a float64 LU, the default blobs unchanged, the float32 run of the reference alone inside the suite's
bounds on every case of the GPU tests, refusals by message, the script's record, the ABI.  The device side: test_gpu_karman3d_periodic.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import sol_amd
import sol_oracle as o2
import sol_oracle3d as o
from sol_amd import _lib, karman3d as k3, precond3d as p3

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import karman3d_shapes as ks
import periodic3d_cases as pc
from karman3d_shapes import TOL_FIELD, TOL_GRAD, TRIM, rel, sid, trimmed_rel

FAKE = C.c_void_p(4096)          # never dereferenced: every library case below fails validation first
B = pc.B
PZ = "periodic-z"
# the blobs hold float32 tables (relative rounding 6e-8 per entry) and the restatement applies twelve transforms and two scalings of them:
# 1e-6 relative L2 against the float64 LU (a tenth of TOL_FIELD)
TOL_BLOB = 1e-6
case_id = lambda c: "%s-%s" % (sid(c[0]), c[1])


def active_of(cell, obstacle):
    return np.ones(cell) if obstacle == "empty" else o.geometry(*cell, obstacle=obstacle).active


@pytest.mark.parametrize("kw", [{}, dict(grad_pad="dirichlet0", inflow_order="before")], ids=["default", "dirichlet0-before"])
@pytest.mark.parametrize("case", [((22, 10, 12), "sphere"), ((16, 8, 8), "cylinder")], ids=case_id)
def test_reference_with_periodic_off_is_the_oracle(case, kw):
    """periodic3d_step(pz=False) equals sol_oracle3d.karman3d_step to float64 round-off"""
    cell, obstacle = case
    g = o.geometry(*cell, obstacle=obstacle)
    d, v, re = ks.state(B, cell, ks.SEED, g)
    with torch.no_grad():
        od, ov = o.karman3d_step(d, v, re, g, **kw)
        pd, pv = pc.periodic3d_step(d, v, re, g, False, **kw)
    for a, b in zip((od,) + tuple(ov), (pd,) + tuple(pv)):
        assert float((a - b).abs().max()) < 1e-13


def test_z_invariant_state_reduces_to_the_2d_oracle():
    """a z-invariant state with v_z = 0 on the extruded cylinder: every plane of the periodic reference equals sol_oracle.karman_step of
    the plane -- the new reference tied to the committed 2-D oracle"""
    from large2d_scenes import geometry as geometry2d
    import copy
    cell = (22, 10, 12)
    Y, X, Z = cell
    g = copy.copy(pc.scene_geometry(cell, "cylinder"))
    g2 = geometry2d(Y, X, g.active[:, :, 0])
    assert np.array_equal(g2.bc_mask, g.bc_mask[:, :, 0]) and g2.dx == g.dx
    g.inflow = k3.extrude_mask(g2.inflow, Z)
    d2, vy2, vx2 = o2.synthetic_state(B, Y, X, 5, project_it=False)
    re = ks.reynolds(B)
    ex = lambda t: t.unsqueeze(-1).expand(*t.shape, Z).contiguous()
    with torch.no_grad():
        d2, vy2, vx2 = (t.float().double() for t in o2.karman_step(d2, vy2, vx2, re, g2))
        rd, ry, rx = o2.karman_step(d2, vy2, vx2, re, g2)
        od, ov = pc.periodic3d_step(ex(d2), (ex(vy2), ex(vx2), torch.zeros(B, Y, X, Z + 1, dtype=torch.float64)), re, g, True)
    for a, b in zip((od, ov[0], ov[1]), (rd, ry, rx)):
        assert float((a - ex(b)).abs().max()) < 1e-13
    assert float(ov[2].abs().max()) < 1e-13


@pytest.mark.parametrize("obstacle", ["sphere", "cylinder", "empty"])
@pytest.mark.parametrize("cell", [(22, 10, 12), (16, 8, 8)], ids=sid)
def test_periodic_blobs_solve_the_periodic_system(cell, obstacle):
    """periodic_solve_reference3d on both periodic blobs (where they build) against a dense float64 solve of scene_matrix3d(active, True);
    header word 6 = 8; Q_z is the Hartley matrix: symmetric, its own inverse"""
    act = active_of(cell, obstacle)
    M = p3.scene_matrix3d(act, True).toarray()
    assert np.array_equal(M, M.T)
    b = np.random.default_rng(0).standard_normal(cell)
    x = np.linalg.solve(M, b.ravel()).reshape(cell)
    why = []
    dense = p3.periodic_solver_blob3d(act, why)
    assert dense is not None, why
    built = [dense]
    ext = p3.extruded_solver_blob3d(act, why, periodic=True)
    if obstacle == "cylinder":
        assert ext is not None, why
        built.append(ext)
    else:
        assert ext is None and ("depends on z" in why[-1] or "no obstacle" in why[-1])
    Y, X, Z = cell
    for blob in built:
        hdr = blob[:16].view(np.int32)
        assert p3.blob_periodic_bits3d(blob) == p3.PERIODIC_Z == 8 and list(hdr[1:4]) == list(cell)
        Qz = blob[16 + Y * Y + X * X:16 + Y * Y + X * X + Z * Z].astype(np.float64).reshape(Z, Z)
        assert np.array_equal(Qz, Qz.T) or np.abs(Qz - Qz.T).max() < 1e-7
        assert np.abs(Qz @ Qz - np.eye(Z)).max() < 1e-6
        e = rel(p3.periodic_solve_reference3d(blob, b), x)
        print("periodic blob %s %s magic %x: %.3e" % (sid(cell), obstacle, hdr[0], e))
        assert e < TOL_BLOB, e
    with pytest.raises(AssertionError, match="not a z-periodic blob"):
        p3.periodic_solve_reference3d(p3.direct_solver_blob3d(act), b)


def test_open_scene_matrix_is_the_oracles():
    g = o.geometry(22, 10, 12, obstacle="sphere")
    assert abs(p3.scene_matrix3d(g.active) + g.pressure_matrix()).max() == 0.0


def test_default_blobs_are_what_they_were():
    """with the keyword absent the extruded builder, which gained the keyword in place, gives the blob it gave before: compared with
    tests/golden/extruded_blob_default_cylinder_16x8x8.npz, written by the builder as it stood before the keyword existed (the recipe of
    test_scattered_direct_cpu.test_one_window_blob_is_the_parents: integer sections exact, float sections to the last bits that BLAS kernels may
    move).  The dense open builder is pinned by test_karman3d_extruded_cpu.py.  The periodic blob differs in Q_z, 1 / lambda, K' and word 6."""
    Y, X, Z = cell = (16, 8, 8)
    act = o.geometry(*cell, obstacle="cylinder").active
    blob = p3.extruded_solver_blob3d(act)
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "extruded_blob_default_cylinder_16x8x8.npz"))["blob_16x8x8"]
    assert blob.shape == gold.shape and blob.dtype == gold.dtype
    SP2 = int(gold[:16].view(np.int32)[5])
    k0 = 16 + Y * Y + X * X + Z * Z + Y * X * Z
    i0 = k0 + Z * SP2 * SP2
    assert i0 + SP2 == gold.size
    np.testing.assert_array_equal(blob[:16].view(np.int32), gold[:16].view(np.int32))
    np.testing.assert_array_equal(blob[i0:].view(np.int32), gold[i0:].view(np.int32))
    print("default extruded blob 16x8x8 byte-identical to the golden one: %s" % np.array_equal(blob.view(np.int32), gold.view(np.int32)))
    np.testing.assert_allclose(blob[16:k0], gold[16:k0], rtol=0, atol=2 ** -22)          # |Q| <= 1, 1 / lambda < 4 at this grid: one float32 ulp there
    np.testing.assert_allclose(blob[k0:i0], gold[k0:i0], rtol=1e-6, atol=1e-6 * float(np.abs(gold[k0:i0]).max()))
    assert p3.blob_periodic_bits3d(blob) == 0 and blob.tobytes() == p3.extruded_solver_blob3d(act, periodic=False).tobytes()
    per = p3.extruded_solver_blob3d(act, periodic=True)
    assert per.shape == blob.shape and p3.blob_periodic_bits3d(per) == 8
    assert not np.allclose(per[16 + Y * Y + X * X:k0], gold[16 + Y * Y + X * X:k0], rtol=0, atol=1e-3)      # Q_z and 1 / lambda are other tables
    assert p3.blob_periodic_bits3d(p3.direct_solver_blob3d(act)) == 0


def test_a_seam_crossing_obstacle_spans_the_axis():
    """the dense periodic builder's window rule: an obstacle lying across the z seam has a window over the whole axis; where that window
    is too large the builder refuses with a sentence"""
    cell = (64, 32, 64)
    act = np.ones(cell)
    act[20:40, 6:26, :3] = 0.0
    act[20:40, 6:26, -3:] = 0.0
    why = []
    assert p3.periodic_solver_blob3d(act, why) is None and "does not fit one window" in why[0] and "seam" in why[0]
    inside = np.ones(cell)
    inside[28:32, 14:18, 30:34] = 0.0
    assert p3.periodic_solver_blob3d(inside) is not None


@pytest.mark.parametrize("case", pc.SCENES, ids=case_id)
def test_float32_reference_alone_stays_inside_the_bounds(case):
    """TRIM is a cap, not a knob: the float32 run of the reference alone, against float64, stays inside TOL_FIELD and TOL_GRAD with at most
    the TRIM share left out, on every case of the GPU tests (a case that does not gets another seed in periodic3d_cases.SEEDS)"""
    cell, obstacle = case
    out, grads, st, w, reached = pc.reference(cell, obstacle)
    assert abs(reached - pc.CFL_TARGET) < 0.01
    assert torch.equal(out[3][..., -1], out[3][..., 0]) and float(grads[2][..., -1].abs().max()) == 0.0
    g = pc.scene_geometry(cell, obstacle)
    d, v, re = st
    leaves = [t.float().clone().requires_grad_(True) for t in v]
    od, ov = pc.periodic3d_step(d.float(), tuple(leaves), re.float(), g, True)
    sum((a * b.float()).sum() for a, b in zip(ov, w)).backward()
    ef = [rel(a, b) for a, b in zip((od,) + tuple(ov), out)]
    eg = [trimmed_rel(l.grad, gr) for l, gr in zip(leaves, grads)]
    print("float32 reference alone %s %s: fields %s, gradients %s" % (sid(cell), obstacle, ["%.2e" % e for e in ef], ["%.2e (%d out)" % (e[0], e[1]) for e in eg]))
    assert max(ef) < TOL_FIELD, ef
    for (e, k, _), gr in zip(eg, grads):
        assert k <= int(TRIM * gr.numel()) and e < TOL_GRAD, (e, k)


def test_float32_reference_alone_on_the_drift_state():
    """the true-modulo state (a z drift of 10.5 cells per step at 16 x 8 x 8): the float32 run of the reference alone stays inside
    TOL_FIELD, and the departure points do lie more than a period away"""
    g = pc.scene_geometry((16, 8, 8), "cylinder")
    d, v, re = pc.drift_state()
    assert float(v[2].min()) / g.dx > 8.0
    with torch.no_grad():
        rd, rv = pc.periodic3d_step(d, v, re, g, True)
        fd, fv = pc.periodic3d_step(d.float(), tuple(t.float() for t in v), re.float(), g, True)
    errs = [rel(a, b) for a, b in zip((fd,) + tuple(fv), (rd,) + tuple(rv))]
    print("float32 reference alone on the drift state:", ["%.2e" % e for e in errs])
    assert max(errs) < TOL_FIELD / 10, errs


def test_duplicate_plane_of_the_reference_is_never_read():
    cell = (16, 8, 8)
    g = pc.scene_geometry(cell, "cylinder")
    (d, v, re), _ = pc.state(cell, "cylinder")
    poisoned = (v[0], v[1], v[2].clone())
    poisoned[2][..., -1] = float("nan")
    with torch.no_grad():
        a = pc.periodic3d_step(d, v, re, g, True)
        b = pc.periodic3d_step(d, poisoned, re, g, True)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


def test_boundaries_argument_and_scene_refusals():
    assert k3.boundaries_arg3d("open") == (False, False, False) and k3.boundaries_arg3d(PZ) == (False, False, True)
    assert k3.boundaries_arg3d(("open", "open", "periodic")) == (False, False, True) and k3.boundaries_name3d((False, False, True)) == PZ
    for b, msg in ((("periodic", "open", "open"), "a periodic y axis is not built for karman-3d"), (("open", "periodic", "periodic"), "a periodic x axis is not built"),
                   ("periodic", "must be 'open', 'periodic-z' or a triple"), (("open", "open"), "must be 'open', 'periodic-z' or a triple"),
                   (("open", "open", "wall"), "must be 'open', 'periodic-z' or a triple"), (None, "must be 'open', 'periodic-z' or a triple")):
        with pytest.raises(ValueError, match=msg):
            k3.boundaries_arg3d(b)
    cell = (22, 10, 12)
    g = pc.scene_geometry(cell, "cylinder")
    kw = dict(device="cpu", active=g.active, inflow=g.inflow)
    with pytest.raises(ValueError, match="'cg' is not built for periodic scenes"):
        k3.Scene3D(*cell, pressure_solver="cg", boundaries=PZ, **kw)
    scattered = np.ones(cell)
    scattered[2:20:2, 1:9:2, ::2] = 0.0
    with pytest.raises(ValueError, match="does not support this z-periodic scene.*pressure_solver='direct_extruded' takes an obstacle extruded along z"):
        k3.Scene3D(*cell, pressure_solver="auto", boundaries=PZ, device="cpu", active=scattered, inflow=g.inflow)
    with pytest.raises(ValueError, match="direct_extruded' does not support this scene.*depends on z"):
        k3.Scene3D(*cell, pressure_solver="direct_extruded", boundaries=PZ, device="cpu", active=scattered, inflow=g.inflow)
    for solver, magic in (("auto", p3.FD3_MAGIC), ("direct", p3.FD3_MAGIC), ("direct_extruded", p3.FD3E_MAGIC)):
        sc = k3.Scene3D(*cell, pressure_solver=solver, boundaries=PZ, **kw)
        assert sc.periodic == (False, False, True) and sc.periodic_bits == 8 and list(sc.direct_header[[0, 6]]) == [magic, 8]
        assert sc.pressure_solver == ("direct_extruded" if solver == "direct_extruded" else "direct")
        assert float(sc.velBCyMask[:, 1:-1, 0].sum()) == 2 * 8 and float(sc.velBCyMask[:, 0].min()) == 1.0      # no z walls on a periodic span
    sc0 = k3.Scene3D(*cell, **kw)
    assert sc0.periodic == (False, False, False) and sc0.periodic_bits == 0 and int(sc0.direct_header[6]) == 0
    assert float(sc0.velBCyMask[:, :, 0].min()) == 1.0
    # what is not built for periodic scenes is refused at construction, by name, before the device is asked for
    for ctor_kw, msg in ((dict(advection="mac_cormack"), "advection='mac_cormack' is not built for periodic scenes"),
                         (dict(buoyancy=(0.1, 0.0, 0.0)), "a non-zero buoyancy is not built for periodic scenes"),
                         (dict(diffusion_substeps=2), "diffusion_substeps > 1 is not built for periodic scenes"),
                         (dict(density_grad=True), "density_grad is not built for periodic scenes"),
                         (dict(re_grad=True), "re_grad is not built for periodic scenes")):
        with pytest.raises(ValueError, match=msg):
            k3.Karman3DFlow(sc, B, **ctor_kw)


def hdr3(magic=p3.FD3_MAGIC, Y=32, X=16, Z=16, nS=0, SP=0, flags=8):
    h = np.zeros(16, dtype=np.int32)
    h[:7] = [magic, Y, X, Z, nS, SP, flags]
    return h


def cfg_of(h, solver=0):
    Y, X, Z, SP = (int(v) for v in (h[1], h[2], h[3], h[5]))
    words = 16 + Y * Y + X * X + Z * Z + Y * X * Z + (Z * SP * SP if h[0] == p3.FD3E_MAGIC else SP * SP) + SP
    c = _lib.Karman3DCfg(2, Y, X, Z, 100.0 / X, 1.0, float(X), 0, 0, words, FAKE.value)
    c.pressure_solver, c.cg_max_iter, c.cg_rtol, c.cg_atol = solver, 100, 1e-6, 1e-9
    return c


def test_library_dispatches_on_the_flags_word_and_refuses_by_message():
    """header word 6: 0 and 8 pass the check (and stop at the workspace size, before any launch), 2 and 4 are rejected; on a periodic blob
    CG and the _buoy, _adv and _re forms return SOL_ERR_ARG with a message; the ABI number is 216 and sizeof the cfg is unchanged"""
    lib = sol_amd.load()
    assert lib.sol_version() == _lib.ABI_VERSION == 216
    assert lib.sol_abi_size_karman3d() == C.sizeof(_lib.Karman3DCfg) == 72
    P = lambda h: h.ctypes.data_as(C.c_void_p)
    fwd_head = lambda c: (C.byref(c), None, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 0, FAKE, FAKE, FAKE, FAKE, None, None, None, None, None)
    bwd_head = lambda c: (C.byref(c), None, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 0, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE)
    err = lambda: lib.sol_last_error().decode()
    for flags in (0, 8):
        for magic, nS, SP in ((p3.FD3_MAGIC, 0, 0), (p3.FD3E_MAGIC, 20, 32)):
            h = hdr3(magic, nS=nS, SP=SP, flags=flags)
            c = cfg_of(h)
            assert lib.sol_karman3d_step_fwd(*fwd_head(c), P(h), FAKE, 0) == -1 and "workspace too small" in err(), err()
            assert lib.sol_karman3d_step_bwd(*bwd_head(c), P(h), FAKE, 0) == -1 and "workspace too small" in err(), err()
            assert lib.sol_karman3d_pressure_solve(C.byref(c), None, FAKE, FAKE, FAKE, P(h), FAKE, 0) == -1 and "workspace too small" in err(), err()
    for flags in (2, 4, 10, 1):
        h = hdr3(flags=flags)
        assert lib.sol_karman3d_step_fwd(*fwd_head(cfg_of(h)), P(h), FAKE, 1 << 40) == -1 and "only the z axis (8) is built" in err(), err()
    h = hdr3()
    c = cfg_of(h)
    big = 1 << 40
    assert lib.sol_karman3d_step_fwd(*fwd_head(cfg_of(h, solver=1)), P(h), FAKE, big) == -1 and "pressure_solver = 1 (CG) is not built for a z-periodic blob" in err()
    assert lib.sol_karman3d_step_fwd_buoy(*fwd_head(c), P(h), FAKE, big, 0.0, 0.0, 0.0) == -1
    assert "sol_karman3d_step_fwd_buoy is not built for a z-periodic blob" in err(), err()
    assert lib.sol_karman3d_step_fwd_adv(*fwd_head(c), P(h), FAKE, big, 0.0, 0.0, 0.0, 0, 1.0) == -1
    assert "sol_karman3d_step_fwd_adv is not built for a z-periodic blob" in err(), err()
    assert lib.sol_karman3d_step_bwd_re(*bwd_head(c), P(h), FAKE, big, FAKE, FAKE, FAKE, FAKE, 0) == -1
    assert "sol_karman3d_step_bwd_re is not built for a z-periodic blob" in err(), err()
    assert lib.sol_karman3d_step_bwd_buoy(*bwd_head(c), P(h), FAKE, big, 0.0, 0.0, 0.0, None, FAKE) == -1
    assert "sol_karman3d_step_bwd_buoy is not built for a z-periodic blob" in err(), err()
    assert lib.sol_karman3d_step_bwd_adv(*bwd_head(c), P(h), FAKE, big, 0.0, 0.0, 0.0, None, None, 0, 1.0) == -1
    assert "sol_karman3d_step_bwd_adv is not built for a z-periodic blob" in err(), err()
    # the seam entries: 0 launches nothing, 2 and 4 are refused
    assert lib.sol_karman3d_seam_sync(None, FAKE, 2, 16, 8, 8, 0) == 0 and lib.sol_karman3d_seam_fold(None, FAKE, 2, 16, 8, 8, 0) == 0
    for bits in (2, 4):
        assert lib.sol_karman3d_seam_sync(None, FAKE, 2, 16, 8, 8, bits) == -1 and "only the z axis (8) is built" in err()
        assert lib.sol_karman3d_seam_fold(None, FAKE, 2, 16, 8, 8, bits) == -1 and "only the z axis (8) is built" in err()
    assert {"sol_karman3d_seam_sync", "sol_karman3d_seam_fold"} <= set(_lib.declared_symbols())


def test_the_scripts_boundaries_flag_parses_records_and_agrees():
    """scripts/karman3d.py --boundaries open|periodic-z: recorded in the parameters (what params.pickle holds) as "boundaries", a model's
    record wins, and with --obstacle cylinder it selects direct_extruded unless another solver is named"""
    import importlib.util
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    sys.path.insert(0, sdir)
    spec = importlib.util.spec_from_file_location("sol_script_karman3d_periodic_cpu", os.path.join(sdir, "karman3d.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rec = lambda *a, model_record=None: mod.apply_model_record(mod.parse_params(list(a)), model_record)
    assert mod.parse_params([])["boundaries"] is None and rec()["boundaries"] == "open" and rec("--boundaries", PZ)["boundaries"] == PZ
    assert rec()["pressure_solver"] == "auto" and rec("--boundaries", PZ)["pressure_solver"] == "auto"
    assert rec("--obstacle", "cylinder")["pressure_solver"] == "auto"
    assert rec("--boundaries", PZ, "--obstacle", "cylinder")["pressure_solver"] == "direct_extruded"
    assert rec("--boundaries", PZ, "--obstacle", "cylinder", "--pressure-solver", "direct")["pressure_solver"] == "direct"
    with pytest.raises(SystemExit):
        mod.parse_params(["--boundaries", "periodic-x"])
    model = {"obstacle": "cylinder", "boundaries": PZ, "buoyancy": None}
    got = rec("--model", "m.pt", model_record=model)
    assert got["boundaries"] == PZ and got["pressure_solver"] == "direct_extruded"
    assert rec("--model", "m.pt", "--boundaries", PZ, model_record=model)["boundaries"] == PZ
    with pytest.raises(SystemExit, match="--boundaries open contradicts"):
        rec("--model", "m.pt", "--boundaries", "open", model_record=model)
    assert rec("--model", "m.pt", model_record={"buoyancy": None})["boundaries"] == "open"          # no record: open
