"""karman-3d with a periodic spanwise (z) axis, Scene3D(boundaries="periodic-z") (pytest -m gpu): csrc/karman3d_periodic.hip and the
periodic blobs of precond3d against the float64 reference of periodic3d_cases.py -- forward under every transform kernel of a cell, the
velocity adjoint in both scatter forms, the duplicate plane, the true modulo, translation along z, the z-invariant state against the
committed 2-D oracle, the solve alone, the trainer (both schedules, eager and captured), the roll-out, the torch op, the script and
every refusal.  The host side: tests/test_karman3d_periodic_cpu.py.

Tolerances are the suite's (karman3d_shapes): TOL_FIELD = 1e-5 relative L2 on fields and pressures, TOL_GRAD = 1e-4 on gradients in the
trimmed metric (at most TRIM = 1e-3 of the entries left out).  Bit comparisons are torch.equal.  B = 2 throughout."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import sol_amd
import sol_oracle as o2
import sol_oracle3d as o
from sol_amd import _lib
from sol_amd import karman3d as k3
from sol_amd import precond3d as p3

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import karman3d_shapes as ks
import periodic3d_cases as pc
from karman3d_shapes import DEV, TOL_FIELD, TOL_GRAD, f32, rel, sid
from periodic3d_cases import B

pytestmark = pytest.mark.gpu
PZ = "periodic-z"
case_id = lambda c: "%s-%s" % (sid(c[0]), c[1])


@functools.lru_cache(maxsize=None)
def scene(cell, obstacle):
    g = pc.scene_geometry(tuple(cell), obstacle)
    sc = k3.Scene3D(*cell, device=DEV, active=g.active, inflow=g.inflow, velBCy=g.bc_mask, velBCyMask=g.bc_mask,
                    pressure_solver=pc.SOLVER[obstacle], boundaries=PZ)
    assert sc.periodic == (False, False, True) and sc.periodic_bits == 8 and int(sc.direct_header[6]) == 8
    assert int(sc.direct_header[0]) == (p3.FD3E_MAGIC if obstacle == "cylinder" else p3.FD3_MAGIC)
    return g, sc


class options:
    """process-wide kernel options for the block, restored to what they were"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: _lib.get_option(k) for k in self.kw}
        for k, v in self.kw.items():
            _lib.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            _lib.set_option(k, v)


def kernels_of(p):
    return {k.strip("()").replace(" ", "") for k in p.kernels}


def dev_state(st):
    d, v, re = st
    return [f32(d), f32(v[0]), f32(v[1]), f32(v[2]), f32(re)]


def hip_grad(sim, st, w):
    hs = dev_state(st)
    for t in hs[1:4]:
        t.requires_grad_(True)
    out = sim.step(*hs)
    sum((a * f32(b)).sum() for a, b in zip(out[1:], w)).backward()
    torch.cuda.synchronize()
    return tuple(t.detach() for t in out), tuple(h.grad for h in hs[1:4])


# ---- forward -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.SCENES, ids=case_id)
def test_forward_against_the_reference(case):
    """One step at CFL 3 against the float64 reference, TOL_FIELD, under every transform_settings of the cell; the LDS-tile advection and
    the global one agree to 1e-6; the periodic stencil kernels are asserted by name.  On a periodic blob the transforms run as
    fp64-accumulating GEMMs under every setting, so the settings give equal bits.
    Measured on an MI355X: d 7e-8, v_y 9e-8 ... 1.5e-7, v_x 4.5e-7 ... 6.1e-7, v_z 1.2e-6 ... 1.8e-6 (the largest at 32 x 32 x 32, which read
    1.09e-5 with fp32 sums in the matrix-core transforms); tile against global: 0."""
    cell, obstacle = case
    g, sc = scene(cell, obstacle)
    ref, _, st, _, reached = pc.reference(cell, obstacle)
    sim = k3.Karman3DFlow(sc, B)
    outs = {}
    for mfma, fused in ks.transform_settings(*cell):
        for tile in (1, 0):
            if tile == 0 and (mfma, fused) != (1, 1):
                continue
            with options(k3d_mfma_tf=mfma, k3d_fused_tf=fused, k3d_tile=tile), _lib.profile() as prof:
                out = sim.step(*dev_state(st))
                torch.cuda.synchronize()
            ran = kernels_of(prof)
            assert {"k3p_diffuse", "k3p_div", "k3p_project"} <= ran and not ran & {"k3_diffuse", "k3_advect", "k3_advect_tile", "k3_div", "k3_project"}, ran
            assert ("k3p_advect_tile" in ran) == bool(tile and ks.advect_tile_fits(cell[2])), ran
            # the solve of a periodic blob: fp64-accumulating GEMMs only, whatever the transform options say
            assert "k_p_gemm" in ran and not {k for k in ran if k.startswith(("k3_tzx", "k3_ty", "k_l_gemm"))}, ran
            errs = [rel(a, b) for a, b in zip(out, ref)]
            print("periodic forward %s %s cfl %.2f mfma %d fused %d tile %d: %s" % (sid(cell), obstacle, reached, mfma, fused, tile, ["%.3e" % e for e in errs]))
            assert all(bool(torch.isfinite(t).all()) for t in out)
            assert max(errs) < TOL_FIELD, errs
            assert torch.equal(out[3][..., -1], out[3][..., 0])
            outs[(mfma, fused, tile)] = out
    if ks.advect_tile_fits(cell[2]):
        d = [rel(a, b) for a, b in zip(outs[(1, 1, 1)], outs[(1, 1, 0)])]
        print("tile against global advection:", ["%.3e" % e for e in d])
        assert max(d) < 1e-6, d


def test_forward_odd_extents():
    """16 x 9 x 9 (odd Z): the forward step runs (the adjoint refuses odd face counts as on open scenes)"""
    g = pc.scene_geometry(pc.ODD, "cylinder")
    sc = k3.Scene3D(*pc.ODD, device=DEV, active=g.active, inflow=g.inflow, velBCy=g.bc_mask, velBCyMask=g.bc_mask, pressure_solver="direct_extruded", boundaries=PZ)
    (d, v, re), reached = pc.state(pc.ODD, "cylinder")
    with torch.no_grad():
        rd, rv = pc.periodic3d_step(d, v, re, g, True)
    out = k3.Karman3DFlow(sc, B).step(*dev_state((d, v, re)))
    errs = [rel(a, b) for a, b in zip(out, (rd,) + tuple(rv))]
    print("periodic forward 16x9x9 cfl %.2f: %s" % (reached, ["%.3e" % e for e in errs]))
    assert max(errs) < TOL_FIELD, errs


# ---- adjoint -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.SCENES, ids=case_id)
def test_adjoint_against_the_reference_autograd(case):
    """The velocity adjoint against autograd through the float64 reference, TOL_GRAD in the trimmed metric; run twice: bit-identical;
    g_vz_in[..., Z] is exactly zero; on 22 x 10 x 12 and 32 x 32 x 32 the LDS window equals the global atomics bit for bit."""
    cell, obstacle = case
    g, sc = scene(cell, obstacle)
    ref, gref, st, w, _ = pc.reference(cell, obstacle)
    sim = k3.Karman3DFlow(sc, B)
    with _lib.profile() as prof:
        out, grads = hip_grad(sim, st, w)
    ran = kernels_of(prof)
    assert {"k3pb_rhs", "k3pb_gva", "k3pb_diffuse_adj"} <= ran and not ran & {"k3b_rhs", "k3b_gva", "k3b_advect_adj", "k3b_advect_adj_tile", "k3b_diffuse_adj"}, ran
    assert ("k3pb_advect_adj_tile" in ran) == (cell[2] <= 64), ran
    ks.check_grads(grads, gref, "periodic adjoint %s %s" % (sid(cell), obstacle))
    assert float(grads[2][..., -1].abs().max()) == 0.0
    _, again = hip_grad(sim, st, w)
    assert all(torch.equal(a, b) for a, b in zip(grads, again))
    if cell in ((22, 10, 12), (32, 32, 32)):
        with options(k3d_adj_tile=0), _lib.profile() as prof:
            _, glob = hip_grad(sim, st, w)
        assert "k3pb_advect_adj" in kernels_of(prof)
        assert all(torch.equal(a, b) for a, b in zip(grads, glob))


# ---- the duplicate plane -----------------------------------------------------------------------------------------------------------------------
def test_duplicate_plane():
    """NaN in the input v_z[..., Z] changes no output bit; vz_out[..., Z] and saved_vz[..., Z] equal plane 0 bit for bit; a cotangent placed
    on the duplicate plane gives the gradients of the same cotangent on plane 0."""
    cell = (22, 10, 12)
    g, sc = scene(cell, "cylinder")
    _, _, st, w, _ = pc.reference(cell, "cylinder")
    sim = k3.Karman3DFlow(sc, B)
    hs = dev_state(st)
    saved = [torch.empty_like(t) for t in hs[1:4]]
    out = sim._fwd(*hs, saved=saved)
    poisoned = list(hs)
    poisoned[3] = hs[3].clone()
    poisoned[3][..., -1] = float("nan")
    saved2 = [torch.empty_like(t) for t in hs[1:4]]
    out2 = sim._fwd(*poisoned, saved=saved2)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, out2)) and all(torch.equal(a, b) for a, b in zip(saved, saved2))
    assert torch.equal(out[3][..., -1], out[3][..., 0]) and torch.equal(saved[2][..., -1], saved[2][..., 0])
    wz = torch.zeros_like(w[2])
    wz[..., 0] = w[2][..., 0]
    wdup = torch.zeros_like(w[2])
    wdup[..., -1] = w[2][..., 0]
    zero = [torch.zeros_like(t) for t in w[:2]]
    ga = sim._bwd(saved, hs[4], f32(zero[0]), f32(zero[1]), f32(wz))
    gb = sim._bwd(saved, hs[4], f32(zero[0]), f32(zero[1]), f32(wdup))
    torch.cuda.synchronize()
    assert float(ga[2].abs().max()) > 0
    assert all(torch.equal(a, b) for a, b in zip(ga, gb))
    assert float(ga[2][..., -1].abs().max()) == 0.0


# ---- true modulo, translation, the z-invariant state ---------------------------------------------------------------------------------------------
def test_true_modulo_uniform_drift():
    """16 x 8 x 8, a uniform z drift of 10.5 cells per step (more than a period): the departure points wrap by a true modulo"""
    cell = (16, 8, 8)
    g, sc = scene(cell, "cylinder")
    d, v, re = pc.drift_state(cell)
    with torch.no_grad():
        rd, rv = pc.periodic3d_step(d, v, re, g, True)
    for tile in (1, 0):
        with options(k3d_tile=tile):
            out = k3.Karman3DFlow(sc, B).step(*dev_state((d, v, re)))
        errs = [rel(a, b) for a, b in zip(out, (rd,) + tuple(rv))]
        print("uniform z drift of 10.5 cells, tile %d: %s" % (tile, ["%.3e" % e for e in errs]))
        assert max(errs) < TOL_FIELD, errs


def test_translation_along_z():
    """the cylinder at 22 x 10 x 12 with a z-invariant inflow: rolling the unique planes of the input by 3 along z rolls every output by 3"""
    cell = (22, 10, 12)
    g = pc.scene_geometry(cell, "cylinder")
    inflow = np.repeat(g.inflow.max(axis=2, keepdims=True), cell[2], axis=2)
    sc = k3.Scene3D(*cell, device=DEV, active=g.active, inflow=inflow, velBCy=g.bc_mask, velBCyMask=g.bc_mask, pressure_solver="direct_extruded", boundaries=PZ)
    (d, v, re), _ = pc.state(cell, "cylinder")
    roll = lambda t: torch.roll(t, 3, dims=3)
    rolled = (roll(d), pc.seam_sync((roll(v[0]), roll(v[1]), roll(v[2][..., :-1])[..., list(range(cell[2])) + [0]]), True), re)
    sim = k3.Karman3DFlow(sc, B)
    a = sim.step(*dev_state((d, v, re)))
    b = sim.step(*dev_state(rolled))
    expect = (roll(a[0]), roll(a[1]), roll(a[2]), roll(a[3][..., :-1]))
    got = (b[0], b[1], b[2], b[3][..., :-1])
    errs = [rel(x, y) for x, y in zip(got, expect)]
    print("translation by 3 along z:", ["%.3e" % e for e in errs])
    assert max(errs) < TOL_FIELD, errs


def test_z_invariant_state_reduces_to_the_2d_oracle():
    """A z-invariant state with v_z = 0 on the extruded cylinder: every z plane equals sol_oracle.karman_step of the plane (the committed
    2-D oracle; independent of the new reference)"""
    from large2d_scenes import geometry as geometry2d
    cell = (22, 10, 12)
    Y, X, Z = cell
    g = pc.scene_geometry(cell, "cylinder")
    g2 = geometry2d(Y, X, g.active[:, :, 0])
    assert np.array_equal(g2.bc_mask, g.bc_mask[:, :, 0]) and g2.dx == g.dx
    sc = k3.Scene3D(*cell, device=DEV, active=g.active, inflow=k3.extrude_mask(g2.inflow, Z), velBCy=g.bc_mask, velBCyMask=g.bc_mask,
                    pressure_solver="direct_extruded", boundaries=PZ)
    d2, vy2, vx2 = o2.synthetic_state(B, Y, X, 5, project_it=False)
    re = ks.reynolds(B)
    with torch.no_grad():
        d2, vy2, vx2 = (t.float().double() for t in o2.karman_step(d2, vy2, vx2, re, g2))       # spun up
        rd, ry, rx = o2.karman_step(d2, vy2, vx2, re, g2)
    ex = lambda t, n=Z: t.unsqueeze(-1).expand(*t.shape, n).contiguous()
    st = (ex(d2), (ex(vy2), ex(vx2), torch.zeros(B, Y, X, Z + 1, dtype=torch.float64)), re)
    out = k3.Karman3DFlow(sc, B).step(*dev_state(st))
    errs = [rel(out[0], ex(rd)), rel(out[1], ex(ry)), rel(out[2], ex(rx))]
    print("z-invariant state against the 2-D oracle: d, v_y, v_x %s, max |v_z| %.3e" % (["%.3e" % e for e in errs], float(out[3].abs().max())))
    assert max(errs) < TOL_FIELD, errs
    assert float(out[3].abs().max()) < TOL_FIELD * float(ry.abs().max())


# ---- the solve alone ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [((22, 10, 12), "cylinder"), ((22, 10, 12), "sphere"), ((22, 10, 12), "empty"), ((32, 32, 32), "cylinder")], ids=case_id)
def test_pressure_solve_against_float64(case):
    """sol_karman3d_pressure_solve on the periodic blob against the float64 solve, TOL_FIELD; the residual rule of the full-size step test:
    M p - rhs below 2e-5 for right-hand sides of magnitude ~1"""
    cell, obstacle = case
    g, sc = scene(cell, obstacle)
    rhs = pc.periodic_rhs(cell, obstacle)
    ref = pc.solver_of(g, True)(rhs.numpy())
    p = k3.Karman3DFlow(sc, B).pressure_solve(f32(rhs))
    torch.cuda.synchronize()
    e = [rel(p[b], ref[b]) for b in range(B)]
    M = p3.scene_matrix3d(g.active, True)
    pd = p.double().cpu().numpy().reshape(B, -1)
    resid = float(np.abs(np.stack([M @ q for q in pd]) - rhs.numpy().reshape(B, -1)).max())
    print("periodic solve %s %s: %s, residual %.3e (max |rhs| %.3e)" % (sid(cell), obstacle, ["%.3e" % v for v in e], resid, float(rhs.abs().max())))
    assert max(e) < TOL_FIELD, e
    assert resid < 2e-5, resid


# ---- trainer, roll-out, torch op, script -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trainer_case():
    p = pc.trainer_problem()
    return p, pc.trainer_reference(p)


def run_trainer(p, schedule, use_graph):
    g, sc = scene(pc.TRAINER_CELL, "cylinder")
    net = k3.MarsMoon3D(device=DEV)
    net.set_weights([q.detach().numpy() for q in p["params"]])
    tr = k3.Karman3DTrainer(net, sc, B, pc.TRAINER_MS, pc.TRAINER_STD_V, o.STD_RE, use_graph=use_graph, schedule=schedule)
    for _ in range(2 if use_graph else 1):                      # (graph: the second call is a pure replay)
        tr._grads.zero_()
        loss = tr.fwd_bwd(p["d"], *p["v"], p["re"], p["gts"])
    torch.cuda.synchronize()
    return tr, float(loss)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_trainer_sol2_against_the_reference(use_graph):
    """Karman3DTrainer SOL-2 at 16 x 8 x 8 on the periodic cylinder, manual and autograd schedules: loss and gradient against the float64
    reference (the bounds of test_karman3d_trainer_sol2_against_oracle: loss 1e-5, gradient TOL_GRAD, per tensor 3 TOL_GRAD); manual
    against autograd (the bounds of test_karman3d_manual_schedule_equals_autograd_composition); the capture goes through the
    kernel-nodes-only guard (_lib.capture_graph), so the seam sync and fold are kernel nodes."""
    p, (loss, losses, gref, final) = trainer_case()
    res = {}
    for schedule in ("manual", "autograd"):
        tr, hl = run_trainer(p, schedule, use_graph)
        assert (tr._graph is not None) == use_graph
        print("periodic trainer %s %s: loss %.6e against %.6e, gradient %.3e" % (schedule, "graph" if use_graph else "eager", hl, loss, rel(tr.grads, gref)))
        assert abs(hl - loss) < 1e-5 * abs(loss), (hl, loss)
        assert rel(tr.grads, gref) < TOL_GRAD, rel(tr.grads, gref)
        off = tr.net.offsets
        shapes = [q.numel() for q in p["params"]]
        per, at = [], 0
        for k, nk in enumerate(shapes):
            per.append(rel(tr.grads[off[k]:off[k + 1]], gref[at:at + nk]))
            at += nk
        assert max(per) < 3 * TOL_GRAD, per
        for a, b in zip(tr.final, final):
            assert rel(a, b) < TOL_FIELD
        assert torch.equal(tr.final[3][..., -1], tr.final[3][..., 0])
        res[schedule] = (hl, tr.loss_steps.clone(), tr.grads.clone(), [t.clone() for t in tr.final])
        del tr
    lm, la = res["manual"], res["autograd"]
    assert abs(lm[0] - la[0]) < 2e-6 * abs(la[0]), (lm[0], la[0])
    assert rel(lm[1], la[1]) < 2e-6
    assert rel(lm[2], la[2]) < 2e-5, rel(lm[2], la[2])
    for a, b in zip(lm[3], la[3]):
        assert rel(a, b) < 2e-6


def test_rollout_three_steps_against_the_reference():
    p, _ = trainer_case()
    g, sc = scene(pc.TRAINER_CELL, "cylinder")
    net = k3.MarsMoon3D(device=DEV)
    net.set_weights([q.detach().numpy() for q in p["params"]])
    ro = k3.Karman3DRollout(net, sc, B, pc.TRAINER_STD_V, o.STD_RE)
    out = ro.run(f32(p["d"]), *(f32(t) for t in p["v"]), f32(p["re"]), 3)
    torch.cuda.synchronize()
    ref = pc.rollout_reference(p, 3)
    errs = [rel(a, b) for a, b in zip(out, ref)]
    print("periodic roll-out, 3 steps:", ["%.3e" % e for e in errs])
    assert max(errs) < 3 * TOL_FIELD, errs                     # (three steps: three times one step's bound)
    assert torch.equal(out[3][..., -1], out[3][..., 0])


def test_torch_op_backward():
    """torch.ops.sol.karman3d_step on a periodic scene: the outputs and gradients of Karman3DFlow.step, bit for bit"""
    import sol_amd.torch_ops as tops
    cell = (22, 10, 12)
    g, sc = scene(cell, "cylinder")
    _, gref, st, w, _ = pc.reference(cell, "cylinder")
    sim = k3.Karman3DFlow(sc, B)
    h = tops.register_scene3d(sim)
    hs = dev_state(st)
    for t in hs[1:4]:
        t.requires_grad_(True)
    out = torch.ops.sol.karman3d_step(*hs, h)
    sum((a * f32(b)).sum() for a, b in zip(out[1:], w)).backward()
    out2, grads2 = hip_grad(sim, st, w)
    assert all(torch.equal(a, b) for a, b in zip(out, out2))
    assert all(torch.equal(a.grad, b) for a, b in zip(hs[1:4], grads2))
    ks.check_grads([t.grad for t in hs[1:4]], gref, "torch op, periodic")


def test_script_end_to_end(tmp_path):
    """scripts/karman3d.py --boundaries periodic-z at -r 8: generation with the cylinder (direct_extruded is selected), a SOL-2 training demo,
    a corrected roll-out with the model, the setting recorded in params.pickle and with the model and picked up from there"""
    import importlib.util
    import pickle
    from sol_amd import scene as scn
    sdir = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts")
    sys.path.insert(0, sdir)
    spec = importlib.util.spec_from_file_location("sol_script_karman3d_periodic", os.path.join(sdir, "karman3d.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["-r", "8", "-t", "6", "--re", "1.6e5", "-o", str(tmp_path / "run"), "--obstacle", "cylinder", "--boundaries", PZ,
                    "--train-sol", "2", "--train-steps", "2"])
    with open(out + "/params.pickle", "rb") as f:
        params = pickle.load(f)
    assert params["boundaries"] == PZ and params["pressure_solver"] == "direct_extruded"
    v = scn.read_zipped_array(out + "/velo_000005.npz")
    assert np.isfinite(v).all() and np.array_equal(v[0, :16, :8, 8, 2], v[0, :16, :8, 0, 2])          # the duplicate plane of v_z
    assert torch.load(out + "/model3d.pt", weights_only=False)["boundaries"] == PZ
    out2 = mod.main(["-r", "8", "-t", "4", "--re", "1.6e5", "-o", str(tmp_path / "run2"), "--obstacle", "cylinder", "--model", out + "/model3d.pt"])
    with open(out2 + "/params.pickle", "rb") as f:
        assert pickle.load(f)["boundaries"] == PZ               # picked up from the model
    v2 = scn.read_zipped_array(out2 + "/velo_000003.npz")
    assert np.isfinite(v2).all() and np.abs(v2 - scn.read_zipped_array(out + "/velo_000003.npz")).max() > 0


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_message():
    cell = (22, 10, 12)
    g, sc = scene(cell, "cylinder")
    kw = dict(device=DEV, active=g.active, inflow=g.inflow)
    with pytest.raises(ValueError, match="'cg' is not built for periodic scenes"):
        k3.Scene3D(*cell, pressure_solver="cg", boundaries=PZ, **kw)
    scattered = np.ones(cell)
    scattered[2:20:2, 1:9:2, ::2] = 0.0                      # 216 solid cells and their neighbours: more than an eighth of the grid
    with pytest.raises(ValueError, match="does not support this z-periodic scene.*pressure_solver='direct_extruded' takes an obstacle extruded along z"):
        k3.Scene3D(*cell, pressure_solver="auto", boundaries=PZ, active=scattered, inflow=g.inflow, device=DEV)
    for b, msg in ((("periodic", "open", "open"), "a periodic y axis is not built"), (("open", "periodic", "periodic"), "a periodic x axis is not built"),
                   ("periodic", "must be 'open', 'periodic-z' or a triple"), (("open", "open"), "must be 'open', 'periodic-z' or a triple")):
        with pytest.raises(ValueError, match=msg):
            k3.Scene3D(*cell, boundaries=b, **kw)
    assert k3.Scene3D(*cell, boundaries=("open", "open", "periodic"), pressure_solver="direct_extruded", **kw).periodic_bits == 8
    for ctor_kw, msg in ((dict(advection="mac_cormack"), "advection='mac_cormack' is not built for periodic scenes"),
                         (dict(buoyancy=(0.1, 0.0, 0.0)), "a non-zero buoyancy is not built for periodic scenes"),
                         (dict(diffusion_substeps=2), "diffusion_substeps > 1 is not built for periodic scenes"),
                         (dict(density_grad=True), "density_grad is not built for periodic scenes"),
                         (dict(re_grad=True), "re_grad is not built for periodic scenes")):
        with pytest.raises(ValueError, match=msg):
            k3.Karman3DFlow(sc, B, **ctor_kw)
    sim = k3.Karman3DFlow(sc, B)
    _, _, st, w, _ = pc.reference(cell, "cylinder")
    hs = dev_state(st)
    saved = [torch.empty_like(t) for t in hs[1:4]]
    sim._fwd(*hs, saved=saved)
    gd = torch.zeros_like(hs[0])
    for call, msg in ((lambda: k3.density_bwd(sim, hs[0], saved, hs[4], gd), "density_bwd is not built for periodic scenes"),
                      (lambda: k3.advect3d(sim, hs[0], *saved), "advect3d is not built for periodic scenes"),
                      (lambda: k3.advect3d_bwd(sim, hs[0], *saved, gd, *saved), "advect3d_bwd is not built for periodic scenes"),
                      (lambda: k3.diffuse_sub(sim, *hs[1:4], hs[4], 2), "diffuse_sub is not built for periodic scenes")):
        with pytest.raises(ValueError, match=msg):
            call()
    # the C entries on a periodic blob: SOL_ERR_ARG with a message
    import ctypes as C
    from sol_amd._lib import SolError, check, ptr, stream
    lib, hdr = sim.lib, sc.direct_header.ctypes.data_as(C.c_void_p)
    out = [torch.empty_like(t) for t in hs[:4]]
    fwd_args = (C.byref(sim.cfg), stream(), *(ptr(t) for t in hs), ptr(sc.active), ptr(sc.inflow), ptr(sc.velBCy), ptr(sc.velBCyMask), sc.bc_stride,
                *(ptr(t) for t in out), None, None, None, None, None, hdr, ptr(sim.workspace), sim.workspace_bytes)
    with pytest.raises(SolError, match="sol_karman3d_step_fwd_buoy is not built for a z-periodic blob"):
        check(lib.sol_karman3d_step_fwd_buoy(*fwd_args, 0.0, 0.0, 0.0))
    with pytest.raises(SolError, match="sol_karman3d_step_fwd_adv is not built for a z-periodic blob"):
        check(lib.sol_karman3d_step_fwd_adv(*fwd_args, 0.0, 0.0, 0.0, 0, 1.0))
    gi = [torch.empty_like(t) for t in saved]
    bwd_args = (C.byref(sim.cfg), stream(), *(ptr(t) for t in saved), ptr(hs[4]), ptr(sc.active), ptr(sc.velBCyMask), sc.bc_stride,
                *(ptr(t) for t in saved), *(ptr(t) for t in gi), hdr, ptr(sim.workspace), sim.workspace_bytes)
    g_re = torch.zeros(B, dtype=torch.float32, device=DEV)      # (explicit: another module of the suite may have left float64 as the default dtype)
    sim._ws(lib.sol_karman3d_step_bwd_re_workspace_bytes(C.byref(sim.cfg)))
    bwd_args = bwd_args[:-2] + (ptr(sim.workspace), sim.workspace_bytes)
    with pytest.raises(SolError, match="sol_karman3d_step_bwd_re is not built for a z-periodic blob"):
        check(lib.sol_karman3d_step_bwd_re(*bwd_args, *(ptr(t) for t in hs[1:4]), ptr(g_re), 0))
    with pytest.raises(SolError, match="sol_karman3d_step_bwd_buoy is not built for a z-periodic blob"):
        check(lib.sol_karman3d_step_bwd_buoy(*bwd_args, 0.0, 0.0, 0.0, None, ptr(gd)))
    cg = k3.Karman3DCfg.from_buffer_copy(sim.cfg)
    cg.pressure_solver = 1
    with pytest.raises(SolError, match=r"pressure_solver = 1 \(CG\) is not built for a z-periodic blob"):
        check(lib.sol_karman3d_pressure_solve(C.byref(cg), stream(), ptr(sc.active), ptr(hs[0]), ptr(out[0]), hdr, ptr(sim.workspace), sim.workspace_bytes))
    bad = sc.direct_header.copy()
    bad[6] = 2
    with pytest.raises(SolError, match="only the z axis"):
        check(lib.sol_karman3d_pressure_solve(C.byref(sim.cfg), stream(), ptr(sc.active), ptr(hs[0]), ptr(out[0]), bad.ctypes.data_as(C.c_void_p),
                                              ptr(sim.workspace), sim.workspace_bytes))
    with pytest.raises(SolError, match="only the z axis"):
        check(lib.sol_karman3d_seam_sync(stream(), ptr(hs[3]), B, *cell, 4))
    # the helpers: sync copies plane 0, fold is its adjoint
    vz = hs[3].clone()
    vz[..., -1] = 7.0
    assert torch.equal(k3.seam_sync3d(sc, vz)[..., -1], hs[3][..., 0])
    gz = f32(w[2]).clone()
    k3.seam_fold3d(sc, gz)
    assert torch.equal(gz[..., 0], f32(w[2])[..., 0] + f32(w[2])[..., -1]) and float(gz[..., -1].abs().max()) == 0.0
