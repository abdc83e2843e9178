"""Adjoint of the karman-3d marker density and gradient with respect to the Reynolds number, CPU side (no GPU needed): the new C entry
points' declarations, bindings, workspace sizes and argument checks (rejected before any launch), the new option, the two flags of
Karman3DFlow, to_feature3d's gradient with respect to re, and the input condition of the GPU tests
(test_gpu_karman3d_density_re_adjoint.py): for every case of karman3d_adjoint_cases.py the oracle in float32 agrees with the oracle in
float64 UNTRIMMED -- no departure point sits close enough to a cell boundary for fp32 to decide it differently.  Measured 6.4e-6 at most
(g_vx of 20_comb); pinned below 2e-5, the project's figure from test_karman2d_density_adjoint_cpu.py.  If an oracle default moves, this
test fails and the GPU test's inputs are re-examined rather than silently trimmed."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import sol_amd
import sol_oracle3d as o
from sol_amd import _lib
from sol_amd import karman3d as k3

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import karman3d_adjoint_cases as kc
from large2d_scenes import rel

NEW = ("sol_karman3d_density_bwd_workspace_bytes", "sol_karman3d_density_bwd", "sol_karman3d_density_bwd_re_workspace_bytes",
       "sol_karman3d_density_bwd_re", "sol_karman3d_step_bwd_re_workspace_bytes", "sol_karman3d_step_bwd_re")
P = lambda v: C.c_void_p(v)
FD3_MAGIC = 0x46443333


@pytest.fixture(scope="module")
def lib():
    return sol_amd.load()


def cfg3d(Y=16, X=8, Z=8, B=2, **kw):
    """cfg with a fake device blob pointer (never dereferenced) of the size the empty-box blob has"""
    c = _lib.Karman3DCfg(B, Y, X, Z, 100.0 / X, 1.0, float(X), 0, 0, 16 + Y * Y + X * X + Z * Z + Y * X * Z, 1 << 20, 0, 0, 0.0, 0.0, None)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def header(c):
    h = np.zeros(16, dtype=np.int32)
    h[:4] = (FD3_MAGIC, c.Y, c.X, c.Z)
    return h


def partial_bytes(c):
    """the partial sums of the Reynolds-number reduction: one double per workgroup of 256 threads x 8 faces (256 workgroups at most) and
    simulation, eight bytes of alignment, 256-byte granule"""
    faces = (c.Y + 1) * c.X * c.Z + c.Y * (c.X + 1) * c.Z + c.Y * c.X * (c.Z + 1)
    nblk = min(max(-(-faces // 2048), 1), 256)
    return -(-(c.B * nblk * 8 + 8) // 256) * 256


def dens_call(lib, c, ws=1 << 40, re_form=False, **kw):
    """sol_karman3d_density_bwd(_re) on fake device pointers: never dereferenced, every case below fails validation first"""
    a = dict(d_in=P(4096), inflow=P(8192), saved_vy=P(12288), saved_vx=P(16384), saved_vz=P(20480), re=P(24576), bcm=P(28672),
             g_d_out=P(32768), g_d_in=P(36864), g_vy_in=P(40960), g_vx_in=P(45056), g_vz_in=P(49152), workspace=P(1 << 16),
             vy_in=P(3 << 16), vx_in=P(4 << 16), vz_in=P(5 << 16), g_re=P(6 << 16))
    a.update(kw)
    args = [C.byref(c) if c is not None else None, None, a["d_in"], a["inflow"], a["saved_vy"], a["saved_vx"], a["saved_vz"], a["re"], a["bcm"], 0,
            a["g_d_out"], a["g_d_in"], a["g_vy_in"], a["g_vx_in"], a["g_vz_in"], 0, a["workspace"], ws]
    if re_form:
        return lib.sol_karman3d_density_bwd_re(*args, a["vy_in"], a["vx_in"], a["vz_in"], a["g_re"], 0)
    return lib.sol_karman3d_density_bwd(*args)


def step_re_call(lib, c, ws=1 << 40, **kw):
    a = dict(saved_vy=P(12288), saved_vx=P(16384), saved_vz=P(20480), re=P(24576), active=P(8192), bcm=P(28672),
             g_vy_out=P(32768), g_vx_out=P(36864), g_vz_out=P(4096), g_vy_in=P(40960), g_vx_in=P(45056), g_vz_in=P(49152), workspace=P(1 << 16),
             vy_in=P(3 << 16), vx_in=P(4 << 16), vz_in=P(5 << 16), g_re=P(6 << 16))
    a.update(kw)
    h = header(c)
    return lib.sol_karman3d_step_bwd_re(C.byref(c), None, a["saved_vy"], a["saved_vx"], a["saved_vz"], a["re"], a["active"], a["bcm"], 0,
                                        a["g_vy_out"], a["g_vx_out"], a["g_vz_out"], a["g_vy_in"], a["g_vx_in"], a["g_vz_in"],
                                        h.ctypes.data_as(C.c_void_p), a["workspace"], ws, a["vy_in"], a["vx_in"], a["vz_in"], a["g_re"], 0)


def test_new_symbols_are_declared_exported_and_bound(lib):
    assert lib.sol_version() == _lib.ABI_VERSION == 216          # additions only: the ABI number stays
    assert lib.sol_abi_size_karman3d() == C.sizeof(_lib.Karman3DCfg)
    decl = _lib.declared_symbols()
    for name in NEW:
        assert name in decl and name in _lib._SIGS and hasattr(lib, name)
    assert _lib.get_option("k3d_dens_adj_tile") == 1
    _lib.set_option("k3d_dens_adj_tile", 0)
    try:
        assert _lib.get_option("k3d_dens_adj_tile") == 0
    finally:
        _lib.set_option("k3d_dens_adj_tile", 1)
    with pytest.raises(_lib.SolError, match="must be in"):
        _lib.set_option("k3d_dens_adj_tile", 2)


def test_workspaces_are_the_plain_calls_plus_the_partial_sums(lib):
    for B in (1, 2, 6):
        for Y, X, Z in ((16, 8, 8), (20, 10, 10), (32, 16, 16), (128, 64, 64)):
            c = cfg3d(Y, X, Z, B)
            n = lib.sol_karman3d_density_bwd_workspace_bytes(C.byref(c))
            own = B * Y * X * Z * (8 + 4 + 4 + 4) + B * 64 * 4          # int64 accumulators, gU_y, gU_x, gU_z, absmax slots
            assert own <= n < own + 4096, (B, Y, X, Z, n, own)
            assert lib.sol_karman3d_density_bwd_re_workspace_bytes(C.byref(c)) == n + partial_bytes(c)
            plain = lib.sol_karman3d_step_bwd_workspace_bytes(C.byref(c))
            assert lib.sol_karman3d_step_bwd_re_workspace_bytes(C.byref(c)) == plain + partial_bytes(c)
            cg = cfg3d(Y, X, Z, B, pressure_solver=1, cg_max_iter=10)
            plain_cg = lib.sol_karman3d_step_bwd_workspace_bytes(C.byref(cg))
            assert plain_cg > plain and lib.sol_karman3d_step_bwd_re_workspace_bytes(C.byref(cg)) == plain_cg + partial_bytes(cg)
    for f in (lib.sol_karman3d_density_bwd_workspace_bytes, lib.sol_karman3d_density_bwd_re_workspace_bytes, lib.sol_karman3d_step_bwd_re_workspace_bytes):
        assert f(None) == 0


@pytest.mark.parametrize("re_form", [False, True])
def test_density_bwd_rejects_bad_arguments_with_their_message(lib, re_form):
    who = b"sol_karman3d_density_bwd_re" if re_form else b"sol_karman3d_density_bwd"
    size = lib.sol_karman3d_density_bwd_re_workspace_bytes if re_form else lib.sol_karman3d_density_bwd_workspace_bytes
    need = size(C.byref(cfg3d()))
    cases = [(dict(c=None), b"cfg is NULL"),
             (dict(c=cfg3d(B=0)), b"B in [1, 65535]"),
             (dict(c=cfg3d(B=65536)), b"B in [1, 65535]"),
             (dict(c=cfg3d(Y=7)), b"Y, X, Z >= 8"),
             (dict(c=cfg3d(Z=4)), b"Y, X, Z >= 8"),
             (dict(c=cfg3d(Y=1 << 11, X=1 << 10, Z=1 << 10)), b"grid too large"),
             (dict(c=cfg3d(Y=16, X=9, Z=9)), b"odd face count"),
             (dict(workspace=P((1 << 16) + 4)), b"16-byte aligned"),
             (dict(ws=0), b"workspace too small"),
             (dict(ws=need - 1), b"workspace too small"),
             (dict(c=cfg3d(inflow_before=1), inflow=None), b"inflow_before needs the inflow mask"),
             (dict(g_d_in=P(4096)), b"alias"),                       # = d_in
             (dict(g_vy_in=P(12288)), b"alias"),                     # = saved_vy
             (dict(g_vz_in=P(32768)), b"alias"),                     # = g_d_out
             (dict(g_vy_in=P(45056)), b"buffers of their own"),      # = g_vx_in
             (dict(g_d_in=P(49152)), b"buffers of their own")]       # = g_vz_in
    names = ["d_in", "saved_vy", "saved_vx", "saved_vz", "re", "bcm", "g_d_out", "g_d_in", "g_vy_in", "g_vx_in", "g_vz_in", "workspace"]
    if re_form:
        names += ["vy_in", "vx_in", "vz_in", "g_re"]
        cases += [(dict(g_re=P(24576)), b"alias"), (dict(g_vx_in=P(5 << 16)), b"alias"), (dict(g_re=P(36864)), b"buffers of their own")]
    for name in names:
        cases.append(({name: None}, b"NULL pointer"))
    for kw, msg in cases:
        kw = dict(kw)
        c = kw.pop("c", cfg3d())
        assert dens_call(lib, c, re_form=re_form, **kw) == -1, (kw, msg)
        err = lib.sol_last_error()
        assert msg in err and (c is None or who + b":" in err), (kw, msg, err)
    # the plain form does not ask for the partial sums
    if re_form:
        assert dens_call(lib, cfg3d(), ws=need - partial_bytes(cfg3d()), re_form=True) == -1 and b"workspace too small" in lib.sol_last_error()


def test_step_bwd_re_rejects_bad_arguments_with_their_message(lib):
    need = lib.sol_karman3d_step_bwd_re_workspace_bytes(C.byref(cfg3d()))
    plain = lib.sol_karman3d_step_bwd_workspace_bytes(C.byref(cfg3d()))
    cases = [(dict(c=cfg3d(Y=7)), b"Y, X, Z >= 8"),
             (dict(c=cfg3d(B=0)), b"B >= 1"),
             (dict(c=cfg3d(Y=16, X=9, Z=9)), b"odd face count"),
             (dict(workspace=P((1 << 16) + 8)), b"16-byte aligned"),
             (dict(ws=plain), b"workspace too small"),                # the plain call's size does not hold the partial sums
             (dict(ws=need - 1), b"workspace too small"),
             (dict(g_re=P(40960)), b"buffer of its own"),            # = g_vy_in
             (dict(vx_in=P(49152)), b"alias"),                       # = g_vz_in
             (dict(g_re=P(24576)), b"alias")]                        # = re
    for name in ("saved_vy", "saved_vx", "saved_vz", "re", "active", "bcm", "g_vy_out", "g_vx_out", "g_vz_out", "g_vy_in", "g_vx_in", "g_vz_in",
                 "workspace", "vy_in", "vx_in", "vz_in", "g_re"):
        cases.append(({name: None}, b"NULL pointer"))
    for kw, msg in cases:
        kw = dict(kw)
        c = kw.pop("c", cfg3d())
        assert step_re_call(lib, c, **kw) == -1, (kw, msg)
        assert msg in lib.sol_last_error(), (kw, msg, lib.sol_last_error())


def test_karman3d_flow_takes_the_two_flags():
    p = inspect.signature(k3.Karman3DFlow.__init__).parameters
    assert p["density_grad"].default is False and p["re_grad"].default is False
    assert callable(k3.density_bwd)


def test_to_feature3d_keeps_a_tensor_re_in_the_graph():
    B, Y, X, Z = 2, 4, 3, 5
    gen = torch.Generator().manual_seed(1)
    v = [torch.randn(s, generator=gen, dtype=torch.float64) for s in ((B, Y + 1, X, Z), (B, Y, X + 1, Z), (B, Y, X, Z + 1))]
    w = torch.randn(B, Y, X, Z, 4, generator=gen, dtype=torch.float64)
    grads = []
    for fn in (lambda a, r: k3.to_feature3d(a[0], a[1], a[2], r), o.to_feature):
        leaves = [t.clone().requires_grad_(True) for t in v] + [torch.tensor([3.0, 5.0], dtype=torch.float64, requires_grad=True)]
        f = fn(leaves[:3], leaves[3])
        assert f.requires_grad
        (f * w).sum().backward()
        grads.append([t.grad for t in leaves])
    for a, b in zip(*grads):
        assert a is not None and torch.allclose(a, b, rtol=1e-14, atol=0)
    # an re without a gradient: as before, none is formed
    leaves = [t.clone().requires_grad_(True) for t in v]
    re = torch.tensor([3.0, 5.0], dtype=torch.float64)
    (k3.to_feature3d(*leaves, re) * w).sum().backward()
    assert re.grad is None and all(torch.equal(a.grad, b) for a, b in zip(leaves, grads[1][:3]))


def test_the_cases_module_spells_the_oracles_step():
    for name in ("16_dens", "16_dirichlet", "32_cfl"):
        c = kc.case(name)
        d, v, re = kc.state(name)
        B, Y, X, Z = c["shape"]
        with torch.no_grad():
            got = kc.step(d, v, re, name)
            ref = o.karman3d_step(d, v, re, o.geometry(Y, X, Z), dt=c["dt"], res=X, grad_pad=c["kw"].get("grad_pad", "replicate"),
                                  inflow_order=c["kw"].get("inflow_order", "after"))
        assert torch.equal(got[0], ref[0]) and all(torch.equal(a, b) for a, b in zip(got[1], ref[1]))
    d0, v0 = o.synthetic_state(2, 16, 8, 8, kc.SEED)
    d, v, re = kc.state("16_dens")
    assert torch.equal(d, d0.float().double()) and torch.equal(v[1], v0[1].float().double()) and re.tolist() == o.RE_TRAIN[:2]
    assert kc.cfl_of("32_cfl") > 2.0 and kc.cfl_of("16_dens") < 1.0          # the window case really leaves the two halo columns


@pytest.mark.parametrize("name", sorted(kc.CASES))
def test_the_gpu_tests_inputs_keep_clear_of_cell_boundaries(name):
    _, g64 = kc.oracle_case(name)
    _, g32 = kc.oracle_case(name, torch.float32)
    errs = {n: rel(a, b) for n, a, b in zip(kc.NAMES, g32, g64) if float(b.abs().max()) > 0}
    print("oracle float32 against float64, %s, untrimmed:" % name, errs)
    assert "g_re" in errs and max(errs.values()) < 2e-5, errs
