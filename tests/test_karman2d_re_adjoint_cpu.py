"""Gradient of the karman-2d step with respect to the Reynolds number, CPU side (no GPU needed): the four new C entry points'
declarations, bindings, workspace sizes and argument checks (rejected before any launch), KarmanFlow(re_grad=True), that to_feature keeps
a tensor `re` in the graph, the refusal of grids below 16 cells, and the two input conditions of the GPU tests
(test_gpu_karman2d_re_adjoint.py; re_adjoint_cases.py derives the bound TOL_GRAD S_b):
  * |ref_b| >= 0.3 S_b on every case the GPU tests use -- the sum does not cancel, so the bound is not vacuous (measured 0.43 - 0.56 on the
    velocity path, 0.35 - 0.45 on the density path);
  * the oracle in float32 deviates from float64 by less than TOL_GRAD S_b on these inputs (measured below 4e-7 S_b).
If an oracle default moves, these fail and the inputs are re-examined."""
import ctypes as C
import os
import sys

import pytest
import torch

import sol_amd
from sol_amd import _lib, fluid, karman, ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sol_oracle as o
from large2d_scenes import TOL_GRAD, state, table_geometry
from re_adjoint_cases import SEED, oracle_case, step_parts

NEW = ("sol_karman_step_bwd_large_re_workspace_bytes_for", "sol_karman_step_bwd_large_re",
       "sol_karman_density_bwd_re_workspace_bytes", "sol_karman_density_bwd_re")
P = lambda v: C.c_void_p(v)
# every case of the GPU tests: (Y, X, B, scene, grad_pad, paths)
GPU_CASES = [(32, 16, 2, "default", "replicate", ("velocity",)),
             (64, 32, 3, "default", "replicate", ("velocity", "density")),
             (130, 65, 2, "default", "replicate", ("velocity", "density")),
             (130, 65, 2, "two", "replicate", ("velocity",)),
             (64, 32, 3, "default", "dirichlet0", ("velocity",))]


@pytest.fixture(scope="module")
def lib():
    return sol_amd.load()


def cfg2d(Y=130, X=65, B=2, **kw):
    c = _lib.KarmanCfg(B, Y, X, 100.0 / X, 1.0, float(X), 1e-6, 1e-9, 2000, 0, 0, 0, None, 0, None)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def partial_bytes(B, Y, X):
    faces = (Y + 1) * X + Y * (X + 1)
    nblk = min(max((faces + 2047) // 2048, 1), 256)          # a function of the grid alone: 2048 faces per workgroup, 256 workgroups at most
    return (B * nblk * 8 + 255) // 256 * 256


def test_new_symbols_are_declared_exported_and_bound(lib):
    assert lib.sol_version() == _lib.ABI_VERSION          # additions only: the ABI number stays
    decl = _lib.declared_symbols()
    for name in NEW:
        assert name in decl and name in _lib._SIGS and hasattr(lib, name)


def test_workspaces_are_the_plain_calls_plus_the_partial_sums(lib):
    last_v = last_d = 0
    for B in (1, 2, 6):
        for Y, X in ((32, 16), (64, 32), (130, 65), (256, 128), (1024, 512)):
            c = cfg2d(Y, X, B)
            plain_v = lib.sol_karman_step_bwd_large_workspace_bytes_for(C.byref(c), None)
            plain_d = lib.sol_karman_density_bwd_workspace_bytes(C.byref(c))
            assert lib.sol_karman_step_bwd_large_re_workspace_bytes_for(C.byref(c), None) == plain_v + partial_bytes(B, Y, X), (B, Y, X)
            assert lib.sol_karman_density_bwd_re_workspace_bytes(C.byref(c)) == plain_d + partial_bytes(B, Y, X), (B, Y, X)
        v = lib.sol_karman_step_bwd_large_re_workspace_bytes_for(C.byref(cfg2d(B=B)), None)
        d = lib.sol_karman_density_bwd_re_workspace_bytes(C.byref(cfg2d(B=B)))
        assert v > last_v and d > last_d
        last_v, last_d = v, d
    assert lib.sol_karman_step_bwd_large_re_workspace_bytes_for(None, None) == 0
    assert lib.sol_karman_density_bwd_re_workspace_bytes(None) == 0


def call_density(lib, c, ws=1 << 40, **kw):
    """sol_karman_density_bwd_re on fake device pointers: never dereferenced, every case below fails validation first"""
    a = dict(d_in=P(4096), inflow=P(8192), saved_vy=P(12288), saved_vx=P(16384), re=P(20480), bcm=P(24576), g_d_out=P(28672),
             g_d_in=P(32768), g_vy_in=P(36864), g_vx_in=P(40960), workspace=P(45056), vy_in=P(49152), vx_in=P(53248), g_re=P(57344))
    a.update(kw)
    return lib.sol_karman_density_bwd_re(C.byref(c) if c is not None else None, None, a["d_in"], a["inflow"], a["saved_vy"], a["saved_vx"],
                                         a["re"], a["bcm"], 0, a["g_d_out"], a["g_d_in"], a["g_vy_in"], a["g_vx_in"], 0, a["workspace"], ws,
                                         a["vy_in"], a["vx_in"], a["g_re"], 0)


def call_velocity(lib, c, ws=1 << 40, **kw):
    """sol_karman_step_bwd_large_re on fake device pointers, CG form (cfg.direct = NULL): rejected before any launch"""
    hdr = (C.c_int32 * 16)(0x46443032, c.Y if c is not None else 0, c.X if c is not None else 0)
    a = dict(saved_vy=P(4096), saved_vx=P(8192), re=P(12288), active=P(16384), bcm=P(20480), g_vy_out=P(24576), g_vx_out=P(28672),
             g_vy_in=P(32768), g_vx_in=P(36864), box=P(40960), cg_info=P(45056), workspace=P(49152), vy_in=P(53248), vx_in=P(57344),
             g_re=P(61440))
    a.update(kw)
    return lib.sol_karman_step_bwd_large_re(C.byref(c) if c is not None else None, None, a["saved_vy"], a["saved_vx"], a["re"], a["active"],
                                            a["bcm"], 0, a["g_vy_out"], a["g_vx_out"], a["g_vy_in"], a["g_vx_in"], None, a["box"], hdr,
                                            a["cg_info"], a["workspace"], ws, a["vy_in"], a["vx_in"], a["g_re"], 0)


def test_density_form_rejects_bad_arguments_with_their_message(lib):
    need = lib.sol_karman_density_bwd_re_workspace_bytes(C.byref(cfg2d()))
    cases = [(dict(c=None), b"cfg is NULL"),
             (dict(c=cfg2d(B=0)), b"B in [1, 65535]"),
             (dict(c=cfg2d(B=65536)), b"B in [1, 65535]"),
             (dict(c=cfg2d(Y=1)), b"Y, X >= 2"),
             (dict(c=cfg2d(Y=1 << 15, X=1 << 15)), b"grid too large"),
             (dict(ws=0), b"workspace too small"),
             (dict(ws=need - 1), b"workspace too small"),                                  # the plain call's size does not do
             (dict(ws=lib.sol_karman_density_bwd_workspace_bytes(C.byref(cfg2d()))), b"workspace too small"),
             (dict(c=cfg2d(inflow_before=1), inflow=None), b"inflow_before needs the inflow mask"),
             (dict(g_d_in=P(4096)), b"alias"),                       # = d_in
             (dict(g_re=P(20480)), b"alias"),                        # = re
             (dict(g_re=P(49152)), b"alias"),                        # = vy_in
             (dict(g_vy_in=P(49152)), b"alias"),                     # = vy_in
             (dict(g_vx_in=P(53248)), b"alias"),                     # = vx_in
             (dict(g_vy_in=P(40960)), b"buffers of their own"),      # = g_vx_in
             (dict(g_re=P(36864)), b"g_re must be a buffer of its own")]       # = g_vy_in
    for name in ("d_in", "saved_vy", "saved_vx", "re", "bcm", "g_d_out", "g_d_in", "g_vy_in", "g_vx_in", "workspace", "vy_in", "vx_in", "g_re"):
        cases.append(({name: None}, b"NULL pointer"))
    for kw, msg in cases:
        kw = dict(kw)
        c = kw.pop("c", cfg2d())
        assert call_density(lib, c, **kw) == -1, (kw, msg)
        assert b"sol_karman_density_bwd_re" in lib.sol_last_error() and msg in lib.sol_last_error(), (kw, msg, lib.sol_last_error())


def test_velocity_form_rejects_bad_arguments_with_their_message(lib):
    need = lib.sol_karman_step_bwd_large_re_workspace_bytes_for(C.byref(cfg2d()), None)
    cases = [(dict(c=None), b"cfg is NULL"),
             (dict(c=cfg2d(B=0)), b"B in [1, 65535]"),
             (dict(c=cfg2d(B=65536)), b"B in [1, 65535]"),
             (dict(c=cfg2d(Y=16, X=8)), b"Y, X >= 16"),
             (dict(c=cfg2d(Y=1 << 15, X=1 << 15)), b"grid too large"),
             (dict(ws=0), b"workspace too small"),
             (dict(ws=need - 1), b"workspace too small"),
             (dict(ws=lib.sol_karman_step_bwd_large_workspace_bytes_for(C.byref(cfg2d()), None)), b"workspace too small"),
             (dict(g_vy_in=P(4096)), b"alias"),                      # = saved_vy
             (dict(g_re=P(12288)), b"alias"),                        # = re
             (dict(g_re=P(53248)), b"alias"),                        # = vy_in
             (dict(g_vx_in=P(57344)), b"alias"),                     # = vx_in
             (dict(g_vy_in=P(36864)), b"buffers of their own"),      # = g_vx_in
             (dict(g_re=P(32768)), b"g_re must be a buffer of its own"),       # = g_vy_in
             (dict(g_re=P(45056)), b"g_re must be a buffer of its own")]       # = cg_info
    for name in ("saved_vy", "saved_vx", "re", "active", "bcm", "g_vy_out", "g_vx_out", "g_vy_in", "g_vx_in", "workspace", "vy_in", "vx_in", "g_re"):
        cases.append(({name: None}, b"NULL pointer"))
    for kw, msg in cases:
        kw = dict(kw)
        c = kw.pop("c", cfg2d())
        assert call_velocity(lib, c, **kw) == -1, (kw, msg)
        assert b"sol_karman_step_bwd_large_re" in lib.sol_last_error() and msg in lib.sol_last_error(), (kw, msg, lib.sol_last_error())


def test_karman_flow_takes_re_grad():
    assert karman.KarmanFlow(re_grad=True)._re_grad is True
    assert karman.KarmanFlow()._re_grad is False
    assert karman.KarmanFlow(re_grad=True, density_grad=True)._density_grad is True


def test_to_feature_keeps_a_tensor_re_in_the_graph():
    B, Y, X = 2, 16, 8
    dom = fluid.Domain([Y, X], box=fluid.box[0:200, 0:100])
    s = fluid.Fluid(dom, density=0.0, velocity=1.0, batch_size=B, device="cpu")
    re = torch.tensor([1e5, 2e5], requires_grad=True)
    feat = karman.to_feature(s, re)
    assert feat.shape == (B, Y, X, 3) and feat.requires_grad
    feat[..., 2].sum().backward()
    assert torch.equal(re.grad, torch.full((B,), float(Y * X)))


def test_grids_below_16_cells_are_refused_under_re_grad():
    B, Y, X = 2, 16, 8
    cfg = ops.karman_cfg(B, Y, X, 100.0 / X)
    re = torch.tensor([1e5, 2e5], requires_grad=True)
    z = torch.zeros
    with pytest.raises(_lib.SolError, match="Y, X >= 16; this one is 16x8"):
        ops.karman_step(z(B, Y, X), z(B, Y + 1, X), z(B, Y, X + 1), re, cfg, None, re_grad=True)
    with pytest.raises(_lib.SolError, match="Y, X >= 16; this one is 16x8"):
        ops.karman_step_large_bwd_re(z(B, Y + 1, X), z(B, Y, X + 1), re.detach(), z(B, Y + 1, X), z(B, Y, X + 1), z(B, Y + 1, X), z(B, Y, X + 1),
                                     cfg, None)


def test_the_cases_module_spells_the_oracles_step():
    g = table_geometry("default", 64, 32)
    st = state(3, 64, 32, SEED, g)
    with torch.no_grad():
        mine, _ = step_parts(*st[:3], st[3], g)
        ref = o.karman_step(*st, g)
    for a, b in zip(mine, ref):
        assert torch.equal(a, b)


@pytest.mark.parametrize("Y,X,B,scene,grad_pad,paths", GPU_CASES)
def test_the_gpu_tests_inputs_are_well_conditioned(Y, X, B, scene, grad_pad, paths):
    for path in paths:
        r64 = oracle_case(Y, X, B, scene, path, grad_pad)
        r32 = oracle_case(Y, X, B, scene, path, grad_pad, dtype=torch.float32)
        ratio = (r64["g_re"].abs() / r64["S"]).tolist()
        dev = ((r32["g_re"] - r64["g_re"]).abs() / r64["S"]).tolist()
        formula = float(((r64["direct"] - r64["g_re"]).abs() / r64["g_re"].abs()).max())
        print("%dx%d B=%d %s %s %s: |ref| / S %s, float32 - float64 in units of S %s, formula against autograd %.1e"
              % (Y, X, B, scene, grad_pad, path, ratio, dev, formula))
        assert min(ratio) >= 0.3, (path, ratio)                 # the sum does not cancel: the bound TOL_GRAD S is not vacuous
        assert max(dev) < TOL_GRAD, (path, dev)                 # fp32 can reach the bound on these inputs
        assert formula < 1e-12, (path, formula)                 # g_re = -(dt res^2 / re^2) <g', L v_in>
