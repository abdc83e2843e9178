"""Adjoint of the karman-2d marker density, CPU side (no GPU needed): the new C entry points' declarations, bindings, workspace size and
argument checks (rejected before any launch), the new option, KarmanFlow(density_grad=True), and the input condition of the GPU tests
(test_gpu_karman2d_density_adjoint.py): at state seed 11 with the masked density cotangent the oracle in float32 agrees with the oracle in
float64 UNTRIMMED -- no departure point sits close enough to a cell boundary for fp32 to decide it differently.  Measured 8.3e-6 at most
over all shapes of the GPU tests; pinned below 2e-5 (a 2.4x margin).  If an oracle default moves, this test fails and the GPU test's
inputs are re-examined rather than silently trimmed."""
import ctypes as C
import os
import sys

import pytest
import torch

import sol_amd
from sol_amd import _lib, karman

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from density_adjoint_cases import oracle_case
from large2d_scenes import rel

NEW = ("sol_karman_density_bwd_workspace_bytes", "sol_karman_density_bwd")
P = lambda v: C.c_void_p(v)


@pytest.fixture(scope="module")
def lib():
    return sol_amd.load()


def cfg2d(Y=130, X=65, B=2, **kw):
    c = _lib.KarmanCfg(B, Y, X, 100.0 / X, 1.0, float(X), 1e-6, 1e-9, 2000, 0, 0, 0, None, 0, None)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def call(lib, c, ws=1 << 40, **kw):
    """sol_karman_density_bwd on fake device pointers: never dereferenced, every case below fails validation first"""
    a = dict(d_in=P(4096), inflow=P(8192), saved_vy=P(12288), saved_vx=P(16384), re=P(20480), bcm=P(24576), g_d_out=P(28672),
             g_d_in=P(32768), g_vy_in=P(36864), g_vx_in=P(40960), workspace=P(45056))
    a.update(kw)
    return lib.sol_karman_density_bwd(C.byref(c) if c is not None else None, None, a["d_in"], a["inflow"], a["saved_vy"], a["saved_vx"],
                                      a["re"], a["bcm"], 0, a["g_d_out"], a["g_d_in"], a["g_vy_in"], a["g_vx_in"], 0, a["workspace"], ws)


def test_new_symbols_are_declared_exported_and_bound(lib):
    assert lib.sol_version() == _lib.ABI_VERSION          # additions only: the ABI number stays
    decl = _lib.declared_symbols()
    for name in NEW:
        assert name in decl and name in _lib._SIGS and hasattr(lib, name)
    assert _lib.get_option("k2d_dens_adj_tile") == 1
    _lib.set_option("k2d_dens_adj_tile", 0)
    try:
        assert _lib.get_option("k2d_dens_adj_tile") == 0
    finally:
        _lib.set_option("k2d_dens_adj_tile", 1)
    with pytest.raises(_lib.SolError, match="must be in"):
        _lib.set_option("k2d_dens_adj_tile", 2)


def test_workspace_is_positive_and_grows_with_the_batch(lib):
    last = 0
    for B in (1, 2, 6):
        for Y, X in ((32, 16), (130, 65), (256, 128)):
            n = lib.sol_karman_density_bwd_workspace_bytes(C.byref(cfg2d(Y, X, B)))
            own = B * Y * X * (8 + 4 + 4) + B * 64 * 4          # int64 accumulators, gU_y, gU_x, absmax slots
            assert own <= n < own + 4096, (B, Y, X, n, own)
        n = lib.sol_karman_density_bwd_workspace_bytes(C.byref(cfg2d(B=B)))
        assert n > last > -1
        last = n
    assert lib.sol_karman_density_bwd_workspace_bytes(None) == 0


def test_bad_arguments_are_rejected_with_their_message(lib):
    need = lib.sol_karman_density_bwd_workspace_bytes(C.byref(cfg2d()))
    cases = [(dict(c=None), b"cfg is NULL"),
             (dict(c=cfg2d(B=0)), b"B in [1, 65535]"),
             (dict(c=cfg2d(B=65536)), b"B in [1, 65535]"),
             (dict(c=cfg2d(Y=1)), b"Y, X >= 2"),
             (dict(c=cfg2d(Y=1 << 15, X=1 << 15)), b"grid too large"),
             (dict(ws=0), b"workspace too small"),
             (dict(ws=need - 1), b"workspace too small"),
             (dict(c=cfg2d(inflow_before=1), inflow=None), b"inflow_before needs the inflow mask"),
             (dict(g_d_in=P(4096)), b"alias"),                       # = d_in
             (dict(g_vy_in=P(12288)), b"alias"),                     # = saved_vy
             (dict(g_vx_in=P(28672)), b"alias"),                     # = g_d_out
             (dict(g_vy_in=P(40960)), b"buffers of their own"),      # = g_vx_in
             (dict(g_d_in=P(36864)), b"buffers of their own")]       # = g_vy_in
    for name in ("d_in", "saved_vy", "saved_vx", "re", "bcm", "g_d_out", "g_d_in", "g_vy_in", "g_vx_in", "workspace"):
        cases.append(({name: None}, b"NULL pointer"))
    for kw, msg in cases:
        kw = dict(kw)
        c = kw.pop("c", cfg2d())
        assert call(lib, c, **kw) == -1, (kw, msg)
        assert b"sol_karman_density_bwd" in lib.sol_last_error() and msg in lib.sol_last_error(), (kw, msg, lib.sol_last_error())


def test_karman_flow_takes_density_grad():
    assert karman.KarmanFlow(density_grad=True)._density_grad is True
    assert karman.KarmanFlow()._density_grad is False


@pytest.mark.parametrize("Y,X,B", [(64, 32, 3), (130, 65, 2)])
def test_the_gpu_tests_inputs_keep_clear_of_cell_boundaries(Y, X, B):
    _, g64 = oracle_case(Y, X, B)
    _, g32 = oracle_case(Y, X, B, dtype=torch.float32)
    errs = {n: rel(a, b) for n, a, b in zip(("g_d", "g_vy", "g_vx"), g32, g64)}
    print("oracle float32 against float64, %dx%d B=%d, untrimmed:" % (Y, X, B), errs)
    assert max(errs.values()) < 2e-5, errs
