"""Adjoint of the large-grid karman-2d step, CPU side (no GPU needed): the new C entry points' declarations, bindings and argument
checks (rejected before any launch), the workspace sizes, the trimmed metric of the GPU tests on synthetic vectors, and the trainers'
refusal of a large domain."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import sol_amd
from sol_amd import _lib, precond

FAKE = C.c_void_p(4096)          # never dereferenced: every case below fails validation first
NEW = ("sol_karman_step_bwd_large_workspace_bytes", "sol_karman_step_fwd_large_saved", "sol_karman_step_bwd_large")


@pytest.fixture(scope="module")
def lib():
    return sol_amd.load()


def gpu_tests():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_karman2d_large_adjoint.py")
    spec = importlib.util.spec_from_file_location("k2d_large_adjoint_gpu_tests", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cfg2d(Y=256, X=128, B=2, direct=False, **kw):
    c = _lib.KarmanCfg(B, Y, X, 100.0 / X, 1.0, float(X), 1e-6, 1e-9, 2000, 0, 0, 0, None, 0, None)
    if direct:
        c.direct, c.direct_n = 8192, 1 << 20          # a non-NULL device pointer selects the direct solve; never dereferenced here
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def header(Y=256, X=128, nS=0, SP=0, win=0):
    h = np.zeros(16, dtype=np.int32)
    h[:8] = [precond.FD_MAGIC, Y, X, 0, 0, nS, SP, win]
    return h


def hp(h):
    return None if h is None else h.ctypes.data_as(C.c_void_p)


def bwd(lib, c, dhdr=None, bhdr=None, ws=1 << 40, info=C.c_void_p(20480), blob=C.c_void_p(24576), g_in=C.c_void_p(16384), wsp=FAKE):
    return lib.sol_karman_step_bwd_large(C.byref(c) if c is not None else None, None, FAKE, FAKE, FAKE, FAKE, FAKE, 0,
                                         C.c_void_p(8192), C.c_void_p(8192), g_in, C.c_void_p(12288),
                                         hp(dhdr), blob, hp(bhdr), info, wsp, ws)


def fwd(lib, c, dhdr=None, bhdr=None, ws=1 << 40, info=C.c_void_p(20480), blob=C.c_void_p(24576), saved=C.c_void_p(28672), wsp=FAKE):
    return lib.sol_karman_step_fwd_large_saved(C.byref(c) if c is not None else None, None, None, FAKE, FAKE, FAKE, FAKE, None, FAKE, FAKE, 0,
                                               None, C.c_void_p(8192), C.c_void_p(12288), saved, C.c_void_p(16384),
                                               hp(dhdr), blob, hp(bhdr), info, wsp, ws)


def test_new_symbols_are_declared_exported_and_bound(lib):
    assert lib.sol_version() == _lib.ABI_VERSION
    decl = _lib.declared_symbols()
    for name in NEW:
        assert name in decl and name in _lib._SIGS and hasattr(lib, name)
    assert _lib.get_option("k2d_adj_tile") == 1


def test_backward_workspace_covers_the_solver_part_of_the_forward_one(lib):
    for B, Y, X in ((1, 256, 128), (2, 256, 128), (6, 256, 128), (3, 128, 96)):
        faces = (Y + 1) * X + Y * (X + 1)
        for direct, fwd_bytes in ((True, lib.sol_karman_step_large_workspace_bytes), (False, lib.sol_karman_step_large_cg_workspace_bytes)):
            c = cfg2d(Y, X, B, direct=direct)
            n = lib.sol_karman_step_bwd_large_workspace_bytes(C.byref(c))
            solver = fwd_bytes(C.byref(c)) - 4 * B * faces              # the forward workspace without sv_y, sv_x
            own = B * faces * (8 + 4) + B * 64 * 4                      # int64 accumulators, g_a, absmax slots
            assert n >= solver + own - 1024, (B, Y, X, direct, n, solver, own)
            assert n < solver + own + (1 << 16), (B, Y, X, direct, n, solver, own)
    assert lib.sol_karman_step_bwd_large_workspace_bytes(None) == 0


@pytest.mark.parametrize("entry", [bwd, fwd])
def test_cg_validation_messages(lib, entry):
    h0 = header()
    cases = [(dict(c=cfg2d(cg_max_iter=0)), b"cg_max_iter must be >= 1"),
             (dict(c=cfg2d(cg_rtol=float("nan"))), b"must be >= 0 and finite"),
             (dict(c=cfg2d(cg_rtol=0.0, cg_atol=0.0)), b"both zero"),
             (dict(bhdr=header(Y=128)), b"the box blob is for a 128x128 grid"),
             (dict(bhdr=header(nS=32, SP=64)), b"needs the empty-box blob"),
             (dict(bhdr=np.zeros(16, dtype=np.int32)), b"first 16 words of the blob"),
             (dict(bhdr=None), b"NULL pointer"),
             (dict(info=None), b"NULL pointer"),
             (dict(blob=None), b"NULL pointer"),
             (dict(wsp=None), b"NULL pointer"),
             (dict(ws=0), b"workspace too small"),
             (dict(ws=4 * 2 * 256 * 128), b"workspace too small"),
             (dict(c=cfg2d(B=0)), b"B in [1, 65535]"),
             (dict(c=cfg2d(Y=8)), b"Y, X >= 16"),
             (dict(c=cfg2d(Y=1 << 15, X=1 << 15)), b"grid too large")]
    for kw, msg in cases:
        kw = dict(kw)
        c = kw.pop("c", cfg2d())
        kw.setdefault("bhdr", h0)
        rc = entry(lib, c, **kw)
        assert rc == -1, (kw, msg)
        assert msg in lib.sol_last_error(), (kw, msg, lib.sol_last_error())
    assert entry(lib, None) == -1 and b"cfg is NULL" in lib.sol_last_error()


@pytest.mark.parametrize("entry", [bwd, fwd])
def test_direct_validation_messages(lib, entry):
    good = header(SP=64, nS=40, win=32)
    cases = [(dict(dhdr=None), b"first 16 words of the blob"),
             (dict(dhdr=np.zeros(16, dtype=np.int32)), b"first 16 words of the blob"),
             (dict(dhdr=header(Y=128, SP=64, nS=40, win=32)), b"blob is for a 128x128 grid"),
             (dict(dhdr=header(SP=64, nS=40, win=48)), b"unsupported window"),
             (dict(dhdr=header(SP=8, nS=40, win=32)), b"header is inconsistent"),
             (dict(dhdr=good, ws=0), b"workspace too small"),
             (dict(dhdr=good, wsp=None), b"NULL pointer")]
    for kw, msg in cases:
        # the CG arguments are not read with the direct solve: NULL is accepted for them
        rc = entry(lib, cfg2d(direct=True), info=None, blob=None, **kw)
        assert rc == -1, (kw, msg)
        assert msg in lib.sol_last_error(), (kw, msg, lib.sol_last_error())


def test_aliasing_is_rejected(lib):
    h0 = header()
    assert bwd(lib, cfg2d(), bhdr=h0, g_in=FAKE) == -1 and b"alias" in lib.sol_last_error()
    assert bwd(lib, cfg2d(), bhdr=h0, g_in=C.c_void_p(12288)) == -1 and b"buffers of their own" in lib.sol_last_error()
    assert fwd(lib, cfg2d(), bhdr=h0, saved=FAKE) == -1 and b"alias" in lib.sol_last_error()
    assert fwd(lib, cfg2d(), bhdr=h0, saved=C.c_void_p(8192)) == -1 and b"buffers of their own" in lib.sol_last_error()


# ---- the trimmed metric of the GPU tests ----------------------------------------------------------------------------------------------
def test_trimmed_metric_on_synthetic_vectors():
    t = gpu_tests()
    assert t.TRIM == 1e-3 and t.TOL_GRAD == 1e-4
    B, Yp, Xn = 2, 257, 128
    n = B * Yp * Xn
    cap = int(t.TRIM * n)
    assert cap == 65                      # 0.1 % of 65 792, rounded down: never more than the cap
    gen = torch.Generator().manual_seed(0)
    ref = torch.randn(B, Yp, Xn, generator=gen, dtype=torch.float64)
    noise = 1e-5 * torch.randn(B, Yp, Xn, generator=gen, dtype=torch.float64)
    # round-off only: nothing to hide, both metrics pass
    v, k, worst = t.trimmed_rel(ref + noise, ref)
    assert k == cap and v < t.TOL_GRAD and v <= t.rel(ref + noise, ref)
    # twenty entries off by O(1) (faces decided differently): the untrimmed metric fails, the trimmed one passes and reports them
    bad = ref + noise
    idx = torch.randperm(n, generator=gen)[:20]
    bad.view(-1)[idx] += 1.0
    assert t.rel(bad, ref) > t.TOL_GRAD
    v, k, worst = t.trimmed_rel(bad, ref)
    assert k == cap and v < t.TOL_GRAD and 0.9 < worst < 1.1
    # exactly as many wrong entries as the cap: still hidden; one more: not
    bad = ref.clone()
    bad.view(-1)[:cap] += 1.0
    assert t.trimmed_rel(bad, ref)[0] == 0.0
    bad.view(-1)[cap] += 1.0
    assert t.trimmed_rel(bad, ref)[0] > t.TOL_GRAD
    # a full boundary row of ONE simulation wrong (128 faces): more than the cap hides
    bad = ref + noise
    bad[1, 0, :] += 0.5
    assert t.trimmed_rel(bad, ref)[0] > t.TOL_GRAD
    # a full column (257 faces) likewise, and a uniformly wrong scale
    bad = ref + noise
    bad[0, :, 5] *= 1.5
    assert t.trimmed_rel(bad, ref)[0] > t.TOL_GRAD
    assert t.trimmed_rel(ref * 1.001, ref)[0] > t.TOL_GRAD
    # it never drops anything from a short vector
    assert t.trimmed_rel(torch.ones(10), torch.ones(10) * 2)[1] == 0


# ---- the trainers stop at the one-workgroup grids -------------------------------------------------------------------------------------
def test_trainers_refuse_a_large_domain_at_construction():
    for make in (lambda: sol_amd.GraphTrainer(None, 1, 256, 128, 2, (0.2, 0.25), 1.0),
                 lambda: sol_amd.SolTrainer(None, None, 1, 256, 128, 2, 100.0 / 128, (0.2, 0.25), 1.0),
                 lambda: sol_amd.GraphTrainer(None, 1, 64, 128, 2, (0.2, 0.25), 1.0)):
        with pytest.raises(ValueError, match="W <= 64"):
            make()
