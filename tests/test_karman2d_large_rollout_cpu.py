"""Large-grid karman-2d roll-out, CPU side (no GPU needed): the new C symbols declared / exported / bound with matching argument counts,
their argument checks (rejected before any launch), the refusals of LargeGridRollout / make_rollout / ops.karman_step_large that come
before any device call, and the roll-out script's new flag."""
import ctypes as C
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

import sol_amd
from sol_amd import _lib, ops, precond

FAKE = C.c_void_p(4096)          # never dereferenced: every case below fails validation first
NEW = ("sol_karman_correct", "sol_karman_step_fwd_large_cg_warm")


@pytest.fixture(scope="module")
def lib():
    return sol_amd.load()


def declared_arg_count(name):
    with open(_lib.HEADER) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_new_symbols_are_declared_exported_and_bound(lib):
    assert lib.sol_version() == _lib.ABI_VERSION == 216          # additions only: the ABI number stays
    decl = _lib.declared_symbols()
    for name in NEW:
        assert name in decl and name in _lib._SIGS and hasattr(lib, name)
        assert len(_lib._SIGS[name][1]) == declared_arg_count(name), name
    # the warm entry point = the cold one + p_inout
    assert len(_lib._SIGS["sol_karman_step_fwd_large_cg_warm"][1]) == len(_lib._SIGS["sol_karman_step_fwd_large_cg"][1]) + 1


def test_correct_rejects_bad_arguments(lib):
    ok = dict(out=FAKE, vy=C.c_void_p(8192), vx=C.c_void_p(12288), cy=None, cx=None, B=1, Y=5, X=7)
    cases = [(dict(out=None), b"NULL"), (dict(vy=None), b"NULL"), (dict(vx=None), b"NULL"), (dict(cy=FAKE), b"both or neither"),
             (dict(cx=FAKE), b"both or neither"), (dict(B=0), b"B, Y, X >= 1"), (dict(Y=0), b"B, Y, X >= 1"), (dict(X=-3), b"B, Y, X >= 1")]
    for kw, msg in cases:
        a = dict(ok, **kw)
        rc = lib.sol_karman_correct(None, a["out"], a["vy"], a["vx"], a["cy"], a["cx"], a["B"], a["Y"], a["X"], 1.0, 1.0)
        assert rc == -1 and msg in lib.sol_last_error(), (kw, lib.sol_last_error())


def cfg2d(Y=256, X=128, B=2):
    return _lib.KarmanCfg(B, Y, X, 100.0 / X, 1.0, float(X), 1e-6, 1e-9, 2000, 0, 0, 0, None, 0, None)


def warm(lib, p_inout=C.c_void_p(20480), ws=1 << 40, hdr=None, vy_out=C.c_void_p(16384)):
    """(every call below changes ONE argument into a rejected one: the defaults together would be a valid call on fake pointers)"""
    h = np.zeros(16, dtype=np.int32)
    h[:7] = [precond.FD_MAGIC, 256, 128, 0, 0, 0, 0]
    h = h if hdr is None else hdr
    return lib.sol_karman_step_fwd_large_cg_warm(C.byref(cfg2d()), None, None, FAKE, C.c_void_p(8192), FAKE, FAKE, None, FAKE, FAKE, 0,
                                                 None, vy_out, C.c_void_p(12288), None, None, FAKE, h.ctypes.data_as(C.c_void_p), C.c_void_p(24576),
                                                 p_inout, FAKE, ws)


def test_warm_entry_point_rejects_bad_arguments(lib):
    assert warm(lib, p_inout=None) == -1 and b"p_inout" in lib.sol_last_error()
    assert warm(lib, ws=0) == -1 and b"workspace too small" in lib.sol_last_error()
    assert warm(lib, hdr=np.zeros(16, dtype=np.int32)) == -1 and b"first 16 words of the blob" in lib.sol_last_error()
    assert warm(lib, vy_out=FAKE) == -1 and b"alias" in lib.sol_last_error()
    assert warm(lib, p_inout=FAKE) == -1 and b"alias" in lib.sol_last_error()          # the guess buffer is an output too
    # the guess needs no scratch of its own: one sizing function serves both entry points (and did not change)
    n = lib.sol_karman_step_large_cg_workspace_bytes(C.byref(cfg2d()))
    assert 4 * 2 * 256 * 128 * 10 <= n < 4 * 2 * 256 * 128 * 11 + (1 << 20)


def fake_masks(solver):
    return types.SimpleNamespace(pressure_solver=solver, direct=object() if solver == "direct" else None)


@pytest.mark.parametrize("Y,X,kw,solver,words", [
    (256, 96, {}, "direct", ("LargeGridRollout", "64")),
    (128, 64, {}, "direct", ("LargeGridRollout", "SolRollout")),
    (256, 128, {"use_graph": True}, "cg", ("LargeGridRollout", "use_graph=False", "cg_max_iter")),
    (256, 128, {}, "cg", ("LargeGridRollout", "use_graph=False", "cg_max_iter")),          # use_graph defaults to True
])
def test_large_grid_rollout_refuses_before_touching_a_device(Y, X, kw, solver, words):
    net = object()                                       # never looked at: the grid and the solver are checked first
    with pytest.raises(ValueError) as e:
        sol_amd.LargeGridRollout(net, fake_masks(solver), 1, Y, X, 100.0 / X, (0.2, 0.2), 1e4, **kw)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_p_guess_on_a_direct_scene_is_an_error():
    with pytest.raises(ValueError) as e:
        ops.karman_step_large(None, None, None, None, cfg2d(), fake_masks("direct"), p_guess=object())
    assert "p_guess" in str(e.value) and "direct" in str(e.value)


def test_make_rollout_refuses_a_large_grid_it_cannot_serve():
    with pytest.raises(ValueError) as e:
        sol_amd.make_rollout(object(), fake_masks("direct"), 1, 256, 96, 100.0 / 96, (0.2, 0.2), 1e4)
    assert "LargeGridRollout" in str(e.value)


def test_apply_script_lists_the_warm_start_flag():
    script = os.path.join(os.path.dirname(os.path.abspath(sol_amd.__file__)), "scripts", "karman_apply.py")
    r = subprocess.run([sys.executable, script, "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "--cg-warm-start" in r.stdout and "--pressure-solver" in r.stdout, r.stdout[-2000:]
