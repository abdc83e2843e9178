"""CPU-side checks of the large-grid Burgers adjoint (no GPU): the new entry points are declared and exported, the workspace size is
the documented one, bad arguments are refused before any launch, and the Python surface takes the new keyword."""
import ctypes as C

import pytest

import sol_amd
from sol_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return sol_amd.load()


def test_new_symbols_are_declared_and_exported(lib):
    decl = sol_amd.declared_symbols()
    for name in ("sol_burgers_step_bwd_large", "sol_burgers_step_bwd_large_workspace_bytes"):
        assert name in decl and name in _lib._SIGS and hasattr(lib, name)
    assert lib.sol_version() == _lib.ABI_VERSION == 216          # additions only: the ABI number stays


@pytest.mark.parametrize("B,Y,X", [(1, 2, 2), (2, 70, 36), (5, 128, 128), (3, 1024, 1024)])
def test_workspace_bytes_is_the_documented_size(lib, B, Y, X):
    """include/sol_hip.h: r(8 B F) + 2 r(4 B F) + r(256 B) + 256 with F = (Y+1) X + Y (X+1), r = round up to 256"""
    r = lambda n: (n + 255) // 256 * 256
    F = (Y + 1) * X + Y * (X + 1)
    cfg = _lib.BurgersCfg(B, Y, X, 1.0, 0.1)
    assert lib.sol_burgers_step_bwd_large_workspace_bytes(C.byref(cfg)) == r(8 * B * F) + 2 * r(4 * B * F) + r(256 * B) + 256


def test_workspace_bytes_is_zero_for_a_bad_cfg(lib):
    assert lib.sol_burgers_step_bwd_large_workspace_bytes(None) == 0
    for B, Y, X in ((0, 32, 32), (1, 1, 32), (1, 32, 1), (1, 1025, 32), (1, 32, 1025)):
        assert lib.sol_burgers_step_bwd_large_workspace_bytes(C.byref(_lib.BurgersCfg(B, Y, X, 1.0, 0.1))) == 0, (B, Y, X)


def test_bad_arguments_are_refused_before_any_launch(lib):
    one = C.c_void_p(256)
    cfg = _lib.BurgersCfg(2, 70, 36, 0.5, 0.1)
    nbytes = lib.sol_burgers_step_bwd_large_workspace_bytes(C.byref(cfg))
    assert lib.sol_burgers_step_bwd_large(C.byref(cfg), None, *([None] * 11), nbytes) == -1 and b"NULL" in lib.sol_last_error()
    assert lib.sol_burgers_step_bwd_large(C.byref(cfg), None, *([one] * 11), nbytes - 1) == -1 and b"workspace too small" in lib.sol_last_error()
    big = _lib.BurgersCfg(2, 1025, 36, 0.5, 0.1)
    assert lib.sol_burgers_step_bwd_large(C.byref(big), None, *([one] * 11), nbytes) == -1 and b"1024" in lib.sol_last_error()
    assert lib.sol_burgers_step_bwd_large(None, None, *([one] * 11), nbytes) == -1


def test_python_surface_takes_the_keyword_and_validates_shapes():
    assert sol_amd.BurgersTest(large_grid_grad=True).large_grid_grad is True
    assert sol_amd.BurgersTest().large_grid_grad is False
    net = sol_amd.model_mars_moon(cin=4, cout=2, device="cpu")
    for Y, X, ok_words in ((24, 100, "multiple of 64"), (24, 48, "64 % X == 0"), (5, 32, "Y % (64 / X) == 0")):
        dom = sol_amd.Domain([Y, X], box=sol_amd.box([Y, X]), boundaries=sol_amd.PERIODIC)
        with pytest.raises(sol_amd.SolError) as e:
            sol_amd.BurgersTrainer(net, dom, 2, 2, 0.1, (0.2, 0.2), (0.1, 0.1))
        assert ok_words in str(e.value) and "%dx%d" % (Y, X) in str(e.value)
