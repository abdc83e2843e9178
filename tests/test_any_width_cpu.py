"""Training and roll-out on any row width, CPU side (no GPU needed): the pitch table of schedule2d.row_pitch, the argument checks of
sol_conv5x5_cols (rejected before any launch) and the refusal of any_width=True together with schedule="autograd"."""
import ctypes as C

import pytest

import sol_amd
from sol_amd import burgers, schedule2d

FAKE = C.c_void_p(4096)          # never dereferenced: every case below fails validation first


@pytest.fixture(scope="module")
def lib():
    return sol_amd.load()


@pytest.mark.parametrize("H,W,pitch", [(8, 32, 32), (8, 64, 64), (8, 128, 128), (8, 72, 128), (8, 40, 64), (3, 32, 64), (8, 130, 192)])
def test_row_pitch_table(H, W, pitch):
    assert schedule2d.row_pitch(H, W) == pitch


def cols(lib, x, packed, y, W, WV):
    return lib.sol_conv5x5_cols(None, x, packed, None, None, None, y, 1, 8, W, WV, 32, 32, 0, 0.3, None, None)


@pytest.mark.parametrize("W,WV,words", [(96, 72, ("multiple of 64", "96")), (128, 0, ("WV", "0")), (128, 129, ("WV", "129"))])
def test_cols_rejects_a_bad_pitch_or_width_with_a_message(lib, W, WV, words):
    assert cols(lib, FAKE, FAKE, FAKE, W, WV) != 0
    msg = lib.sol_last_error().decode()
    assert "sol_conv5x5_cols" in msg and all(w in msg for w in words), msg


@pytest.mark.parametrize("args", [(None, FAKE, FAKE), (FAKE, None, FAKE), (FAKE, FAKE, None)])
def test_cols_rejects_null_pointers_with_a_message(lib, args):
    assert cols(lib, *args, 128, 72) != 0
    msg = lib.sol_last_error().decode()
    assert "sol_conv5x5_cols" in msg and "NULL" in msg, msg


def test_any_width_with_the_autograd_schedule_raises():
    net = object()                                       # never looked at: the keywords are checked first
    with pytest.raises(ValueError) as e:
        sol_amd.LargeGridTrainer(net, 1, 144, 72, 2, (0.2, 0.2), 1e4, any_width=True, schedule="autograd")
    assert "any_width" in str(e.value) and "autograd" in str(e.value), str(e.value)
    with pytest.raises(ValueError) as e:
        burgers.BurgersTrainer(net, None, 1, 2, 0.1, (1.0, 1.0), any_width=True, schedule="autograd")
    assert "any_width" in str(e.value) and "autograd" in str(e.value), str(e.value)
    with pytest.raises(ValueError) as e:                 # without the keyword the width is refused as before
        sol_amd.LargeGridTrainer(net, 1, 144, 72, 2, (0.2, 0.2), 1e4)
    assert "64" in str(e.value)
