"""Large-grid karman-2d training, CPU side (no GPU needed): the weight-gradient workspace size with and without column tiles, the
argument checks of sol_conv5x5_bwd_weight (rejected before any launch) and LargeGridTrainer's refusals."""
import ctypes as C

import pytest

import sol_amd

FAKE = C.c_void_p(4096)          # never dereferenced: every case below fails validation first


@pytest.fixture(scope="module")
def lib():
    return sol_amd.load()


@pytest.mark.parametrize("cin,cout,IP,OP", [(4, 32, 16, 32), (32, 32, 32, 32), (32, 2, 32, 16), (4, 2, 16, 16)])
def test_workspace_counts_column_tiles_beyond_64_pixels_only(lib, cin, cout, IP, OP):
    unit = 25 * IP * OP + OP
    for B, H in ((2, 32), (1, 256), (3, 21)):
        nblk = (B * H + 7) // 8                          # 8 image rows per workgroup
        assert lib.sol_conv5x5_bwd_weight_ws_floats(B, H, 32, cin, cout) == nblk * unit
        assert lib.sol_conv5x5_bwd_weight_ws_floats(B, H, 64, cin, cout) == nblk * unit
        assert lib.sol_conv5x5_bwd_weight_ws_floats(B, H, 128, cin, cout) == 2 * nblk * unit
        assert lib.sol_conv5x5_bwd_weight_ws_floats(B, H, 192, cin, cout) == 3 * nblk * unit


def test_bad_arguments_are_rejected_with_a_message(lib):
    assert lib.sol_conv5x5_bwd_weight(None, FAKE, FAKE, FAKE, 1, 8, 96, 32, 32) != 0
    msg = lib.sol_last_error().decode()
    assert "multiple of 64" in msg and "96" in msg, msg
    for args in ((None, FAKE, FAKE), (FAKE, None, FAKE), (FAKE, FAKE, None)):
        assert lib.sol_conv5x5_bwd_weight(None, *args, 1, 8, 128, 32, 32) != 0
        assert "NULL" in lib.sol_last_error().decode()
    assert lib.sol_conv5x5_bwd_weight_reduce(None, FAKE, FAKE, FAKE, 1, 8, 96, 32, 32, 0) != 0
    assert "multiple of 64" in lib.sol_last_error().decode()


@pytest.mark.parametrize("Y,X,word", [(128, 64, "GraphTrainer"), (256, 96, "64")])
def test_large_grid_trainer_refuses_before_touching_a_device(Y, X, word):
    net = object()                                       # never looked at: the grid is checked first
    with pytest.raises(ValueError) as e:
        sol_amd.LargeGridTrainer(net, 1, Y, X, 2, (0.2, 0.2), 1e4)
    assert "LargeGridTrainer" in str(e.value) and word in str(e.value), str(e.value)
