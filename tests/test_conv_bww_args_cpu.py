"""5x5 weight gradient, CPU side (no GPU needed): the argument checks of sol_conv5x5_bwd_weight, its reduce and the segmented entry
(everything is rejected before any launch, with a message that names the offending value), the workspace arithmetic for ragged row
counts, the refusal of rows narrower than 4 cells at construction, and the condition on the integer data of the exact GPU tests."""
import ctypes as C

import numpy as np
import pytest

import sol_amd
from sol_amd import _lib, burgers
from conv_bww_cases import DZ_UNIT, EXACT_SHAPES, PAIRS, integer_tensors, tap_gradient

FAKE = C.c_void_p(4096)          # never dereferenced: every case below fails validation first


@pytest.fixture(scope="module")
def lib():
    return sol_amd.load()


def err(lib):
    return lib.sol_last_error().decode()


@pytest.mark.parametrize("W", [2, 6, 68])
def test_row_widths_outside_the_contract_are_rejected(lib, W):
    assert lib.sol_conv5x5_bwd_weight(None, FAKE, FAKE, FAKE, 1, 8, W, 32, 32) != 0
    assert "sol_conv5x5_bwd_weight" in err(lib) and str(W) in err(lib), err(lib)
    assert lib.sol_conv5x5_bwd_weight_segments(None, FAKE, FAKE, FAKE, 2, 64, 64, 1, 1, 8, W, 32, 32, None, None, 0, 0) != 0
    assert str(W) in err(lib), err(lib)


@pytest.mark.parametrize("cin,cout,bad", [(3, 32, "3,32"), (32, 3, "32,3"), (4, 3, "4,3"), (8, 32, "8,32")])
def test_channel_counts_outside_the_contract_are_rejected(lib, cin, cout, bad):
    assert lib.sol_conv5x5_bwd_weight(None, FAKE, FAKE, FAKE, 1, 8, 64, cin, cout) != 0
    assert "supported (cin,cout)" in err(lib) and "got %s" % bad in err(lib), err(lib)
    assert lib.sol_conv5x5_bwd_weight_segments(None, FAKE, FAKE, FAKE, 1, 0, 0, 1, 1, 8, 64, cin, cout, None, None, 0, 0) != 0
    assert "got %s" % bad in err(lib), err(lib)


def test_null_pointers_are_rejected(lib):
    for args in ((None, FAKE, FAKE), (FAKE, None, FAKE), (FAKE, FAKE, None)):
        assert lib.sol_conv5x5_bwd_weight(None, *args, 1, 8, 64, 32, 32) != 0
        assert "NULL" in err(lib), err(lib)
        assert lib.sol_conv5x5_bwd_weight_segments(None, *args, 2, 64, 64, 1, 1, 8, 64, 32, 32, None, None, 0, 0) != 0
        assert "NULL" in err(lib), err(lib)
        assert lib.sol_conv5x5_bwd_weight_reduce(None, *args, 1, 8, 64, 32, 32, 0) != 0
        assert "NULL" in err(lib), err(lib)
        assert lib.sol_conv5x5_bwd_weight_segments_reduce(None, *args, 1, 1, 8, 32, 32, 0) != 0
        assert "NULL" in err(lib), err(lib)


def test_the_segmented_entry_takes_rows_up_to_64_pixels_and_at_least_one_segment(lib):
    assert lib.sol_conv5x5_bwd_weight_segments(None, FAKE, FAKE, FAKE, 2, 64, 64, 1, 1, 8, 128, 32, 32, None, None, 0, 0) != 0
    assert "W <= 64" in err(lib) and "128" in err(lib), err(lib)
    for nseg in (0, -3):
        assert lib.sol_conv5x5_bwd_weight_segments(None, FAKE, FAKE, FAKE, nseg, 64, 64, 1, 1, 8, 64, 32, 32, None, None, 0, 0) != 0
        assert "nseg" in err(lib) and str(nseg) in err(lib), err(lib)
        assert lib.sol_conv5x5_bwd_weight_segments_reduce(None, FAKE, FAKE, FAKE, nseg, 1, 8, 32, 32, 0) != 0
        assert "nseg" in err(lib) and str(nseg) in err(lib), err(lib)
        assert lib.sol_conv5x5_bwd_weight_segments_ws_floats(nseg, 1, 8, 32, 32) == 0
    assert lib.sol_conv5x5_bwd_weight_segments(None, FAKE, FAKE, FAKE, 1, 0, 0, 1, 1, 8, 64, 4, 32, None, None, 0, 5) != 0
    assert "cin_real" in err(lib) and "5" in err(lib), err(lib)


@pytest.mark.parametrize("cin,cout,IP,OP", [(4, 32, 16, 32), (32, 32, 32, 32), (32, 2, 32, 16), (4, 2, 16, 16)])
def test_workspace_follows_the_block_arithmetic_for_ragged_rows(lib, cin, cout, IP, OP):
    unit = 25 * IP * OP + OP
    for B, H, nblk in ((3, 5, 2), (1, 1, 1), (2, 3, 1), (1, 13, 2), (1, 136, 17), (1, 8, 1), (1, 9, 2)):
        assert (B * H + 7) // 8 == nblk
        for W in (4, 20, 64):
            assert lib.sol_conv5x5_bwd_weight_ws_floats(B, H, W, cin, cout) == nblk * unit
        assert lib.sol_conv5x5_bwd_weight_segments_ws_floats(1, B, H, cin, cout) == nblk * unit      # one segment, <= 4096 rows: the same layout
    # segments: one row sequence of nseg * B * H rows; 8 rows per block up to 4096 rows, then 256 blocks (1024 for the thin layers)
    thin = cin == 4 or cout == 2
    for nseg, B, H in ((3, 1, 5), (3, 2, 8), (32, 1, 136), (33, 1, 128), (2, 16, 128)):
        rows = nseg * B * H
        rb = 8 if rows <= 4096 else ((rows + 1023) // 1024 if thin else (rows + 255) // 256)
        assert lib.sol_conv5x5_bwd_weight_segments_ws_floats(nseg, B, H, cin, cout) == (rows + rb - 1) // rb * unit
    if not thin:
        assert lib.sol_conv5x5_bwd_weight_segments_ws_floats(32, 1, 136, cin, cout) == 256 * unit         # 4352 rows at 17 per block
        assert lib.sol_conv5x5_bwd_weight_segments_ws_floats(33, 1, 128, cin, cout) == 249 * unit         # 4224 rows at 17 per block


def test_rows_narrower_than_four_cells_are_refused_at_construction(lib):
    """64 % 2 == 0 let X = 2 through _check_net_shape although every convolution of the network refuses W < 4: the forward
    convolution (pinned here) and the weight gradient (above).  The trainers now refuse at construction."""
    assert lib.sol_conv5x5(None, FAKE, FAKE, None, None, None, FAKE, 1, 32, 2, 32, 32, 0, 0.0) != 0
    assert "W=2" in err(lib), err(lib)
    for who in ("BurgersTrainer", "BurgersRollout"):
        with pytest.raises(_lib.SolError) as e:
            burgers._check_net_shape(who, 32, 2)
        assert who in str(e.value) and "X = 2" in str(e.value) and "at least 4" in str(e.value), str(e.value)
    burgers._check_net_shape("BurgersTrainer", 16, 4)            # the narrowest row the kernels take
    burgers._check_net_shape("BurgersTrainer", 32, 2, True)      # pitched rows: every width runs
    with pytest.raises(_lib.SolError):
        burgers._check_net_shape("BurgersTrainer", 5, 12)        # 64 % 12 != 0: refused as before


@pytest.mark.parametrize("cin,cout", PAIRS)
@pytest.mark.parametrize("B,H,W", EXACT_SHAPES)
def test_the_integer_data_of_the_exact_gpu_tests_is_exact_in_float32(B, H, W, cin, cout):
    """The condition the bit-for-bit GPU tests rest on, checked on the inputs: every sum stays below 2^24 units, and a float32 numpy
    evaluation (another summation order again) equals the float64 one."""
    x, dz = integer_tensors(B, H, W, cin, cout)
    assert x.abs().max() <= 4 and (dz / DZ_UNIT).abs().max() <= 3 and bool((x == x.round()).all()) and bool((dz / DZ_UNIT == (dz / DZ_UNIT).round()).all())
    assert 2 * B * H * W * 4 * 3 < 2 ** 24               # (2 x: two accumulating calls stay exact too)
    w32, b32 = tap_gradient(x.numpy(), dz.numpy(), np.float32)
    w64, b64 = tap_gradient(x.numpy(), dz.numpy(), np.float64)
    assert w32.dtype == np.float32 and np.array_equal(w32.astype(np.float64), w64) and np.array_equal(b32.astype(np.float64), b64)
    assert np.abs(w64).max() > 0
