"""The launch arithmetic behind the batch-regime tests, CPU side (no GPU needed).  tests/test_gpu_parity.py (DX_SHAPES),
tests/test_gpu_train2d_batch_regimes.py, tests/test_gpu_determinism.py (band launch) and the roll-out cases quote rows, forms, grids,
tails and thresholds; here the launchers' rules are restated in Python, tied to their source lines by text, and every quoted number
is asserted -- so that the shape lists cannot drift from what they claim to reach.

The rules (solver-in-the-loop_amd/csrc):
  conv5x5_dx.hip, dx_rows_per_wg:       three rows per workgroup iff H >= 2 and ceil(rows / 3) * tiles_x >= 128, else one
  conv5x5_dx.hip, sol_conv_dx_launch:   grid = ceil(rows / R) * tiles_x, above 64 rounded up to a multiple of 8 (padding tiles own no rows)
  conv5x5.hip, conv_t3_usable:          the three-row thin-input kernel up to B * H <= 1024 rows
  karman_step.hip, sol_karman_fwd_bands_usable / k_karman_fwd_bands:  8 * (BD_N + 1) * ceil(B / 8) + B <= 256 workgroups, BD_N = 4
  train.hip, train_fused_rb:            fused weight-gradient jobs of 32 (128x64) or 16 (64x32, transposed) rows: B * cY % rb == 0"""
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "solver-in-the-loop_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return re.sub(r"\s+", " ", f.read())


def dx_rows_per_wg(nrows, tiles_x, H):
    return 3 if H >= 2 and ((nrows + 2) // 3) * tiles_x >= 128 else 1


def dx_launch(B, H, W):
    """(rows, rows per workgroup, workgroups that own rows, launched grid, rows of the last row group)"""
    nrows, tiles_x = B * H, W // 64
    R = dx_rows_per_wg(nrows, tiles_x, H)
    own = ((nrows + R - 1) // R) * tiles_x
    grid = (own + 7) // 8 * 8 if own > 64 else own
    return nrows, R, own, grid, nrows - (nrows - 1) // R * R


def bands_usable(B):
    return 8 * (4 + 1) * ((B + 7) // 8) + B <= 256


def t3_usable(B, H):
    return B * H <= 1024


def test_the_restated_rules_are_the_launchers_own():
    dx = source("conv5x5_dx.hip")
    assert "static int dx_rows_per_wg(int nrows, int tiles_x, int H) { return H >= 2 && ((nrows + 2) / 3) * tiles_x >= 128 ? 3 : 1; }" in dx
    assert "int grid = ((nrows + R - 1) / R) * a.tiles_x; if (grid > 64) grid = (grid + 7) / 8 * 8;" in dx
    assert "const int R = dx_rows_per_wg(nrows, a.tiles_x, a.H);" in dx and "dx_rows_per_wg(ntiles / a.tiles_x, a.tiles_x, a.H) == 1" in dx
    assert "(cout_padded == 32 || cout_padded == 16) && B * H <= 1024;" in source("conv5x5.hip")
    ks = source("karman_step.hip")
    assert "constexpr int BD_N = 4," in ks and "8 * (BD_N + 1) * ((cfg->B + 7) / 8) + cfg->B <= 256;" in ks
    assert "nsol = 8 * (BD_N + 1) * ((a.B + 7) >> 3);" in ks
    tr = source("train.hip")
    assert "const int rb = sol_karman_bwd_fusable(kc) ? 32 : (sol_karman_bwd_fusable_small(kc) ? 16 : 0);" in tr
    assert "(kc->B * cY) % rb != 0" in tr


# (B, H, W): rows, rows per workgroup, workgroups with rows, grid, rows of the last row group -- the table of DX_SHAPES
@pytest.mark.parametrize("shape,expect", [
    ((6, 128, 64), (768, 3, 256, 256, 3)),
    ((3, 128, 64), (384, 3, 128, 128, 3)),          # the threshold, exactly
    ((2, 190, 64), (380, 1, 380, 384, 1)),          # 127 three-row workgroups would not do: one-row form, four padding tiles
    ((4, 128, 64), (512, 3, 171, 176, 2)),
    ((5, 128, 64), (640, 3, 214, 216, 1)),
    ((2, 200, 64), (400, 3, 134, 136, 1)),
    ((1, 384, 64), (384, 3, 128, 128, 3)),
    ((2, 97, 128), (194, 3, 130, 136, 2)),
    ((130, 3, 64), (390, 3, 130, 136, 3)),
    ((200, 2, 64), (400, 3, 134, 136, 1)),
    ((384, 1, 64), (384, 1, 384, 384, 1)),          # one-row images: never the three-row form
    ((2, 96, 128), (192, 3, 128, 128, 3)),          # the masked form's exact case (tests/test_gpu_conv_cols.py) next to its (2, 97, 128)
    # the trainer's and the roll-out's 32 -> 32 launches: [B, 128, 64], and [B, 32, 64] in the transposed 64x32 recipe
    ((1, 128, 64), (128, 1, 128, 128, 1)),
    ((17, 128, 64), (2176, 3, 726, 728, 1)),
    ((41, 128, 64), (5248, 3, 1750, 1752, 1)),
    ((1, 32, 64), (32, 1, 32, 32, 1)),
    ((5, 32, 64), (160, 1, 160, 160, 1)),
    ((13, 32, 64), (416, 3, 139, 144, 2)),
    ((33, 32, 64), (1056, 3, 352, 352, 3)),
])
def test_dx_launch_table(shape, expect):
    assert dx_launch(*shape) == expect


def test_power_of_two_heights():
    """a.RPW = log2 H or -1 (sol_conv_dx_launch): which of the three-row shapes take the division"""
    assert "for (int k = 0; k < 20; ++k) if ((1 << k) == a.H) a.RPW = k;" in source("conv5x5_dx.hip")
    pow2 = lambda h: h & (h - 1) == 0
    assert [pow2(h) for h in (128, 32, 2, 1)] == [True] * 4
    assert [pow2(h) for h in (190, 200, 384, 97, 3)] == [False] * 5


def test_every_workgroup_of_200_by_2_spans_two_images_or_more_rows_than_one_image():
    """(200, 2, 64): a three-row workgroup holds rows of two images whatever its first row; (130, 3, 64): one image each"""
    for g0 in range(0, 400, 3):
        assert len({r // 2 for r in range(g0, min(g0 + 3, 400))}) == (2 if g0 + 1 < 400 else 1)
    for g0 in range(0, 390, 3):
        assert len({r // 3 for r in range(g0, g0 + 3)}) == 1
    for g0 in range(0, 384, 3):                     # H = 1 in three-row workgroups would be THREE images: the form is refused
        assert len({r // 1 for r in range(g0, g0 + 3)}) == 3


def test_band_launch_limits():
    assert [B for B in range(1, 64) if bands_usable(B)] == list(range(1, 41))          # B = 40 the last, 41 the first refused
    grid = lambda B, dens: 8 * 5 * ((B + 7) // 8) + (B if dens else 0)
    assert grid(8, False) == 40 and grid(16, False) == 80                              # one and two full groups (ms = 1: no density riding)
    assert grid(17, True) == 120 + 17                                                  # the third group holds one simulation
    assert grid(40, True) == 200 + 40 and grid(40, True) <= 256
    assert grid(41, True) == 240 + 41 > 256


def test_thin_input_kernel_limits():
    """conv_t3_usable: the 3 -> 32 layer and the seed launch leave k_conv5x5_t3 from B = 9 at 128x64, from B = 33 in the transposed 64x32 recipe"""
    assert [B for B in range(1, 64) if not t3_usable(B, 128)][0] == 9
    assert [B for B in range(1, 64) if not t3_usable(B, 32)][0] == 33
    assert t3_usable(5, 128) and not t3_usable(17, 128) and not t3_usable(41, 128) and t3_usable(13, 32)


def test_fused_weight_gradient_jobs_divide_every_case():
    for B in (1, 4, 5, 17, 41):
        assert B * 128 % 32 == 0
    for B in (1, 5, 13, 33):
        assert B * 32 % 16 == 0
