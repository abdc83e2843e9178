"""Cases shared by test_gpu_conv_bww_narrow.py and test_conv_bww_args_cpu.py (no test, no device): the channel pairs and shapes of the
narrow weight-gradient tests, the integer-valued data of the exact tests and a plain numpy evaluation of the gradient."""
import numpy as np
import torch

PAIRS = [(3, 32), (4, 32), (32, 32), (32, 2), (3, 2)]        # (real cin, cout); x is padded to 4 channels for cin <= 4

# (B, H, W), the smallest shapes that reach each edge (RB = 8 image rows per workgroup)
SHAPES = [
    (1, 1, 64),       # one row: every dy != 2 tap row lies outside the image
    (2, 3, 64),       # H < 5; 6 rows = one ragged block holding two images
    (3, 5, 64),       # 15 rows: the second block is ragged and straddles images
    (1, 13, 64),
    (1, 2, 32),
    (3, 6, 32),
    (2, 20, 16),      # five blocks
    (1, 16, 4),
    (2, 16, 8),       # the shape of test_conv5x5_against_oracle: the anchor
    (1, 136, 64),     # 17 blocks: two-stage reduce with a last chunk of one block
    (2, 5, 12), (2, 5, 20), (2, 5, 36), (2, 5, 60),      # widths the header admits that no trainer reaches
]
EXACT_SHAPES = [(3, 5, 64), (2, 3, 64), (3, 6, 32), (2, 5, 20)]
DZ_UNIT = 2.0 ** -7      # the fixed power of two of the integer dz


def integer_tensors(B, H, W, cin, cout, seed=23):
    """x in {-4..4}, dz in {-3..3} * 2^-7 (CPU float32): every product and every partial sum of the gradient is an integer multiple of
    2^-7 below 2^24 * 2^-7 (B*H*W * 12 < 2^24 for every shape used), so the float64 result is a float32 number and every summation
    order, every operand split (three bf16 parts, two fp16 parts at a power-of-two scale) and the fp32 MFMA must reproduce it bit for
    bit."""
    gen = torch.Generator().manual_seed(seed + 1000 * cin + cout)
    x = torch.randint(-4, 5, (B, H, W, cin), generator=gen).to(torch.float32)
    dz = torch.randint(-3, 4, (B, H, W, cout), generator=gen).to(torch.float32) * DZ_UNIT
    return x, dz


def tap_gradient(x, dz, dtype):
    """dW [5,5,cin,cout], db [cout] of dW[dy][dx] = sum_{b,y,px} x[b, y+dy-2, px+dx-2] dz[b, y, px] in numpy at `dtype` (zero padding)."""
    x, dz = np.asarray(x, dtype=dtype), np.asarray(dz, dtype=dtype)
    B, H, W, cin = x.shape
    xp = np.zeros((B, H + 4, W + 4, cin), dtype=dtype)
    xp[:, 2:H + 2, 2:W + 2] = x
    dw = np.zeros((5, 5, cin, dz.shape[-1]), dtype=dtype)
    for dy in range(5):
        for dx in range(5):
            dw[dy, dx] = np.einsum("byxi,byxo->io", xp[:, dy:dy + H, dx:dx + W], dz).astype(dtype)
    return dw, dz.sum(axis=(0, 1, 2), dtype=dtype)
