"""The shape table, the restated dispatch and the references of the karman-3d NETWORK shape tests (test_gpu_karman3d_net_shapes.py and its
CPU twin test_karman3d_net_shapes_cpu.py).  A plain module: importing it touches no device.

The rest of the 3-D suite runs MarsMoon3D, schedule3d.NetSchedule3D, Karman3DTrainer and Karman3DRollout on (2r, r, r) grids with Z in
{8, 16, 64} and X = Z only.  "Which kernel a launch runs ... is a matter of its shape alone" (schedule3d.py), so the table lists the smallest
shapes that reach the other branches, and the dispatch is restated here as functions of the shape (conv3d_launches, thin_launches,
bww_launches, thin_bww_kernel, one_launch): the GPU tests compare what they predict with what the launch profiler saw, the CPU twin ties
them to the C sources by text.

Cells are (B, D = Y, H = X, W = Z) for layers and networks, (Y, X, Z) for trainers and roll-outs (B = 2, SOL-2, the oracle's cylinder
scene passed as active= / inflow=).

MEASURED on an MI355X (relative L2, printed by the GPU tests), next to the bound each is held to (BOUNDS: the suite's own, measured until now at
W in {16, 64} only).  No bound was widened and no kernel defect was found: every cell meets the suite's bounds with a factor of 5 or more.

(a) layers against float64 (bound 2e-6 forward, 5e-6 gradients); 32 -> 32 conv3d LeakyReLU / DLRELU; thin 4 -> 32 / 32 -> 3; weight gradients
    dW, worst of 32 -> 32, 4 -> 32, 32 -> 3 (and the depth-packed pair at W = 64), single call / two calls accumulated; kernels the profiler saw
  2x5x6x32    2.2e-7 / 2.8e-7;  2.2e-7 / 3.5e-7;  2.6e-7 / 2.6e-7   k_conv5x5_c32<2> x 9 (4 B + 1), x 1 thin; k_conv5x5_bww<32,32> / <4,32> x 10 (5 B)
  2x5x12x16   2.6e-7 / 3.0e-7;  2.7e-7 / 2.7e-7;  2.0e-7 / 2.0e-7   as above
  1x6x8x8     2.2e-7 / 2.8e-7;  1.7e-7 / 2.5e-7;  1.3e-7 / 1.4e-7   k_conv5x5_c32<2> x 5, x 1; k_conv5x5_bww<32,32> / <4,32> x 5
  1x3x16x4    1.7e-7 / 2.3e-7;  1.4e-7 / 2.6e-7;  9.6e-8 / 1.0e-7   as above
  2x5x10x64   1.9e-7 / 2.2e-7;  1.0e-7 / 1.9e-7;  2.3e-7 / 2.4e-7   k_conv3d_sb8<2,0> x 1; k_conv5x5_dx<1,1,true> x 1 thin; k_conv5x5_bww_sb_jobs<2> x 2 (B),
                                                                    k_conv5x5_bww_thin<0,2> x 10, depth-packed k_conv5x5_bww_sb<0> x 1
  1x3x8x64    1.4e-7 / 1.8e-7;  8.8e-8 / 9.8e-8;  1.9e-7 / 2.0e-7   k_conv3d_sb8<2,0> x 1; k_conv5x5_dx<1,1,true>; k_conv5x5_bww_sb_jobs<2> x 1, depth-packed k_conv5x5_bww_sb<2> x 1
  1x4x6x128   9.8e-8 / 1.2e-7;  1.1e-7 / 9.9e-8;  --                k_conv5x5_dx<1,1,true> x 5, x 1 thin
  db 3.1e-8 ... 3.1e-7; two calls accumulated against the sum of two single calls 4.6e-8 ... 1.2e-7 (bound 2e-6); y_absmax exact in every case;
  an all-zero dz gives dW = db = 0 exactly from every form; an all-zero x gives epi(bias + residual) exactly, slots finite
  persistent form (k_conv3d_sb8<2,0,true>, 2 and 3 tiles per workgroup) against five passes (k_conv5x5_dx<3,2> x 5) 2.5e-7 ... 3.0e-7 (bound 1e-6),
  against one tile per workgroup: bit-equal
(b) network against torch float64 autograd, out / dx / worst parameter tensor (bounds 5e-6 / 1e-5 / 1e-5; no activation sign differed), and beside
    it FP32_ALONE (torch fp32 against torch float64 on the CPU, same inputs and masks, no project code):
  2x5x6x32    7.9e-7 / 7.9e-7 / 8.3e-7      fp32 alone 1.09e-6 / 1.08e-6 / 1.14e-6
  2x5x12x16   9.1e-7 / 8.5e-7 / 9.6e-7                 1.29e-6 / 1.17e-6 / 1.38e-6
  1x6x8x8     8.1e-7 / 7.7e-7 / 8.8e-7                 1.17e-6 / 1.10e-6 / 1.34e-6
  1x3x16x4    5.6e-7 / 6.2e-7 / 6.7e-7                 7.20e-7 / 6.93e-7 / 1.03e-6
  2x5x10x64   5.6e-7 / 5.4e-7 / 6.7e-7                 1.28e-6 / 1.19e-6 / 1.77e-6
  1x3x8x64    3.9e-7 / 4.0e-7 / 6.0e-7                 9.32e-7 / 8.67e-7 / 1.12e-6
  fused reverse sweep against the per-layer composition: outputs bit-equal; dx 3.8e-7 ... 6.5e-7, flat gradient 1.4e-8 ... 3.4e-8, per tensor
  <= 6.8e-7 at W < 64, all bit-equal at W = 64 (bounds 2e-6 / 2e-6 / 1e-5)
  kernels of a network pass at W < 64: k_conv5x5_c32<2> x (2 + 10 (4 B + 1)) forward and again in the reverse sweep, k_conv5x5_bww<32,32> x 55 B,
  k_conv5x5_bww<4,32> x 5 B; at 2x5x10x64: k_conv3d_sb8<2,0> x 10 + k_conv5x5_dx<1,1,true> x 2 each way, k_conv5x5_bww_sb_jobs<2> x 20,
  k_conv5x5_bww_sb<0> x 2; at 2x20x10x64 the thin layers run k_conv5x5_dx<3,2> and the thin weight gradients k_conv5x5_bww_sb<2>
(c) trainer, B = 2, SOL-2, cylinder: manual against autograd schedule -- loss and per-step losses bit-equal, gradient 9.2e-8 ... 1.1e-7 (bound 2e-5),
  final state 2.3e-7 ... 4.5e-7 (2e-6); second replay of the captured graph bit-equal to eager; roll-out over two steps bit-equal to the training
  forward and to the trainer's final state; 16 x 8 x 32 against the float64 oracle: loss 1.3e-9 (1e-5), gradient 1.7e-7 (1e-4), per tensor 1.8e-7 (3e-4)
(d) Z = 128: forward schedule 3.2e-7 at 1x4x6x128 (k_conv5x5_dx<1,1,true> x 52) and 3.8e-7 at 2x16x8x128 (k_conv5x5_dx<1,1,true> x 80,
  k_conv5x5_dx<3,2> x 12) against torch float64 (bound 5e-6; fp32 alone 1.0e-6); one roll-out step at 16 x 8 x 128: network output 4.2e-7, corrected
  velocities 2.4e-8 / 6.1e-8 / 2.2e-7 against the hand composition (bound 1e-5)
(e) dynamic range of k_conv3d_sb8 against the strict-fp32 form (k_conv5x5_r3<2> x 5, 5.0e-7 alone): SPLIT3D_MEASURED, 0.68 ... 0.70 in every case,
  whole tensor and small half: the claim "ratio <= 1.0, no allowance" holds for the 3-D kernel as it stands."""
import collections

import numpy as np
import torch
import torch.nn.functional as F

from large2d_scenes import DEV, TOL_FIELD, TOL_GRAD, f32, rel   # noqa: F401  (re-exported: one definition)

SLOPE = 0.3

# ---- the table ------------------------------------------------------------------------------------------------------------------------
# cell (B, D, H, W) -> what it reaches
CELLS = {
    (2, 5, 6, 32): "Z = 32: five-pass form, 2 image rows per tile, 3 tiles per plane, odd D, two samples; plain weight gradients",
    (2, 5, 12, 16): "Z = 16 with X != Z: 4 rows per tile, 3 tiles per plane",
    (1, 6, 8, 8): "Z = 8: one tile per plane",
    (1, 3, 16, 4): "Z = 4 and D = 3, the smallest the entry points accept: 16 rows per tile, every depth tap but the centre one reads across "
                   "a volume face (network only; the step needs Z >= 8)",
    (2, 5, 10, 64): "one-launch kernels with 100 rows: 13 eight-row tiles on a 16-workgroup grid, tiles spanning planes and samples, H below "
                    "and not a multiple of 8; depth-packed thin weight gradients at H = 10 (100 rows are no multiple of the 8 rows of a "
                    "weight-gradient block: the bf16 six-product body k_conv5x5_bww_sb<0>); 32 -> 32 weight gradients as one jobs launch per sample",
    (1, 3, 8, 64): "Z = 64 with 24 rows (a multiple of 8): the depth-packed thin weight gradients on the fp16 three-product body "
                   "k_conv5x5_bww_sb<2>, D = 3",
    (1, 4, 6, 128): "Z = 128: wide-row five-pass form (two 64-pixel column tiles per row), forward only",
    (1, 64, 64, 64): "layer level only: persistent one-launch form (k3d_conv_persist = 1) with 2 tiles per workgroup (512 tiles)",
    (1, 96, 64, 64): "layer level only: persistent one-launch form with 3 tiles per workgroup (768 tiles)",
}
PERSIST_CELLS = [(1, 64, 64, 64), (1, 96, 64, 64)]
WIDE_CELL = (1, 4, 6, 128)
LAYER_CELLS = [c for c in CELLS if c not in PERSIST_CELLS]           # against float64
GRAD_CELLS = [c for c in LAYER_CELLS if c[3] <= 64]                 # the weight gradients take W <= 64
NET_CELLS = [c for c in LAYER_CELLS if c != WIDE_CELL]
# trainer and roll-out cells (Y, X, Z), B = 2, SOL-2, cylinder
TRAIN_B, TRAIN_MS, TRAIN_OBSTACLE = 2, 2, "cylinder"
TRAIN_CELLS = {
    (16, 8, 32): "Z = 32; the float64 oracle runs here (half the cells of test_karman3d_trainer_sol2_against_oracle's grid)",
    (24, 12, 16): "Z = 16 with X != Z",
    (20, 10, 64): "Z = 64 with X = 10: one-launch kernels, depth-packed thin weight gradients (400 rows: the fp16 three-product body)",
}
ORACLE_CELL = (16, 8, 32)
Z128_CELL = (16, 8, 128)
STD_V = (0.2, 0.25, 0.3)

# grids the network refuses (Y, X, Z, train-only?) -> words the message must hold
REFUSED = {
    (24, 12, 12, False): ("Z = 12", "multiple of 64"),
    (24, 12, 24, False): ("Z = 24", "multiple of 64"),
    (24, 12, 72, False): ("Z = 72", "multiple of 64"),
    (20, 10, 16, False): ("X = 10", "64/Z"),
    (16, 8, 128, True): ("Z = 128", "Z <= 64", "roll-out"),
}

# the bounds the suite already holds these operations to (tests/test_gpu_karman3d.py), and where each is asserted there
BOUNDS = {
    "conv_forward": 2e-6,           # test_conv3d_against_oracle
    "conv_gradient": 5e-6,          # test_conv3d_gradients_against_oracle
    "absmax": 1e-6,                 # test_conv3d_against_oracle: published y_absmax against max|y|
    "one_launch_vs_five_pass": 1e-6,    # test_conv3d_full_size_one_launch_against_five_pass_and_shift_property
    "net_out": 5e-6, "net_dx": 1e-5, "net_param": 1e-5,                     # test_network_w64_against_torch_float64_autograd
    "fused_dx": 2e-6, "fused_flat": 2e-6, "fused_param": 1e-5,              # test_network_fused_reverse_sweep_equals_per_layer_autograd
    "manual_loss": 2e-6, "manual_steps": 2e-6, "manual_grad": 2e-5, "manual_final": 2e-6,   # test_karman3d_manual_schedule_equals_autograd_composition
    "oracle_loss": 1e-5, "oracle_grad": TOL_GRAD, "oracle_param": 3 * TOL_GRAD,             # test_karman3d_trainer_sol2_against_oracle
}
# The rule for a bound that fails at a new cell: where the fp32-alone figure of the cell (FP32_ALONE) sits within a factor of 4 of the
# suite's bound, the cell's bound is 4 x that figure (the factor 4: summation order, what separates the fp32 kernels of this suite
# from each other); otherwise the kernel is wrong at that shape.  Cells that needed it: none.
NET_BOUNDS = {c: (BOUNDS["net_out"], BOUNDS["net_dx"], BOUNDS["net_param"]) for c in NET_CELLS + [WIDE_CELL]}

# fp32 alone (out, dx, largest parameter tensor), measured by the CPU twin, which pins each within a factor of 2 (another BLAS or thread count
# moves the summation order, not the magnitude)
FP32_ALONE = {
    (2, 5, 6, 32): (1.09e-6, 1.08e-6, 1.14e-6),
    (2, 5, 12, 16): (1.29e-6, 1.17e-6, 1.38e-6),
    (1, 6, 8, 8): (1.17e-6, 1.10e-6, 1.34e-6),
    (1, 3, 16, 4): (7.20e-7, 6.93e-7, 1.03e-6),
    (2, 5, 10, 64): (1.28e-6, 1.19e-6, 1.77e-6),
    (1, 3, 8, 64): (9.32e-7, 8.67e-7, 1.12e-6),
    (1, 4, 6, 128): (9.98e-7, None, None),
}

def sid(c):
    return "x".join(str(v) for v in c)


# ---- the dispatch, restated -----------------------------------------------------------------------------------------------------------
# default options (csrc/train.hip, sol_opt): conv_precision 0, conv_dx 11, conv_r3 1, conv_thin 1, conv_bww32 1, k3d_conv_fused 1,
# k3d_conv_rows 8, k3d_conv_persist 0, k3d_bww_jobs 2.  Kernel names are spelled as SOL_LAUNCH spells them, without blanks and parentheses.
RB = 8                              # csrc/conv5x5.hip: image rows per weight-gradient workgroup


def net_shape_reason(Y, X, Z, train):
    """check_shape of csrc/conv5x5.hip, sol_conv3d's D >= 3 and bww_launch's W <= 64, written as the C conditions stand -> refused or not"""
    B, H, W, D = 1, X, Z, Y
    ok = B >= 1 and H >= 1 and W >= 4                                                        # SOL_REQUIRE(B >= 1 && H >= 1 && W >= 4, ...)
    ok = ok and ((W <= 64 and 64 % W == 0 and H % (64 // W) == 0) or W % 64 == 0)            # ... W must divide 64 (with H % (64/W) == 0) or ...
    ok = ok and D >= 3                                                                       # sol_conv3d: B >= 1, D >= 3
    if train:
        ok = ok and W <= 64                                                                  # the batched forms take W <= 64
    return not ok


def dx_kernel(nrows, tiles_x, H):
    """sol_conv_dx_launch for a dense 32 -> 32 launch under conv_dx = 11 (bit 3: one-row launches as two half-channel workgroups per tile)"""
    R = 3 if H >= 2 and ((nrows + 2) // 3) * tiles_x >= 128 else 1
    return "k_conv5x5_dx<1,1,true>" if R == 1 else "k_conv5x5_dx<3,2>"


def conv2d_kernel(nimg, H, W, absmax=True, precision=0):
    """conv_impl (csrc/conv5x5.hip) for one 32 -> 32 launch over nimg images of H rows"""
    if W % 64 == 0:
        if precision == 2:
            return "k_conv5x5_r3<2>"
        if absmax and precision == 0:
            return dx_kernel(nimg * H, W // 64, H)
        return "k_conv5x5_sb<2,0>"
    assert W <= 64 and 64 % W == 0 and H % (64 // W) == 0, (H, W)
    return "k_conv5x5_c32<2>"       # narrow rows: 64 / W image rows per tile, whatever conv_precision says


def one_launch(B, D, H, persist=0):
    """sol_conv3d_sb_launch at W = 64, 32 -> 32, k3d_conv_rows = 8: rows belong to B D H, eight per tile, the grid padded to a multiple of 8
    workgroups; persistent (option k3d_conv_persist) iff the tile count is a multiple of 256 and at least 512"""
    nrows = B * D * H
    nt8 = (nrows + 7) // 8
    pers = bool(persist) and nt8 % 256 == 0 and nt8 >= 512
    return dict(rows=nrows, tiles=nt8, grid=256 if pers else (nt8 + 7) // 8 * 8, persistent=pers, tiles_per_wg=nt8 // 256 if pers else 1,
                kernel="k_conv3d_sb8<2,0,true>" if pers else "k_conv3d_sb8<2,0>")


def conv_form(B, D, H, W, cin, cout, absmax, precision=0, fused=1):
    """sol_conv3d's predicate (csrc/karman3d.hip) -> "one_launch" or "five_pass" """
    fusable = cin == 32 and (cout == 32 or cout <= 16)
    return "one_launch" if fusable and W == 64 and absmax and precision == 0 and fused else "five_pass"


def conv3d_launches(B, D, H, W, absmax=True, precision=0, fused=1, persist=0):
    """{convolution kernel: launches} of one 32 -> 32 sol_conv3d call"""
    if conv_form(B, D, H, W, 32, 32, absmax, precision, fused) == "one_launch":
        return collections.Counter({one_launch(B, D, H, persist)["kernel"]: 1})
    out = collections.Counter()
    # per simulation the slices kd = 0, 4 over D - 2 planes and kd = 1, 3 over D - 1, then the centre slice over all B D planes
    for nimg, n in ((D - 2, 2 * B), (D - 1, 2 * B), (B * D, 1)):
        out[conv2d_kernel(nimg, H, W, absmax, precision)] += n
    return out


def thin_launches(B, D, H, W):
    """sol_conv3d_thin / sol_conv3d_thin_out: ONE 2-D 32 -> 32 launch over the B D planes, absmax slots always given"""
    return collections.Counter({conv2d_kernel(B * D, H, W): 1})


def pick_rb(rows):
    return (rows + 255) // 256 if rows > 4096 else RB


def bww_launches(B, D, H, W, cin_k, co_k, precision=0):
    """{weight-gradient kernel: launches} of sol_conv3d_bwd_weight(_acc) (absmax of both operands given where both have 32 channels, as
    karman3d.conv3d_bwd_weight does); None: refused (bww_launch: the batched forms take W <= 64)"""
    if W > 64:
        return None
    if cin_k == 32 and co_k == 32 and W == 64 and precision != 2:
        return collections.Counter({"k_conv5x5_bww_sb_jobs<2>" if precision == 0 else "k_conv5x5_bww_sb_jobs<0>": B})     # the five slices of a simulation in one launch
    if W == 64 and (cin_k, co_k) == (4, 32):
        name = "k_conv5x5_bww_thin<0,2>"
    elif W == 64 and (cin_k, co_k) == (32, 32):
        name = "k_conv5x5_bww32"
    else:
        name = "k_conv5x5_bww<%d,%d>" % (cin_k, co_k)
    return collections.Counter({name: 5 * B})


def thin_bww_kernel(B, D, H):
    """sol_conv3d_thin(_out)_bwd_weight_acc at W = 64: one pass of the split 32 -> 32 body over B D H rows -- the fp16 three-product kernel
    iff no workgroup of pick_rb rows is ragged ((planes * H) % rb == 0), else the bf16 six-product one"""
    rows = B * D * H
    return "k_conv5x5_bww_sb<2>" if rows % pick_rb(rows) == 0 else "k_conv5x5_bww_sb<0>"


def net_forward_launches(B, D, H, W):
    """NetSchedule3D.forward: thin, ten 32 -> 32 layers, thin-out"""
    out = thin_launches(B, D, H, W) + thin_launches(B, D, H, W)
    for _ in range(10):
        out += conv3d_launches(B, D, H, W)
    return out


def net_backward_launches(B, D, H, W):
    """NetSchedule3D.backward of a 4 -> 3 network: (convolution kernels, weight-gradient kernels)"""
    conv = thin_launches(B, D, H, W) + thin_launches(B, D, H, W)          # the output layer's and the first layer's data gradients
    for _ in range(10):
        conv += conv3d_launches(B, D, H, W)
    bww = collections.Counter()
    for _ in range(10):
        bww += bww_launches(B, D, H, W, 32, 32)
    if W == 64:
        bww[thin_bww_kernel(B, D, H)] += 2
    else:
        bww += bww_launches(B, D, H, W, 32, 32)                          # 32 -> 3, dz padded to 32 channels
        bww += bww_launches(B, D, H, W, 4, 32)
    return conv, bww


def conv_kernels(p):
    """{convolution kernel: launches} of a _lib.profile() block: the 3-D one-launch kernels and the 2-D forward kernels"""
    names = {k.strip("()").replace(" ", ""): v[0] for k, v in p.kernels.items()}
    return collections.Counter({k: n for k, n in names.items() if k.startswith(("k_conv3d", "k_conv5x5")) and "bww" not in k})


def bww_kernels(p):
    names = {k.strip("()").replace(" ", ""): v[0] for k, v in p.kernels.items()}
    return collections.Counter({k: n for k, n in names.items() if k.startswith("k_conv5x5_bww")})


# ---- metrics --------------------------------------------------------------------------------------------------------------------------
def per_plane(a, b):
    """relative L2 per (sample, plane): a wrong plane range at a sample boundary shows here, not averaged away"""
    return [["%.1e" % rel(a[s, d], b[s, d]) for d in range(a.shape[1])] for s in range(a.shape[0])]


def per_slice(a, b):
    return ["%.1e" % rel(a[kd], b[kd]) for kd in range(5)]


# ---- references in plain torch (any device, any dtype) --------------------------------------------------------------------------------
def ncdhw(t):
    return t.permute(0, 4, 1, 2, 3)


def ndhwc(t):
    return t.permute(0, 2, 3, 4, 1)


def conv3d_ref(x, w, b=None):
    """x [B,D,H,W,ci], w [5,5,5,ci,co] (DHWIO) -> [B,D,H,W,co], zero padding 2, in the dtype of x"""
    return ndhwc(F.conv3d(ncdhw(x), w.permute(4, 3, 0, 1, 2), b, padding=2))


def lrelu_masked(z, m):
    return z * torch.where(m, 1.0, SLOPE).to(z.dtype)


def golden_params():
    """the golden network's parameters (make_golden.k3d_params: fp32 values held in float64).  make_golden sets torch's default dtype to
    float64 on import, for the whole process, and draws the biases in it: they are drawn under float64 here and the default is put back"""
    prev = torch.get_default_dtype()
    try:
        import make_golden as mg
        torch.set_default_dtype(torch.float64)
        return mg.k3d_params()
    finally:
        torch.set_default_dtype(prev)


def network_case(shape, seed=21):
    """(x, gy, params) of a network test: fp32 tensors on the CPU; the upstream gradient lives on another scale (x 1e-3); the parameters are
    the golden network's (small non-zero biases, the last layer scaled by 0.05)"""
    B, D, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, D, H, W, 4, generator=gen, dtype=torch.float32)
    gy = torch.randn(B, D, H, W, 3, generator=gen, dtype=torch.float32) * 1e-3
    return x, gy, [p.float() for p in golden_params()]


def torch_network(x, gy, params, masks=None, dtype=torch.float64, device="cpu"):
    """model_mars_moon3d in plain torch (F.conv3d and its autograd), NCDHW, kernels DHWIO -> OIDHW.  masks: the eleven LeakyReLU sign masks
    [B,D,H,W,32] to apply (None: the network's own) -> (out [B,D,H,W,3], dx, the 24 parameter gradients, the masks of its own
    pre-activations, how many block-output signs differ from the masks applied); gy = None: forward only"""
    tp = [p.to(device=device, dtype=dtype).requires_grad_(gy is not None) for p in params]
    conv = lambda t, k: F.conv3d(t, tp[2 * k].permute(4, 3, 0, 1, 2), tp[2 * k + 1], padding=2)
    xt = ncdhw(x.to(device=device, dtype=dtype)).contiguous().requires_grad_(gy is not None)
    own, flips = [], 0
    mk = lambda z: (z > 0) if masks is None else ncdhw(masks[len(own)].to(device))

    def act(z):
        nonlocal flips
        m = mk(z)
        flips += int(((z > 0) != m).sum())
        own.append(ndhwc((z > 0).detach()))
        return lrelu_masked(z, m)

    with torch.set_grad_enabled(gy is not None):
        h = act(conv(xt, 0))
        for k in range(5):
            a = act(conv(h, 1 + 2 * k))
            h = act(conv(a, 2 + 2 * k) + h)
        out = conv(h, 11)
        if gy is None:
            return ndhwc(out), None, None, own, flips
        (out * ncdhw(gy.to(device=device, dtype=dtype))).sum().backward()
    return ndhwc(out.detach()), ndhwc(xt.grad), [p.grad for p in tp], own, flips


def fp32_alone(shape, grads=True):
    """(out, dx, largest parameter tensor) of torch fp32 against torch float64 on the CPU, the fp32 run with the float64 run's masks: what
    fp32 arithmetic alone costs at this shape, no project code involved"""
    x, gy, params = network_case(shape)
    gy = gy if grads else None
    o64, dx64, g64, m64, _ = torch_network(x, gy, params)
    o32, dx32, g32, _, _ = torch_network(x, gy, params, masks=m64, dtype=torch.float32)
    if not grads:
        return rel(o32, o64), None, None
    return rel(o32, o64), rel(dx32, dx64), max(rel(a, b) for a, b in zip(g32, g64))


def hip_network_against_float64(shape, dev=DEV):
    """The body of test_network_w64_against_torch_float64_autograd at any shape: MarsMoon3D (one autograd node over its schedule) against
    torch_network in float64 on the same device, LeakyReLU applied with the HIP forward's sign masks -> (out, dx, [24 per-tensor], flips)"""
    from sol_amd import karman3d as k3
    x, gy, params = network_case(shape)
    net = k3.MarsMoon3D(device=dev)
    net.set_weights([p.numpy() for p in params])
    net.params.requires_grad_(True)
    xd = x.to(dev)
    xi = xd.clone().requires_grad_(True)
    out = net(xi)
    (out * gy.to(dev)).sum().backward()
    masks = [t > 0 for t in net.activations(xd)]
    torch.cuda.synchronize()
    ref, dx, grads, _, flips = torch_network(x, gy, params, masks=masks, device=dev)
    off = net.offsets
    per = [rel(net.params.grad[off[k]:off[k + 1]], grads[k].reshape(-1)) for k in range(24)]
    return rel(out.detach(), ref), rel(xi.grad, dx), per, flips


# ---- scenes and states of the trainer cells ---------------------------------------------------------------------------------------------
def geometry(cell, obstacle=TRAIN_OBSTACLE):
    import sol_oracle3d as o
    return o.geometry(*cell, obstacle=obstacle)


def train_case(cell, B=TRAIN_B, ms=TRAIN_MS, seed=77):
    """(d, (vy, vx, vz), re, gts) of a trainer cell: the oracle's synthetic state and ground-truth frames, fp32 values held in float64"""
    import sol_oracle3d as o
    d, v = o.synthetic_state(B, *cell, seed)
    d, v = d.float().double(), tuple(c.float().double() for c in v)
    re = torch.tensor(o.RE_TRAIN[:B], dtype=torch.float64)
    gts = []
    for i in range(ms):
        _, gv = o.synthetic_state(B, *cell, 500 + i)
        gts.append(tuple(c.float().double() for c in gv))
    return d, v, re, gts


# ---- dynamic range of the one-launch kernel's own fp16 x 3 split ------------------------------------------------------------------------
SPLIT3D_SHAPE = (1, 4, 64, 64)
SPLIT3D_RATIOS = (("mixed_1e-3", 1e-3), ("mixed_1e-5", 1e-5), ("mixed_2^-18", 2.0 ** -18), ("mixed_2^-19", 2.0 ** -19),
                  ("mixed_2^-20", 2.0 ** -20), ("mixed_2^-22", 2.0 ** -22))
# ratio allowed per case: (one-launch kernel's relative L2 against float64) / (strict-fp32 five-pass form's), whole tensor and small half.
# 1.0, no allowance, is the claim the 2-D kernels meet (test_split_conv_relative_l2_not_worse_than_fp32_mfma).
SPLIT3D_BOUND = {name: 1.0 for name in ("normal", "heavy") + tuple(n for n, _ in SPLIT3D_RATIOS)}
# measured on an MI355X: (whole tensor, small half)
SPLIT3D_MEASURED = {"normal": (0.686, 0.683), "heavy": (0.695, 0.698), "mixed_1e-3": (0.690, 0.684), "mixed_1e-5": (0.688, 0.686),
                    "mixed_2^-18": (0.687, 0.685), "mixed_2^-19": (0.686, 0.686), "mixed_2^-20": (0.689, 0.687), "mixed_2^-22": (0.689, 0.687)}


def split3d_cases():
    """the cases of test_gpu_parity._split_conv_cases on a (1, 4, 64, 64, 32) volume: normal, heavy-tailed, and the left half of every row
    scaled by r (2^-19 of the tensor maximum is where the fp16 lo plane starts to underflow) -> ({name: x}, w [5,5,5,32,32])"""
    gen = torch.Generator().manual_seed(5)
    s = SPLIT3D_SHAPE + (32,)
    cases = {"normal": torch.randn(s, generator=gen, dtype=torch.float32),
             "heavy": torch.randn(s, generator=gen, dtype=torch.float32) * torch.exp(2.0 * torch.randn(s, generator=gen, dtype=torch.float32))}
    for name, ratio in SPLIT3D_RATIOS:
        m = torch.randn(s, generator=gen, dtype=torch.float32)
        m[:, :, :, :32] *= ratio
        cases[name] = m
    w = torch.randn(5, 5, 5, 32, 32, generator=gen, dtype=torch.float32) * (0.05 / np.sqrt(5.0))
    return cases, w
