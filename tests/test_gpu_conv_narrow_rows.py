"""Forward / backward-data 5x5 convolutions on rows narrower than 64 pixels (pytest -m gpu): sol_conv5x5 / sol_conv5x5_scaled at
W in {4, 8, 16, 32}, where a 64-pixel tile is RPW = 64 / W image rows with a (RPW + 4) x (W + 4) halo and the launch runs
k_conv5x5<4, NT> (thin input) or k_conv5x5_c32<NT> (32 input channels) whatever conv_precision says -- against
torch.nn.functional.conv2d in float64 on the same fp32-valued operands (independent of oracle/), the way test_gpu_conv_cols.py does it
for W >= 64.

Shapes (B, H, W), the smallest per tile form: one tile that is the whole image (every halo row outside), an odd number of tiles (9 or 15
workgroups: k_conv5x5<4, .> does not remap them) and a grid that is a multiple of 8 (it does, through xcd_tile).  Channel families: the
thin input 4 -> 32 / 16 / 2 with a zero fourth channel, 32 -> 32 / 17 / 16 / 3 / 2 / 1 (both paddings of NT = 1 and NT = 2).  Epilogues:
the five forms of test_gpu_conv_cols.py with a bias far from zero, and the plain one once more with bias NULL; slope 0.3.

Asserted for every (shape, family, epilogue): relative L2 against float64 below 2e-6 (the tolerance test_conv5x5_against_oracle and
test_gpu_conv_cols.py hold this fp32-MFMA arithmetic to); no NaN of the pre-filled output buffer is left; the ops.* call returns the bits
of the call into the pre-filled buffer; conv_precision 0, 1 and 2 give equal bits (narrow rows take no split kernel); through
sol_conv5x5_scaled the largest y_absmax slot is max|y| exactly under conv_precision 0 and 1 and the slots stay zero under 2.
Backward data (weights packed with CONV_BWD_DATA) against float64 autograd of conv2d, plain and with SOL_EPI_DLRELU / act_ref against
autograd through leaky_relu; the packed fp32 section is the flipped, transposed weight exactly.  The launch profiler names the four
kernel forms at every W, and shapes the ABI does not take are refused without a launch.

Measured on an MI355X, worst relative L2 per kernel form over every shape and epilogue (printed by every test):
  kernel form         forward (108 cases x 6 epilogue forms)   backward data (4 shapes, plain and DLRELU)
  k_conv5x5<4, 1>     1.6e-07                                  --
  k_conv5x5<4, 2>     1.5e-07                                  1.2e-07
  k_conv5x5_c32<1>    6.5e-07                                  4.7e-07
  k_conv5x5_c32<2>    4.8e-07                                  4.8e-07
No case sets itself apart: whole-image tiles 9.3e-08 .. 6.4e-07, 9 / 15 workgroups 1.3e-07 .. 5.1e-07, 8 workgroups 1.3e-07 .. 6.5e-07.
"""
import pytest
import torch
import torch.nn.functional as F

from sol_amd import _lib, ops
from test_gpu_conv_cols import DEV, EPILOGUES, SLOPE, case, epilogue, rel

pytestmark = pytest.mark.gpu
TOL = 2e-6
SHAPES = [(1, 16, 4), (1, 8, 8), (1, 4, 16), (1, 2, 32),              # one tile that is the whole image
          (3, 48, 4), (3, 24, 8), (3, 12, 16), (5, 6, 32),            # 9 or 15 workgroups
          (2, 64, 4), (2, 32, 8), (2, 16, 16), (4, 4, 32)]            # 8 workgroups
ODD = SHAPES[4:8]                                                     # one shape per W
FAMILIES = [(4, 32), (4, 16), (4, 2), (32, 32), (32, 17), (32, 16), (32, 3), (32, 2), (32, 1)]
FORMS = EPILOGUES + ("none, bias NULL",)


def kernel_form(cin, cout):
    return ("k_conv5x5<4, %d>" if cin == 4 else "k_conv5x5_c32<%d>") % (2 if cout > 16 else 1)


def conv_kernels(p):
    return {k.strip("()") for k in p.kernels if "conv5x5" in k}


def launch(x, packed, bias, res, act, cout, epi, xmax=None, ymax=None, scaled=False):
    """sol_conv5x5 (scaled: sol_conv5x5_scaled) into an output buffer pre-filled with NaN"""
    b, h, w, cin = x.shape
    y = torch.full((b, h, w, cout), float("nan"), dtype=torch.float32, device=DEV)
    p = _lib.ptr
    head = (_lib.stream(), p(x), p(packed), p(bias), p(res), p(act), p(y), b, h, w, cin, cout, epi, float(SLOPE))
    if scaled:
        _lib.check(_lib.load().sol_conv5x5_scaled(*head, p(xmax), p(ymax)))
    else:
        _lib.check(_lib.load().sol_conv5x5(*head))
    return y


def check_form(name, x, packed, bias, res, act, cout, epi, ref, xmax, what):
    """every assertion of the module docstring on one launch form -> its relative L2"""
    prev = _lib.get_option("conv_precision")
    try:
        first = None
        for precision in (0, 1, 2):
            _lib.set_option("conv_precision", precision)
            y = launch(x, packed, bias, res, act, cout, epi)
            assert not bool(torch.isnan(y).any()), (what, name, precision, "NaN left of the pre-fill")
            assert torch.equal(ops.conv5x5_raw(x, packed, bias, res, act, cout, epi, SLOPE), y), (what, name, precision, "two calls")
            ymax = torch.zeros(ops.AMAX_SLOTS, dtype=torch.int32, device=DEV)
            ys = launch(x, packed, bias, res, act, cout, epi, xmax, ymax, scaled=True)
            assert torch.equal(ys, y), (what, name, precision, "sol_conv5x5_scaled")
            assert torch.equal(ops.conv5x5_scaled_raw(x, packed, bias, res, act, cout, epi, SLOPE, xmax, None), y), (what, name, precision)
            if precision != 2:
                assert float(ymax.max().view(torch.float32).item()) == float(y.abs().max()), (what, name, precision, "y_absmax")
            else:
                assert int(ymax.max()) == 0, (what, name, "strict fp32 leaves the slots alone")
            if first is None:
                first = y
            assert torch.equal(y, first), (what, name, precision, "conv_precision changes the bits")
    finally:
        _lib.set_option("conv_precision", prev)
    e = rel(first, ref)
    print("%s %s: %.2e" % (what, name, e))
    assert e < TOL, (what, name, e)
    return e


@pytest.mark.parametrize("cin,cout", FAMILIES)
@pytest.mark.parametrize("b,h,w", SHAPES)
def test_narrow_row_convolution_against_float64(b, h, w, cin, cout):
    c = case(b, h, w, w, cin, cout)
    what = "%s %d->%d [%d,%d,%d]" % (kernel_form(cin, cout), cin, cout, b, h, w)
    worst = 0.0
    for name in FORMS:
        bias, res, act, epi, ref = epilogue(c, name.split(",")[0])
        if "NULL" in name:
            bias, ref = None, c["conv"]
        worst = max(worst, check_form(name, c["x"], c["packed"], bias, c["res"] if res else None, c["act"] if act else None, cout, epi,
                                      ref, c["xmax"], what))
    print("%s worst %.2e" % (what, worst))


# backward data: (channels of dz as run, channels of dx, input channels of the launch)
BWD = [(32, 32, 32),        # a 32 -> 32 layer
       (32, 3, 32),         # the input gradient of a 3 -> 32 layer
       (2, 32, 4)]          # the input gradient of a 32 -> 2 layer: dz runs as 4 channels of which two are real


@pytest.mark.parametrize("czr,cdx,crun", BWD)
@pytest.mark.parametrize("b,h,w", ODD)
def test_backward_data_against_float64_autograd(b, h, w, czr, cdx, crun):
    gen = torch.Generator().manual_seed(100 * w + czr + cdx)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32).to(DEV)
    wgt, dz, pre = r(5, 5, cdx, czr) * 0.05, r(b, h, w, czr), r(b, h, w, cdx)          # forward layer cdx -> czr, HWIO; pre-activation of its input
    packed = ops._pack(wgt, czr, cdx, ops.CONV_BWD_DATA)
    ip, op = crun, 16 if cdx <= 16 else 32
    section = packed[:25 * op * ip].view(25, op, ip)
    expect = torch.zeros_like(section)
    expect[:, :cdx, :czr] = wgt.view(25, cdx, czr).flip(0)                              # packed[tap][o][i] = w[24 - tap][o][i]
    assert torch.equal(section, expect), "CONV_BWD_DATA packing"
    w64 = wgt.double().permute(3, 2, 0, 1)
    dzk = ops._pad_channels(dz, crun)
    what = "%s bwd-data %d->%d [%d,%d,%d]" % (kernel_form(crun, cdx), czr, cdx, b, h, w)
    # plain: the gradient with respect to the layer's input
    x64 = torch.zeros(b, cdx, h, w, dtype=torch.float64, device=DEV, requires_grad=True)
    F.conv2d(x64, w64, None, padding=2).backward(dz.double().permute(0, 3, 1, 2))
    check_form("none", dzk, packed, None, None, None, cdx, ops.EPI_NONE, x64.grad.permute(0, 2, 3, 1), ops.absmax_slots(dzk), what)
    # DLRELU: the gradient with respect to the pre-activation whose LeakyReLU is the layer's input
    a64 = pre.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    F.conv2d(F.leaky_relu(a64, SLOPE), w64, None, padding=2).backward(dz.double().permute(0, 3, 1, 2))
    check_form("dlrelu", dzk, packed, None, None, pre, cdx, ops.EPI_DLRELU, a64.grad.permute(0, 2, 3, 1), ops.absmax_slots(dzk), what)


@pytest.mark.parametrize("b,h,w", ODD + SHAPES[8:])
def test_launch_profiler_names_the_four_kernel_forms(b, h, w):
    for cin, cout in ((4, 2), (4, 32), (32, 2), (32, 32)):
        c = case(b, h, w, w, cin, cout)
        with _lib.profile() as p:
            ops.conv5x5_scaled_raw(c["x"], c["packed"], c["bias"], None, None, cout, ops.EPI_LRELU, SLOPE, c["xmax"], None)
        assert conv_kernels(p) == {kernel_form(cin, cout)}, (cin, cout, sorted(p.kernels))


@pytest.mark.parametrize("b,h,w,cin,cout,words", [
    (1, 32, 2, 32, 32, "bad image shape"), (1, 16, 12, 32, 32, "W must divide 64"), (1, 8, 24, 32, 32, "W must divide 64"),
    (1, 4, 48, 32, 32, "W must divide 64"), (1, 6, 16, 32, 32, "W must divide 64"), (1, 3, 32, 4, 32, "W must divide 64"),
    (1, 4, 16, 8, 32, "input channels"), (1, 4, 16, 32, 0, "output channels"), (1, 4, 16, 32, 33, "output channels")])
def test_shapes_outside_the_abi_are_refused_without_a_launch(b, h, w, cin, cout, words):
    packed = case(1, 4, 16, 16, 32, 32)["packed"]
    x = torch.zeros(b, h, w, cin, dtype=torch.float32, device=DEV)
    with _lib.profile() as p:
        with pytest.raises(_lib.SolError, match=words):
            ops.conv5x5_raw(x, packed, None, None, None, cout, ops.EPI_NONE, SLOPE)
        with pytest.raises(_lib.SolError, match=words):
            ops.conv5x5_scaled_raw(x, packed, None, None, None, cout, ops.EPI_NONE, SLOPE, None, None)
    assert not p.kernels, p.kernels
