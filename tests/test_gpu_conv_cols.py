"""Column-masked 5x5 convolutions on pitched rows (pytest -m gpu): sol_conv5x5_cols -- rows of pitch W = 64 * tiles of which the first
WV pixels are data -- against torch.nn.functional.conv2d in float64 on the DENSE [B,H,WV,C] tensors (independent of oracle/), for
every (cin, cout) family, every epilogue and every conv_precision; the pad columns of the output are exactly zero although the output
buffer is pre-filled with NaN, the published absmax is that of the valid columns, WV == W is sol_conv5x5_scaled bit for bit, two calls
agree bit for bit; and the unchanged weight gradient at the pitch returns the dense image's gradient when the pad columns are zero.

Tolerances (relative L2), those of the existing convolution tests of tests/test_gpu_parity.py for the same arithmetic:
  conv_precision 0 (fp16 x 3 with the operand's absmax): 1e-6, test_conv5x5_scaled_fp16_path_against_float64;
  conv_precision 1 (bf16 x 6) and 2 (strict fp32 MFMA):  2e-6, test_conv5x5_against_oracle.
Weight gradient: TOL_DW / TOL_DB of tests/test_gpu_conv_wide_bww.py.

The absmax slots: the strict-fp32 kernels (conv_precision 2) neither consume nor publish them -- sol_conv5x5_scaled attaches y_absmax
to the split-precision kernels only, and sol_conv5x5_cols launches what it launches -- so there the slots must stay untouched."""
import pytest
import torch
import torch.nn.functional as F

import sol_amd
from sol_amd import _lib, ops
from test_gpu_conv_wide_bww import TOL_DB, TOL_DW, bww, reference as bww_reference

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {0: 1e-6, 1: 2e-6, 2: 2e-6}
B, H = 2, 6
WIDTHS = [(128, 65), (128, 72), (128, 100), (128, 127), (64, 40), (192, 130)]     # (pitch W, valid WV)
CHANNELS = [(4, 32), (32, 32), (32, 2)]
SLOPE = 0.3
EPILOGUES = ("none", "lrelu", "lrelu+res", "dlrelu", "dlrelu+skip")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


@pytest.fixture
def precision(request):
    prev = _lib.get_option("conv_precision")
    _lib.set_option("conv_precision", request.param)
    yield request.param
    _lib.set_option("conv_precision", prev)


def pitched(t, W):
    """[B,H,WV,C] -> [B,H,W,C] with zero pad columns"""
    out = torch.zeros(t.shape[0], t.shape[1], W, t.shape[3], dtype=t.dtype, device=t.device)
    out[:, :, :t.shape[2]] = t
    return out


_CASES = {}


def case(b, h, W, WV, cin, cout):
    """dense operands, their pitched copies, the packed weights and the float64 convolution of one shape -- computed once, never modified"""
    key = (b, h, W, WV, cin, cout)
    if key not in _CASES:
        gen = torch.Generator().manual_seed(1000 * W + 10 * WV + cin + cout)
        r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)
        x = r(b, h, WV, cin)
        if cin == 4:
            x[..., 3] = 0.0                              # the zero-padded fourth channel of a three-channel input
        w, bias = r(5, 5, cin, cout) * 0.05, r(cout) + 0.5          # (a bias far from zero: an unmasked pad pixel would hold it)
        res, act = r(b, h, WV, cout), r(b, h, WV, cout)
        x, w, bias, res, act = (t.to(DEV) for t in (x, w, bias, res, act))
        conv = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(3, 2, 0, 1), None, padding=2).permute(0, 2, 3, 1)
        c = dict(x=x, bias=bias, res=res, act=act, conv=conv, xp=pitched(x, W), resp=pitched(res, W), actp=pitched(act, W),
                 packed=ops._pack(w, cin, cout, ops.CONV_FWD))
        c["xmax"] = ops.absmax_slots(x) if cin == 32 else None
        torch.cuda.synchronize()
        _CASES[key] = c
    return _CASES[key]


def epilogue(c, name):
    """(bias, residual, act_ref, epilogue code, float64 reference on the dense tensors) of one epilogue form"""
    bias = c["bias"] if "dlrelu" not in name else None              # (the backward-data launches carry no bias)
    res = name in ("lrelu+res", "dlrelu+skip")
    ref = c["conv"] + (bias.double() if bias is not None else 0.0) + (c["res"].double() if res else 0.0)
    if name.startswith("lrelu"):
        return bias, res, False, ops.EPI_LRELU, torch.where(ref > 0, ref, SLOPE * ref)
    if name.startswith("dlrelu"):
        return bias, res, True, ops.EPI_DLRELU, ref * torch.where(c["act"].double() > 0, 1.0, SLOPE)
    return bias, res, False, ops.EPI_NONE, ref


def run_cols(c, name, W, WV, cout, ymax=None, prefill=float("nan")):
    bias, res, act, epi, ref = epilogue(c, name)
    y = torch.full((c["xp"].shape[0], c["xp"].shape[1], W, cout), prefill, dtype=torch.float32, device=DEV)
    ops.conv5x5_cols_raw(c["xp"], c["packed"], bias, c["resp"] if res else None, c["actp"] if act else None, cout, epi, SLOPE, WV,
                         c["xmax"], ymax, y=y)
    return y, ref


def check_cols(c, W, WV, cout, precision, what):
    for name in EPILOGUES:
        ymax = torch.zeros(ops.AMAX_SLOTS, dtype=torch.int32, device=DEV)
        y, ref = run_cols(c, name, W, WV, cout, ymax)
        e = rel(y[:, :, :WV], ref)
        print("%s %s precision %d: valid columns %.2e" % (what, name, precision, e))
        assert e < TOL[precision], (name, e)
        assert bool((y[:, :, WV:] == 0.0).all()), (name, "pad columns")                   # also: no NaN of the pre-fill left
        if precision != 2:
            assert float(ymax.max().view(torch.float32).item()) == float(y[:, :, :WV].abs().max()), name
        else:
            assert int(ymax.max()) == 0, name                                             # strict fp32: slots untouched (module docstring)
        y2, _ = run_cols(c, name, W, WV, cout, prefill=0.0)
        assert torch.equal(y, y2), (name, "two calls")


@pytest.mark.parametrize("precision", [0, 1, 2], indirect=True)
@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("W,WV", WIDTHS)
def test_masked_convolution_against_float64_on_the_dense_tensors(W, WV, cin, cout, precision):
    check_cols(case(B, H, W, WV, cin, cout), W, WV, cout, precision, "cols %d->%d [%d,%d,%d|%d]" % (cin, cout, B, H, WV, W))


@pytest.mark.parametrize("opts,b,h,W,WV,cin,cout,kernel", [
    ({"conv_dx": 0}, 2, 6, 128, 100, 32, 32, "k_conv5x5_sb<2, 2, true>"),               # row-per-wave fp16 kernels
    ({"conv_dx": 0, "conv_thin_valu": 0}, 2, 6, 64, 40, 32, 2, "k_conv5x5_sb<1, 2, true>"),
    ({"conv_dx": 3}, 2, 6, 128, 100, 32, 32, "k_conv5x5_dx<1, 2, false, true>"),        # dx-major, one row, both channel tiles
    ({}, 2, 6, 128, 100, 32, 32, "k_conv5x5_dx<1, 1, true, true>"),                     # ... as two half-channel workgroups (default)
    ({}, 2, 96, 128, 100, 32, 32, "k_conv5x5_dx<3, 2, false, true>"),                   # 128 three-row workgroups: the chip-filling form
    ({"conv_dx": 15}, 2, 96, 128, 100, 32, 2, "k_conv5x5_dx<3, 1, false, true>"),
    ({}, 2, 6, 128, 100, 32, 2, "k_conv5x5_dx<1, 1, false, true>"),
    ({}, 2, 6, 64, 40, 32, 2, "k_conv5x5_thin32<2, 16, true>"),                         # exact-fp32 VALU form (plain epilogue only)
    ({"conv_thin_valu": 2}, 2, 6, 64, 40, 32, 3, "k_conv5x5_thin32<4, 8, true>"),
    ({}, 2, 6, 64, 40, 4, 32, "k_conv5x5_t3<2, true>"),                                 # thin input, three rows per workgroup
    ({}, 2, 6, 64, 40, 4, 16, "k_conv5x5_t3<1, true>"),
    ({"conv_thin_t3": 0}, 2, 6, 64, 40, 4, 32, "k_conv5x5<4, 2, true>"),
    ({}, 2, 6, 128, 100, 4, 2, "k_conv5x5<4, 1, true>"),
    ({"conv_precision": 2, "conv_r3": 0}, 2, 6, 128, 100, 32, 32, "k_conv5x5_c32<2, true>"),
    ({"conv_precision": 2, "conv_r3": 0}, 2, 6, 128, 100, 32, 2, "k_conv5x5_c32<1, true>"),
    ({"conv_precision": 2}, 2, 6, 128, 100, 32, 2, "k_conv5x5_r3<1, true>"),
    ({"conv_precision": 1}, 2, 6, 128, 100, 32, 2, "k_conv5x5_sb<1, 0, true>"),
    # the chip-filling dx form where its grid is not exact: last workgroup of two rows, 130 -> 136 workgroups (padding tiles), odd H
    ({}, 2, 97, 128, 100, 32, 32, "k_conv5x5_dx<3, 2, false, true>"),
])
def test_every_masked_kernel_form_runs_and_is_right(opts, b, h, W, WV, cin, cout, kernel):
    """the forms the default options do not reach at B = 2, H = 6 (launch profiler: the named masked instantiation did run)"""
    saved = {k: _lib.get_option(k) for k in opts}
    try:
        for k, v in opts.items():
            _lib.set_option(k, v)
        precision = _lib.get_option("conv_precision")
        c = case(b, h, W, WV, cin, cout)
        check_cols(c, W, WV, cout, precision, kernel)
        with _lib.profile() as p:
            run_cols(c, "dlrelu+skip" if "thin32" not in kernel else "none", W, WV, cout)
        names = [k.strip("()").replace(" ", "") for k in p.kernels]
        assert kernel.replace(" ", "") in names, p.kernels
    finally:
        for k, v in saved.items():
            _lib.set_option(k, v)


@pytest.mark.parametrize("precision", [0, 1, 2], indirect=True)
@pytest.mark.parametrize("cin,cout", CHANNELS)
def test_full_width_is_sol_conv5x5_scaled_bit_for_bit(cin, cout, precision):
    W = 128
    c = case(B, H, W, W, cin, cout)
    for name in EPILOGUES:
        bias, res, act, epi, _ = epilogue(c, name)
        ya, yb = (torch.zeros(ops.AMAX_SLOTS, dtype=torch.int32, device=DEV) for _ in range(2))
        y_cols, _ = run_cols(c, name, W, W, cout, ya)
        y_scaled = ops.conv5x5_scaled_raw(c["xp"], c["packed"], bias, c["resp"] if res else None, c["actp"] if act else None, cout, epi,
                                          SLOPE, c["xmax"], yb)
        assert torch.equal(y_cols, y_scaled) and torch.equal(ya, yb), name
    bias, _, _, epi, _ = epilogue(c, "lrelu")
    with _lib.profile() as p:
        run_cols(c, "lrelu", W, W, cout)
    with _lib.profile() as q:
        ops.conv5x5_scaled_raw(c["xp"], c["packed"], bias, None, None, cout, epi, SLOPE, c["xmax"], None)
    assert set(p.kernels) == set(q.kernels), (p.kernels, q.kernels)            # the same kernel, not its masked instantiation


@pytest.mark.parametrize("precision", [0, 1, 2], indirect=True)
@pytest.mark.parametrize("cin,cout", [(3, 32), (32, 32), (32, 2), (3, 2)])
@pytest.mark.parametrize("WV", [72, 100])
def test_weight_gradient_at_the_pitch_is_the_dense_gradient(WV, cin, cout, precision):
    """sol_conv5x5_bwd_weight + reduce, unchanged, at pitch 128 on zero-padded x and dz: the pad pixels contribute exact zeros, so the
    result is the dense [B,H,WV] image's dw / db -- asserted against the float64 reference on the DENSE tensors."""
    b, h, W = 2, 40, 128
    gen = torch.Generator().manual_seed(WV + cin + cout)
    x = torch.randn(b, h, WV, cin, generator=gen, dtype=torch.float32).to(DEV)
    dz = (torch.randn(b, h, WV, cout, generator=gen, dtype=torch.float32) * 1e-2).to(DEV)
    dw, db, _ = bww(pitched(x, W), pitched(dz, W))
    rw, rb = bww_reference(x, dz)
    e_w, e_b = rel(dw, rw), rel(db, rb)
    print("pitched bww %d->%d WV %d precision %d: dW %.2e db %.2e" % (cin, cout, WV, precision, e_w, e_b))
    assert e_w < TOL_DW and e_b < TOL_DB, (e_w, e_b)
