"""5x5 weight gradient on image rows wider than 64 pixels (pytest -m gpu): sol_conv5x5_bwd_weight + its reduce for W = 64 * tiles
against torch float64 conv2d autograd (independent of oracle/), the tiling identity with and without halo traffic, accumulation,
bit reproducibility, W = 192 and the rejection of W = 96.

Tolerances: those of test_gpu_parity.test_mars_moon_network_full_size_against_torch_float64_autograd (kernels 3e-5, biases 1e-4
relative L2), for every conv_precision."""
import pytest
import torch

import sol_amd
from sol_amd import _lib, ops
from sol_amd._lib import check, ptr, stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL_DW, TOL_DB = 3e-5, 1e-4
SHAPES = [(3, 32), (32, 32), (32, 2)]


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


@pytest.fixture
def precision(request):
    prev = _lib.get_option("conv_precision")
    _lib.set_option("conv_precision", request.param)
    yield request.param
    _lib.set_option("conv_precision", prev)


def tensors(B, H, W, cin, cout, seed=7):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, cin, generator=gen, dtype=torch.float32)
    dz = torch.randn(B, H, W, cout, generator=gen, dtype=torch.float32) * 1e-2
    return x.to(DEV), dz.to(DEV)


def bww(x, dz, part=None, reduce=True, accumulate=0):
    """dW [5,5,cin,cout], db [cout] (and the partial buffer) of the library for x [B,H,W,cin], dz [B,H,W,cout]"""
    lib = sol_amd.load()
    B, H, W, cin = x.shape
    cout = dz.shape[-1]
    cin_k = 4 if cin <= 4 else 32
    xk = ops._pad_channels(x, cin_k)
    if part is None:
        part = torch.zeros(lib.sol_conv5x5_bwd_weight_ws_floats(B, H, W, cin_k, cout), dtype=torch.float32, device=DEV)
    check(lib.sol_conv5x5_bwd_weight(stream(), ptr(xk), ptr(dz.contiguous()), ptr(part), B, H, W, cin_k, cout))
    if not reduce:
        return part
    dw = torch.zeros(5, 5, cin, cout, dtype=torch.float32, device=DEV)
    db = torch.zeros(cout, dtype=torch.float32, device=DEV)
    check(lib.sol_conv5x5_bwd_weight_reduce(stream(), ptr(part.clone()), ptr(dw), ptr(db), B, H, W, cin, cout, accumulate))
    torch.cuda.synchronize()
    return dw, db, part


def reference(x, dz):
    import torch.nn.functional as F
    cin, cout = x.shape[-1], dz.shape[-1]
    w = torch.zeros(cout, cin, 5, 5, dtype=torch.float64, device=DEV, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, device=DEV, requires_grad=True)
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w, b, padding=2)
    (y * dz.double().permute(0, 3, 1, 2)).sum().backward()
    return w.grad.permute(2, 3, 1, 0), b.grad


@pytest.mark.parametrize("precision", [0, 1, 2], indirect=True)
@pytest.mark.parametrize("cin,cout", SHAPES)
@pytest.mark.parametrize("B,H,W", [(2, 32, 128), (1, 256, 128)])
def test_wide_weight_gradient_against_torch_float64(B, H, W, cin, cout, precision):
    x, dz = tensors(B, H, W, cin, cout)
    dw, db, _ = bww(x, dz)
    rw, rb = reference(x, dz)
    e_w, e_b = rel(dw, rw), rel(db, rb)
    print("wide bww %d->%d [%d,%d,%d] precision %d: dW %.2e db %.2e" % (cin, cout, B, H, W, precision, e_w, e_b))
    assert e_w < TOL_DW and e_b < TOL_DB, (e_w, e_b)


@pytest.mark.parametrize("precision", [0, 2], indirect=True)
@pytest.mark.parametrize("cin,cout", SHAPES)
def test_wide_equals_the_sum_of_its_halves_when_the_halo_is_empty_and_differs_when_not(cin, cout, precision):
    """columns 62..65 of x zero: neither half sees the other through its halo, so the W = 128 result is the sum of the two W = 64
    results (reordered fp32 sums: 1e-6 relative, as the manual == autograd tests); random x there: the halo carries data, the sum
    of the halves must miss it."""
    B, H = 2, 32
    x, dz = tensors(B, H, 128, cin, cout, seed=11)
    for empty in (True, False):
        xx = x.clone()
        if empty:
            xx[:, :, 62:66] = 0.0
        dw, db, _ = bww(xx, dz)
        halves = [bww(xx[:, :, s].contiguous(), dz[:, :, s].contiguous()) for s in (slice(0, 64), slice(64, 128))]
        sw, sb = halves[0][0] + halves[1][0], halves[0][1] + halves[1][1]
        e_w, e_b = rel(dw, sw), rel(db, sb)
        print("tiling identity %d->%d precision %d, halo %s: dW %.2e db %.2e" % (cin, cout, precision, "empty" if empty else "full", e_w, e_b))
        assert e_b < 1e-6                       # the bias gradient never sees x
        if empty:
            assert e_w < 1e-6, e_w
        else:
            assert e_w > 1e-3, e_w


@pytest.mark.parametrize("cin,cout", SHAPES)
def test_two_calls_accumulate_into_partial(cin, cout):
    """(at the default conv_precision: accumulation is the partial slice's read-add-store, the same code for every precision's kernel
    family member that serves the shape)"""
    x, dz = tensors(1, 32, 128, cin, cout, seed=13)
    dw1, db1, part = bww(x, dz)
    dw2, db2, _ = bww(x, dz, part=part.clone())
    assert rel(dw2, 2 * dw1) < 1e-6 and rel(db2, 2 * db1) < 1e-6
    x64, dz64 = x[:, :, :64].contiguous(), dz[:, :, :64].contiguous()      # "exactly as at W = 64"
    n1, m1, p64 = bww(x64, dz64)
    n2, m2, _ = bww(x64, dz64, part=p64.clone())
    assert rel(n2, 2 * n1) < 1e-6 and rel(m2, 2 * m1) < 1e-6


@pytest.mark.parametrize("cin,cout", SHAPES)
def test_wide_weight_gradient_is_bit_reproducible(cin, cout):
    x, dz = tensors(2, 64, 128, cin, cout, seed=17)
    a, b = bww(x, dz), bww(x, dz)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize("cin,cout", SHAPES)
def test_three_tiles(cin, cout):
    x, dz = tensors(1, 40, 192, cin, cout, seed=19)
    dw, db, _ = bww(x, dz)
    rw, rb = reference(x, dz)
    assert rel(dw, rw) < TOL_DW and rel(db, rb) < TOL_DB


def test_a_width_that_is_no_multiple_of_64_is_rejected():
    lib = sol_amd.load()
    x, dz = tensors(1, 8, 96, 32, 32)
    part = torch.zeros(1 << 16, dtype=torch.float32, device=DEV)
    assert lib.sol_conv5x5_bwd_weight(stream(), ptr(x), ptr(dz), ptr(part), 1, 8, 96, 32, 32) != 0
    msg = lib.sol_last_error().decode()
    assert "multiple of 64" in msg and "96" in msg, msg
