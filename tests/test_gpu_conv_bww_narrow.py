"""5x5 weight gradient on image rows of up to 64 pixels (pytest -m gpu): every kernel form of sol_conv5x5_bwd_weight, its reduce, the
reduce of twelve layers and the scaled, segmented launch of the fused trainers (sol_conv5x5_bwd_weight_segments), against torch
float64 conv2d autograd (independent of oracle/), at ragged shapes: a last row block shorter than 8 rows, row blocks holding rows of
two images, images shorter than the 5-row tap window, a ragged last chunk of the two-stage reduce.

Every case asserts through _lib.profile() which kernel ran.  Metrics:
  whole tensor   relative L2 of dW < 3e-5 and of db < 1e-4 (the limits of test_gpu_conv_wide_bww and of the mars_moon float64 test);
  per tap        max over the 25 taps of |dW[tap] - ref[tap]| / |ref[tap]| <= max(4 x the same figure of a plain float32 evaluation
                 (torch float32 conv2d autograd on the CPU, same tensors), 1e-6): the kernels claim fp32-equivalent products and sum
                 in another order; a fault in one tap (a halo column, a tap row at the image edge) is not diluted by the other 24.
                 Taps whose reference is zero (H < 3) must be exactly zero.
  exact          integer-valued data (conv_bww_cases.integer_tensors): bit-for-bit equality with float64; one-hot probes; scaling by
                 2^+-40; accumulation.

Measured on an MI355X (per-tap error, kernel / float32 baseline, maxima over the cases of each group):
  public entry, W = 64 (all ten shapes' maxima; thin / bww32 = the options of the case)
    3->32  k_conv5x5_bww_thin<0,2> 2.6e-07 / 2.3e-06    conv_thin 0, k_conv5x5_bww<4,32>  4.9e-07 / 2.3e-06
    4->32  k_conv5x5_bww_thin<0,2> 2.7e-07 / 2.0e-06    conv_thin 0, k_conv5x5_bww<4,32>  5.0e-07 / 2.0e-06
    32->32 k_conv5x5_bww_sb<0>     2.7e-07 / 4.0e-07    precision 2: k_conv5x5_bww32 2.3e-07, conv_bww32 0: k_conv5x5_bww<32,32> 4.3e-07 / 4.0e-07
    32->2  k_conv5x5_bww_thin<1,2> 2.6e-07 / 5.5e-07    conv_thin 0, k_conv5x5_bww<32,2>  5.3e-07 / 5.5e-07
    3->2   k_conv5x5_bww<4,2>      8.4e-07 / 3.5e-06
  public entry, W < 64 (k_conv5x5_bww<...>): 3->32 4.0e-07 / 3.9e-07, 4->32 3.8e-07 / 3.6e-07, 32->32 3.8e-07 / 1.3e-07,
    32->2 4.1e-07 / 1.4e-07, 3->2 9.0e-07 / 8.0e-07
  segments: 3 x [2,8,64] fp16 body 2.4e-07 / 2.3e-07 (also each segment alone, and heavy-tailed x); 3 x [1,5,64] fallback 2.6e-07 / 1.3e-07;
    32 x [1,136,64] fp16 body at 17 rows 3.5e-07 / 6.1e-07; 33 x [1,128,64] fallback 5.0e-07 / 9.0e-07; overwrite <= 2.9e-07; cin_real <= 2.7e-07;
    slots 2^6 too large: 2.01e-07, the figure with exact slots (a power-of-two scale moves exponents, and nothing underflows here)
  The kernel never used more than 0.53 of its limit (whole tensor: dW <= 4.7e-07, db <= 4.4e-07).  The whole file runs in 4 s.
"""
import contextlib
import ctypes as C

import pytest
import torch

import sol_amd
from sol_amd import _lib
from sol_amd._lib import check, ptr, stream
from conv_bww_cases import DZ_UNIT, EXACT_SHAPES, PAIRS, SHAPES, integer_tensors
from test_gpu_conv_wide_bww import TOL_DB, TOL_DW, bww, precision, reference, rel, tensors      # noqa: F401  (precision: a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAP_FACTOR, TAP_FLOOR = 4.0, 1e-6
NAN = float("nan")


@contextlib.contextmanager
def options(**kw):
    prev = {k: _lib.get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            _lib.set_option(k, v)
        yield
    finally:
        for k, v in prev.items():
            _lib.set_option(k, v)


def bww_kernels(p):
    """the weight-gradient kernels a profile saw, spelled without blanks: {'k_conv5x5_bww_thin<0,2>'}"""
    names = {k.strip("()").replace(" ", "") for k in p.kernels}
    return {n for n in names if n.startswith("k_conv5x5_bww")}


def expected_kernel(cin, cout, W, prec, thin=1, bww32=1):
    """the choice of bww_launch for the public entry (no absmax slots)"""
    ck = 4 if cin <= 4 else 32
    if W == 64 and thin and (ck, cout) == (4, 32):
        return "k_conv5x5_bww_thin<0,2>"
    if W == 64 and thin and (ck, cout) == (32, 2):
        return "k_conv5x5_bww_thin<1,2>"
    if (ck, cout) == (32, 32) and W == 64 and prec != 2:
        return "k_conv5x5_bww_sb<0>"
    if (ck, cout) == (32, 32) and W == 64 and bww32:
        return "k_conv5x5_bww32"
    return "k_conv5x5_bww<%d,%d>" % (ck, cout)


def profiled_bww(x, dz, expect, **kw):
    with _lib.profile() as p:
        out = bww(x, dz, **kw)
    assert bww_kernels(p) == {expect}, (expect, sorted(p.kernels))
    return out


def fp32_baseline(x, dz):
    """the same gradient in plain float32: torch conv2d autograd on the CPU"""
    import torch.nn.functional as F
    xc, zc = x.detach().float().cpu(), dz.detach().float().cpu()
    w = torch.zeros(zc.shape[-1], xc.shape[-1], 5, 5, dtype=torch.float32, requires_grad=True)
    y = F.conv2d(xc.permute(0, 3, 1, 2), w, None, padding=2)
    (y * zc.permute(0, 3, 1, 2)).sum().backward()
    return w.grad.permute(2, 3, 1, 0)


def per_tap(dw, ref):
    """(max over the taps with a non-zero reference of the relative L2 error, every other tap exactly zero)"""
    dw, ref = dw.detach().double().cpu().reshape(25, -1), ref.detach().double().cpu().reshape(25, -1)
    d, r = (dw - ref).norm(dim=1), ref.norm(dim=1)
    live = r > 0
    return float((d[live] / r[live]).max()), bool((dw[~live] == 0).all())


_REF = {}


def with_reference(x, dz, key=None):
    """(x, dz, float64 dW, float64 db, per-tap error of the float32 baseline), computed once per key"""
    if key is None or key not in _REF:
        rw, rb = reference(x, dz)
        base, _ = per_tap(fp32_baseline(x, dz), rw)
        if key is None:
            return x, dz, rw, rb, base
        _REF[key] = (x, dz, rw, rb, base)
    return _REF[key]


def random_case(B, H, W, cin, cout, seed=7):
    key = (B, H, W, cin, cout, seed)
    if key not in _REF:
        with_reference(*tensors(B, H, W, cin, cout, seed), key=key)
    return _REF[key]


def assert_close(label, dw, db, rw, rb, base):
    e_w, e_b = rel(dw, rw), rel(db, rb)
    e_tap, dead_zero = per_tap(dw, rw)
    limit = max(TAP_FACTOR * base, TAP_FLOOR)
    print("bww %s: dW %.2e db %.2e per-tap %.2e (float32 %.2e, limit %.2e)" % (label, e_w, e_b, e_tap, base, limit))
    assert dead_zero, "%s: a tap whose reference is zero is not exactly zero" % label
    assert e_w < TOL_DW and e_b < TOL_DB, (label, e_w, e_b)
    assert e_tap <= limit, (label, e_tap, base, limit)
    return e_tap


# ---- 1. the public entry, W <= 64, against float64 ---------------------------------------------------------------------------------
def _public_cases():
    out = []
    for B, H, W in SHAPES:
        for cin, cout in PAIRS:
            if W != 64:
                out.append((B, H, W, cin, cout, 0, 1, 1))
                continue
            out += [(B, H, W, cin, cout, p, 1, 1) for p in (0, 1, 2)]
            if (cin <= 4 and cout == 32) or (cin, cout) == (32, 2):
                out.append((B, H, W, cin, cout, 0, 0, 1))
            if (cin, cout) == (32, 32):
                out.append((B, H, W, cin, cout, 2, 1, 0))
    return out


@pytest.mark.parametrize("B,H,W,cin,cout,prec,thin,bww32", _public_cases(), ids=lambda v: str(v))
def test_narrow_weight_gradient_against_torch_float64(B, H, W, cin, cout, prec, thin, bww32):
    x, dz, rw, rb, base = random_case(B, H, W, cin, cout)
    with options(conv_precision=prec, conv_thin=thin, conv_bww32=bww32):
        dw, db, _ = profiled_bww(x, dz, expected_kernel(cin, cout, W, prec, thin, bww32))
    assert_close("%d->%d [%d,%d,%d] precision %d thin %d bww32 %d" % (cin, cout, B, H, W, prec, thin, bww32), dw, db, rw, rb, base)


# ---- 2. exact tests ------------------------------------------------------------------------------------------------------------------
def _variants(cin, cout, W):
    """(conv_thin, conv_bww32) settings that change the kernel of this pair at this width"""
    v = [(1, 1)]
    if W == 64 and ((cin <= 4 and cout == 32) or (cin, cout) == (32, 2)):
        v.append((0, 1))
    if W == 64 and (cin, cout) == (32, 32):
        v.append((1, 0))
    return v


@pytest.mark.parametrize("precision", [0, 1, 2], indirect=True)
@pytest.mark.parametrize("cin,cout", PAIRS)
@pytest.mark.parametrize("B,H,W", EXACT_SHAPES)
def test_integer_data_is_reproduced_bit_for_bit(B, H, W, cin, cout, precision):
    x, dz = (t.to(DEV) for t in integer_tensors(B, H, W, cin, cout))
    rw, rb = reference(x, dz)
    assert float(rw.abs().max()) > 0
    for thin, b32 in _variants(cin, cout, W):
        with options(conv_thin=thin, conv_bww32=b32):
            dw, db, _ = profiled_bww(x, dz, expected_kernel(cin, cout, W, precision, thin, b32))
        assert torch.equal(dw.double(), rw), (thin, b32, float((dw.double() - rw).abs().max()))
        assert torch.equal(db.double(), rb), (thin, b32)


def _probes(W, cin, cout):
    """one-hot probes ((b, y) of x, (b, y) of dz), (px of x, px of dz), (ci, co) at B = 2, H = 12: image 0 is rows 0..11, image 1 rows
    12..23 of the row sequence, so rows 7 | 8 and 15 | 16 are row-block boundaries and the image boundary 11 | 12 lies inside block 1"""
    rp_in = [((0, 0), (0, 0)), ((0, 11), (0, 11)), ((1, 0), (1, 0)), ((1, 11), (1, 11)), ((0, 7), (0, 7)), ((0, 8), (0, 8)),
             ((0, 7), (0, 8)), ((0, 8), (0, 7)), ((0, 0), (0, 1)), ((0, 1), (0, 0)), ((1, 11), (1, 10)), ((1, 10), (1, 11)),
             ((0, 6), (0, 8)), ((0, 8), (0, 6)), ((0, 7), (0, 9)), ((0, 9), (0, 7)), ((0, 0), (0, 2)), ((0, 2), (0, 0)),
             ((1, 3), (1, 4)), ((1, 4), (1, 3)), ((1, 9), (1, 11)), ((1, 11), (1, 9))]
    rp_out = [((0, 5), (0, 8)), ((0, 8), (0, 5)), ((0, 11), (1, 0)), ((1, 0), (0, 11)), ((0, 10), (1, 0)), ((1, 1), (0, 11)),
              ((0, 3), (1, 3)), ((1, 11), (0, 0))]
    m = W // 2
    cp_in = [(0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1), (1, 3), (3, 1), (W - 1, W - 1), (W - 1, W - 2), (W - 2, W - 1), (W - 1, W - 3),
             (W - 3, W - 1), (W - 2, W - 2), (W - 2, W - 4), (W - 4, W - 2), (m - 1, m), (m, m - 1), (m - 1, m + 1), (m + 1, m - 1)]
    if W == 64:
        cp_in += [(15, 16), (16, 15), (15, 17), (17, 15), (47, 48), (48, 47), (3, 4), (4, 3), (59, 60), (60, 59)]
    cp_out = [(0, 3), (3, 0), (W - 1, W - 4), (W - 4, W - 1), (0, W - 1), (W - 1, 0)]
    chans = [(ci, co) for ci in sorted({0, min(15, cin - 1), min(16, cin - 1), cin - 1})
             for co in sorted({0, min(15, cout - 1), min(16, cout - 1), cout - 1})]
    out = [(rp, cp_in[i % len(cp_in)], chans[i % len(chans)]) for i, rp in enumerate(rp_in + rp_out)]
    out += [(rp_in[(5 * i) % len(rp_in)], cp, chans[(i + 1) % len(chans)]) for i, cp in enumerate(cp_in + cp_out)]
    out += [(rp_in[(3 * i + 6) % len(rp_in)], cp_in[(7 * i + 1) % len(cp_in)], ch) for i, ch in enumerate(chans)]
    return out


@pytest.mark.parametrize("cin,cout", PAIRS)
def test_one_hot_probes_land_on_their_tap_and_nowhere_else(cin, cout):
    B, H, XV, ZV = 2, 12, 3.0, 0.5
    runs = [(64, dict(conv_precision=0, conv_thin=1, conv_bww32=1)), (16, dict(conv_precision=0))]
    if (cin <= 4 and cout == 32) or (cin, cout) == (32, 2):
        runs.append((64, dict(conv_precision=0, conv_thin=0)))
    if (cin, cout) == (32, 32):
        runs += [(64, dict(conv_precision=2, conv_bww32=1)), (64, dict(conv_precision=2, conv_bww32=0))]
    for W, opts in runs:
        probes = _probes(W, cin, cout)
        x = torch.zeros(B, H, W, cin, dtype=torch.float32, device=DEV)
        dz = torch.zeros(B, H, W, cout, dtype=torch.float32, device=DEV)
        want_w = torch.zeros(len(probes), 5, 5, cin, cout, dtype=torch.float32)
        want_b = torch.zeros(len(probes), cout, dtype=torch.float32)
        got_w, got_b, hits = [], [], 0
        expect = expected_kernel(cin, cout, W, opts.get("conv_precision", 0), opts.get("conv_thin", 1), opts.get("conv_bww32", 1))
        with options(**opts):
            for n, (((bx, yx), (bz, yz)), (px, pz), (ci, co)) in enumerate(probes):
                x[bx, yx, px, ci] = XV
                dz[bz, yz, pz, co] = ZV
                dw, db, _ = profiled_bww(x, dz, expect) if n == 0 else bww(x, dz)
                got_w.append(dw)
                got_b.append(db)
                x[bx, yx, px, ci] = 0.0
                dz[bz, yz, pz, co] = 0.0
                want_b[n, co] = ZV
                if bx == bz and abs(yx - yz) <= 2 and abs(px - pz) <= 2:      # x position = dz position + (dy - 2, dx - 2)
                    want_w[n, yx - yz + 2, px - pz + 2, ci, co] = XV * ZV
                    hits += 1
        assert hits == len(probes) - 14                 # every probe but the 8 row pairs and 6 column pairs out of reach
        got_w, got_b = torch.stack(got_w).cpu(), torch.stack(got_b).cpu()
        bad = [(probes[n], got_w[n].nonzero().tolist()[:4]) for n in range(len(probes)) if not (torch.equal(got_w[n], want_w[n]) and torch.equal(got_b[n], want_b[n]))]
        assert not bad, (expect, W, len(bad), bad[:5])


@pytest.mark.parametrize("precision", [0, 1, 2], indirect=True)
@pytest.mark.parametrize("cin,cout", PAIRS)
def test_a_power_of_two_factor_changes_no_mantissa_bit(cin, cout, precision):
    x, dz = tensors(3, 5, 64, cin, cout, seed=29)
    expect = expected_kernel(cin, cout, 64, precision)
    dw, db, _ = profiled_bww(x, dz, expect)
    assert float(dw.abs().max()) > 0
    for s in (2.0 ** -40, 2.0 ** 40):
        dws, dbs, _ = profiled_bww(x, dz * s, expect)
        assert torch.equal(dws, dw * s) and torch.equal(dbs, db * s), s


# ---- 3. accumulation and the reduce --------------------------------------------------------------------------------------------------
def reduce_into(part, dw, db, B, H, W, accumulate):
    """sol_conv5x5_bwd_weight_reduce of a CLONE of part (the reduce folds chunk sums into the buffer it is given)"""
    check(sol_amd.load().sol_conv5x5_bwd_weight_reduce(stream(), ptr(part.clone()), ptr(dw), ptr(db), B, H, W, dw.shape[2], dw.shape[3], accumulate))
    torch.cuda.synchronize()
    return dw, db


@pytest.mark.parametrize("cin,cout", PAIRS)
@pytest.mark.parametrize("B,H,W", [(3, 5, 64), (3, 6, 32)])
def test_two_calls_into_one_partial_give_exactly_twice_the_gradient(B, H, W, cin, cout):
    x, dz = (t.to(DEV) for t in integer_tensors(B, H, W, cin, cout))
    rw, rb = reference(x, dz)
    part = bww(x, dz, reduce=False)
    dw2, db2, _ = bww(x, dz, part=part)
    assert torch.equal(dw2.double(), 2 * rw) and torch.equal(db2.double(), 2 * rb)


@pytest.mark.parametrize("cin,cout", PAIRS)
@pytest.mark.parametrize("B,H,W", [(3, 5, 64), (1, 136, 64)])
def test_the_reduce_adds_onto_dw_and_db_when_told_to_accumulate(B, H, W, cin, cout):
    """(1,136,64): two-stage reduce; B*H*W*12 = 104448 units and the integers added below stay far below 2^24"""
    x, dz = (t.to(DEV) for t in integer_tensors(B, H, W, cin, cout))
    rw, rb = reference(x, dz)
    part = bww(x, dz, reduce=False)
    gen = torch.Generator().manual_seed(31)
    dw0 = (torch.randint(-9, 10, (5, 5, cin, cout), generator=gen).float() * DZ_UNIT).to(DEV)
    db0 = (torch.randint(1, 10, (cout,), generator=gen).float() * DZ_UNIT).to(DEV)
    dw, db = reduce_into(part, dw0.clone(), db0.clone(), B, H, W, 1)
    assert torch.equal(dw.double(), dw0.double() + rw) and torch.equal(db.double(), db0.double() + rb)
    dw, db = reduce_into(part, dw0.clone(), db0.clone(), B, H, W, 0)
    assert torch.equal(dw.double(), rw) and torch.equal(db.double(), rb)


MARS_MOON = [(3, 32)] + [(32, 32)] * 10 + [(32, 2)]


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("B,H,W", [(1, 136, 64), (2, 5, 64)])
def test_the_reduce_of_twelve_layers_equals_twelve_reduces(B, H, W, accumulate):
    lib = sol_amd.load()
    parts = [bww(*tensors(B, H, W, ci, co, seed=40 + k), reduce=False) for k, (ci, co) in enumerate(MARS_MOON)]
    n_flat = sum(25 * ci * co + co for ci, co in MARS_MOON)
    grads0 = torch.randn(n_flat, generator=torch.Generator().manual_seed(37), dtype=torch.float32).to(DEV)
    grads, single = grads0.clone(), grads0.clone()
    offs, o = [], 0
    for ci, co in MARS_MOON:                                    # Keras get_weights() order: kernel, bias, kernel, bias, ...
        offs.append((o, o + 25 * ci * co))
        o += 25 * ci * co + co
    clones = [p.clone() for p in parts]
    arr = lambda ptrs: (C.c_void_p * 12)(*ptrs)
    i32 = lambda v: (C.c_int32 * 12)(*v)
    check(lib.sol_conv5x5_bwd_weight_reduce_jobs(stream(), 12, arr([p.data_ptr() for p in clones]),
                                                 arr([grads.data_ptr() + 4 * ow for ow, _ in offs]), arr([grads.data_ptr() + 4 * ob for _, ob in offs]),
                                                 B, H, W, i32([ci for ci, _ in MARS_MOON]), i32([co for _, co in MARS_MOON]), accumulate))
    for (ci, co), p, (ow, ob) in zip(MARS_MOON, parts, offs):
        reduce_into(p, single[ow:ob].view(5, 5, ci, co), single[ob:ob + co], B, H, W, accumulate)
    torch.cuda.synchronize()
    assert torch.equal(grads, single)
    assert not torch.equal(grads, grads0)
    if not accumulate:                                          # and it is the gradient: the first and the last layer against float64
        for k in (0, 11):
            ci, co = MARS_MOON[k]
            rw, rb = reference(*tensors(B, H, W, ci, co, seed=40 + k))
            ow, ob = offs[k]
            assert rel(grads[ow:ob].view(5, 5, ci, co), rw) < TOL_DW and rel(grads[ob:ob + co], rb) < TOL_DB


@pytest.mark.parametrize("cin,cout", [(3, 32), (32, 32), (32, 2)])
def test_the_reduce_folds_in_place_and_is_reproducible_from_fresh_clones(cin, cout):
    """include/sol_hip.h: beyond 16 row blocks the reduce writes chunk sums into `partial`.  Nothing here reads a buffer after it
    was reduced: each reduce gets a fresh clone of the kernel's output."""
    lib = sol_amd.load()
    B, H, W = 1, 136, 64
    x, dz, rw, rb, base = random_case(B, H, W, cin, cout)
    part = bww(x, dz, reduce=False)
    outs = []
    for _ in range(2):
        fresh = part.clone()
        dw = torch.full((5, 5, cin, cout), NAN, dtype=torch.float32, device=DEV)
        db = torch.full((cout,), NAN, dtype=torch.float32, device=DEV)
        check(lib.sol_conv5x5_bwd_weight_reduce(stream(), ptr(fresh), ptr(dw), ptr(db), B, H, W, cin, cout, 0))
        torch.cuda.synchronize()
        outs.append((dw, db))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert_close("fresh clone %d->%d" % (cin, cout), outs[0][0], outs[0][1], rw, rb, base)


# ---- 4. the scaled, segmented form the trainers launch ---------------------------------------------------------------------------------
SLOTS = 256
FAR = 2.0 ** 40          # what the words between two segments' slots hold: a scale read from there flushes every operand to zero


def bits(v):
    return int(torch.tensor(float(v), dtype=torch.float32).view(torch.int32))


def make_slots(t, stride, over=1.0):
    """[nseg, stride] int32: segment s has its SOL_ABSMAX_SLOTS slots at s * stride (max|t[s]| * over in one of them)"""
    s = torch.full((t.shape[0], stride), bits(FAR), dtype=torch.int32)
    s[:, :SLOTS] = 0
    for k in range(t.shape[0]):
        s[k, (37 * k + 5) % SLOTS] = bits(float(t[k].abs().max()) * over)
    return s.to(DEV)


def seg_bww(x, dz, expect, slots="own", stride=2 * SLOTS, over=1.0, overwrite=1, cin_real=0, fill=0.0):
    """dW, db of sol_conv5x5_bwd_weight_segments + its reduce for x [nseg,B,H,W,cin], dz [nseg,B,H,W,cout]"""
    lib = sol_amd.load()
    assert sol_amd.load().sol_absmax_slots() == SLOTS
    nseg, B, H, W, cin = x.shape
    cout = dz.shape[-1]
    part = torch.full((lib.sol_conv5x5_bwd_weight_segments_ws_floats(nseg, B, H, cin, cout),), fill, dtype=torch.float32, device=DEV)
    if slots == "own":
        slots = (make_slots(x, stride, over), make_slots(dz, stride, over))
    xs, zs = slots if slots else (None, None)
    with _lib.profile() as p:
        check(lib.sol_conv5x5_bwd_weight_segments(stream(), ptr(x), ptr(dz), ptr(part), nseg, x[0].numel(), dz[0].numel(), overwrite, B, H, W, cin, cout,
                                                  ptr(xs), ptr(zs), stride, cin_real))
    assert bww_kernels(p) == {expect}, (expect, sorted(p.kernels))
    cr = cin_real or cin
    dw = torch.full((5, 5, cr, cout), NAN, dtype=torch.float32, device=DEV)
    db = torch.full((cout,), NAN, dtype=torch.float32, device=DEV)
    check(lib.sol_conv5x5_bwd_weight_segments_reduce(stream(), ptr(part), ptr(dw), ptr(db), nseg, B, H, cr, cout, 0))
    torch.cuda.synchronize()
    return dw, db, slots


def flat(t):
    return t.reshape((-1,) + tuple(t.shape[2:]))


def segments(nseg, B, H, cin, cout, x_scale, dz_scale, seed, heavy=False):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(nseg, B, H, 64, cin, generator=gen, dtype=torch.float32)
    if heavy:
        x = x * torch.exp(2 * torch.randn(nseg, B, H, 64, cin, generator=gen, dtype=torch.float32))
    dz = torch.randn(nseg, B, H, 64, cout, generator=gen, dtype=torch.float32) * 1e-2
    sx = torch.tensor(x_scale, dtype=torch.float32).reshape(-1, 1, 1, 1, 1)
    sz = torch.tensor(dz_scale, dtype=torch.float32).reshape(-1, 1, 1, 1, 1)
    return (x * sx).to(DEV), (dz * sz).to(DEV)


DECAY = ([1.0, 2.0 ** 5, 2.0 ** -5], [1.0, 2.0 ** -10, 2.0 ** -20])     # x, dz: how gradients decay across unrolled steps


def check_segments(label, x, dz, expect):
    """the sum over the segments, and every segment on its own (the others' dz zero, the slots unchanged): in the sum a segment whose
    dz is 2^-20 of another's could be lost, or read at another's scale, without moving any metric"""
    dw, db, slots = seg_bww(x, dz, expect)
    assert_close(label, dw, db, *with_reference(flat(x), flat(dz))[2:])
    for s in range(x.shape[0]):
        only = torch.zeros_like(dz)
        only[s] = dz[s]
        dw, db, _ = seg_bww(x, only, expect, slots=slots)
        assert_close("%s, segment %d alone" % (label, s), dw, db, *with_reference(x[s], dz[s])[2:])


@pytest.mark.parametrize("heavy", [False, True])
def test_segments_with_very_different_scales_take_the_fp16_body(heavy):
    x, dz = segments(3, 2, 8, 32, 32, *DECAY, seed=51, heavy=heavy)
    check_segments("segments 3 x [2,8,64] %s" % ("heavy-tailed x" if heavy else "normal x"), x, dz, "k_conv5x5_bww_sb<2>")


def test_row_blocks_that_straddle_segments_fall_back_to_the_six_product_body():
    x, dz = segments(3, 1, 5, 32, 32, *DECAY, seed=53)              # 15 rows, 5 % 8 != 0
    check_segments("segments 3 x [1,5,64] straddling", x, dz, "k_conv5x5_bww_sb<0>")


@pytest.mark.parametrize("nseg,H,expect", [(32, 136, "k_conv5x5_bww_sb<2>"), (33, 128, "k_conv5x5_bww_sb<0>")])
def test_more_than_4096_rows_run_17_rows_per_workgroup(nseg, H, expect):
    """32 x 136 = 4352 rows: 17 per workgroup and 136 % 17 == 0, the fp16 body; 33 x 128 = 4224 rows: 17 again, 128 % 17 != 0, the fallback"""
    x, dz = segments(nseg, 1, H, 32, 32, [2.0 ** ((s % 5) - 2) for s in range(nseg)], [2.0 ** -(s % 7) for s in range(nseg)], seed=57 + nseg)
    dw, db, _ = seg_bww(x, dz, expect)
    assert_close("segments %d x [1,%d,64]" % (nseg, H), dw, db, *with_reference(flat(x), flat(dz))[2:])


@pytest.mark.parametrize("cin,cout,expect", [(4, 32, "k_conv5x5_bww_thin<0,2>"), (32, 32, "k_conv5x5_bww_sb<2>"), (32, 2, "k_conv5x5_bww_thin<1,2>")])
@pytest.mark.parametrize("nseg,B,H", [(2, 2, 8), (3, 1, 5)])
def test_overwrite_stores_every_word_the_reduce_reads(nseg, B, H, cin, cout, expect):
    if (cin, cout) == (32, 32) and (B * H) % 8:
        expect = "k_conv5x5_bww_sb<0>"
    x, dz = segments(nseg, B, H, cin, cout, [1.0] * nseg, [1.0] * nseg, seed=61)
    clean = seg_bww(x, dz, expect, overwrite=1, fill=0.0)
    dirty = seg_bww(x, dz, expect, overwrite=1, fill=NAN)
    added = seg_bww(x, dz, expect, overwrite=0, fill=0.0)
    assert bool(torch.isfinite(dirty[0]).all()) and bool(torch.isfinite(dirty[1]).all())
    assert torch.equal(dirty[0], clean[0]) and torch.equal(dirty[1], clean[1])
    assert torch.equal(added[0], clean[0]) and torch.equal(added[1], clean[1])
    assert_close("overwrite %d->%d %d x [%d,%d,64]" % (cin, cout, nseg, B, H), dirty[0], dirty[1], *with_reference(flat(x), flat(dz))[2:])


@pytest.mark.parametrize("cin_real", [1, 2, 3])
def test_cin_real_skips_the_padding_channels_and_changes_no_bit_of_the_others(cin_real):
    x, dz = segments(2, 2, 8, 4, 32, [1.0, 4.0], [1.0, 0.25], seed=67)
    x[..., cin_real:] = 0.0
    full_w, full_b, _ = seg_bww(x, dz, "k_conv5x5_bww_thin<0,2>", slots=None)
    assert bool((full_w[:, :, cin_real:] == 0).all()) and float(full_w[:, :, :cin_real].abs().max()) > 0
    dw, db, _ = seg_bww(x, dz, "k_conv5x5_bww_thin<0,1>", slots=None, cin_real=cin_real, fill=NAN)     # reduced with the real channel count
    assert dw.shape[2] == cin_real and torch.equal(dw, full_w[:, :, :cin_real]) and torch.equal(db, full_b)
    assert_close("cin_real %d" % cin_real, dw, db, *with_reference(flat(x)[..., :cin_real].contiguous(), flat(dz))[2:])


def test_slots_that_over_report_the_maximum_cost_accuracy_only():
    """2^6 too large: six binades of fp16 range given away, still inside the limits (measured: the same bits -- the two fp16 parts keep
    their 22 mantissa bits until the low part underflows, 2^-19 below the reported maximum).  Slots that under-report overflow fp16 by
    design and are not tested."""
    x, dz = segments(3, 2, 8, 32, 32, *DECAY, seed=51)
    ref = with_reference(flat(x), flat(dz))[2:]
    dw, db, _ = seg_bww(x, dz, "k_conv5x5_bww_sb<2>")
    exact = assert_close("exact slots", dw, db, *ref)
    dw, db, _ = seg_bww(x, dz, "k_conv5x5_bww_sb<2>", over=64.0)
    stale = assert_close("slots 2^6 too large", dw, db, *ref)
    print("stale absmax: per-tap %.2e with exact slots, %.2e with slots 2^6 too large" % (exact, stale))


def test_integer_data_is_reproduced_bit_for_bit_by_the_fp16_body():
    x, dz = (torch.stack(p).to(DEV) for p in zip(integer_tensors(2, 8, 64, 32, 32, seed=71), integer_tensors(2, 8, 64, 32, 32, seed=73)))
    rw, rb = reference(flat(x), flat(dz))
    for expect, prec in (("k_conv5x5_bww_sb<2>", 0), ("k_conv5x5_bww_sb<0>", 1)):
        with options(conv_precision=prec):
            dw, db, _ = seg_bww(x, dz, expect)
        assert torch.equal(dw.double(), rw) and torch.equal(db.double(), rb), expect
