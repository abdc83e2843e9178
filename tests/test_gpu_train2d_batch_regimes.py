"""The fused 2-D training step along the BATCH axis (pytest -m gpu): sol_train_fwd_bwd against the float64 oracle at the batch
sizes and unroll depths where the launches of its hot path change shape.  Every other suite of the 2-D path runs at B = 2 or 3 (or
the exact grids of B = 3, 6, 9, 12); tests/test_train2d_batch_regimes_cpu.py restates the launch arithmetic quoted here.

128 x 64 (rows of 64 pixels, 128 rows per image):
  (B, ms) = (1, 1)   ms = 1: the reverse sweep has no solver adjoint -- the weight-gradient jobs go out alone (one k_karman_bwd_bww
                     launch without solver workgroups) and the density has only its own k_density_step launch
            (4, 2)   512 rows: every 32 -> 32 launch, forward and backward-data, is k_conv5x5_dx<3, 2> with a last workgroup of two
                     rows and five padding tiles (171 -> 176); the density rides in the band launch of step 1
            (5, 1)   640 rows: a last workgroup of one row (214 -> 216)
            (17, 1)  a third group of eight simulations in k_karman_fwd_bands; 2176 rows > 1024: the 3 -> 32 layer and the seed launch
                     fall back from k_conv5x5_t3 to k_conv5x5<4, 2>
            (41, 1)  the first batch the band launch refuses (option fwd_bands still on); 5248 rows in the thin weight gradients
 64 x 32 (the CNN runs on the transposed images: rows of 64 pixels, 32 rows per image):
            (1, 1)   the density advection rides in the jobs-only launch (k_karman_bwd_bww_small, once)
            (5, 3)   160 rows: an odd batch in the one-row form k_conv5x5_dx<1, 1, true>
            (13, 2)  416 rows: the three-row form, last workgroup of two rows, 139 -> 144, images of 32 rows straddle workgroups
            (33, 1)  1056 rows > 1024: the thin-input fallback kernel in the transposed order

Each case asserts what test_train_step_full_size_against_oracle asserts, with the same bounds (TOL_GRAD, TOL_FIELD of
tests/test_gpu_parity.py): the loss and every per-step loss to 1e-5 relative, the full gradient in relative L2 < TOL_GRAD and its
worst tensor < 3 TOL_GRAD, the final d, v_y, v_x < TOL_FIELD against the oracle's own final state, zero solver iterations, and a
second call that returns the same bits; then the kernels the case is there for, from the launch profiler.

Measured on an MI355X (loss: relative; grad: relative L2 of the whole gradient / of the worst tensor; field: worst of d, v_y, v_x):
  grid    (B, ms)   loss     per-step  grad     worst tensor  field    wall time of the test
  128x64  (1, 1)    2.7e-07  2.7e-07   3.1e-07  3.5e-07       7.9e-07   0.9 s
  128x64  (4, 2)    2.9e-07  2.6e-07   2.8e-07  3.2e-07       6.3e-07   3.5 s
  128x64  (5, 1)    2.0e-07  2.0e-07   3.8e-06  5.8e-06       9.3e-07   2.2 s
  128x64  (17, 1)   2.9e-07  2.9e-07   7.0e-07  1.8e-06       9.9e-07   5.8 s
  128x64  (41, 1)   2.7e-07  2.7e-07   2.0e-06  4.5e-06       1.0e-06  11.6 s
  64x32   (1, 1)    1.7e-07  1.7e-07   2.2e-07  2.5e-07       5.8e-07   0.1 s
  64x32   (5, 3)    4.3e-07  4.1e-07   3.8e-07  4.3e-07       4.4e-07   1.7 s
  64x32   (13, 2)   3.0e-07  3.5e-07   3.1e-06  6.5e-06       5.5e-07   2.1 s
  64x32   (33, 1)   1.6e-07  1.6e-07   3.8e-06  6.1e-06       7.7e-07   2.5 s
Bounds: 1e-5 (loss), TOL_GRAD = 1e-4 and 3e-4 (gradient), TOL_FIELD = 1e-5 (fields).  The gradient of (5, 1), (41, 1), (13, 2) and
(33, 1) is ten times further from the oracle than that of (1, 1) and (4, 2) -- worst tensors: a bias (numbers 11, 13) or a weight of
the early layers (2, 10), each a float32 sum over every pixel of the batch -- and still 25 times inside the bound.  The wall time is almost all the float64
oracle on the CPU, computed once per session and case; (41, 1) is the one case beyond a few seconds, kept because no smaller
batch is refused by the band launch."""
import pytest
import torch

from sol_amd import _lib
from test_gpu_parity import TOL_FIELD, TOL_GRAD, _cached, _oracle_problem, _trainer_from, f32, rel

pytestmark = pytest.mark.gpu

DX3, DX1 = "k_conv5x5_dx<3, 2>", "k_conv5x5_dx<1, 1, true>"
T3, THIN_IN = "k_conv5x5_t3", "k_conv5x5<4, 2>"


def _names(p):
    return {k.strip("()"): v[0] for k, v in p.kernels.items()}


def _ran(names, prefix):
    return sum(c for k, c in names.items() if k == prefix or k.startswith(prefix + "<"))


def k_128_b1_ms1(n, B, ms):
    # jobs-only launch: ONE k_karman_bwd_bww (with ms >= 2 there are ms, ms - 1 of them with solver workgroups), no adjoint kernel
    assert _ran(n, "k_karman_bwd_bww") == 1 and _ran(n, "k_karman_bwd") == 0, n
    assert _ran(n, "k_density_step") == 1 and _ran(n, "k_density_chain") == 0 and _ran(n, "k_karman_fwd_dens") == 0, n
    assert n.get(DX1, 0) > 0 and DX3 not in n, n


def k_128_b4_ms2(n, B, ms):
    assert n.get(DX3) == 10 * ms + 10 * ms and DX1 not in n, n            # every 32 -> 32 launch, forward and backward-data
    assert _ran(n, "k_karman_fwd_bands") == ms and _ran(n, "k_density_step") == 1, n


def k_128_b5_ms1(n, B, ms):
    assert n.get(DX3) == 20 * ms and DX1 not in n, n
    assert _ran(n, "k_karman_fwd_bands") == ms, n


def k_128_b17_ms1(n, B, ms):
    assert _ran(n, "k_karman_fwd_bands") == ms, n
    assert n.get(THIN_IN, 0) > 0 and _ran(n, T3) == 0, n


def k_128_b41_ms1(n, B, ms):
    assert _lib.get_option("fwd_bands") == 1 and _ran(n, "k_karman_fwd_bands") == 0, n
    assert n.get(THIN_IN, 0) > 0 and _ran(n, T3) == 0, n


def k_64_b1_ms1(n, B, ms):
    assert n.get("k_karman_bwd_bww_small") == ms and "k_density_chain" not in n and "k_density_step" not in n and "k_correct_loss" not in n, n
    assert not any(k.startswith("k_transpose_cells") for k in n), n
    assert n.get(DX1, 0) > 0 and DX3 not in n, n


def k_64_b5_ms3(n, B, ms):
    assert n.get("k_karman_bwd_bww_small") == ms and "k_density_chain" not in n, n
    assert n.get(DX1) == 20 * ms and DX3 not in n, n


def k_64_b13_ms2(n, B, ms):
    assert n.get("k_karman_bwd_bww_small") == ms and "k_density_chain" not in n, n
    assert n.get(DX3) == 20 * ms and DX1 not in n, n


def k_64_b33_ms1(n, B, ms):
    assert n.get("k_karman_bwd_bww_small") == ms, n
    assert n.get(THIN_IN, 0) > 0 and _ran(n, T3) == 0, n


CASES = [(128, 64, 1, 1, k_128_b1_ms1), (128, 64, 4, 2, k_128_b4_ms2), (128, 64, 5, 1, k_128_b5_ms1), (128, 64, 17, 1, k_128_b17_ms1),
         (128, 64, 41, 1, k_128_b41_ms1),
         (64, 32, 1, 1, k_64_b1_ms1), (64, 32, 5, 3, k_64_b5_ms3), (64, 32, 13, 2, k_64_b13_ms2), (64, 32, 33, 1, k_64_b33_ms1)]


@pytest.mark.parametrize("Y,X,B,ms,kernels", CASES, ids=["%dx%d-B%d-ms%d" % c[:4] for c in CASES])
def test_train_step_against_oracle_where_the_launches_change_with_the_batch(Y, X, B, ms, kernels):
    g, d, vy, vx, re, gts, params, std_v, loss, losses, (rd, ry, rx) = _cached(
        ("regime", B, Y, X, ms), lambda: _oracle_problem(B, Y, X, ms, with_states=True))
    net, tr = _trainer_from(params, g, B, Y, X, ms, std_v)
    assert tr.masks.direct is not None
    args = (f32(d), f32(vy), f32(vx), f32(re), f32(torch.stack([s[1] for s in gts])), f32(torch.stack([s[2] for s in gts])))
    hl = tr.fwd_bwd(*args, want_final=True)
    gref = torch.cat([p.grad.reshape(-1) for p in params])
    off = net.offsets
    per_tensor = [rel(tr.grads[off[k]:off[k + 1]], params[k].grad.reshape(-1)) for k in range(len(params))]
    e_loss = abs(float(hl) - float(loss.detach())) / abs(float(loss.detach()))
    e_steps = max(abs(float(a) - b) / abs(b) for a, b in zip(tr.loss_steps.cpu(), losses))
    e_grad, e_field = rel(tr.grads, gref), max(rel(tr.final[0], rd), rel(tr.final[1], ry), rel(tr.final[2], rx))
    print("regime %dx%d B %d ms %d: loss %.1e, per-step loss %.1e, grad %.1e (worst tensor %.1e, number %d), field %.1e" % (
        Y, X, B, ms, e_loss, e_steps, e_grad, max(per_tensor), per_tensor.index(max(per_tensor)), e_field))
    assert e_loss < 1e-5 and e_steps < 1e-5, (e_loss, e_steps)
    assert e_grad < TOL_GRAD, e_grad
    assert max(per_tensor) < 3 * TOL_GRAD, per_tensor
    assert rel(tr.final[0], rd) < TOL_FIELD and rel(tr.final[1], ry) < TOL_FIELD and rel(tr.final[2], rx) < TOL_FIELD
    assert int(tr.iters_fwd.max()) == 0 and int(tr.iters_bwd.max()) == 0          # direct solver: no CG iterations
    first = [tr.grads.clone(), tr.loss_steps.clone()] + [t.clone() for t in tr.final]
    tr.fwd_bwd(*args, want_final=True)
    for a, b in zip(first, [tr.grads, tr.loss_steps] + list(tr.final)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "a second call returns other bits"
    with _lib.profile() as p:
        tr.fwd_bwd(*args, want_final=True, eager=True)
    kernels(_names(p), B, ms)
