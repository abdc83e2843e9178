"""Hand-written forward pass and reverse sweep of the 2-D correction networks over the C ABI.

`model_mars_moon` (/root/reference/karman-2d/karman_train.py:101-138) and `model_mercury` (:92-99) differentiated by hand, layer by
layer, exactly as csrc/train.hip does it for the fused C++ trainer and karman3d._MarsMoon3DFn for the 3-D network -- for the
trainers that are composed in Python (trainer.GraphTrainer: model_mercury and any network on the karman scene, burgers.BurgersTrainer):

  * the weights are packed ONCE per training step (forward and backward-data form of every layer), not once per convolution call;
  * a backward-data launch applies the skip gradient and LeakyReLU'(saved activation) in its epilogue (SOL_EPI_DLRELU): no
    compare / where / multiply / add kernels between the launches;
  * every layer's weight gradient is ACCUMULATED over the unrolled steps in that layer's partial buffer (sol_conv5x5_bwd_weight adds
    into `partial`) and reduced once per step (sol_conv5x5_bwd_weight_reduce);
  * on 64-pixel rows the 32-channel layers run the fp16 three-product kernels, each producer publishing the absmax slots its
    consumer scales by (sol_conv5x5_scaled) -- no pass over a tensor just to find its maximum.

No autograd graph is built; the torch operations left between the launches are allocations, zero fills and concatenations (kernels).
The autograd compositions (model.MarsMoon.__call__, model.Mercury.__call__ over ops.Conv5x5Fn) stay as the cross-check.
"""
import ctypes as C

import torch

from . import _lib, ops
from ._lib import check, ptr, stream


class _Unit:
    """one convolution of the network: its kernel w [5,5,cin,cout] and bias (views of the flat parameter buffer, or persistent copies of
    the halves model_mercury splits a kernel into), its packed forms and its slice of the weight-gradient partial buffer"""
    __slots__ = ("cin", "cout", "cin_k", "w", "b", "pf", "pb", "part", "ws", "dw", "db", "src")


def _ptr_array(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _int_array(vals):
    return (C.c_int32 * len(vals))(*[int(v) for v in vals])


def row_pitch(H, W):
    """Pixels per row of the buffers an [H, W] image runs in: W itself for the shapes the convolutions take as they are (check_shape of
    csrc/conv5x5.hip: W >= 4 divides 64 with H % (64 / W) == 0, or W is a multiple of 64), else the next multiple of 64 -- the pitched
    layout of NetSchedule2D(any_width=True) / sol_conv5x5_cols."""
    H, W = int(H), int(W)
    if W >= 4 and (W % 64 == 0 or (W <= 64 and 64 % W == 0 and H % (64 // W) == 0)):
        return W
    return 64 * ((W + 63) // 64)


class NetSchedule2D:
    def __init__(self, net, B, H, W, train=True, any_width=False, padding="zeros", periodic=(False, False)):
        """train=False (a roll-out: forward only): no weight-gradient partial buffers, no backward-data packs, and the absmax slots of the
        forward are persistent buffers cleared by one library launch per call (no torch fill between the launches).

        any_width=True: a width the convolutions refuse (row_pitch(H, W) != W) runs in PITCHED rows -- every activation, absmax slot set
        and dz is a [B,H,P,c] buffer with P = row_pitch(H, W) whose columns >= W are zero.  The input is copied into the valid columns of
        a zero-initialised [B,H,P,4] buffer, every convolution is sol_conv5x5_cols (the 64-pixel-tile kernels with a column-masked
        epilogue: the pad columns of every output are written as zeros, so the next layer reads them as its SAME padding), and the
        weight gradient is the unchanged sol_conv5x5_bwd_weight at the pitch (zero pad columns of x and dz add exact zeros to dw / db).
        forward / backward take and return DENSE [B,H,W,c] tensors.  With any_width=False nothing changes.

        padding="circular", periodic=(py, px): the convolutions pad CIRCULARLY along the periodic axes (include/sol_hip.h, "CIRCULAR
        PADDING").  Whatever any_width says, the network runs in HALO buffers [B, H + 4 py, P, c], P = 64 * ceil((W + 4 px) / 64): the
        valid pixels at rows [2 py, 2 py + H) and columns [2 px, 2 px + W), two halo rows / columns on either side of a periodic axis,
        zero pad columns beyond.  Every convolution is sol_conv5x5_cols at the pitch with WV = W + 4 px; what it writes into the halo
        (computed with zeros beyond the buffer edge) is wrong and is replaced by one sol_conv_halo launch: `wrap` on every activation
        and on a dz before its backward-data convolution, `zero` on a dz before its weight gradient (x wrapped, dz zero in the halo:
        dw and db sum over the valid pixels only).  padding="zeros" (the default): nothing changes."""
        if padding not in ("zeros", "circular"):
            raise _lib.SolError("NetSchedule2D: padding must be 'zeros' or 'circular' (got %r)" % (padding,))
        py, px = (bool(periodic[0]), bool(periodic[1]))
        self.circular = padding == "circular"
        if self.circular and not (py or px):
            raise _lib.SolError("NetSchedule2D: padding='circular' needs a periodic axis (periodic=%r)" % (tuple(periodic),))
        if net.name not in ("mars_moon", "mercury"):
            raise _lib.SolError("NetSchedule2D: no hand-written schedule for network %r" % net.name)
        _lib.require_gpu()
        self.lib = lib = _lib.load()
        self.net, self.B, self.H, self.W = net, int(B), int(H), int(W)
        self.P = row_pitch(H, W) if any_width else self.W      # pixels per buffer row
        self.pitched = self.P != self.W
        self.HB, self.WV, self.r0, self.c0, self.halo_bits = self.H, self.W, 0, 0, 0     # buffer rows, data pixels per row, where the image sits
        if self.circular:
            self.r0, self.c0, self.halo_bits = 2 * py, 2 * px, 2 * py + 4 * px
            self.HB, self.WV = self.H + 2 * self.r0, self.W + 2 * self.c0
            self.P, self.pitched = 64 * ((self.WV + 63) // 64), True
        self.scaled = self.P % 64 == 0               # 64-pixel rows: the split-precision kernels + absmax hand-over
        self.train = bool(train)
        if net.cin > 4:
            raise _lib.SolError("NetSchedule2D: at most 4 input channels (got %d)" % net.cin)
        if net.cout != 2:
            raise _lib.SolError("NetSchedule2D: the weight-gradient kernels take 2 or 32 output channels (network output: %d)" % net.cout)
        mm = net.name == "mars_moon"
        dims = [(net.cin, 32)] + [(32, 32)] * 10 + [(32, net.cout)] if mm else [(net.cin, 32), (32, 32), (32, 32), (32, net.cout), (32, net.cout)]
        dev = net.params.device
        f = lambda n: torch.empty(int(n), dtype=torch.float32, device=dev)
        self.units = []
        total = 0
        for cin, cout in dims:
            u = _Unit()
            u.cin, u.cout, u.cin_k = cin, cout, (4 if cin <= 4 else 32)
            u.ws = int(lib.sol_conv5x5_bwd_weight_ws_floats(self.B, self.HB, self.P, u.cin_k, cout)) if self.train else 0
            total += (u.ws + 3) // 4 * 4
            u.pf = f(lib.sol_conv5x5_packed_floats(cin, cout, ops.CONV_FWD))
            u.pb = f(lib.sol_conv5x5_packed_floats(cout, cin, ops.CONV_BWD_DATA)) if self.train else None
            self.units.append(u)
        self._partials = f(total)
        off = 0
        for u in self.units:
            u.part = self._partials[off:off + u.ws]
            off += (u.ws + 3) // 4 * 4
        self._zero_bias = torch.zeros(net.cout, dtype=torch.float32, device=dev)
        if self.pitched:
            # the dense input / output gradient land in the valid columns of these; nothing ever writes their pad columns or spare channels
            self._xin = torch.zeros(self.B, self.HB, self.P, 4, dtype=torch.float32, device=dev)
            self._gin = torch.zeros(self.B, self.HB, self.P, 4, dtype=torch.float32, device=dev) if self.train else None
        # kernels / biases: views of the flat parameter buffer (updated in place by Adam: the addresses are stable), or persistent copies of the
        # halves of model_mercury's 32 -> 64 / 64 -> 2 kernels (refreshed by begin_step)
        p = [t.detach() for t in net.tensors()]
        self.flat = f(net.n_params)                   # the step's gradient, Keras get_weights() order
        g = [t for t in self.net.tensors(self.flat)]
        if mm:
            for l, u in enumerate(self.units):
                u.w, u.b, u.src = p[2 * l], p[2 * l + 1], None
                u.dw, u.db = g[2 * l], g[2 * l + 1]    # the reduction writes straight into the flat gradient
        else:
            U = self.units
            U[0].w, U[0].b, U[0].src = p[0], p[1], None
            U[0].dw, U[0].db = g[0], g[1]
            for u, src, b in ((U[1], p[2][..., :32], p[3][:32]), (U[2], p[2][..., 32:], p[3][32:]), (U[3], p[4][:, :, :32], p[5]), (U[4], p[4][:, :, 32:], self._zero_bias)):
                u.src, u.w, u.b = src, torch.empty(src.shape, dtype=torch.float32, device=dev), b
                u.dw, u.db = torch.empty(src.shape, dtype=torch.float32, device=dev), f(u.cout)
        n = len(self.units)
        if not self.train:
            self._fwd_slots = torch.zeros(11 if mm else 3, ops.AMAX_SLOTS, dtype=torch.int32, device=dev) if self.scaled else None
            self._pack_args = (n, _ptr_array([u.w for u in self.units]), _int_array([u.cin for u in self.units]), _int_array([u.cout for u in self.units]),
                               _int_array([ops.CONV_FWD] * n), _ptr_array([u.pf for u in self.units]))
            return
        self._pack_args = (2 * n, _ptr_array([u.w for u in self.units] * 2), _int_array([u.cin for u in self.units] + [u.cout for u in self.units]),
                           _int_array([u.cout for u in self.units] + [u.cin for u in self.units]), _int_array([ops.CONV_FWD] * n + [ops.CONV_BWD_DATA] * n),
                           _ptr_array([u.pf for u in self.units] + [u.pb for u in self.units]))
        self._reduce_args = (n, _ptr_array([u.part for u in self.units]), _ptr_array([u.dw for u in self.units]), _ptr_array([u.db for u in self.units]),
                             self.B, self.HB, self.P, _int_array([u.cin for u in self.units]), _int_array([u.cout for u in self.units]), 0)

    # ---- once per training step -------------------------------------------------------------------------------------------
    def begin_step(self):
        """pack every layer's weights (forward + backward-data form) from the CURRENT parameters -- ONE launch (sol_conv5x5_pack_jobs) -- and
        clear the weight-gradient partials (one launch)"""
        for u in self.units:
            if u.src is not None:
                u.w.copy_(u.src)                      # (strided halves of a mercury kernel: an elementwise copy kernel)
        check(self.lib.sol_conv5x5_pack_jobs(stream(), *self._pack_args))
        if self.train:
            check(self.lib.sol_copy_words(stream(), ptr(self._partials), None, self._partials.numel()))

    # ---- launches -----------------------------------------------------------------------------------------------------------
    def _conv(self, x, packed, bias, residual, act_ref, cout, epi, xmax, ymax):
        B, H, W, cin = x.shape
        y = torch.empty(B, H, W, cout, dtype=torch.float32, device=x.device)
        sl = float(self.net.slope)
        if self.pitched:
            check(self.lib.sol_conv5x5_cols(stream(), ptr(x), ptr(packed), ptr(bias), ptr(residual), ptr(act_ref), ptr(y),
                                            B, H, W, self.WV, cin, cout, epi, sl, ptr(xmax), ptr(ymax)))
        elif self.scaled:
            check(self.lib.sol_conv5x5_scaled(stream(), ptr(x), ptr(packed), ptr(bias), ptr(residual), ptr(act_ref), ptr(y),
                                              B, H, W, cin, cout, epi, sl, ptr(xmax), ptr(ymax)))
        else:
            check(self.lib.sol_conv5x5(stream(), ptr(x), ptr(packed), ptr(bias), ptr(residual), ptr(act_ref), ptr(y),
                                       B, H, W, cin, cout, epi, sl))
        return y

    def _bww(self, u, xk, dz):
        """u.part += the weight-gradient partial sums of this step"""
        check(self.lib.sol_conv5x5_bwd_weight(stream(), ptr(xk), ptr(dz), ptr(u.part), self.B, self.HB, self.P, u.cin_k, u.cout))

    def _slots(self, n, dev):
        if not self.train and self.scaled:          # forward only: the persistent slots, cleared by a library launch
            check(self.lib.sol_copy_words(stream(), ptr(self._fwd_slots), None, self._fwd_slots.numel()))
            return self._fwd_slots
        return torch.zeros(n, ops.AMAX_SLOTS, dtype=torch.int32, device=dev) if self.scaled else [None] * n

    # ---- pitched rows: dense <-> pitched copies (kernels: _lib.dcopy_ is a strided copy_ or sol_copy_words, never a memcpy node) ----
    def _pad_in(self, buf, x):
        """the valid pixels of buf = x [B,H,W,c]; the pad columns and the spare channels of buf stay zero (the halo of a circular buffer
        is the caller's: _wrap / _zero_halo)"""
        _lib.dcopy_(buf[:, self.r0:self.r0 + self.H, self.c0:self.c0 + self.W, :x.shape[-1]], x)
        return buf

    def _crop(self, y):
        """dense [B,H,W,c] copy of the valid pixels of y [B,HB,P,c]"""
        return _lib.dcopy_(torch.empty(self.B, self.H, self.W, y.shape[-1], dtype=torch.float32, device=y.device),
                           y[:, self.r0:self.r0 + self.H, self.c0:self.c0 + self.W])

    # ---- circular padding: the halo of a buffer, refreshed in place by one launch (nothing is launched with padding="zeros") ----
    # The absmax slots a producer publishes include its wrong halo outputs.  They remain upper bounds of what the consumer reads: a
    # refreshed halo holds copies of valid values (or zeros), all of which the slots cover, and an over-reported maximum costs fp16 range
    # only (include/sol_hip.h, sol_conv5x5_bwd_weight_segments).
    def _halo(self, buf, mode):
        if self.circular:
            check(self.lib.sol_conv_halo(stream(), ptr(buf), self.B, self.H, self.W, self.P, buf.shape[-1], self.halo_bits, mode))
        return buf

    def _wrap(self, buf):
        """halo := the valid pixels at the wrapped index (an activation; a dz before its backward-data convolution)"""
        return self._halo(buf, 0)

    def _zero_halo(self, buf):
        """halo := 0 (a dz before its weight gradient: only valid pixels contribute)"""
        return self._halo(buf, 1)

    # ---- forward ------------------------------------------------------------------------------------------------------------
    def forward(self, x):
        """x [B,H,W,cin] -> (out [B,H,W,cout], state for backward)"""
        if self.pitched:
            xk = self._wrap(self._pad_in(self._xin, _lib.f32(x.detach())))
            if self.train:
                xk = _lib.dclone(xk)                  # the reverse sweep reads this step's input after later steps have overwritten the buffer
        else:
            xk = ops._pad_channels(_lib.f32(x.detach()), 4)
        U, L, N, Wr = self.units, ops.EPI_LRELU, ops.EPI_NONE, self._wrap
        if self.net.name == "mars_moon":
            am = self._slots(11, xk.device)
            acts = [Wr(self._conv(xk, U[0].pf, U[0].b, None, None, 32, L, None, am[0]))]
            for k in range(5):
                a = Wr(self._conv(acts[-1], U[1 + 2 * k].pf, U[1 + 2 * k].b, None, None, 32, L, am[2 * k], am[2 * k + 1]))
                acts.append(a)
                acts.append(Wr(self._conv(a, U[2 + 2 * k].pf, U[2 + 2 * k].b, acts[-2], None, 32, L, am[2 * k + 1], am[2 * k + 2])))
            out = self._conv(acts[-1], U[11].pf, U[11].b, None, None, self.net.cout, N, am[10], None)
        else:
            am = self._slots(3, xk.device)
            h = Wr(self._conv(xk, U[0].pf, U[0].b, None, None, 32, L, None, am[0]))
            ha = Wr(self._conv(h, U[1].pf, U[1].b, None, None, 32, L, am[0], am[1]))
            hb = Wr(self._conv(h, U[2].pf, U[2].b, None, None, 32, L, am[0], am[2]))
            oa = self._conv(ha, U[3].pf, U[3].b, None, None, self.net.cout, N, am[1], None)
            out = self._conv(hb, U[4].pf, U[4].b, oa, None, self.net.cout, N, am[2], None)
            acts = [h, ha, hb]
        if self.pitched:
            out = self._crop(out)
        return out, (xk, am, acts)

    # ---- reverse sweep ------------------------------------------------------------------------------------------------------
    def backward(self, state, g_out):
        """d loss / d x [B,H,W,cin] for the output gradient g_out [B,H,W,cout]; the weight gradients of this call are added to the layers'
        partial buffers (end_step reduces them).  padding="circular", per layer: the dz a convolution hands over has wrong halo values ->
        zero its halo -> the weight gradient -> wrap it -> the backward-data convolution (the adjoint of a circular convolution is the
        circular correlation); Z / Wr launch nothing with padding="zeros"."""
        if not self.train:
            raise _lib.SolError("NetSchedule2D(train=False) runs the forward pass only")
        xk, am, acts = state
        U, D, N, Z, Wr = self.units, ops.EPI_DLRELU, ops.EPI_NONE, self._zero_halo, self._wrap
        g = _lib.f32(g_out).contiguous()
        if self.pitched:
            g4 = Z(self._pad_in(self._gin, g))        # (the previous call left its wrapped halo in the buffer)
            g = g4[..., :g.shape[-1]].contiguous()    # [B,H,P,cout], zero pad columns: the last layer's dz
        else:
            g4 = ops._pad_channels(g, 4)
        if self.net.name == "mars_moon":
            zm = self._slots(11, xk.device)
            self._bww(U[11], acts[10], g)
            dz = self._conv(Wr(g4), U[11].pb, None, None, acts[10], 32, D, None, zm[10])
            for k in range(4, -1, -1):
                a, hprev = acts[1 + 2 * k], acts[2 * k]
                self._bww(U[2 + 2 * k], a, Z(dz))
                dz1 = self._conv(Wr(dz), U[2 + 2 * k].pb, None, None, a, 32, D, zm[2 * k + 2], zm[2 * k + 1])
                self._bww(U[1 + 2 * k], hprev, Z(dz1))
                dz = self._conv(Wr(dz1), U[1 + 2 * k].pb, None, dz, hprev, 32, D, zm[2 * k + 1], zm[2 * k])
            self._bww(U[0], xk, Z(dz))
            dx = self._conv(Wr(dz), U[0].pb, None, None, None, U[0].cin, N, zm[0], None)
            return self._crop(dx) if self.pitched else dx
        h, ha, hb = acts
        zm = self._slots(3, xk.device)
        self._bww(U[3], ha, g)
        self._bww(U[4], hb, g)
        dha = self._conv(Wr(g4), U[3].pb, None, None, ha, 32, D, None, zm[1])
        dhb = self._conv(g4, U[4].pb, None, None, hb, 32, D, None, zm[2])
        self._bww(U[1], h, Z(dha))
        self._bww(U[2], h, Z(dhb))
        t = self._conv(Wr(dha), U[1].pb, None, None, None, 32, N, zm[1], None)
        dh = self._conv(Wr(dhb), U[2].pb, None, t, h, 32, D, zm[2], zm[0])
        self._bww(U[0], xk, Z(dh))
        dx = self._conv(Wr(dh), U[0].pb, None, None, None, U[0].cin, N, zm[0], None)
        return self._crop(dx) if self.pitched else dx

    # ---- once per training step ---------------------------------------------------------------------------------------------
    def end_step(self):
        """reduce every layer's partial sums (sol_conv5x5_bwd_weight_reduce_jobs: two launches for all layers); returns the flat gradient in
        Keras get_weights() order (self.flat: model_mars_moon's layers reduce straight into it)"""
        if not self.train:
            raise _lib.SolError("NetSchedule2D(train=False) runs the forward pass only")
        check(self.lib.sol_conv5x5_bwd_weight_reduce_jobs(stream(), *self._reduce_args))
        if self.net.name == "mercury":
            # kernel 2 is [5,5,32,64] = the two output halves side by side, kernel 4 is [5,5,64,2] = the two input halves stacked;
            # the output bias receives its gradient once (both last-layer halves see the same dz)
            U = self.units
            g = self.net.tensors(self.flat)
            g[2][..., :32].copy_(U[1].dw)
            g[2][..., 32:].copy_(U[2].dw)
            _lib.dcopy_(g[3][:32], U[1].db)          # (contiguous pieces: kernel copies -- a contiguous copy_ is a memcpy node, refused under capture)
            _lib.dcopy_(g[3][32:], U[2].db)
            g[4][:, :, :32].copy_(U[3].dw)
            g[4][:, :, 32:].copy_(U[4].dw)
            _lib.dcopy_(g[5], U[3].db)
        return self.flat
