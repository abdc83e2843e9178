"""Hand-written forward pass and reverse sweep of the 3-D correction network over the C ABI: the 3-D twin of schedule2d.NetSchedule2D.

`model_mars_moon` (karman_train.py:101-138) with Conv3D(5) layers, differentiated by hand.  A NetSchedule3D is the ONLY place that knows how
karman3d.MarsMoon3D is launched at one shape [B,Y,X,Z]; the autograd node, `MarsMoon3D.__call__` / `.activations` and both schedules of
Karman3DTrainer run the net's schedule of that shape (`MarsMoon3D.schedule`), Karman3DRollout owns a forward-only one (train=False):

  * the weights are packed into persistent buffers by begin_step() -- per layer the forward and (train) the backward-data form, and the
    depth-packed forms of the two thin layers (4 -> 32 and 32 -> cout <= 4) --, again whenever the net's `params_key()` has moved;
  * forward: twelve launches, every layer handing the absmax slots it published to its consumer (no pass over a tensor just to find
    its maximum);
  * reverse sweep: per layer the weight gradient, ACCUMULATED over the calls of an unrolled sweep in that layer's partial buffers (held
    here) and reduced with the last call, and ONE data-gradient launch whose epilogue adds the skip gradient of the residual block and
    multiplies by LeakyReLU'(saved activation) (SOL_EPI_DLRELU).

Which kernel a launch runs (one-launch or five-pass Conv3D, depth-packed or plain weight gradient) is a matter of its shape alone.

padding="circular" (a z-periodic scene; include/sol_hip.h, "CIRCULAR PADDING, KARMAN-3D"): the same launches on the TRANSPOSED volume
[B, Y, HB, X, C] -- depth y, image rows z with a two-row circular halo on either side (HB = karman3d.circular_rows3d(X, Z) rows), pixels x --
with every layer's kernel axes 1 and 2 swapped.  The public contract stays [B,Y,X,Z,.] on both ends: sol_conv3d_circ_pack on entry,
sol_conv3d_circ_unpack on exit, sol_conv3d_halo between the launches (wrap on every activation and before a backward-data convolution,
zero before a weight gradient), the weight gradients swapped back before they enter the flat gradient.  The kernel that runs is then a
matter of the buffer shape (B, Y, HB, X).  A published absmax also covers what a launch wrote into halo and pad rows before the refresh:
an upper bound of the true maximum.
"""
import torch

from . import _lib
from ._lib import check, ptr, stream
from .karman3d import (_pack3d, _pack3d_thin, _pack3d_thin_out, _pad_ch, conv3d, conv3d_bwd_weight, conv3d_thin, conv3d_thin_bwd_weight,
                       conv3d_thin_out, circular_rows3d, net3d_circular_shape_reason, net3d_shape_reason)


class _Unit:
    """one convolution of the network: kernel w [5,5,5,cin,cout] and bias b (views of the flat parameter buffer, refreshed by begin_step), the
    packed forms pf (forward; cin_k = 4 / 32 input channels run) and pb (backward-data), and for a thin layer the depth-packed forms: `thin`
    = sol_conv3d_thin's (the first layer's forward, the output layer's data gradient), `thin_out` = sol_conv3d_thin_out's (the other two)"""
    __slots__ = ("cin", "cout", "cin_k", "w", "b", "pf", "pb", "thin", "thin_out")


class NetSchedule3D:
    def __init__(self, net, B, Y, X, Z, train=True, padding="zeros"):
        """padding: "zeros" (Conv3D's padding='same') or "circular" along z (the module docstring).
        train=False (a roll-out: forward only): no backward-data packs, no weight-gradient state, and forward() runs in persistent
        buffers -- three rotating 32-channel tensors, the output, the absmax slots and one thin-layer workspace."""
        if padding not in ("zeros", "circular"):
            raise _lib.SolError("NetSchedule3D: padding must be 'zeros' or 'circular' (got %r)" % (padding,))
        self.padding, self.circ = padding, padding == "circular"
        why = (net3d_circular_shape_reason if self.circ else net3d_shape_reason)(Y, X, Z, train)          # before anything is allocated or launched
        if why is not None:
            raise _lib.SolError("NetSchedule3D(%s%s) at %d x %d x %d: %s" % ("train=True" if train else "train=False",
                                                                            ", padding='circular'" if self.circ else "", Y, X, Z, why))
        _lib.require_gpu()
        lib = _lib.load()
        if self.circ and net.cout not in (3, 4):
            raise _lib.SolError("NetSchedule3D(padding='circular'): 3 or 4 output channels (got %d)" % net.cout)
        if net.cin > 4 or not net.params.is_cuda:
            raise _lib.SolError("NetSchedule3D: at most 4 input channels (got %d) and parameters on the GPU (on %s)" % (net.cin, net.params.device))
        self.net, self.shape, self.train = net, (int(B), int(Y), int(X), int(Z)), bool(train)
        # the shape the kernels run at: circular = the transposed halo buffer (B, Y, HB, X)
        self.kshape = (int(B), int(Y), circular_rows3d(X, Z), int(X)) if self.circ else self.shape
        self.lib = lib
        dev = net.params.device
        f = lambda *n: torch.empty(*[int(v) for v in n], dtype=torch.float32, device=dev)
        self.units = []
        for l in range(12):
            u = _Unit()
            u.cin, u.cout, u.cin_k = net.chans[l], net.chans[l + 1], (4 if net.chans[l] <= 4 else 32)
            u.pf = f(lib.sol_conv3d_packed_floats(u.cin_k, u.cout))
            u.pb = f(lib.sol_conv3d_packed_floats(u.cout, u.cin)) if self.train else None
            u.thin = u.thin_out = None
            self.units.append(u)
        first, last = self.units[0], self.units[11]
        first.thin = f(lib.sol_conv3d_thin_packed_floats())
        first.thin_out = f(lib.sol_conv3d_thin_packed_floats()) if self.train else None
        if net.cout <= 4:
            last.thin_out = f(lib.sol_conv3d_thin_packed_floats())
            last.thin = f(lib.sol_conv3d_thin_packed_floats()) if self.train else None
        self._key = None                             # net.params_key() of the packed weights
        if self.train:
            # per layer: the weight-gradient partials of a reverse sweep (the acc state of conv3d_bwd_weight, which sizes and fills it on the
            # first sweep and checks every later call against it)
            self.wstate = [dict() for _ in range(12)]
        else:
            self.h = [f(*self.kshape, 32) for _ in range(3)]          # block input / intermediate / block output, rotated
            self.out = f(B, Y, X, Z, net.cout)
            self.amax = torch.zeros(12, 256, dtype=torch.int32, device=dev)      # absmax slots of the 32-channel activations
            self.ws = f(lib.sol_conv3d_thin_ws_floats(*self.kshape))
            if self.circ:                                # the packed features and the output in the buffer layout
                self.xk, self.out_k = f(*self.kshape, 4), f(*self.kshape, net.cout)

    # ---- once per training step, and whenever the parameters moved ---------------------------------------------------------
    def begin_step(self):
        """pack every layer from the CURRENT parameters: per layer the forward and (train) backward-data form, then the depth-packed forms of
        the two thin layers -- for the convolution that is RUN (the first layer's forward is the output layer's data gradient in shape)"""
        net = self.net
        p = [t.detach() for t in net.tensors()]
        for l, u in enumerate(self.units):
            u.w, u.b = p[2 * l], p[2 * l + 1]
            if self.circ:                                # kernel axes 1 and 2 swapped: a permuted copy (a kernel, never a memcpy node)
                u.w = u.w.permute(0, 2, 1, 3, 4).contiguous()
            wf = u.w if u.cin_k == u.cin else torch.nn.functional.pad(u.w, (0, 0, 0, u.cin_k - u.cin))   # the forward kernels read cin_k input channels
            _pack3d(wf, u.cin_k, u.cout, 0, out=u.pf)
            if self.train:
                _pack3d(u.w, u.cout, u.cin, 1, out=u.pb)
        first, last = self.units[0], self.units[11]
        _pack3d_thin(first.w, net.cin, 0, out=first.thin)
        if last.thin is not None:
            _pack3d_thin(last.w, net.cout, 1, out=last.thin)
        if last.thin_out is not None:
            _pack3d_thin_out(last.w, net.cout, 0, out=last.thin_out)
        if first.thin_out is not None:
            _pack3d_thin_out(first.w, net.cin, 1, out=first.thin_out)
        self._key = net.params_key()

    def _fresh(self):
        if self._key != self.net.params_key():
            self.begin_step()

    def layer_packs(self):
        """per layer (forward-packed, backward-data-packed) weights, for the per-layer composition (karman3d.conv3d_fn)"""
        self._fresh()
        return [(u.pf, u.pb) for u in self.units]

    # ---- the halo buffers of padding="circular" ------------------------------------------------------------------------------
    def _pack(self, t4, mode, out=None):
        """t4 [B,Y,X,Z,4] -> [B,Y,HB,X,4], halo rows wrapped (mode 0) or zero (mode 1)"""
        (B, Y, X, Z), HB = self.shape, self.kshape[2]
        dst = out if out is not None else torch.empty(B, Y, HB, X, 4, dtype=torch.float32, device=t4.device)
        check(self.lib.sol_conv3d_circ_pack(stream(), ptr(t4), ptr(dst), B, Y, X, Z, HB, 4, mode))
        return dst

    def _unpack(self, t, out=None):
        """t [B,Y,HB,X,C] -> [B,Y,X,Z,C], C = 3 or 4"""
        (B, Y, X, Z), HB, c = self.shape, self.kshape[2], t.shape[-1]
        dst = out if out is not None else torch.empty(B, Y, X, Z, c, dtype=torch.float32, device=t.device)
        check(self.lib.sol_conv3d_circ_unpack(stream(), ptr(t), ptr(dst), B, Y, X, Z, HB, c))
        return dst

    def _halo(self, t, mode):
        """padding="circular": refresh the halo and pad rows of t in place (0 = wrap, 1 = zero); "zeros": nothing"""
        if self.circ:
            (B, Y, X, Z), HB = self.shape, self.kshape[2]
            check(self.lib.sol_conv3d_halo(stream(), ptr(t), B * Y, Z, HB, X, t.shape[-1], mode))
        return t

    # ---- forward ------------------------------------------------------------------------------------------------------------
    def forward(self, x):
        """x [B,Y,X,Z,cin] -> (out [B,Y,X,Z,cout], state = (xk, absmax slots, the eleven 32-channel activations h0, a1, h1, ..., a5, h5)).
        train=False: out and the activations are the persistent buffers (a block's tensors are overwritten by the next block but one and by
        the next call).  padding="circular": xk and the activations are in the buffer layout [B,Y,HB,X,.], halos wrapped."""
        self._fresh()
        U, sl, cout = self.units, self.net.slope, self.net.cout
        xk = _pad_ch(_lib.f32(x.detach()), 4)
        if self.circ:
            xk = self._pack(xk, 0, out=None if self.train else self.xk)
        if self.train:
            am = torch.zeros(11, 256, dtype=torch.int32, device=xk.device)       # absmax slots of the eleven 32-channel activations
            dst, out, ws = (lambda j: None), None, None
        else:
            am, out, ws = self.amax, self.out, self.ws
            am.zero_()
            dst = lambda j: self.h[1] if j % 2 else self.h[j // 2 % 2 * 2]       # activation j: h0 and every other block output share a buffer
        halo, pub = self._halo, out
        if self.circ:
            out = None if self.train else self.out_k
        acts = [halo(conv3d_thin(xk, U[0].thin, U[0].b, True, sl, am[0], out=dst(0), ws=ws), 0)]
        for k in range(5):
            a = halo(conv3d(acts[-1], U[1 + 2 * k].pf, U[1 + 2 * k].b, None, 32, True, sl, am[2 * k], am[2 * k + 1], out=dst(2 * k + 1)), 0)
            acts.append(a)
            acts.append(halo(conv3d(a, U[2 + 2 * k].pf, U[2 + 2 * k].b, acts[-2], 32, True, sl, am[2 * k + 1], am[2 * k + 2], out=dst(2 * k + 2)), 0))
        if U[11].thin_out is not None:
            out = conv3d_thin_out(acts[-1], U[11].thin_out, U[11].b, cout, am[10], out=out, ws=ws)
        else:
            out = conv3d(acts[-1], U[11].pf, U[11].b, None, cout, False, sl, am[10], None, out=out)
        if self.circ:
            out = self._unpack(out, out=pub)
        return out, (xk, am, acts)

    # ---- reverse sweep ------------------------------------------------------------------------------------------------------
    def backward(self, state, g_out, first=True, last=True):
        """(dx [B,Y,X,Z,4 (padded input channels)], flat gradient in get_weights() order) for the output gradient g_out ([.., cout], or
        already zero padded to 4 channels).  first / last: the calls of an unrolled reverse sweep -- the weight gradients are ACCUMULATED
        inside the layers' partial buffers and reduced once, with the last call; the flat gradient is None before."""
        if not self.train:
            raise _lib.SolError("NetSchedule3D(train=False) runs the forward pass only")
        xk, amax, acts = state
        U, sl, cin, cout = self.units, self.net.slope, self.net.cin, self.net.cout
        A = lambda l: (self.wstate[l], first, last)
        w64 = self.shape[3] == 64                             # the depth-packed weight gradients take 64-pixel rows
        if self.circ:                                         # ... of the buffer: its pixel axis is x
            w64 = self.kshape[3] == 64
        halo = self._halo
        grads = [None] * 24
        zm = torch.zeros(11, 256, dtype=torch.int32, device=xk.device)         # absmax slots of the eleven pre-activation gradients
        g = _lib.f32(g_out).contiguous()
        thin = U[11].thin is not None
        if self.circ:                                         # zero halo: only valid rows enter the weight gradient
            g4, gc = self._pack(_pad_ch(g, 4), 1), None
        elif g.shape[-1] == 4 and cout != 4:
            g4, gc = g, None
        else:
            g4, gc = (_pad_ch(g, 4) if thin else None), g
        if thin and w64:
            grads[22], grads[23] = conv3d_thin_bwd_weight(g4, acts[10], cout, zmax=amax[10], acc=A(11), thin_out=True)
        else:
            gc = gc if gc is not None else g4[..., :cout].contiguous()
            grads[22], grads[23] = conv3d_bwd_weight(acts[10], gc, 32, cout, xmax=amax[10], acc=A(11))
        # d loss / d (pre-activation of the last residual block's output) = conv3d(g, flip(w11)^T) * lrelu'(h5)
        if self.circ:                                         # the adjoint of a circular convolution correlates the WRAPPED cotangent
            halo(g4, 0)
        if thin:
            dz = conv3d_thin(g4, U[11].thin, None, False, sl, zm[10], act_ref=acts[10])
        else:
            dz = conv3d(g4 if g4 is not None else _pad_ch(gc, 4), U[11].pb, None, None, 32, False, sl, None, zm[10], act_ref=acts[10])
        for k in range(4, -1, -1):
            a, hprev = acts[1 + 2 * k], acts[2 * k]
            # block k: h_k = lrelu(conv_b(a) + h_{k-1}), a = lrelu(conv_a(h_{k-1}))
            # (circular: every dz gets a zero halo before its weight gradient and a wrapped one before its backward-data convolution)
            grads[4 + 4 * k], grads[5 + 4 * k] = conv3d_bwd_weight(a, halo(dz, 1), 32, 32, xmax=amax[2 * k + 1], zmax=zm[2 * k + 2], acc=A(2 + 2 * k))
            dz1 = conv3d(halo(dz, 0), U[2 + 2 * k].pb, None, None, 32, False, sl, zm[2 * k + 2], zm[2 * k + 1], act_ref=a)
            grads[2 + 4 * k], grads[3 + 4 * k] = conv3d_bwd_weight(hprev, halo(dz1, 1), 32, 32, xmax=amax[2 * k], zmax=zm[2 * k + 1], acc=A(1 + 2 * k))
            dz = conv3d(halo(dz1, 0), U[1 + 2 * k].pb, None, dz, 32, False, sl, zm[2 * k + 1], zm[2 * k], act_ref=hprev)
        halo(dz, 1)
        if w64:
            grads[0], grads[1] = conv3d_thin_bwd_weight(xk, dz, cin, zmax=zm[0], acc=A(0))
        else:
            grads[0], grads[1] = conv3d_bwd_weight(xk, dz, cin, 32, acc=A(0))
        dx = conv3d_thin_out(halo(dz, 0), U[0].thin_out, None, 4, zm[0])      # (channels >= cin of the packed kernel are zero)
        if self.circ:
            dx = self._unpack(dx)
            if grads[0] is not None:                          # kernels came out (k_y, k_z, k_x, in, out): back to the Keras order (a permuted copy)
                grads = [t.permute(0, 2, 1, 3, 4) if t.dim() == 5 else t for t in grads]
        return dx, (None if grads[0] is None else torch.cat([t.reshape(-1) for t in grads]))
