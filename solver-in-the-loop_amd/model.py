"""Correction networks of the reference on the fp32 MFMA conv kernels.

model_mars_moon / model_mercury: /root/reference/karman-2d/karman_train.py:92-138.
Parameters live in ONE flat fp32 CUDA buffer in Keras get_weights() order
([kernel0 HWIO, bias0, kernel1, bias1, ...]); that buffer is what the fused trainer, Adam and
the RCCL all-reduce operate on.  Keras defaults are kept: glorot_uniform kernels, zero
biases, LeakyReLU(alpha=0.3).
"""
import math

import numpy as np
import torch

from . import ops


def _glorot(shape, gen):
    fan_in = shape[0] * shape[1] * shape[2]
    fan_out = shape[0] * shape[1] * shape[3]
    lim = math.sqrt(6.0 / (fan_in + fan_out))
    return (torch.rand(shape, generator=gen, dtype=torch.float64) * 2 - 1) * lim


class ConvNet:
    """Sequential description: layers = [(cin, cout, act, skip_from)]"""

    name = "net"
    layer_channels = ()
    slope = 0.3
    conv_padding = "zeros"      # what the model was trained with ("zeros" | "circular"): a record save() / load() carry, set by the training script

    def __init__(self, cin=3, cout=2, seed=0, device="cuda"):
        self.cin, self.cout = cin, cout
        self.shapes = []
        chans = self.channels(cin, cout)
        for l in range(len(chans) - 1):
            self.shapes.append((5, 5, chans[l], chans[l + 1]))
            self.shapes.append((chans[l + 1],))
        self.offsets = np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in self.shapes])]).astype(np.int64)
        gen = torch.Generator().manual_seed(seed)
        flat = torch.cat([(_glorot(s, gen) if len(s) == 4 else torch.zeros(s, dtype=torch.float64)).reshape(-1)
                          for s in self.shapes])
        self.params = flat.to(device=device, dtype=torch.float32).contiguous().requires_grad_(True)
        self.losses = []   # no regularisers (karman_train.py:439-444)

    @property
    def n_params(self):
        return int(self.offsets[-1])

    def tensors(self, flat=None):
        flat = self.params if flat is None else flat
        # (ops.split_flat: ONE autograd node whose backward assembles the flat gradient with kernel copies -- plain slices cost a
        #  memcpy node, a zero fill and an add of the whole buffer per tensor and unrolled step in a captured trainer)
        return [t.reshape(s) for t, s in zip(ops.split_flat(flat, self.offsets), self.shapes)]

    # Keras-style API used by the reference scripts
    def get_weights(self):
        return [t.detach().cpu().numpy() for t in self.tensors()]

    def set_weights(self, weights):
        flat = np.concatenate([np.asarray(w, dtype=np.float32).reshape(-1) for w in weights])
        assert flat.size == self.n_params, "weight list does not match %s" % self.name
        with torch.no_grad():
            self.params.copy_(torch.as_tensor(flat, device=self.params.device))

    def clone(self):
        """Independent copy (own parameter buffer) on the same device."""
        other = type(self)(self.cin, self.cout, 0, self.params.device)
        with torch.no_grad():
            other.params.copy_(self.params)
        other.conv_padding = self.conv_padding
        return other

    def save(self, path):
        torch.save({"name": self.name, "cin": self.cin, "cout": self.cout, "conv_padding": self.conv_padding,
                    "weights": [torch.as_tensor(w) for w in self.get_weights()]}, path)

    @classmethod
    def load(cls, path, device="cuda"):
        """`.pt` written by save(), or `.npz` holding the arrays of Keras `model.get_weights()` in order (arr_0, arr_1, ...:
        the bridge from the reference's model.h5 -- h5py is not part of this image -- is `np.savez(path, *model.get_weights())`
        on the TensorFlow side).  The architecture is recognised from the kernel shapes."""
        if str(path).endswith(".npz"):
            z = np.load(path)
            ws = [z[k] for k in sorted(z.files, key=lambda k: int(k.split("_")[-1]))]
            cin, cout = ws[0].shape[2], ws[-2].shape[3]
            name = "mercury" if len(ws) == 6 else "mars_moon"
            net = MODELS[name](cin, cout, device=device)
            net.set_weights(ws)
            return net
        blob = torch.load(path, map_location="cpu")
        net = MODELS[blob["name"]](blob["cin"], blob["cout"], device=device)
        net.set_weights([w.numpy() for w in blob["weights"]])
        net.conv_padding = blob.get("conv_padding", "zeros")
        return net

    def summary(self, print_fn=print):
        print_fn("Model %s: %d parameters" % (self.name, self.n_params))
        for k in range(0, len(self.shapes), 2):
            print_fn("  conv5x5 %-18s bias %s" % (self.shapes[k], self.shapes[k + 1]))

    def predict(self, x):
        with torch.no_grad():
            return self(x)


def _conv_form(x, scaled, nslots):
    """conv(x, w, b, residual, lrelu, slope, i, o): ops.conv5x5, or -- scaled=True on rows that are a multiple of 64 pixels wide -- the
    launches of schedule2d.NetSchedule2D's forward (ops.conv5x5_scaled; i / o: the absmax slot sets of the layer's input / output)."""
    if not (scaled and x.shape[2] % 64 == 0):
        return lambda x_, w, b, r, act, s, i, o: ops.conv5x5(x_, w, b, r, act, s)
    am = torch.zeros(nslots, ops.AMAX_SLOTS, dtype=torch.int32, device=x.device)
    return lambda x_, w, b, r, act, s, i, o: ops.conv5x5_scaled(x_, w, b, r, act, s, None if i is None else am[i], None if o is None else am[o])


def _circular_form(padding, periodic, scaled):
    """padding="circular", periodic=(py, px): conv(...) of _conv_form composed from ops.conv5x5_circular (the linear layer, padded
    circularly along the periodic axes) and torch operations for the skip and the LeakyReLU -- the autograd cross-check of
    NetSchedule2D(padding="circular").  None for padding="zeros"."""
    if padding not in ("zeros", "circular"):
        raise ValueError("padding must be 'zeros' or 'circular' (got %r)" % (padding,))
    if padding == "zeros":
        return None
    if periodic is None or not any(periodic):
        raise ValueError("padding='circular' needs a periodic axis: periodic=(py, px) with one of them true (got %r)" % (periodic,))
    if scaled:
        raise ValueError("padding='circular' composes ops.conv5x5_circular; scaled=True (the absmax hand-over of ops.conv5x5_scaled) does not apply")

    def conv(x, w, b, r, act, s, i, o):
        z = ops.conv5x5_circular(x, w, b, periodic)
        if r is not None:
            z = z + r
        return torch.nn.functional.leaky_relu(z, s) if act else z
    return conv


class MarsMoon(ConvNet):
    """model_mars_moon, karman_train.py:101-138: 12 convs, 260,354 parameters."""
    name = "mars_moon"

    @staticmethod
    def channels(cin, cout):
        return [cin] + [32] * 11 + [cout]

    def __call__(self, x, flat=None, scaled=False, padding="zeros", periodic=None):
        p = self.tensors(flat)
        s = self.slope
        conv = _circular_form(padding, periodic, scaled) or _conv_form(x, scaled, 11)
        h = conv(x, p[0], p[1], None, True, s, None, 0)
        for k in range(5):
            a = conv(h, p[2 + 4 * k], p[3 + 4 * k], None, True, s, 2 * k, 2 * k + 1)
            h = conv(a, p[4 + 4 * k], p[5 + 4 * k], h, True, s, 2 * k + 1, 2 * k + 2)
        return conv(h, p[22], p[23], None, False, s, 10, None)


class Mercury(ConvNet):
    """model_mercury, karman_train.py:92-99: Conv5x5(cin->32)+ReLU, Conv5x5(32->64)+ReLU, Conv5x5(64->2).
    The conv kernels are built for <= 32 channels per side, so the 64-channel layer runs as two 32-channel
    halves (output split for 32->64, input split + residual accumulation for 64->2).  Training: trainer.GraphTrainer."""
    name = "mercury"
    slope = 0.0                                      # ReLU = LeakyReLU with slope 0

    @staticmethod
    def channels(cin, cout):
        return [cin, 32, 64, cout]

    def __call__(self, x, flat=None, scaled=False, padding="zeros", periodic=None):
        p = self.tensors(flat)
        conv = _circular_form(padding, periodic, scaled) or _conv_form(x, scaled, 3)
        h = conv(x, p[0], p[1], None, True, 0.0, None, 0)
        b3a, b3b = ops.split_flat(p[3], (0, 32, 64))           # (1-D halves: not plain slices, see ConvNet.tensors)
        ha = conv(h, p[2][..., :32].contiguous(), b3a, None, True, 0.0, 0, 1)
        hb = conv(h, p[2][..., 32:].contiguous(), b3b, None, True, 0.0, 0, 2)
        oa = conv(ha, p[4][:, :, :32].contiguous(), p[5], None, False, 0.0, 1, None)
        return conv(hb, p[4][:, :, 32:].contiguous(), torch.zeros_like(p[5]), oa, False, 0.0, 2, None)


def model_mercury(tensor_in=None, cin=3, cout=2, seed=0, device="cuda"):
    if tensor_in is not None:
        cin = tensor_in.shape[-1]
    return Mercury(cin, cout, seed, device)


def model_mars_moon(tensor_in=None, cin=3, cout=2, seed=0, device="cuda"):
    if tensor_in is not None:
        cin = tensor_in.shape[-1]
    return MarsMoon(cin, cout, seed, device)


MODELS = {"mars_moon": MarsMoon, "mercury": Mercury}
