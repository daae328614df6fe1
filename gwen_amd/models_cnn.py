"""The U-Net baseline on the HIP kernels of csrc/conv.hip.

Public surface mirrors the reference's src/gwen/models_cnn.py: ``BaseNet``, ``Encoder``, ``Decoder`` and ``UNet`` with the
same parameter tree -- the layers the reference's forward never uses included (``UNet``'s own copies, the encoder's
transposed convolutions, the decoder's convolutions 0-3 and batch-norm 3) -- so its checkpoints load with
``strict=True``.  The forward is inference only (eval or train-mode BatchNorm); there is no backward yet, and a call that
would need one raises instead of returning a tensor without a graph.

Between the two layout changes at the ends (NCHW <-> channels-last, plain torch) everything is a kernel of libgwen_hip.so:
an encoder stage is ONE launch (3x3 conv + 2x2 max-pool + BatchNorm affine + ReLU, ``ops.conv3x3``), a decoder stage a
transposed conv and an upsample + BatchNorm + ReLU written straight into the upper channel slice of the concatenation
buffer (``ops.upsample2x``), the end the 1x1 conv as ``ops.linear``.  In train mode the affine comes from the batch
(``ops.channel_stats``, fp64 sums) and is applied by ``ops.affine_relu_``; the running statistics are updated on the
device as ``nn.BatchNorm2d`` does (momentum 0.1, unbiased variance), without a host synchronisation.
"""
from __future__ import annotations

from typing import Tuple

import torch
from torch import Tensor, nn

from . import ops
from .graph import _version_of

PRECISIONS = ("bf16x6", "3xbf16")
_DEPTH = 4                      # pool / upsample stages


def crop_range(size: int, target: int) -> Tuple[int, int]:
    """``Decoder.crop`` of the reference along one axis: [start, stop) of the encoder layer that is kept for a decoder
    layer of ``target``.  An odd difference drops one more element at the START (the reference's rule)."""
    d = size - target
    return d // 2 + d % 2, size - d // 2


def unet_output_hw(h: int, w: int) -> Tuple[int, int]:
    """Spatial size of ``UNet.forward``'s output for an input of ``h`` x ``w``: the height is the cropped one (floor to
    a multiple of 16), the width is padded back to ``w`` on the left (the reference's two replicate pads)."""
    if h < 2 ** _DEPTH or w < 2 ** _DEPTH:
        raise ValueError(f"the U-Net pools {_DEPTH} times: it needs at least {2 ** _DEPTH} x {2 ** _DEPTH} pixels, got {h} x {w}")
    return (h >> _DEPTH) << _DEPTH, w


class BaseNet(nn.Module):
    """The layers of the encoder and the decoder (the reference's ``BaseNet``, same names and shapes)."""

    def __init__(self, channels_in: int, channels_out: int, hidden_size: int, precision: str = "bf16x6") -> None:
        super().__init__()
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {PRECISIONS}, got {precision!r}")
        self.precision = precision
        self.activation = nn.ReLU(inplace=True)
        self.channels_in = channels_in
        self.channels_out = channels_out
        self.hidden_size = hidden_size
        h = hidden_size
        self.conv_layers = nn.ModuleList([
            nn.Conv2d(channels_in, h // 8, kernel_size=3, padding=1),
            nn.Conv2d(h // 8, h // 4, kernel_size=3, padding=1),
            nn.Conv2d(h // 4, h // 2, kernel_size=3, padding=1),
            nn.Conv2d(h // 2, h, kernel_size=3, padding=1),
            nn.Conv2d(channels_out, channels_out, kernel_size=1, stride=1),
        ])
        self.conv_transposed_layers = nn.ModuleList([
            nn.ConvTranspose2d(h, h // 2, kernel_size=3, padding=1),
            nn.ConvTranspose2d(h, h // 4, kernel_size=3, padding=1),
            nn.ConvTranspose2d(h // 2, h // 8, kernel_size=3, padding=1),
            nn.ConvTranspose2d(h // 4, channels_out, kernel_size=3, padding=1),
        ])
        self.batch_norm_layers = nn.ModuleList([
            nn.BatchNorm2d(h // 8), nn.BatchNorm2d(h // 4), nn.BatchNorm2d(h // 2), nn.BatchNorm2d(h),
        ])
        self.maxpool = nn.MaxPool2d(kernel_size=2, stride=2)
        self.upsample = nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True)
        self._affine_cache = {}          # batch-norm index -> (key, (scale, shift)): the eval-mode affine per version

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_affine_cache"] = {}
        return state

    def forward(self, x):
        raise NotImplementedError

    # ---- shared pieces ----
    def _guard(self, *tensors: Tensor) -> None:
        """No backward yet: refuse a call autograd would record; then refuse CPU tensors (no CPU fallback)."""
        if torch.is_grad_enabled() and (any(t.requires_grad for t in tensors) or
                                        any(p.requires_grad for p in self.parameters())):
            raise RuntimeError("gwen_amd U-Net: the backward is not implemented; call it under torch.no_grad() or with "
                               "requires_grad=False on the input and every parameter")
        for t in tensors:
            if not t.is_cuda:
                raise RuntimeError("gwen_amd U-Net: the input must live on a HIP device (no CPU fallback)")
            if t.dtype != torch.float32 or t.dim() != 4:
                raise TypeError(f"gwen_amd U-Net: expected a float32 [B, C, H, W] tensor, got {t.dtype} {tuple(t.shape)}")

    def _eval_affine(self, i: int):
        """BatchNorm ``i`` on its running statistics as y = x s + t, kept per version of its four tensors."""
        bn = self.batch_norm_layers[i]
        tensors = (bn.weight, bn.bias, bn.running_mean, bn.running_var)
        key = tuple((t.data_ptr(), _version_of(t)) for t in tensors)
        hit = self._affine_cache.get(i)
        if hit is not None and hit[0] == key and all(v is not None for _, v in key):   # (inference-mode tensors
            # carry no version: their affine is computed every call)
            return hit[1]
        with torch.no_grad():
            s = bn.weight.double() * torch.rsqrt(bn.running_var.double() + bn.eps)
            t = bn.bias.double() - bn.running_mean.double() * s
            pair = (s.float(), t.float())
        self._affine_cache[i] = (key, pair)
        return pair

    def _train_norm_relu_(self, i: int, x: Tensor) -> None:
        """x <- relu(BatchNorm_i(x)) on the statistics of x itself (channels-last, a channel slice allowed), and the
        running statistics moved as nn.BatchNorm2d moves them; nothing here reads a value back to the host."""
        bn = self.batch_norm_layers[i]
        n = x.size(0) * x.size(1) * x.size(2)
        if n < 2:
            raise ValueError(f"train-mode BatchNorm needs more than 1 value per channel, got input size {tuple(x.shape)}")
        mean, var = ops.channel_stats(x)
        with torch.no_grad():
            s = bn.weight.double() * torch.rsqrt(var + bn.eps)
            t = bn.bias.double() - mean * s
            ops.affine_relu_(x, s.float(), t.float())
            m = bn.momentum               # 0.1 in the reference's layers (None, a cumulative average, is not built)
            if m is None:
                raise NotImplementedError("gwen_amd U-Net: BatchNorm with momentum=None")
            bn.running_mean.mul_(1.0 - m).add_((m * mean).float())
            bn.running_var.mul_(1.0 - m).add_((m * (n / (n - 1.0)) * var).float())
            bn.num_batches_tracked.add_(1)

    def _conv_pool_norm_relu(self, i: int, x: Tensor) -> Tensor:
        conv = self.conv_layers[i]
        if self.training:
            y = ops.conv3x3(x, conv.weight, conv.bias, pool=True, contract=self.precision)
            self._train_norm_relu_(i, y)
            return y
        return ops.conv3x3(x, conv.weight, conv.bias, pool=True, affine=self._eval_affine(i), relu=True,
                           contract=self.precision)


def _to_nhwc(x: Tensor) -> Tensor:
    return x.permute(0, 2, 3, 1).contiguous()


def _to_nchw(x: Tensor) -> Tensor:
    return x.permute(0, 3, 1, 2).contiguous()


class Encoder(BaseNet):
    """Four stages of conv 3x3 -> max-pool -> BatchNorm -> ReLU; returns the four feature maps."""

    def forward_nhwc(self, x: Tensor):
        x1 = self._conv_pool_norm_relu(0, x)
        x2 = self._conv_pool_norm_relu(1, x1)
        x3 = self._conv_pool_norm_relu(2, x2)
        x4 = self._conv_pool_norm_relu(3, x3)
        return x1, x2, x3, x4

    def forward(self, x: Tensor):
        self._guard(x)
        unet_output_hw(x.size(2), x.size(3))
        return tuple(_to_nchw(t) for t in self.forward_nhwc(_to_nhwc(x)))


class Decoder(BaseNet):
    """Three stages of transposed conv -> upsample -> BatchNorm -> ReLU -> concatenation with the cropped encoder map,
    then transposed conv -> upsample -> ReLU -> 1x1 conv."""

    def crop(self, encoder_layer: Tensor, decoder_layer: Tensor) -> Tensor:
        """The reference's crop, on [B, C, H, W] tensors."""
        y0, y1 = crop_range(encoder_layer.size(2), decoder_layer.size(2))
        x0, x1 = crop_range(encoder_layer.size(3), decoder_layer.size(3))
        return encoder_layer[:, :, y0:y1, x0:x1]

    def _stage(self, k: int, bn: int, low: Tensor, skip: Tensor):
        """(concatenation buffer [skip | up], width the crop left over -- the reference's ``cropped`` term)"""
        tconv = self.conv_transposed_layers[k]
        t = ops.conv3x3(low, tconv.weight, tconv.bias, transposed=True, contract=self.precision)
        b, h, w, c = t.shape
        if skip.shape[1:3] != (2 * h, 2 * w):
            (y0, y1), (x0, x1) = crop_range(skip.size(1), 2 * h), crop_range(skip.size(2), 2 * w)
            skip = skip[:, y0:y1, x0:x1, :]
        cs = skip.size(3)
        buf = torch.empty(b, 2 * h, 2 * w, cs + c, dtype=torch.float32, device=t.device)
        up = buf[..., cs:]
        if self.training:
            ops.upsample2x(t, out=up)
            self._train_norm_relu_(bn, up)
        else:
            ops.upsample2x(t, affine=self._eval_affine(bn), relu=True, out=up)
        buf[..., :cs].copy_(skip)
        # (the reference's second ReLU after the concatenation acts on non-negative values: no launch)
        # The second value restates the reference's ``cropped += x.shape[3] - y.shape[3]``, taken AFTER its crop: the
        # crop leaves exactly the decoder's width, so it is always 0 and the ``cropped * 2`` pad in the callers never
        # runs -- in the reference either.  Kept so the forward reads line for line like the reference's.
        return buf, skip.size(2) - 2 * w

    def forward_nhwc(self, x):
        x1, x2, x3, x4 = x
        cropped = 0
        y1, d = self._stage(0, 2, x4, x3)
        cropped += d
        y2, d = self._stage(1, 1, y1, x2)
        cropped += d
        y3, d = self._stage(2, 0, y2, x1)
        cropped += d
        tconv = self.conv_transposed_layers[3]
        t = ops.conv3x3(y3, tconv.weight, tconv.bias, transposed=True, contract=self.precision)
        y4 = ops.upsample2x(t, relu=True)
        last = self.conv_layers[4]
        co = self.channels_out
        out = ops.linear(y4.view(-1, co), last.weight.detach().view(co, co), last.bias.detach(), contract=self.precision)
        return out.view(y4.shape), cropped

    def forward(self, x):
        self._guard(*x)
        out, cropped = self.forward_nhwc(tuple(_to_nhwc(t) for t in x))
        out = _to_nchw(out)
        if cropped > 0:
            out = nn.functional.pad(out, (cropped * 2, 0, 0, 0), mode="replicate")
        return out


class UNet(BaseNet):
    """``UNet(channels_in, channels_out, hidden_size)`` of the reference; ``precision``: "bf16x6" (fp32-class, default)
    or "3xbf16" for every contraction.  ``forward(x)``: [B, channels_in, H, W] -> [B, channels_out, H', W] with H' = H
    floored to a multiple of 16 (the crops) and the width padded back on the left by replication, as the reference does."""

    def __init__(self, channels_in: int, channels_out: int, hidden_size: int, precision: str = "bf16x6") -> None:
        super().__init__(channels_in, channels_out, hidden_size, precision)
        self.encoder = Encoder(channels_in, channels_out, hidden_size, precision)
        self.decoder = Decoder(channels_in, channels_out, hidden_size, precision)

    @staticmethod
    def output_hw(h: int, w: int) -> Tuple[int, int]:
        return unet_output_hw(h, w)

    def forward(self, x: Tensor) -> Tensor:
        self._guard(x)
        if x.size(1) != self.channels_in:
            raise ValueError(f"x has {x.size(1)} channels, the model expects {self.channels_in}")
        unet_output_hw(x.size(2), x.size(3))
        out, cropped = self.decoder.forward_nhwc(self.encoder.forward_nhwc(_to_nhwc(x)))
        out = _to_nchw(out)
        if cropped > 0:
            out = nn.functional.pad(out, (cropped * 2, 0, 0, 0), mode="replicate")
        if x.shape[3] != out.shape[3]:
            out = nn.functional.pad(out, (x.shape[3] - out.shape[3], 0, 0, 0), mode="replicate")
        return out
