"""The U-Net baseline on the HIP kernels of csrc/conv.hip.

Public surface mirrors the reference's src/gwen/models_cnn.py: ``BaseNet``, ``Encoder``, ``Decoder`` and ``UNet`` with the
same parameter tree -- the layers the reference's forward never uses included (``UNet``'s own copies, the encoder's
transposed convolutions, the decoder's convolutions 0-3 and batch-norm 3) -- so its checkpoints load with
``strict=True``.  By default the forward is inference only (eval or train-mode BatchNorm) and a call that would need a
backward raises instead of returning a tensor without a graph; with ``grad=True`` a recorded forward keeps what the
backward needs and ``backward()`` runs on the kernels of csrc/conv_bwd.hip (atomic-free, bitwise reproducible).

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

    def __init__(self, channels_in: int, channels_out: int, hidden_size: int, precision: str = "bf16x6",
                 grad: bool = False) -> None:
        super().__init__()
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {PRECISIONS}, got {precision!r}")
        self.precision = precision
        self.grad = bool(grad)
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
        """Without ``grad=True``: refuse a call autograd would record; then refuse CPU tensors (no CPU fallback)."""
        if not self.grad and self._autograd_records(*tensors):
            raise RuntimeError("gwen_amd U-Net: the backward is not implemented; call it under torch.no_grad() or with "
                               "requires_grad=False on the input and every parameter")
        for t in tensors:
            if not t.is_cuda:
                raise RuntimeError("gwen_amd U-Net: the input must live on a HIP device (no CPU fallback)")
            if t.dtype != torch.float32 or t.dim() != 4:
                raise TypeError(f"gwen_amd U-Net: expected a float32 [B, C, H, W] tensor, got {t.dtype} {tuple(t.shape)}")

    def _autograd_records(self, *tensors: Tensor) -> bool:
        return torch.is_grad_enabled() and (any(t.requires_grad for t in tensors) or
                                            any(p.requires_grad for p in self.parameters()))

    def _recording(self, *tensors: Tensor) -> bool:
        """grad=True and autograd recording: the forward goes through the Functions below and keeps what they save."""
        return self.grad and self._autograd_records(*tensors)

    def _eval_stats(self, i: int):
        """(mean, rstd) of BatchNorm ``i`` on its running statistics, fp64 -- what the eval-mode backward reads."""
        bn = self.batch_norm_layers[i]
        with torch.no_grad():
            return bn.running_mean.double(), torch.rsqrt(bn.running_var.double() + bn.eps)

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

    def _train_norm_relu_(self, i: int, x: Tensor):
        """x <- relu(BatchNorm_i(x)) on the statistics of x itself (channels-last, a channel slice allowed), and the
        running statistics moved as nn.BatchNorm2d moves them; nothing here reads a value back to the host.  Returns
        the batch's (mean, rstd) in fp64, which the backward keeps."""
        bn = self.batch_norm_layers[i]
        n = x.size(0) * x.size(1) * x.size(2)
        if n < 2:
            raise ValueError(f"train-mode BatchNorm needs more than 1 value per channel, got input size {tuple(x.shape)}")
        mean, var = ops.channel_stats(x)
        with torch.no_grad():
            rstd = torch.rsqrt(var + bn.eps)
            s = bn.weight.double() * rstd
            t = bn.bias.double() - mean * s
            ops.affine_relu_(x, s.float(), t.float())
            m = bn.momentum               # 0.1 in the reference's layers (None, a cumulative average, is not built)
            if m is None:
                raise NotImplementedError("gwen_amd U-Net: BatchNorm with momentum=None")
            bn.running_mean.mul_(1.0 - m).add_((m * mean).float())
            bn.running_var.mul_(1.0 - m).add_((m * (n / (n - 1.0)) * var).float())
            bn.num_batches_tracked.add_(1)
        return mean, rstd

    def _encode(self, i: int, x: Tensor, weight: Tensor, bias: Tensor, keep: bool = False):
        """y = relu(BatchNorm_i(pool(conv(x)))); ``keep``: (y, pooled value before BatchNorm, argmax, mean, rstd) --
        the same launches, which also write what the backward reads."""
        if self.training:
            r = ops.conv3x3(x, weight, bias, pool=True, contract=self.precision, argmax=keep)
            y = r[0] if keep else r
            stats = self._train_norm_relu_(i, y)
        else:
            r = ops.conv3x3(x, weight, bias, pool=True, affine=self._eval_affine(i), relu=True, contract=self.precision,
                            argmax=keep)
            y = r[0] if keep else r
            stats = self._eval_stats(i) if keep else None
        return (y, r[2], r[1]) + tuple(stats) if keep else y

    def _decode(self, k: int, bn: int, low: Tensor, skip: Tensor, weight: Tensor, bias: Tensor, keep: bool = False):
        """buf = [skip | relu(BatchNorm_bn(up(tconv(low))))], the upsample written straight into the buffer's upper
        channel slice; ``keep``: (buf, t, mean, rstd) with t the transposed conv's output."""
        t = ops.conv3x3(low, weight, bias, transposed=True, contract=self.precision)
        b, h, w, c = t.shape
        cs = skip.size(3)
        buf = torch.empty(b, 2 * h, 2 * w, cs + c, dtype=torch.float32, device=t.device)
        up = buf[..., cs:]
        if self.training:
            ops.upsample2x(t, out=up)
            stats = self._train_norm_relu_(bn, up)
        else:
            ops.upsample2x(t, affine=self._eval_affine(bn), relu=True, out=up)
            stats = self._eval_stats(bn) if keep else None
        buf[..., :cs].copy_(skip)
        return (buf, t) + tuple(stats) if keep else buf

    def _conv_pool_norm_relu(self, i: int, x: Tensor) -> Tensor:
        conv = self.conv_layers[i]
        if self._recording(x):
            bn = self.batch_norm_layers[i]
            return _EncoderStage.apply(self, i, x, conv.weight, conv.bias, bn.weight, bn.bias)
        return self._encode(i, x, conv.weight, conv.bias)


# ---- the recorded forward and its backward: one Function per stage, every arithmetic step a kernel of the library ----

def _conv_grads(ctx, g: Tensor, x: Tensor, weight: Tensor, layer_transposed: bool, at):
    """(g_x, g_W, g_b) of a 3x3 layer from the gradient ``g`` of its output: the data gradient is the convolution with
    the weight read as the other layer type; ``at`` = the positions of x, weight and bias among the Function's inputs."""
    need, precision = ctx.needs_input_grad, ctx.precision
    gx = ops.conv3x3(g, weight, None, transposed=not layer_transposed, contract=precision) if need[at[0]] else None
    gw = ops.conv3x3_grad_weight(g, x, transposed=layer_transposed, contract=precision) if need[at[1]] else None
    gb = ops.grad_bias(g) if need[at[2]] else None
    return gx, gw, gb


class _EncoderStage(torch.autograd.Function):
    """y = relu(BatchNorm_i(pool(conv_i(x)))): keeps x, the pooled value before BatchNorm, the pool's argmax and y."""

    @staticmethod
    def forward(ctx, net, i, x, weight, bias, gamma, beta):
        y, p, am, mean, rstd = net._encode(i, x, weight, bias, keep=True)
        ctx.train, ctx.precision = net.training, net.precision
        ctx.save_for_backward(x, weight, gamma, p, am, y, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, g_y):
        x, weight, gamma, p, am, y, mean, rstd = ctx.saved_tensors
        g_p, g_gamma, g_beta = ops.norm_relu_backward(g_y.contiguous(), y, p, gamma, mean, rstd, ctx.train)
        g_c = ops.unpool2x2(g_p, am, x.size(1), x.size(2))
        need = ctx.needs_input_grad
        gx = ops.conv3x3(g_c, weight, None, transposed=True, contract=ctx.precision) if need[2] else None
        gw = ops.conv3x3_grad_weight(g_c, x, contract=ctx.precision) if need[3] else None
        gb = ops.grad_bias(g_p) if need[4] else None          # (the column sums of g_c are those of g_p)
        return None, None, gx, gw, gb, g_gamma.float() if need[5] else None, g_beta.float() if need[6] else None


class _DecoderStage(torch.autograd.Function):
    """buf = [skip | relu(BatchNorm(up(tconv_k(low))))]: keeps low, the transposed conv's output t and buf; up(t) before
    BatchNorm is recomputed from t in the backward (one launch instead of a full-resolution tensor kept)."""

    @staticmethod
    def forward(ctx, net, k, bn, low, skip, weight, bias, gamma, beta):
        buf, t, mean, rstd = net._decode(k, bn, low, skip, weight, bias, keep=True)
        ctx.train, ctx.precision, ctx.cs = net.training, net.precision, skip.size(3)
        ctx.save_for_backward(low, weight, gamma, t, buf, mean, rstd)
        return buf

    @staticmethod
    def backward(ctx, g_buf):
        low, weight, gamma, t, buf, mean, rstd = ctx.saved_tensors
        cs = ctx.cs
        g_buf = g_buf.contiguous()
        g_u, g_gamma, g_beta = ops.norm_relu_backward(g_buf[..., cs:], buf[..., cs:], ops.upsample2x(t), gamma, mean,
                                                      rstd, ctx.train)
        g_t = ops.upsample2x_backward(g_u)
        g_low, gw, gb = _conv_grads(ctx, g_t, low, weight, True, (3, 5, 6))
        need = ctx.needs_input_grad
        # the lower slice goes back to the cropped skip (its second ReLU passes what the encoder's own ReLU passes)
        g_skip = g_buf[..., :cs] if need[4] else None
        return (None, None, None, g_low, g_skip, gw, gb, g_gamma.float() if need[7] else None,
                g_beta.float() if need[8] else None)


class _LastStage(torch.autograd.Function):
    """y4 = relu(up(tconv_3(y3))): keeps y3 and y4."""

    @staticmethod
    def forward(ctx, net, y3, weight, bias):
        t = ops.conv3x3(y3, weight, bias, transposed=True, contract=net.precision)
        y4 = ops.upsample2x(t, relu=True)
        ctx.precision = net.precision
        ctx.save_for_backward(y3, weight, y4)
        return y4

    @staticmethod
    def backward(ctx, g_y4):
        y3, weight, y4 = ctx.saved_tensors
        g_t = ops.upsample2x_backward(g_y4.contiguous(), mask_from=y4)
        return (None,) + _conv_grads(ctx, g_t, y3, weight, True, (1, 2, 3))


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
        h, w = low.size(1), low.size(2)
        if skip.shape[1:3] != (2 * h, 2 * w):
            (y0, y1), (x0, x1) = crop_range(skip.size(1), 2 * h), crop_range(skip.size(2), 2 * w)
            skip = skip[:, y0:y1, x0:x1, :]
        if self._recording(low, skip):
            norm = self.batch_norm_layers[bn]
            buf = _DecoderStage.apply(self, k, bn, low, skip, tconv.weight, tconv.bias, norm.weight, norm.bias)
        else:
            buf = self._decode(k, bn, low, skip, tconv.weight, tconv.bias)
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
        last = self.conv_layers[4]
        co = self.channels_out
        if self._recording(y3):
            y4 = _LastStage.apply(self, y3, tconv.weight, tconv.bias)
            out = ops.LinearFunction.apply(y4.view(-1, co), last.weight.view(co, co), last.bias, False, self.precision)
            return out.view(y4.shape), cropped
        t = ops.conv3x3(y3, tconv.weight, tconv.bias, transposed=True, contract=self.precision)
        y4 = ops.upsample2x(t, relu=True)
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
    or "3xbf16" for every contraction; ``grad=True``: a forward that autograd records returns a tensor with a graph
    (train or eval mode), otherwise it is the inference path.  ``forward(x)``: [B, channels_in, H, W] -> [B, channels_out, H', W] with H' = H
    floored to a multiple of 16 (the crops) and the width padded back on the left by replication, as the reference does."""

    def __init__(self, channels_in: int, channels_out: int, hidden_size: int, precision: str = "bf16x6",
                 grad: bool = False) -> None:
        super().__init__(channels_in, channels_out, hidden_size, precision, grad)
        self.encoder = Encoder(channels_in, channels_out, hidden_size, precision, grad)
        self.decoder = Decoder(channels_in, channels_out, hidden_size, precision, grad)

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
