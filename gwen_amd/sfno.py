"""Spherical Fourier neural operator: spectral convolution, block and model on the transforms of ``gwen_amd.spectral``.

The spectral convolution is the learned linear map of an SFNO layer, applied to spherical harmonic coefficients::

    out[..., l^2 + j, :] = coef[..., l^2 + j, :] @ weight[l]          0 <= j <= 2l,  weight [lmax + 1, Cin, Cout]

The weight is real and depends on the degree ``l`` only.  That is the spherical convolution theorem: convolution with a
zonal filter multiplies every order ``m`` of a degree by the same factor, so the layer commutes with every rotation of the
sphere.  One launch of ``csrc/spectral_conv.hip`` runs all degrees as a grouped GEMM (group sizes 1, 3, 5, ...; the batch
folded into the row axis so that each ``weight[l]`` is read once); the gradient in ``coef`` is the same kernel on the
transposed weight, the gradient in ``weight`` a second kernel that sums in a fixed order without atomics.  Both run on
the layer's own contraction: ``"f16x3"`` (the default: fp32-class, bf16x6 here as in K3) or ``"3xbf16"``.

On top of it: ``SpectralConv`` (analysis, convolution, synthesis -- onto another grid of the same ``lmax`` if asked),
``SFNOBlock`` (spectral convolution plus a pointwise skip, then a pointwise MLP, both residual, pre-norm) and ``SFNO``
(pointwise encoder, blocks, pointwise decoder).  The pointwise pieces are the package's own: ``ops.layer_norm``,
``ops.linear_autograd`` and the activation Function of ``attention.py``.

Out of scope: complex or per-``m`` weights (they break rotation equivariance), block-diagonal or factorised weights, a
spectral bias, fp64 coefficients into the convolution, wiring into ``InteractionForecaster`` (its processors live on the
mesh, not on the grid), and any change to the transforms.  There is no CPU fallback: CPU tensors raise RuntimeError.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor, nn

from . import _lib, ops
from .graph import _ptr, _stream

PRECISIONS = ("f16x3", "bf16x6", "3xbf16")
MIN_CHANNELS, MAX_CHANNELS, CHANNEL_STEP = 16, 512, 16
MAX_LMAX = 1023


def spectral_conv_supported(cin: int, cout: int) -> bool:
    """Channel counts the kernels take: multiples of 16 in [16, 512] (``gwen_spectral_conv_supported`` gives the same
    answer).  No device is touched."""
    return all(isinstance(c, int) and MIN_CHANNELS <= c <= MAX_CHANNELS and c % CHANNEL_STEP == 0 for c in (cin, cout))


def _contract(precision: str) -> int:
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {PRECISIONS} (got {precision!r})")
    return _lib.CONTRACT_NAMES[precision]


def _check_channels(cin: int, cout: int) -> None:
    if not spectral_conv_supported(cin, cout):
        raise ValueError(f"spectral_conv needs channel counts that are multiples of {CHANNEL_STEP} in "
                         f"[{MIN_CHANNELS}, {MAX_CHANNELS}]; got {cin} -> {cout}")


def _launch(coef: Tensor, weight: Tensor, batch: int, lmax: int, cin: int, cout: int, transpose_w: bool,
            code: int, out: Optional[Tensor] = None) -> Tensor:
    """``gwen_spectral_conv_f32`` on contiguous device tensors: ``coef [batch, T, cin]`` -> ``[batch, T, cout]`` (into
    ``out`` when given: contiguous, of that shape)."""
    dev = coef.device
    if out is None:
        out = torch.empty(*coef.shape[:-1], cout, dtype=torch.float32, device=dev)
    if batch:
        with torch.cuda.device(dev):
            rc = _lib.lib().gwen_spectral_conv_f32(_ptr(coef), _ptr(weight), _ptr(out), batch, lmax, cin, cout,
                                                   int(transpose_w), code, _stream(dev))
        _lib.check(rc, "gwen_spectral_conv_f32")
    return out


class _SpectralConvFunction(torch.autograd.Function):
    """out = coef . W[deg]; g_coef = g . W[deg]^T (the forward kernel reading W transposed in place); g_W[l] = the
    degree's coef^T g (``gwen_spectral_conv_grad_weight_f32``).  All three on one contraction."""

    @staticmethod
    def forward(ctx, coef: Tensor, weight: Tensor, lmax: int, code: int) -> Tensor:
        c = coef.detach().contiguous()
        w = weight.detach().contiguous()
        cin, cout = w.shape[1], w.shape[2]
        batch = c.numel() // (c.shape[-2] * cin)
        ctx.save_for_backward(c, w)
        ctx.sizes = (batch, lmax, cin, cout, code)
        return _launch(c, w, batch, lmax, cin, cout, False, code)

    @staticmethod
    def backward(ctx, g: Tensor):
        c, w = ctx.saved_tensors
        batch, lmax, cin, cout, code = ctx.sizes
        g = g.contiguous()
        g_coef = g_w = None
        if ctx.needs_input_grad[0]:
            g_coef = _launch(g, w, batch, lmax, cout, cin, True, code)
        if ctx.needs_input_grad[1]:
            if batch:
                g_w = torch.empty_like(w)
                with torch.cuda.device(w.device):
                    rc = _lib.lib().gwen_spectral_conv_grad_weight_f32(_ptr(c), _ptr(g), _ptr(g_w), batch, lmax, cin,
                                                                       cout, code, _stream(w.device))
                _lib.check(rc, "gwen_spectral_conv_grad_weight_f32")
            else:
                g_w = torch.zeros_like(w)
        return g_coef, g_w, None, None


def spectral_conv(coef: Tensor, weight: Tensor, lmax: Optional[int] = None, precision: str = "f16x3") -> Tensor:
    """``coef [..., T, Cin]`` fp32, ``weight [lmax + 1, Cin, Cout]`` fp32 -> ``[..., T, Cout]`` with every row of degree
    ``l`` times ``weight[l]`` (module docstring).  ``T = (lmax + 1)^2``; ``lmax`` defaults to ``weight.shape[0] - 1``.
    Leading axes are flattened into one batch.  Differentiable in ``coef`` and ``weight``.  Checks: shapes (ValueError),
    then dtypes (TypeError), then devices (RuntimeError)."""
    code = _contract(precision)
    if not isinstance(coef, Tensor) or not isinstance(weight, Tensor):
        raise ValueError("coef and weight must be tensors")
    if weight.dim() != 3 or weight.shape[0] < 1:
        raise ValueError(f"weight must be [lmax + 1, Cin, Cout], got {tuple(weight.shape)}")
    lmax = weight.shape[0] - 1 if lmax is None else int(lmax)
    if lmax < 0 or lmax > MAX_LMAX or weight.shape[0] != lmax + 1:
        raise ValueError(f"weight must hold lmax + 1 = {lmax + 1} matrices with 0 <= lmax <= {MAX_LMAX}, got "
                         f"{tuple(weight.shape)}")
    cin, cout = int(weight.shape[1]), int(weight.shape[2])
    t = (lmax + 1) ** 2
    if coef.dim() < 2 or coef.shape[-2] != t or coef.shape[-1] != cin:
        raise ValueError(f"coef must be [..., T = {t}, Cin = {cin}], got {tuple(coef.shape)}")
    _check_channels(cin, cout)
    for name, x in (("coef", coef), ("weight", weight)):
        if x.dtype != torch.float32:
            raise TypeError(f"gwen_amd: {name} must be float32 (got {x.dtype})")
    for name, x in (("coef", coef), ("weight", weight)):
        if not x.is_cuda:
            raise RuntimeError(f"gwen_amd: {name} must live on a HIP device (no CPU fallback)")
    if coef.device != weight.device:
        raise RuntimeError(f"gwen_amd: coef is on {coef.device}, weight on {weight.device}")
    return _SpectralConvFunction.apply(coef, weight, lmax, code)


def _check_transform(name: str, sh) -> None:
    for attr in ("lmax", "rows", "analysis", "synthesis"):
        if not hasattr(sh, attr):
            raise ValueError(f"{name} must be a SphericalHarmonics (it has no {attr!r})")


class SpectralConv(nn.Module):
    """``forward(x [..., nlat * nlon, Cin]) = sh_out.synthesis(spectral_conv(sh.analysis(x), weight))`` -- exactly this
    composition of public pieces, bit for bit.  ``weight [sh.lmax + 1, Cin, Cout]`` is drawn from torch's generator with
    standard deviation ``Cin^-1/2``.  ``sh_out`` (default ``sh``) may be another grid of the same ``lmax``: this is how an
    SFNO changes resolution.  The transforms are settings, not parameters or buffers."""

    def __init__(self, sh, in_channels: int, out_channels: int, precision: str = "f16x3", sh_out=None):
        super().__init__()
        _check_transform("sh", sh)
        sh_out = sh if sh_out is None else sh_out
        _check_transform("sh_out", sh_out)
        if sh_out.lmax != sh.lmax:
            raise ValueError(f"sh_out must have the lmax of sh ({sh.lmax}), got {sh_out.lmax}")
        _check_channels(in_channels, out_channels)
        _contract(precision)
        self.in_channels, self.out_channels, self.precision = in_channels, out_channels, precision
        self.sh, self.sh_out = sh, sh_out
        self.weight = nn.Parameter(torch.empty(sh.lmax + 1, in_channels, out_channels))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        with torch.no_grad():
            self.weight.normal_(0.0, self.in_channels ** -0.5)

    def forward(self, x: Tensor) -> Tensor:
        return self.sh_out.synthesis(spectral_conv(self.sh.analysis(x), self.weight, self.sh.lmax, self.precision))

    def extra_repr(self) -> str:
        return f"{self.in_channels}, {self.out_channels}, lmax={self.sh.lmax}, precision={self.precision!r}"


def _linear(x: Tensor, m: nn.Linear, precision: str) -> Tensor:
    return ops.linear_autograd(x, m.weight, m.bias, contract=precision)


def _norm(x: Tensor, m: Optional[nn.LayerNorm]) -> Tensor:
    if m is None:
        return x
    return ops.layer_norm(x.reshape(-1, x.shape[-1]), m.weight, m.bias, m.eps).view(x.shape)


def _check_field(x, rows: int, channels: int) -> None:
    """The package's order for a field ``[..., rows, channels]``: shape, dtype, device."""
    if not isinstance(x, Tensor) or x.dim() < 2 or x.shape[-2] != rows or x.shape[-1] != channels:
        got = tuple(x.shape) if isinstance(x, Tensor) else type(x).__name__
        raise ValueError(f"x must be [..., nlat * nlon = {rows}, {channels}], got {got}")
    if x.dtype != torch.float32:
        raise TypeError(f"gwen_amd: x must be float32 (got {x.dtype})")
    if not x.is_cuda:
        raise RuntimeError("gwen_amd: x must live on a HIP device (no CPU fallback)")


class SFNOBlock(nn.Module):
    """One SFNO layer on ``x [..., nlat * nlon, channels]``::

        n = norm1(x);  h = x + conv(n) + skip(n);   y = h + mlp.2(act(mlp.0(norm2(h))))

    ``conv`` is a ``SpectralConv``, ``skip`` a pointwise linear without bias, ``mlp`` a pointwise two-layer MLP of width
    ``mlp_ratio * channels``.  Parameters: ``norm1, conv, skip, norm2, mlp.0, mlp.2`` (no norms with
    ``layer_norm=False``).  ``precision`` governs the spectral convolution and every K3 contraction; LayerNorm, the
    activation and the residuals are fp32."""

    def __init__(self, sh, channels: int, mlp_ratio: int = 2, activation: str = "silu", layer_norm: bool = True,
                 precision: str = "f16x3", norm_eps: float = 1e-5):
        super().__init__()
        from .interaction import _ACT
        if activation not in _ACT:
            raise ValueError("activation in (none, relu, silu)")
        if not isinstance(mlp_ratio, int) or mlp_ratio < 1:
            raise ValueError(f"mlp_ratio must be a positive integer (got {mlp_ratio!r})")
        self.channels, self.activation, self.precision = channels, activation, precision
        self.conv = SpectralConv(sh, channels, channels, precision)
        self.norm1 = nn.LayerNorm(channels, eps=norm_eps) if layer_norm else None
        self.norm2 = nn.LayerNorm(channels, eps=norm_eps) if layer_norm else None
        self.skip = nn.Linear(channels, channels, bias=False)
        act = {"none": nn.Identity, "relu": nn.ReLU, "silu": nn.SiLU}[activation]()
        self.mlp = nn.Sequential(nn.Linear(channels, mlp_ratio * channels), act,
                                 nn.Linear(mlp_ratio * channels, channels))

    def forward(self, x: Tensor) -> Tensor:
        from .attention import _ActFunction
        _check_field(x, self.conv.sh.rows, self.channels)
        n = _norm(x, self.norm1)
        h = x + self.conv(n) + _linear(n, self.skip, self.precision)
        t = _linear(_norm(h, self.norm2), self.mlp[0], self.precision)
        if self.activation != "none":
            t = _ActFunction.apply(t.reshape(-1, t.shape[-1]), self.activation).view(t.shape)
        return h + _linear(t, self.mlp[2], self.precision)


class SFNO(nn.Module):
    """``forward(x [..., N, in_channels]) -> [..., N, out_channels]`` on the grid of ``sh`` (``N = nlat * nlon``; leading
    axes are members or batch): pointwise ``encoder`` (in_channels -> channels), ``blocks`` SFNOBlocks, pointwise
    ``decoder`` (channels -> out_channels).  ``residual=True`` adds the first ``out_channels`` input channels to the
    output -- one step of a forecaster (needs ``out_channels <= in_channels``).  ``state_dict``: ``encoder.weight
    [channels, in]``, ``encoder.bias``, ``blocks.K.{norm1, norm2}.{weight, bias}``, ``blocks.K.conv.weight [lmax + 1,
    channels, channels]``, ``blocks.K.skip.weight``, ``blocks.K.mlp.{0, 2}.{weight, bias}``, ``decoder.weight [out,
    channels]``, ``decoder.bias``."""

    def __init__(self, sh, in_channels: int, out_channels: int, channels: int, blocks: int, mlp_ratio: int = 2,
                 activation: str = "silu", layer_norm: bool = True, precision: str = "f16x3", residual: bool = False):
        super().__init__()
        if in_channels < 1 or out_channels < 1 or blocks < 0:
            raise ValueError("SFNO needs in_channels, out_channels >= 1 and blocks >= 0")
        if residual and out_channels > in_channels:
            raise ValueError(f"residual=True adds the first out_channels input channels: out_channels = {out_channels} "
                             f"> in_channels = {in_channels}")
        _check_transform("sh", sh)
        _check_channels(channels, channels)
        _contract(precision)
        self.in_channels, self.out_channels, self.channels = in_channels, out_channels, channels
        self.precision, self.residual = precision, residual
        self.sh = sh
        self.encoder = nn.Linear(in_channels, channels)
        self.blocks = nn.ModuleList(SFNOBlock(sh, channels, mlp_ratio, activation, layer_norm, precision)
                                    for _ in range(blocks))
        self.decoder = nn.Linear(channels, out_channels)

    def forward(self, x: Tensor) -> Tensor:
        _check_field(x, self.sh.rows, self.in_channels)
        h = _linear(x, self.encoder, self.precision)
        for block in self.blocks:
            h = block(h)
        y = _linear(h, self.decoder, self.precision)
        if self.residual:
            y = y + x[..., :self.out_channels]
        return y
