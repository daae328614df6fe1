"""Reproducible per-member Gaussian noise (csrc/noise.hip; the generator is written down in include/gwen_hip.h).

z(seed, tag, draw, member, node, k) is a pure function of its arguments (Philox4x64-10 + Box-Muller), so member m's
noise is the same whichever rank holds it, however the members are batched and whether the step runs eagerly or from
a captured hipGraph.  A ``NoiseStream`` keeps {seed, draw} in device memory: kernels read the draw there, and
``advance`` moves it in stream order, so a captured step draws fresh noise on every replay.  Ranks of one ensemble
hold the same seed and the same draw; ``member0`` (the first global member of a rank's block) tells them apart.

``inject`` is the forecaster's hot path: ``x + z Wz^T`` in one launch.  Its backward regenerates z from a saved copy
of the state instead of storing it.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from . import _lib, ops
from .graph import _ptr, _stream

TAG_LATENT, TAG_INITIAL = 0, 1
INJECT_CHANNELS = (8, 16, 32, 64)
_MASK = (1 << 64) - 1


def _signed(v: int) -> int:
    v = int(v) & _MASK
    return v - (1 << 64) if v >> 63 else v


class NoiseStream:
    """{seed, draw} of the latent noise on ``device`` (a uint64 pair, stored as int64).  ``advance(n)`` adds ``n`` to
    the draw on the current stream (capturable); ``draw`` reads it back (a host sync: for tests and logging)."""

    def __init__(self, seed: int, device, draw: int = 0):
        self.seed = int(seed) & _MASK
        self.state = torch.tensor([_signed(seed), _signed(draw)], dtype=torch.int64, device=device)
        if not self.state.is_cuda:
            raise RuntimeError("gwen_amd: NoiseStream must live on a HIP device (no CPU fallback)")

    @property
    def device(self) -> torch.device:
        return self.state.device

    @property
    def draw(self) -> int:
        return int(self.state[1].item()) & _MASK

    def advance(self, n: int = 1) -> "NoiseStream":
        _advance(self.state, n)
        return self

    def snapshot(self) -> Tensor:
        """A device copy of the state: the draw as it is when this call's launch runs."""
        return self.state.clone()


def _advance(state: Tensor, n: int) -> None:
    with torch.cuda.device(state.device):
        rc = _lib.lib().gwen_noise_advance(_ptr(state), int(n), _stream(state.device))
    _lib.check(rc, "gwen_noise_advance")


def _normal(state: Tensor, members: int, nodes: int, K: int, member0: int, tag: int) -> Tensor:
    out = torch.empty(members, nodes, K, dtype=torch.float32, device=state.device)
    with torch.cuda.device(state.device):
        rc = _lib.lib().gwen_noise_normal_f32(_ptr(state), int(tag) & _MASK, int(member0), int(members), int(nodes),
                                              int(K), _ptr(out), _stream(state.device))
    _lib.check(rc, "gwen_noise_normal_f32")
    return out


def normal(stream: NoiseStream, members: int, nodes: int, K: int, member0: int = 0, tag: int = TAG_LATENT) -> Tensor:
    """[members, nodes, K] fp32: z(seed, tag, draw, member0 + m, n, k) at the stream's current draw."""
    return _normal(stream.state, members, nodes, K, member0, tag)


def _inject(state: Tensor, x: Tensor, wz: Tensor, nodes: int, member0: int, out: Tensor) -> Tensor:
    H, K = wz.shape
    with torch.cuda.device(x.device):
        rc = _lib.lib().gwen_noise_inject_f32(_ptr(state), int(member0), x.size(0), int(nodes), _ptr(x), _ptr(wz), H, K,
                                              _ptr(out), _stream(x.device))
    _lib.check(rc, "gwen_noise_inject_f32")
    return out


class _InjectFunction(torch.autograd.Function):
    """out = x + z Wz^T.  grad_x = grad_out; grad_Wz = grad_out^T z with z regenerated from the saved state (the live
    one has moved on by the time the backward runs) and reduced by ops.grad_weight (fixed order, fp32 products)."""

    @staticmethod
    def forward(ctx, x: Tensor, wz: Tensor, state: Tensor, nodes: int, member0: int) -> Tensor:
        ctx.save_for_backward(state)
        ctx.nodes, ctx.member0, ctx.rows, ctx.K = nodes, member0, x.size(0), wz.size(1)
        return _inject(state, x, wz, nodes, member0, torch.empty_like(x))

    @staticmethod
    def backward(ctx, g: Tensor):
        gx = g if ctx.needs_input_grad[0] else None
        gw = None
        if ctx.needs_input_grad[1]:
            (state,) = ctx.saved_tensors
            members = -(-ctx.rows // ctx.nodes)
            z = _normal(state, members, ctx.nodes, ctx.K, ctx.member0, TAG_LATENT).view(-1, ctx.K)[: ctx.rows]
            gw = ops.grad_weight(g, z)
        return gx, gw, None, None, None


def inject(x: Tensor, wz: Tensor, stream: NoiseStream, nodes: int, member0: int = 0,
           out: Optional[Tensor] = None) -> Tensor:
    """``x + z Wz^T`` for x [rows, H] and Wz [H, K] (an ``nn.Linear(K, H, bias=False)`` weight), row r being node
    ``r % nodes`` of member ``member0 + r // nodes``; K in {8, 16, 32, 64}, H % 4 == 0.  One launch.  ``out`` (may be
    ``x`` itself) only without autograd."""
    ops._require(x, "x")
    ops._require(wz, "wz")
    if x.dim() != 2 or wz.dim() != 2 or wz.size(0) != x.size(1):
        raise ValueError(f"inject: x [rows, H] and wz [H, K] expected, got {tuple(x.shape)} and {tuple(wz.shape)}")
    if not stream.state.is_cuda or stream.device != x.device:
        raise RuntimeError("gwen_amd: the noise stream must live on x's device")
    x = x.contiguous()
    wz = wz.contiguous()
    if torch.is_grad_enabled() and (x.requires_grad or wz.requires_grad):
        if out is not None:
            raise ValueError("inject: out= is not supported under autograd")
        return _InjectFunction.apply(x, wz, stream.snapshot(), int(nodes), int(member0))
    if out is not None and (out.shape != x.shape or out.dtype != x.dtype or out.device != x.device
                            or not out.is_contiguous()):
        raise ValueError("inject: out must be a contiguous tensor like x")
    return _inject(stream.state, x, wz, nodes, member0, torch.empty_like(x) if out is None else out)
