"""Static fields and forcings: inputs the forecaster consumes and never predicts (csrc/forcing.hip; the formulas are
written down in include/gwen_hip.h, "Forcings").

A ``ForcingClock`` keeps {t, dt} in device memory -- t seconds since 2000-01-01 00:00:00 UTC, dt seconds per step.
Kernels read the time there, and ``advance`` moves it in stream order, so a captured step sees the right time on every
replay.  ``solar`` is the 5-channel solar / time vector of every grid point AT the clock's time (start the clock at
t0 + dt for target-time forcings): [e0 max(cos zenith, 0), sin and cos of the local time, sin and cos of the year phase].

``embed`` is the forecaster's hot path: ``x + base + f wf^T`` for all members in one launch, f being the solar vector
(computed in registers, never stored) followed by the given columns.  Its backward regenerates the solar part from a
saved copy of the clock.
"""
from __future__ import annotations

import datetime as _dt
from typing import Optional

import numpy as np
import torch
from torch import Tensor

from . import _lib, ops
from .graph import _ptr, _stream

SOLAR_CHANNELS = 5
MAX_CHANNELS = 64
_EPOCH = _dt.datetime(2000, 1, 1, tzinfo=_dt.timezone.utc)


def seconds(t) -> int:
    """Seconds since 2000-01-01 00:00:00 UTC of an int, a ``datetime`` (naive: UTC) or a ``numpy.datetime64``."""
    if isinstance(t, np.datetime64):
        return int((t - np.datetime64("2000-01-01T00:00:00")) // np.timedelta64(1, "s"))
    if isinstance(t, _dt.datetime):
        if t.tzinfo is None:
            t = t.replace(tzinfo=_dt.timezone.utc)
        d = t - _EPOCH
        return d.days * 86400 + d.seconds
    return int(t)


class ForcingClock:
    """{t, dt} on ``device`` (int64 pair).  ``advance(n)`` adds ``n dt`` to t on the current stream (capturable);
    ``time`` reads t back (a host sync: for tests and logging)."""

    def __init__(self, t, dt: int, device):
        self.dt = int(dt)
        self.state = torch.tensor([seconds(t), self.dt], dtype=torch.int64, device=device)
        if not self.state.is_cuda:
            raise RuntimeError("gwen_amd: ForcingClock must live on a HIP device (no CPU fallback)")

    @property
    def device(self) -> torch.device:
        return self.state.device

    @property
    def time(self) -> int:
        return int(self.state[0].item())

    def advance(self, n: int = 1) -> "ForcingClock":
        _advance(self.state, n)
        return self

    def snapshot(self) -> Tensor:
        """A device copy of the state: the time as it is when this call's launch runs."""
        return self.state.clone()


def _advance(state: Tensor, n: int) -> None:
    with torch.cuda.device(state.device):
        rc = _lib.lib().gwen_forcing_advance(_ptr(state), int(n), _stream(state.device))
    _lib.check(rc, "gwen_forcing_advance")


def _latlon(latlon: Tensor, device) -> Tensor:
    if latlon.dim() != 2 or latlon.size(1) != 2 or latlon.dtype != torch.float64:
        raise ValueError(f"latlon must be float64 [N, 2] (lat, lon in radians), got {latlon.dtype} {tuple(latlon.shape)}")
    if not latlon.is_cuda or latlon.device != device:
        raise RuntimeError("gwen_amd: latlon must live on the clock's device (no CPU fallback)")
    return latlon.contiguous()


def _solar(state: Tensor, latlon: Tensor) -> Tensor:
    out = torch.empty(latlon.size(0), SOLAR_CHANNELS, dtype=torch.float32, device=state.device)
    with torch.cuda.device(state.device):
        rc = _lib.lib().gwen_forcing_solar_f32(_ptr(state), _ptr(latlon), latlon.size(0), _ptr(out),
                                               _stream(state.device))
    _lib.check(rc, "gwen_forcing_solar_f32")
    return out


def solar(clock: ForcingClock, latlon: Tensor) -> Tensor:
    """[N, 5] fp32: the solar vector of every point of ``latlon`` ([N, 2] float64 radians) at the clock's time."""
    return _solar(clock.state, _latlon(latlon, clock.device))


def _embed(state: Optional[Tensor], latlon: Optional[Tensor], given: Optional[Tensor], wf: Tensor,
           base: Optional[Tensor], nodes: int, x: Tensor, out: Tensor) -> Tensor:
    opt = lambda t: None if t is None else _ptr(t)                                   # noqa: E731
    with torch.cuda.device(x.device):
        rc = _lib.lib().gwen_forcing_embed_f32(opt(state), opt(latlon), opt(given), 0 if given is None else given.size(1),
                                               _ptr(wf), opt(base), x.size(0), int(nodes), _ptr(x), x.size(1),
                                               _ptr(out), _stream(x.device))
    _lib.check(rc, "gwen_forcing_embed_f32")
    return out


class _EmbedFunction(torch.autograd.Function):
    """out = x + base + f wf^T.  grad_x = grad_out; grad_base = the sum of grad_out over the members; grad_wf = that
    sum^T f, with the solar part of f regenerated from the saved clock (the live one has moved on by the time the
    backward runs) and reduced by ops.grad_weight (fixed order, fp32 products)."""

    @staticmethod
    def forward(ctx, x: Tensor, wf: Tensor, base: Optional[Tensor], state: Optional[Tensor], latlon: Optional[Tensor],
                given: Optional[Tensor], nodes: int) -> Tensor:
        ctx.save_for_backward(state, latlon, given)
        ctx.nodes = nodes
        return _embed(state, latlon, given, wf, base, nodes, x, torch.empty_like(x))

    @staticmethod
    def backward(ctx, g: Tensor):
        gx = g if ctx.needs_input_grad[0] else None
        gw = gb = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            state, latlon, given = ctx.saved_tensors
            g = g.contiguous()
            gs = g if g.size(0) == ctx.nodes else g.view(-1, ctx.nodes, g.size(1)).sum(0)
            if ctx.needs_input_grad[2]:
                gb = gs
            if ctx.needs_input_grad[1]:
                parts = ([] if state is None else [_solar(state, latlon)]) + ([] if given is None else [given])
                gw = ops.grad_weight(gs, parts[0] if len(parts) == 1 else torch.cat(parts, dim=1))
        return gx, gw, gb, None, None, None, None


def embed(x: Tensor, clock: Optional[ForcingClock], latlon: Optional[Tensor], given: Optional[Tensor], wf: Tensor,
          base: Optional[Tensor], nodes: int, out: Optional[Tensor] = None) -> Tensor:
    """``x + base + f wf^T`` for x [rows, H], row r being grid point ``r % nodes`` of member ``r // nodes`` (members
    share everything but x).  f = the solar vector at the clock's time (``clock`` and ``latlon`` [nodes, 2] float64, or
    None for neither) followed by ``given`` ([nodes, Fg] fp32 or None); wf [H, 5 solar + Fg] (an
    ``nn.Linear(.., H, bias=False)`` weight), 1 to 64 columns; base [nodes, H] or None; H % 4 == 0.  One launch.  ``out``
    (may be ``x`` itself) only without autograd."""
    ops._require(x, "x")
    ops._require(wf, "wf")
    nodes = int(nodes)
    if x.dim() != 2 or wf.dim() != 2 or wf.size(0) != x.size(1) or nodes < 1 or x.size(0) % nodes:
        raise ValueError(f"embed: x [members nodes, H] and wf [H, F] expected, got {tuple(x.shape)} and "
                         f"{tuple(wf.shape)} for {nodes} nodes")
    state = None
    if clock is not None:
        if clock.device != x.device:
            raise RuntimeError("gwen_amd: the forcing clock must live on x's device")
        if latlon is None:
            raise ValueError("embed: a clock needs latlon")
        latlon = _latlon(latlon, x.device)
        if latlon.size(0) != nodes:
            raise ValueError(f"embed: latlon has {latlon.size(0)} rows for {nodes} nodes")
        state = clock.state
    else:
        latlon = None
    if given is not None:
        ops._require(given, "given")
        if given.dim() != 2 or given.size(0) != nodes or given.device != x.device:
            raise ValueError(f"embed: given must be [nodes, Fg] on x's device, got {tuple(given.shape)}")
        given = given.contiguous() if given.size(1) else None
    width = (SOLAR_CHANNELS if state is not None else 0) + (0 if given is None else given.size(1))
    if not 1 <= width <= MAX_CHANNELS or wf.size(1) != width:
        raise ValueError(f"embed: {width} forcing channels (1 .. {MAX_CHANNELS}) against wf {tuple(wf.shape)}")
    if base is not None:
        ops._require(base, "base")
        if base.shape != (nodes, x.size(1)) or base.device != x.device:
            raise ValueError(f"embed: base must be [nodes, H] on x's device, got {tuple(base.shape)}")
        base = base.contiguous()
    x = x.contiguous()
    wf = wf.contiguous()
    if torch.is_grad_enabled() and (x.requires_grad or wf.requires_grad or (base is not None and base.requires_grad)):
        if out is not None:
            raise ValueError("embed: out= is not supported under autograd")
        return _EmbedFunction.apply(x, wf, base, None if clock is None else clock.snapshot(), latlon, given, nodes)
    if out is not None and (out.shape != x.shape or out.dtype != x.dtype or out.device != x.device
                            or not out.is_contiguous()):
        raise ValueError("embed: out must be a contiguous tensor like x")
    return _embed(state, latlon, given, wf, base, nodes, x, torch.empty_like(x) if out is None else out)
