"""Training through rollouts with one step's activations at a time ("Training on rollouts").

A chain of forecaster steps under autograd keeps every step's saved tensors until the backward: each
``_InteractionNetFunction`` holds ``x_src, x_dst, e, agg, proj``, so every processor block of every step owns an
edge-sized fp32 tensor.  ``checkpointed_step`` keeps the state at the step boundary instead and runs the step's forward
again when its backward arrives.  The step is a pure function of {x_t, static embeddings, weights, noise draw, clock
time, forcing_t}; the draw and the time are snapshotted on the device (``NoiseStream.snapshot``,
``ForcingClock.snapshot``: stream-ordered copies, no host sync), so the second forward reproduces the first bit for bit.

No kernel of its own: the hot path is the model's step, forward and backward.  The model is duck-typed on the protocol
``forecaster.ensemble_forecast`` documents -- ``_static(graphs)`` and ``_step(x, graphs, static, noise=, member0=,
clock=, forcing=)``; the stream and the clock need ``state``, ``snapshot()`` and ``advance()``.

The forward sweep runs the step without grad mode, so the model's ``_step`` must compute the same bits with and without
it: the stored x_{t+1} is then the recomputed one.  InteractionForecaster's does, for both processors (tested).
"""
from __future__ import annotations

import copy
from typing import Any, List, Optional, Tuple

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable


def flatten_static(static) -> Tuple[List[Tensor], tuple]:
    """The tensors of a static-embeddings tuple in order, and its layout: -1 for a tensor, n for a list of n tensors
    (the transformer's per-block edge terms)."""
    flat, layout = [], []
    for item in static:
        if isinstance(item, Tensor):
            flat.append(item)
            layout.append(-1)
        elif isinstance(item, (list, tuple)) and all(isinstance(t, Tensor) for t in item):
            flat.extend(item)
            layout.append(len(item))
        else:
            raise TypeError(f"static embeddings hold tensors and lists of tensors, got {type(item).__name__}")
    return flat, tuple(layout)


def restore_static(flat, layout: tuple) -> tuple:
    """``flatten_static`` undone over ``flat`` (the same tensors, or stand-ins of them)."""
    need = sum(1 if n < 0 else n for n in layout)
    if need != len(flat):
        raise ValueError(f"the layout takes {need} tensors, {len(flat)} given")
    out, i = [], 0
    for n in layout:
        if n < 0:
            out.append(flat[i])
            i += 1
        else:
            out.append(list(flat[i:i + n]))
            i += n
    return tuple(out)


def _stand_in(obj: Any, snap: Tensor) -> Any:
    """A shallow copy of a stream / clock whose state is a private copy of the snapshot: the recomputed step reads and
    advances this one, the live object stays where the forward sweep left it."""
    twin = copy.copy(obj)
    twin.state = snap.clone()
    return twin


class _CheckpointedStep(torch.autograd.Function):
    """y = model._step(x, graphs, static, ..); saves x, the static embeddings, the forcing, the two snapshots and the
    parameters (none of them copies but the snapshots, 16 bytes each) and nothing of the step's inside."""

    @staticmethod
    def forward(ctx, model, graphs, layout, noise, member0, clock, forcing, n_static, x, *rest):
        flat, params = rest[:n_static], rest[n_static:]
        z = noise.snapshot() if noise is not None else None          # before the step: it advances both
        c = clock.snapshot() if clock is not None else None
        kw = _keywords(noise, member0, clock, forcing)
        y = model._step(x, graphs, restore_static(flat, layout), **kw)          # (grad mode is off in here)
        ctx.model, ctx.graphs, ctx.layout, ctx.n_static = model, graphs, layout, n_static
        ctx.noise, ctx.member0, ctx.clock = noise, member0, clock
        ctx.params = params                    # the live parameters: the recompute differentiates with respect to them
        # (saved as well: autograd's version check then refuses a backward after an in-place change of any of them)
        ctx.save_for_backward(x, forcing, z, c, *flat, *params)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, forcing, z, c, *rest = ctx.saved_tensors
        flat = rest[:ctx.n_static]
        needs = ctx.needs_input_grad[8:]                              # x, the static embeddings, the parameters
        noise = _stand_in(ctx.noise, z) if z is not None else None
        clock = _stand_in(ctx.clock, c) if c is not None else None
        with torch.enable_grad():
            xd = x.detach().requires_grad_(needs[0])
            fd = [t.detach().requires_grad_(n) for t, n in zip(flat, needs[1:])]
            y = ctx.model._step(xd, ctx.graphs, restore_static(fd, ctx.layout),
                                **_keywords(noise, ctx.member0, clock, forcing))
        inputs = [xd, *fd, *ctx.params]
        wanted = [t for t, n in zip(inputs, needs) if n]
        grads = iter(torch.autograd.grad(y, wanted, g, allow_unused=True) if wanted and y.requires_grad
                     else [None] * len(wanted))
        return (None,) * 8 + tuple(next(grads) if n else None for n in needs)


def _keywords(noise, member0: int, clock, forcing: Optional[Tensor]) -> dict:
    kw = {} if noise is None else {"noise": noise, "member0": member0}
    if clock is not None:
        kw["clock"] = clock
    if forcing is not None:
        kw["forcing"] = forcing
    return kw


def checkpointed_step(model, x: Tensor, graphs, static, noise=None, member0: int = 0, clock=None,
                      forcing: Optional[Tensor] = None) -> Tensor:
    """``model._step(x, graphs, static, ..)`` under autograd, saving its inputs only: the backward runs the step again
    (at the draw, the time and the forcing of this call) and differentiates that.  ``static`` = ``model._static(graphs)``;
    gradients reach ``x``, the static embeddings and every parameter of ``model`` that requires grad.  Advances the live
    stream and clock by one, as ``_step`` does; the backward leaves them alone and may run twice over a retained graph.
    Without grad mode, or when nothing requires grad, this IS ``_step``."""
    kw = _keywords(noise, member0, clock, forcing)
    flat, layout = flatten_static(static)
    params = [p for p in model.parameters() if p.requires_grad]
    if not (torch.is_grad_enabled() and any(t.requires_grad for t in (x, *flat, *params))):
        return model._step(x, graphs, static, **kw)
    return _CheckpointedStep.apply(model, graphs, layout, noise, member0, clock, forcing, len(flat), x, *flat, *params)
