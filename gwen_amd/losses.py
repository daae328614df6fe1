"""Ensemble losses and scores over the members axis: the CRPS of ``[M, N, C]`` predictions against ``[N, C]`` truth.

For one point with members x_1..x_M and truth y (include/gwen_hip.h, ``gwen_ens_crps_f32``):

    CRPS_alpha = (1/M) sum_i |x_i - y| - k_alpha sum_i sum_j |x_i - x_j|,
    k_alpha    = alpha / (2M(M-1)) + (1 - alpha) / (2M^2)

alpha = 1 is the fair CRPS, 0 the ensemble's own, in between the almost-fair one.  Node weights ``w [N]`` (cell areas,
or a bool mask) and channel weights ``v [C]`` default to ones:

    crps_c = sum_n w_n CRPS(n, c) / sum w        loss = sum_c v_c crps_c / sum v

One HIP pass over the ensemble gives the loss, the per-channel scores and -- when asked -- the gradient, already
normalised; nothing synchronises with the host, so a training step with this loss captures into a hipGraph.  There is
no CPU fallback: CPU tensors raise RuntimeError.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
from torch import Tensor, nn

from . import _checks

MAX_MEMBERS = 64


def pair_coef(members: int, alpha: float) -> float:
    """k_alpha of the CRPS for ``members`` members (fp64)."""
    fair = alpha / (2.0 * members * (members - 1)) if alpha > 0 else 0.0
    return fair + (1.0 - alpha) / (2.0 * members * members)


def _check(pred, target, node_weights, channel_weights, alpha) -> None:
    """Shape and argument errors, then dtypes, then devices (``_checks``)."""
    if not isinstance(pred, Tensor) or not isinstance(target, Tensor):
        raise ValueError("pred and target must be tensors")
    _checks.require_members_first(pred)
    _checks.require_target_nc(pred, target)
    _checks.require_sizes(pred, MAX_MEMBERS)
    m, n, c = pred.shape
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha must lie in [0, 1] (got {alpha})")
    if alpha > 0 and m < 2:
        raise ValueError("alpha > 0 needs at least 2 members (alpha = 0 takes one)")
    for name, w, size in (("node_weights", node_weights, n), ("channel_weights", channel_weights, c)):
        _checks.require_weights(name, w, size)
        if w is not None and w.requires_grad:
            raise ValueError(f"{name} requires grad: the loss has no gradient for its weights (detach them)")
    for name, t in (("pred", pred), ("target", target), ("channel_weights", channel_weights)):
        _checks.require_dtype(name, t)
    _checks.require_dtype("node_weights", node_weights, (torch.float32, torch.bool))
    _checks.require_device(("pred", pred), ("target", target), ("node_weights", node_weights),
                           ("channel_weights", channel_weights))


def crps_launch(pred: Tensor, target: Tensor, node_weights: Optional[Tensor], channel_weights: Optional[Tensor],
                coef: float, grad_pred: Optional[Tensor], grad_target: Optional[Tensor], loss: Tensor,
                scores: Optional[Tensor], workspace: Tensor) -> None:
    """``gwen_ens_crps_f32`` on preallocated buffers (contiguous fp32 on one device; tools/ensemble_bench.py times it)."""
    from . import _lib
    from .graph import _ptr, _stream
    m, n, c = pred.shape
    dev = pred.device
    with torch.cuda.device(dev):
        rc = _lib.lib().gwen_ens_crps_f32(_ptr(pred), _ptr(target), _ptr(node_weights), _ptr(channel_weights), m, n, c,
                                          float(coef), _ptr(grad_pred), _ptr(grad_target), _ptr(loss), _ptr(scores),
                                          _ptr(workspace), workspace.numel(), _stream(dev))
    _lib.check(rc, "gwen_ens_crps_f32")


def workspace_floats(members: int, n: int, c: int) -> int:
    from . import _lib
    return int(_lib.lib().gwen_ens_crps_workspace_floats(members, n, c))


def _run(pred, target, node_weights, channel_weights, alpha, want_grad_pred, want_grad_target, want_scores):
    m, n, c = pred.shape
    p, t = pred.detach().contiguous(), target.detach().contiguous()
    w = None if node_weights is None else node_weights.detach().to(torch.float32).contiguous()
    v = None if channel_weights is None else channel_weights.detach().contiguous()
    gp = torch.empty_like(p) if want_grad_pred else None
    gt = torch.empty_like(t) if want_grad_target else None
    loss = torch.empty(1, dtype=torch.float32, device=p.device)
    scores = torch.empty(3, c, dtype=torch.float32, device=p.device) if want_scores else None
    ws = torch.empty(workspace_floats(m, n, c), dtype=torch.float32, device=p.device)
    crps_launch(p, t, w, v, pair_coef(m, float(alpha)), gp, gt, loss, scores, ws)
    return loss, scores, gp, gt


class _EnsembleCRPS(torch.autograd.Function):
    """gwen_ens_crps_f32: the loss and, for the inputs that need it, its gradient in the same pass."""

    @staticmethod
    def forward(ctx, pred: Tensor, target: Tensor, node_weights, channel_weights, alpha: float) -> Tensor:
        loss, _, gp, gt = _run(pred, target, node_weights, channel_weights, alpha,
                               ctx.needs_input_grad[0], ctx.needs_input_grad[1], False)
        ctx.save_for_backward(gp, gt)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        gp, gt = ctx.saved_tensors
        return (gp * g if gp is not None else None), (gt * g if gt is not None else None), None, None, None


def ensemble_crps(pred: Tensor, target: Tensor, node_weights: Optional[Tensor] = None,
                  channel_weights: Optional[Tensor] = None, alpha: float = 1.0) -> Tensor:
    """The weighted CRPS of ``pred [M, N, C]`` against ``target [N, C]`` (module docstring), a 0-dim fp32 tensor.
    Differentiable in ``pred`` and ``target``; the weights must not require grad."""
    _check(pred, target, node_weights, channel_weights, alpha)
    return _EnsembleCRPS.apply(pred, target, node_weights, channel_weights, float(alpha))


def ensemble_scores(pred: Tensor, target: Tensor, node_weights: Optional[Tensor] = None,
                    alpha: float = 1.0) -> Dict[str, Tensor]:
    """Per-channel verification scores, fp32 ``[C]`` each: ``crps`` (CRPS_alpha), ``rmse`` (of the ensemble mean) and
    ``spread`` (root of the mean unbiased ensemble variance), weighted by ``node_weights`` over the N points.  The same
    pass as ``ensemble_crps``, without gradients."""
    _check(pred, target, node_weights, None, alpha)
    _, scores, _, _ = _run(pred, target, node_weights, None, alpha, False, False, True)
    return {"crps": scores[0], "rmse": scores[1].sqrt(), "spread": scores[2].sqrt()}


def _weight_buffer(w) -> Optional[Tensor]:
    if w is None:
        return None
    if isinstance(w, np.ndarray):
        w = torch.from_numpy(w)
    w = torch.as_tensor(w)
    return w if w.dtype == torch.bool else w.detach().to(torch.float32)


class EnsembleCRPSLoss(nn.Module):
    """``loss(pred [M, N, C], target [N, C])`` = ``ensemble_crps`` with the module's alpha and weights.  The weights
    (tensors or numpy arrays, e.g. ``Mesh.face_areas()``) are buffers: ``.to(device)`` moves them, the module pickles."""

    def __init__(self, alpha: float = 1.0, node_weights=None, channel_weights=None):
        super().__init__()
        if not 0.0 <= float(alpha) <= 1.0:
            raise ValueError(f"alpha must lie in [0, 1] (got {alpha})")
        self.alpha = float(alpha)
        self.register_buffer("node_weights", _weight_buffer(node_weights))
        self.register_buffer("channel_weights", _weight_buffer(channel_weights))

    def forward(self, pred: Tensor, target: Tensor) -> Tensor:
        return ensemble_crps(pred, target, self.node_weights, self.channel_weights, self.alpha)

    def extra_repr(self) -> str:
        return f"alpha={self.alpha}"
