"""The reference's loss module (``gwen.loss_functions``) on the MI355X: the same three classes behind one import line.

    from gwen_amd.loss_functions import CRPSLoss, EnsembleVarRegLoss, MaskedLoss

``CRPSLoss``            the Gaussian-CDF score over the members axis: per point mu and sigma = std + 1e-6 of the
                        members, ``(Normal(mu, sigma).cdf(target) - 1/2)^2`` averaged over the three trailing axes.
``EnsembleVarRegLoss``  ``mean |outputs - target| - alpha * mean var(outputs, dim=1)``.
``MaskedLoss``          ``sum(loss_fn(outputs, target) * mask) / sum(mask)``.

Each is one fused HIP pass per direction (csrc/refloss.hip; the formulas are in include/gwen_hip.h), differentiable in
``outputs`` and ``target`` through a ``torch.autograd.Function``; nothing synchronises with the host, so a training step
captures into a hipGraph.  Everything is fp32 on a HIP device: there is no CPU fallback (CPU tensors raise RuntimeError).
``gwen_amd.losses.EnsembleCRPSLoss`` is a different score (the fair CRPS of the members themselves, no Gaussian fit).
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
from torch import Tensor, nn
from torch.autograd.function import once_differentiable

from . import _checks

MAX_MEMBERS = 256          # of the Gaussian CRPS kernel (include/gwen_hip.h)


def _lib():
    from . import _lib as L
    return L


def _check_types(outputs: Tensor, target: Tensor, mask: Optional[Tensor] = None) -> None:
    """After the shape errors: outputs and target are float32, and everything lives on outputs' HIP device."""
    _checks.require_dtype("outputs", outputs)
    _checks.require_dtype("target", target)
    _checks.require_device(("outputs", outputs), ("target", target), ("mask", mask))


# ---- launches on preallocated buffers (contiguous fp32 on one device; tools/ref_losses_bench.py times them) -------------

def gauss_crps_workspace_floats(a: int, m: int, r: int, s: int) -> int:
    return int(_lib().lib().gwen_gauss_crps_workspace_floats(a, m, r, s))


def gauss_crps_launch(pred: Tensor, target: Tensor, a: int, m: int, r: int, s: int, loss: Tensor,
                      workspace: Tensor) -> None:
    from .graph import _ptr, _stream
    L = _lib()
    with torch.cuda.device(pred.device):
        rc = L.lib().gwen_gauss_crps_f32(_ptr(pred), _ptr(target), a, m, r, s, _ptr(loss), _ptr(workspace),
                                         workspace.numel(), _stream(pred.device))
    L.check(rc, "gwen_gauss_crps_f32")


def gauss_crps_bwd_launch(grad_loss: Tensor, pred: Tensor, target: Tensor, a: int, m: int, r: int, s: int,
                          grad_pred: Optional[Tensor], grad_target: Optional[Tensor]) -> None:
    from .graph import _ptr, _stream
    L = _lib()
    with torch.cuda.device(pred.device):
        rc = L.lib().gwen_gauss_crps_bwd_f32(_ptr(grad_loss), _ptr(pred), _ptr(target), a, m, r, s, _ptr(grad_pred),
                                             _ptr(grad_target), _stream(pred.device))
    L.check(rc, "gwen_gauss_crps_bwd_f32")


def varreg_workspace_floats(a: int, m: int, r: int) -> int:
    return int(_lib().lib().gwen_varreg_l1_workspace_floats(a, m, r))


def varreg_launch(pred: Tensor, target: Tensor, a: int, m: int, r: int, broadcast: bool, alpha: float,
                  grad_pred: Optional[Tensor], grad_target: Optional[Tensor], loss: Tensor, workspace: Tensor) -> None:
    from .graph import _ptr, _stream
    L = _lib()
    with torch.cuda.device(pred.device):
        rc = L.lib().gwen_varreg_l1_f32(_ptr(pred), _ptr(target), a, m, r, int(broadcast), float(alpha),
                                        _ptr(grad_pred), _ptr(grad_target), _ptr(loss), _ptr(workspace),
                                        workspace.numel(), _stream(pred.device))
    L.check(rc, "gwen_varreg_l1_f32")


def masked_workspace_floats(outer: int, inner: int) -> int:
    return int(_lib().lib().gwen_masked_mean_workspace_floats(outer, inner))


def masked_launch(out: Tensor, target: Tensor, mask: Tensor, outer: int, inner: int, mask_full: bool, kind: int,
                  grad_out: Optional[Tensor], grad_target: Optional[Tensor], loss: Tensor, workspace: Tensor) -> None:
    from .graph import _ptr, _stream
    L = _lib()
    with torch.cuda.device(out.device):
        rc = L.lib().gwen_masked_mean_f32(_ptr(out), _ptr(target), _ptr(mask), outer, inner, int(mask_full), int(kind),
                                          _ptr(grad_out), _ptr(grad_target), _ptr(loss), _ptr(workspace),
                                          workspace.numel(), _stream(out.device))
    L.check(rc, "gwen_masked_mean_f32")


# ---- CRPSLoss -----------------------------------------------------------------------------------------------------------

def _crps_layout(shape, dim: int) -> Tuple[bool, int, int, int, int]:
    """(direct, A, M, R, S) of a 5-D ``shape`` with members on ``dim``: the kernel reads [A, M, R] with samples of S
    consecutive points, S dividing R.  dim = 0 (A = 1) and dim = 1 (R = S) are read in place; a members axis further
    in leaves R shorter than a sample, and the tensor is moved to members-first once."""
    rest = [n for i, n in enumerate(shape) if i != dim]
    s = rest[1] * rest[2] * rest[3]
    a, r = math.prod(shape[:dim]), math.prod(shape[dim + 1:])
    if r % s == 0:
        return True, a, shape[dim], r, s
    return False, 1, shape[dim], rest[0] * s, s


class _GaussCRPS(torch.autograd.Function):
    """gwen_gauss_crps_f32 / gwen_gauss_crps_bwd_f32."""

    @staticmethod
    def forward(ctx, outputs: Tensor, target: Tensor, dim: int) -> Tensor:
        direct, a, m, r, s = _crps_layout(tuple(outputs.shape), dim)
        p = outputs.detach() if direct else outputs.detach().movedim(dim, 0)
        p, t = p.contiguous(), target.detach().contiguous()
        loss = torch.empty(a * r // s, dtype=torch.float32, device=p.device)
        ws = torch.empty(gauss_crps_workspace_floats(a, m, r, s), dtype=torch.float32, device=p.device)
        gauss_crps_launch(p, t, a, m, r, s, loss, ws)
        ctx.save_for_backward(p, t)
        ctx.layout = (direct, dim, a, m, r, s)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        p, t = ctx.saved_tensors
        direct, dim, a, m, r, s = ctx.layout
        gp = torch.empty_like(p) if ctx.needs_input_grad[0] else None
        gt = torch.empty_like(t) if ctx.needs_input_grad[1] else None
        if gp is not None or gt is not None:
            gauss_crps_bwd_launch(g.contiguous(), p, t, a, m, r, s, gp, gt)
        if gp is not None and not direct:
            gp = gp.movedim(0, dim)
        return gp, gt, None


class CRPSLoss(nn.Module):
    """The reference's CRPSLoss: ``forward(outputs [.., M, ..] 5-D, target 4-D, dim=0) -> [B]`` (module docstring).
    ``target`` has the shape ``outputs`` is left with when ``dim`` is reduced; 2 <= M <= 256."""

    def __init__(self) -> None:
        super().__init__()

    def forward(self, outputs: Tensor, target: Tensor, dim: int = 0) -> Tensor:
        _checks.require_tensors(outputs=outputs, target=target)
        if outputs.dim() != 5:
            raise ValueError(f"CRPSLoss takes 5-D outputs with the members on dim (got {outputs.dim()}-D): the mean "
                             "over the three trailing axes of the reduced tensor is defined for 4-D targets only")
        if not -5 <= dim < 5:
            raise ValueError(f"dim must lie in [-5, 4] (got {dim})")
        dim = dim % 5
        rest = tuple(n for i, n in enumerate(outputs.shape) if i != dim)
        if tuple(target.shape) != rest:
            raise ValueError(f"target must be {rest}, outputs without dim {dim}; got {tuple(target.shape)}")
        m = outputs.shape[dim]
        if m < 2:
            raise ValueError(f"CRPSLoss needs at least 2 members for a standard deviation (got {m})")
        if m > MAX_MEMBERS:
            raise ValueError(f"at most {MAX_MEMBERS} members (got {m})")
        if outputs.numel() == 0:
            raise ValueError(f"outputs is empty: {tuple(outputs.shape)}")
        _check_types(outputs, target)
        return _GaussCRPS.apply(outputs, target, dim)


# ---- EnsembleVarRegLoss -------------------------------------------------------------------------------------------------

class _VarRegL1(torch.autograd.Function):
    """gwen_varreg_l1_f32: the value and, for the inputs that need it, the gradient in the same pass."""

    @staticmethod
    def forward(ctx, outputs: Tensor, target: Tensor, alpha: float) -> Tensor:
        a, m = outputs.shape[0], outputs.shape[1]
        r = outputs.numel() // (a * m)
        p, t = outputs.detach().contiguous(), target.detach().contiguous()
        gp = torch.empty_like(p) if ctx.needs_input_grad[0] else None
        gt = torch.empty_like(t) if ctx.needs_input_grad[1] else None
        loss = torch.empty(1, dtype=torch.float32, device=p.device)
        ws = torch.empty(varreg_workspace_floats(a, m, r), dtype=torch.float32, device=p.device)
        varreg_launch(p, t, a, m, r, t.shape[1] != m, alpha, gp, gt, loss, ws)
        ctx.save_for_backward(gp, gt)
        return loss[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        gp, gt = ctx.saved_tensors
        return (gp * g if gp is not None else None), (gt * g if gt is not None else None), None


class EnsembleVarRegLoss(nn.Module):
    """The reference's EnsembleVarRegLoss: ``forward(outputs [A, M, ...], target) -> scalar``, the variance over dim 1.
    ``target`` has ``outputs``' shape or size 1 on dim 1; any other broadcastable target is expanded first."""

    def __init__(self, alpha: float = 0.1) -> None:
        super().__init__()
        self.alpha = alpha

    def forward(self, outputs: Tensor, target: Tensor) -> Tensor:
        _checks.require_tensors(outputs=outputs, target=target)
        if outputs.dim() < 2:
            raise ValueError(f"outputs needs at least 2 dims, the members on dim 1 (got {tuple(outputs.shape)})")
        if outputs.numel() == 0:
            raise ValueError(f"outputs is empty: {tuple(outputs.shape)}")
        shape = tuple(outputs.shape)
        if tuple(target.shape) != shape and tuple(target.shape) != shape[:1] + (1,) + shape[2:]:
            try:
                ok = torch.broadcast_shapes(tuple(target.shape), shape) == shape
            except RuntimeError:
                ok = False
            if not ok:
                raise ValueError(f"target {tuple(target.shape)} does not broadcast to outputs {shape}")
            target = target.expand(shape)                # autograd sums the gradient back over the expanded axes
        _check_types(outputs, target)
        return _VarRegL1.apply(outputs, target, float(self.alpha))

    def extra_repr(self) -> str:
        return f"alpha={self.alpha}"


# ---- MaskedLoss ---------------------------------------------------------------------------------------------------------

class _MaskedMean(torch.autograd.Function):
    """gwen_masked_mean_f32: the value and, for the inputs that need it, the gradient in the same pass."""

    @staticmethod
    def forward(ctx, outputs: Tensor, target: Tensor, mask: Tensor, kind: int) -> Tensor:
        o, t = outputs.detach().contiguous(), target.detach().contiguous()
        mk = mask.detach().to(torch.float32).contiguous()
        inner = mk.numel()
        outer = o.numel() // inner                       # 1: a full-shape mask
        go = torch.empty_like(o) if ctx.needs_input_grad[0] else None
        gt = torch.empty_like(t) if ctx.needs_input_grad[1] else None
        loss = torch.empty(1, dtype=torch.float32, device=o.device)
        ws = torch.empty(masked_workspace_floats(outer, inner), dtype=torch.float32, device=o.device)
        masked_launch(o, t, mk, outer, inner, outer == 1, kind, go, gt, loss, ws)
        ctx.save_for_backward(go, gt)
        return loss[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        go, gt = ctx.saved_tensors
        return (go * g if go is not None else None), (gt * g if gt is not None else None), None, None


def _fused_kind(loss_fn) -> Optional[int]:
    if getattr(loss_fn, "reduction", None) != "none":
        return None
    if type(loss_fn) is nn.L1Loss:
        return _lib().MASKED_L1
    if type(loss_fn) is nn.MSELoss:
        return _lib().MASKED_MSE
    return None


class MaskedLoss(nn.Module):
    """The reference's MaskedLoss: ``forward(outputs, target, mask) = sum(loss_fn(outputs, target) * mask) / sum(mask)``,
    where ``sum(mask)`` is the sum of the mask as given, not of its broadcast.  ``nn.L1Loss(reduction="none")`` and
    ``nn.MSELoss(reduction="none")`` with a float32 or bool mask over the trailing dims of ``outputs`` (or all of them)
    take the fused kernel; any other ``loss_fn`` or mask shape is the same expression composed from torch ops on the
    device."""

    def __init__(self, loss_fn: nn.Module) -> None:
        super().__init__()
        self.loss_fn = loss_fn

    def forward(self, outputs: Tensor, target: Tensor, mask: Tensor) -> Tensor:
        _checks.require_tensors(outputs=outputs, target=target, mask=mask)
        if outputs.numel() == 0 or mask.numel() == 0:
            raise ValueError(f"outputs {tuple(outputs.shape)} or mask {tuple(mask.shape)} is empty")
        if tuple(target.shape) != tuple(outputs.shape):
            raise ValueError(f"target must have outputs' shape {tuple(outputs.shape)}, got {tuple(target.shape)}")
        try:
            ok = torch.broadcast_shapes(tuple(mask.shape), tuple(outputs.shape)) == tuple(outputs.shape)
        except RuntimeError:
            ok = False
        if not ok:
            raise ValueError(f"mask {tuple(mask.shape)} does not broadcast to outputs {tuple(outputs.shape)}")
        if mask.requires_grad:
            raise ValueError("mask requires grad: the loss has no gradient for its mask (detach it)")
        kind = _fused_kind(self.loss_fn)
        if kind is not None:
            _checks.require_dtype("mask", mask, (torch.float32, torch.bool))
        _check_types(outputs, target, mask)
        mshape = tuple(mask.shape)
        while len(mshape) > 1 and mshape[0] == 1:        # leading ones change neither the broadcast nor the sum
            mshape = mshape[1:]
        trailing = mshape == tuple(outputs.shape)[outputs.dim() - len(mshape):]
        if kind is None or not trailing:
            loss = self.loss_fn(outputs, target)
            return torch.sum(loss * mask) / torch.sum(mask)
        return _MaskedMean.apply(outputs, target, mask, kind)
