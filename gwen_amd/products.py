"""Ensemble products and calibration over the members axis of ``pred [M, N, C]`` (what ``ensemble_forecast`` returns).

Products, one fused HIP pass that reads every point once (include/gwen_hip.h, ``gwen_ens_products_f32``):

    mean, std [N, C]        the ensemble mean and the unbiased spread of every point, from deviations about a member
    quantiles [Q, N, C]     ``numpy.quantile`` / ``torch.quantile`` with the "linear" method, sorted in registers
    prob [T, N, C]          the share of members strictly above a threshold (``[T]``, or ``[T, C]`` per channel)

Calibration (``gwen_ens_rank_hist_f32``): the rank (Talagrand) histogram ``[C, M + 1]`` of the truth among the members,
ties split by mid-rank, node weights optional, bitwise reproducible.

Nothing synchronises with the host.  ``quantiles`` / ``thresholds`` given as fp32 tensors on ``pred``'s device are used
as they are -- no copy, and their values are not read back for checking (a q outside [0, 1] then gives NaN): that is the
form to use under graph capture.  Anything else is checked, converted and copied.  There is no CPU fallback: CPU tensors
raise RuntimeError.  Results never require grad; a ``pred`` that does is read detached.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
from torch import Tensor

from . import _checks

MAX_MEMBERS = 64
MAX_QUANTILES = 32
MAX_THRESHOLDS = 32


def _check_pred(pred) -> None:
    _checks.require_tensors(pred=pred)
    _checks.require_members_first(pred)
    _checks.require_sizes(pred, MAX_MEMBERS)


def _is_device_table(t, pred: Tensor) -> bool:
    return isinstance(t, Tensor) and t.is_cuda and t.dtype == torch.float32 and t.device == pred.device


def _table(name: str, values, pred: Tensor) -> Tensor:
    """A tensor of ``values``: a device fp32 tensor as it is, anything else as fp32 on the host (copied later)."""
    if _is_device_table(values, pred):
        return values.detach()
    if isinstance(values, Tensor):
        t = values.detach().to("cpu", torch.float32)
    else:
        try:
            t = torch.as_tensor(np.asarray(values, dtype=np.float32))
        except (TypeError, ValueError) as exc:
            raise ValueError(f"{name} must be numbers, a sequence of numbers or a tensor") from exc
    return t


def _quantile_table(q, pred: Tensor) -> Tensor:
    t = _table("quantiles", q, pred)
    if t.dim() == 0:
        t = t.reshape(1)
    if t.dim() != 1 or t.numel() < 1:
        raise ValueError(f"quantiles must be [Q], Q >= 1 (got {tuple(t.shape)})")
    if t.numel() > MAX_QUANTILES:
        raise ValueError(f"at most {MAX_QUANTILES} quantiles a call (got {t.numel()})")
    if not t.is_cuda and not bool(((t >= 0) & (t <= 1)).all()):
        raise ValueError("quantiles must lie in [0, 1]")
    return t


def _threshold_table(thr, pred: Tensor) -> Tensor:
    t = _table("thresholds", thr, pred)
    if t.dim() == 0:
        t = t.reshape(1)
    c = pred.shape[2]
    if t.dim() not in (1, 2) or t.shape[0] < 1 or (t.dim() == 2 and t.shape[1] != c):
        raise ValueError(f"thresholds must be [T] or [T, C = {c}] (got {tuple(t.shape)})")
    if t.shape[0] > MAX_THRESHOLDS:
        raise ValueError(f"at most {MAX_THRESHOLDS} thresholds a call (got {t.shape[0]})")
    return t


def products_launch(pred: Tensor, q: Optional[Tensor], thr: Optional[Tensor], mean: Optional[Tensor],
                    std: Optional[Tensor], quantiles: Optional[Tensor], prob: Optional[Tensor]) -> None:
    """``gwen_ens_products_f32`` on preallocated buffers (contiguous fp32 on one device; tools/products_bench.py times
    it).  ``q [Q]``, ``thr [T]`` or ``[T, C]``."""
    from . import _lib
    from .graph import _ptr, _stream
    m, n, c = pred.shape
    dev = pred.device
    nq = 0 if q is None else q.numel()
    nt = 0 if thr is None else thr.shape[0]
    per_channel = int(thr is not None and thr.dim() == 2)
    with torch.cuda.device(dev):
        rc = _lib.lib().gwen_ens_products_f32(_ptr(pred), m, n, c, _ptr(q), nq, _ptr(thr), nt, per_channel, _ptr(mean),
                                              _ptr(std), _ptr(quantiles), _ptr(prob), _stream(dev))
    _lib.check(rc, "gwen_ens_products_f32")


def rank_hist_launch(pred: Tensor, target: Tensor, node_weights: Optional[Tensor], normalize: bool, hist: Tensor,
                     workspace: Tensor) -> None:
    """``gwen_ens_rank_hist_f32`` on preallocated buffers (contiguous fp32 on one device)."""
    from . import _lib
    from .graph import _ptr, _stream
    m, n, c = pred.shape
    dev = pred.device
    with torch.cuda.device(dev):
        rc = _lib.lib().gwen_ens_rank_hist_f32(_ptr(pred), _ptr(target), _ptr(node_weights), m, n, c, int(bool(normalize)),
                                               _ptr(hist), _ptr(workspace), workspace.numel(), _stream(dev))
    _lib.check(rc, "gwen_ens_rank_hist_f32")


def rank_hist_workspace_floats(members: int, n: int, c: int) -> int:
    from . import _lib
    return int(_lib.lib().gwen_ens_rank_hist_workspace_floats(members, n, c))


def ensemble_products(pred: Tensor, quantiles=None, thresholds=None, mean: bool = False,
                      std: bool = False) -> Dict[str, Tensor]:
    """Per-point products of ``pred [M, N, C]`` in one launch; a dict with only what was asked for:

    ``"quantiles" [Q, N, C]`` for ``quantiles`` (each in [0, 1], at most 32; the "linear" definition),
    ``"prob" [T, N, C]`` for ``thresholds`` (``[T]`` shared by the channels or ``[T, C]``, at most 32): the share of
    members strictly above, ``"mean"`` and ``"std" [N, C]`` (unbiased; NaN for one member).  A point with a NaN member
    has NaN quantiles, mean and std; ``prob`` counts it as not exceeding."""
    _check_pred(pred)
    q = None if quantiles is None else _quantile_table(quantiles, pred)
    thr = None if thresholds is None else _threshold_table(thresholds, pred)
    if q is None and thr is None and not mean and not std:
        raise ValueError("ensemble_products: nothing asked for (quantiles, thresholds, mean or std)")
    _checks.require_dtype("pred", pred)
    _checks.require_device(("pred", pred))
    p = pred.detach().contiguous()
    dev = p.device
    _, n, c = p.shape
    q = None if q is None else q.to(dev).contiguous()
    thr = None if thr is None else thr.to(dev).contiguous()
    out: Dict[str, Tensor] = {}
    if q is not None:
        out["quantiles"] = torch.empty(q.numel(), n, c, dtype=torch.float32, device=dev)
    if thr is not None:
        out["prob"] = torch.empty(thr.shape[0], n, c, dtype=torch.float32, device=dev)
    if mean:
        out["mean"] = torch.empty(n, c, dtype=torch.float32, device=dev)
    if std:
        out["std"] = torch.empty(n, c, dtype=torch.float32, device=dev)
    products_launch(p, q, thr, out.get("mean"), out.get("std"), out.get("quantiles"), out.get("prob"))
    return out


def ensemble_quantiles(pred: Tensor, q) -> Tensor:
    """``[Q, N, C]``: the quantiles ``q`` of every point over the members (``ensemble_products``)."""
    return ensemble_products(pred, quantiles=q)["quantiles"]


def exceedance_probability(pred: Tensor, thresholds) -> Tensor:
    """``[T, N, C]``: the share of members strictly above every threshold (``ensemble_products``)."""
    return ensemble_products(pred, thresholds=thresholds)["prob"]


def rank_histogram(pred: Tensor, target: Tensor, node_weights: Optional[Tensor] = None,
                   normalize: bool = True) -> Tensor:
    """The rank histogram ``[C, M + 1]`` of ``target [N, C]`` among the members of ``pred [M, N, C]``: with b members
    below the truth and t equal to it, each of the bins b..b+t receives ``w_n / (t + 1)``.  ``node_weights [N]`` (fp32,
    or a bool mask; e.g. ``Mesh.face_areas()``) default to ones; a point whose truth or any member is NaN is not
    counted.  ``normalize`` divides every channel's row by its own sum (a row that counted nothing is NaN).  Flat rows
    mean a calibrated ensemble, a U an under-dispersive one, a dome an over-dispersive one."""
    _check_pred(pred)
    _checks.require_tensors(target=target)
    _checks.require_target_nc(pred, target)
    m, n, c = pred.shape
    _checks.require_weights("node_weights", node_weights, n)
    _checks.require_dtype("pred", pred)
    _checks.require_dtype("target", target)
    _checks.require_dtype("node_weights", node_weights, (torch.float32, torch.bool))
    _checks.require_device(("pred", pred), ("target", target), ("node_weights", node_weights))
    p, t = pred.detach().contiguous(), target.detach().contiguous()
    w = None if node_weights is None else node_weights.detach().to(torch.float32).contiguous()
    hist = torch.empty(c, m + 1, dtype=torch.float32, device=p.device)
    ws = torch.empty(rank_hist_workspace_floats(m, n, c), dtype=torch.float32, device=p.device)
    rank_hist_launch(p, t, w, normalize, hist, ws)
    return hist
