"""Argument checks of the ensemble losses and products (``losses``, ``products``, ``loss_functions``), in one order:
shape and argument errors first (ValueError), then dtypes (TypeError), then devices (RuntimeError).  A caller runs its
shape helpers, then ``require_dtype`` per tensor, then one ``require_device``."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor


# ---- shapes (ValueError) --------------------------------------------------------------------------------------------

def require_tensors(**named) -> None:
    for name, t in named.items():
        if not isinstance(t, Tensor):
            raise ValueError(f"{name} must be a tensor")


def require_members_first(pred: Tensor) -> None:
    if pred.dim() != 3:
        raise ValueError(f"pred must be [members, N, C], got {tuple(pred.shape)}")


def require_target_nc(pred: Tensor, target: Tensor) -> None:
    if target.dim() != 2 or tuple(target.shape) != tuple(pred.shape[1:]):
        raise ValueError(f"target must be [N, C] = {tuple(pred.shape[1:])}, got {tuple(target.shape)}")


def require_sizes(pred: Tensor, max_members: int) -> None:
    m, n, c = pred.shape
    if not 1 <= m <= max_members:
        raise ValueError(f"1 <= members <= {max_members} (got {m})")
    if n < 1 or c < 1:
        raise ValueError(f"N and C must be >= 1 (got {n}, {c})")


def require_weights(name: str, w, size: int) -> None:
    """``w`` is None or a ``[size]`` tensor."""
    if w is None:
        return
    if not isinstance(w, Tensor):
        raise ValueError(f"{name} must be a tensor or None")
    if w.dim() != 1 or w.numel() != size:
        raise ValueError(f"{name} must be [{size}], got {tuple(w.shape)}")


# ---- dtypes (TypeError), devices (RuntimeError) ---------------------------------------------------------------------

def require_dtype(name: str, t: Optional[Tensor], dtypes: Sequence[torch.dtype] = (torch.float32,)) -> None:
    if t is not None and t.dtype not in dtypes:
        raise TypeError(f"gwen_amd: {name} must be {' or '.join(str(d).replace('torch.', '') for d in dtypes)} "
                        f"(got {t.dtype})")


def require_device(*named: Tuple[str, Optional[Tensor]]) -> None:
    """Every tensor given lives on a HIP device, the first one's."""
    first_name, first = named[0]
    for name, t in named:
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"gwen_amd: {name} must live on a HIP device (no CPU fallback)")
        if t is not None and t.device != first.device:
            raise RuntimeError(f"gwen_amd: {name} is on {t.device}, {first_name} on {first.device}")
