"""fp64 reference of the ensemble CRPS (gwen_amd.losses): the pairwise formula, in chunks of points so that 64 members
fit in memory, and the sorted (mid-rank) form it must agree with."""
from __future__ import annotations

import torch


def pair_coef(m: int, alpha: float) -> float:
    return (alpha / (2.0 * m * (m - 1)) if alpha > 0 else 0.0) + (1.0 - alpha) / (2.0 * m * m)


def crps_points(pred: torch.Tensor, target: torch.Tensor, alpha: float = 1.0, chunk: int = 4096) -> torch.Tensor:
    """CRPS_alpha of every point, [N, C] fp64, by the pairwise formula (differentiable)."""
    x, y = pred.double(), target.double()
    m = x.size(0)
    k = pair_coef(m, alpha)
    out = []
    for lo in range(0, x.size(1), chunk):
        xs, ys = x[:, lo:lo + chunk], y[lo:lo + chunk]
        skill = (xs - ys.unsqueeze(0)).abs().mean(0)
        pair = (xs.unsqueeze(0) - xs.unsqueeze(1)).abs().sum((0, 1))
        out.append(skill - k * pair)
    return torch.cat(out, 0)


def crps_points_sorted(pred: torch.Tensor, target: torch.Tensor, alpha: float = 1.0) -> torch.Tensor:
    """The same by sorting: sum_i sum_j |x_i - x_j| = 2 sum_k (2k - M + 1) x_(k) (0-based)."""
    x, y = pred.double(), target.double()
    m = x.size(0)
    s, _ = torch.sort(x, dim=0)
    coef = (2.0 * torch.arange(m, dtype=torch.float64) - m + 1).view(m, 1, 1)
    pair = 2.0 * (coef * s).sum(0)
    return (x - y.unsqueeze(0)).abs().mean(0) - pair_coef(m, alpha) * pair


def midrank_count_difference(pred: torch.Tensor) -> torch.Tensor:
    """#{x_j < x_i} - #{x_j > x_i} = 2 midrank(x_i) - M - 1 (1-based), from a sort: [M, N, C]."""
    x = pred.double()
    m = x.size(0)
    s, _ = torch.sort(x, dim=0)
    less = torch.searchsorted(s.permute(1, 2, 0).contiguous(), x.permute(1, 2, 0).contiguous(), right=False)
    leq = torch.searchsorted(s.permute(1, 2, 0).contiguous(), x.permute(1, 2, 0).contiguous(), right=True)
    mid = (less + leq + 1).double() / 2.0                              # 1-based mid-rank
    return (2.0 * mid - m - 1).permute(2, 0, 1)


def count_difference(pred: torch.Tensor) -> torch.Tensor:
    """The same by counting, O(M^2)."""
    x = pred.double()
    d = x.unsqueeze(1) - x.unsqueeze(0)                                # [i, j]: x_i - x_j
    return torch.sign(d).sum(1)


def reference(pred, target, node_weights=None, channel_weights=None, alpha: float = 1.0):
    """(loss, scores [3, C]) in fp64, differentiable in pred / target when they require grad."""
    x, y = pred.double(), target.double()
    m, n, c = x.shape
    w = torch.ones(n, dtype=torch.float64) if node_weights is None else node_weights.double().cpu()
    v = torch.ones(c, dtype=torch.float64) if channel_weights is None else channel_weights.double().cpu()
    w, v = w.to(x.device), v.to(x.device)
    crps = crps_points(x, y, alpha)
    sw = w.sum()
    crps_c = (w.unsqueeze(1) * crps).sum(0) / sw
    mse_c = (w.unsqueeze(1) * (x.mean(0) - y) ** 2).sum(0) / sw
    var_c = (w.unsqueeze(1) * x.var(0, unbiased=True)).sum(0) / sw if m > 1 else \
        torch.full((c,), float("nan"), dtype=torch.float64, device=x.device)
    loss = (v * crps_c).sum() / v.sum()
    return loss, torch.stack([crps_c, mse_c, var_c])
