"""fp64 restatements of the ensemble products and the rank histogram (gwen_amd.products), on the fp32 inputs upcast:
the "linear" quantile from a sort, the exceedance counts, mean / std, and the tie-splitting histogram."""
from __future__ import annotations

import torch


def _q64(q) -> torch.Tensor:
    """q as the kernel sees it: the fp32 value, upcast."""
    return torch.as_tensor(q, dtype=torch.float32).reshape(-1).double()


def quantile_parts(pred: torch.Tensor, q):
    """(value, s[lo], s[lo + 1]) of every quantile, [Q, N, C] fp64 each: pos = q (M - 1), lo = floor(pos),
    frac = pos - lo; s[lo] copied when frac == 0, else s[lo] + frac (s[lo + 1] - s[lo])."""
    x = pred.double()
    m = x.size(0)
    s, _ = torch.sort(x, dim=0)
    vals, los, his = [], [], []
    for qv in _q64(q).tolist():
        pos = qv * (m - 1)
        lo = int(pos // 1)
        frac = pos - lo
        a, b = s[lo], s[min(lo + 1, m - 1)]
        vals.append(a.clone() if frac == 0 else a + frac * (b - a))
        los.append(a)
        his.append(b)
    return torch.stack(vals), torch.stack(los), torch.stack(his)


def quantiles(pred: torch.Tensor, q) -> torch.Tensor:
    return quantile_parts(pred, q)[0]


def exceedance_counts(pred: torch.Tensor, thresholds) -> torch.Tensor:
    """#{i : x_i > thr}, [T, N, C] fp64 (integers); thresholds [T] or [T, C].  NaN members do not exceed."""
    x = pred.double()
    t = torch.as_tensor(thresholds, dtype=torch.float32).double()
    t = t.reshape(-1, 1, 1) if t.dim() < 2 else t.unsqueeze(1)
    return (x.unsqueeze(0) > t.unsqueeze(1)).double().sum(1)


def exceedance(pred: torch.Tensor, thresholds) -> torch.Tensor:
    return exceedance_counts(pred, thresholds) / pred.size(0)


def mean_std(pred: torch.Tensor):
    x = pred.double()
    m = x.size(0)
    std = x.std(0, unbiased=True) if m > 1 else torch.full(x.shape[1:], float("nan"), dtype=torch.float64)
    return x.mean(0), std


def rank_histogram(pred: torch.Tensor, target: torch.Tensor, node_weights=None) -> torch.Tensor:
    """[C, M + 1] fp64, not normalised: with b = #{x_i < y} and t = #{x_i == y}, the bins b..b+t receive w / (t + 1)
    each; points with a NaN truth or member are left out."""
    x, y = pred.double(), target.double()
    m, n, c = x.shape
    w = torch.ones(n, dtype=torch.float64) if node_weights is None else node_weights.double()
    b = (x < y).sum(0)
    t = (x == y).sum(0)
    ok = ~(torch.isnan(y) | torch.isnan(x).any(0))
    share = w.unsqueeze(1) / (t + 1).double()
    hist = torch.zeros(c, m + 1, dtype=torch.float64)
    for k in range(m + 1):
        hit = ok & (b <= k) & (k <= b + t)
        hist[:, k] = torch.where(hit, share, torch.zeros_like(share)).sum(0)
    return hist


def counted_weight(pred: torch.Tensor, target: torch.Tensor, node_weights=None) -> torch.Tensor:
    """[C] fp64: the weight of the points the histogram counts."""
    n = pred.size(1)
    w = torch.ones(n, dtype=torch.float64) if node_weights is None else node_weights.double()
    ok = ~(torch.isnan(target) | torch.isnan(pred).any(0))
    return (w.unsqueeze(1) * ok.double()).sum(0)
