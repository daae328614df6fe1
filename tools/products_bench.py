"""Time the fused ensemble products (gwen_ens_products_f32) and the rank histogram (gwen_ens_rank_hist_f32) against the
torch composition of the same outputs, on device events, and print one JSON line.

    python tools/products_bench.py M N C [--calls K] [--rounds R]

Products: quantiles (0.1, 0.5, 0.9), one threshold, mean and std.  The composition is ``torch.sort`` along the members
+ the "linear" interpolation, ``(pred > thr).float().mean(0)``, ``mean`` and ``std``.  Histogram: the fused call against
counting ``pred < target`` and a weighted sum per bin.  The two sides alternate, bracket by bracket, on the same
box; the figure of a side is the median of its brackets.

Compulsory bytes of the fused pass: the ensemble read once and every output written once, 4 N C (M + Q + T + 2); of the
histogram: 4 (M N C + N C + N).  The fraction is of the 8 TB/s HBM peak."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12
QUANTILES = (0.1, 0.5, 0.9)
THRESHOLD = 0.5


def torch_products(pred, q, thr):
    m = pred.shape[0]
    s, _ = torch.sort(pred, dim=0)
    pos = q * (m - 1)
    lo = pos.floor()
    frac = (pos - lo).view(-1, 1, 1)
    lo = lo.long()
    a, b = s[lo], s[(lo + 1).clamp(max=m - 1)]
    quant = a + frac * (b - a)
    prob = (pred > thr).float().mean(0, keepdim=True)
    return quant, prob, pred.mean(0), pred.std(0)


def torch_rank_hist(pred, target, w):
    m, n, c = pred.shape
    rank = (pred < target).sum(0)                                            # [N, C], tie-free inputs
    wn = w.unsqueeze(1)
    hist = torch.stack([(wn * (rank == k)).sum(0) for k in range(m + 1)], 1)  # no atomics: a pass per bin
    return hist / hist.sum(1, keepdim=True)


def bracket(fn, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls * 1e3                                 # us per call


def alternate(a, b, calls, rounds, warmup):
    for _ in range(warmup):
        a()
        b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(bracket(a, calls))
        tb.append(bracket(b, calls))
    return statistics.median(ta), statistics.median(tb)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("M", type=int)
    ap.add_argument("N", type=int)
    ap.add_argument("C", type=int)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("products_bench needs the MI355X")
    from gwen_amd import products
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(23)
    pred = torch.randn(a.M, a.N, a.C, device=dev, generator=g)
    target = torch.randn(a.N, a.C, device=dev, generator=g)
    w = torch.rand(a.N, device=dev, generator=g)
    q = torch.tensor(QUANTILES, device=dev)
    thr = torch.tensor([THRESHOLD], device=dev)
    nq, nt = q.numel(), thr.numel()
    mean, std = torch.empty(a.N, a.C, device=dev), torch.empty(a.N, a.C, device=dev)
    quant, prob = torch.empty(nq, a.N, a.C, device=dev), torch.empty(nt, a.N, a.C, device=dev)
    hist = torch.empty(a.C, a.M + 1, device=dev)
    ws = torch.empty(products.rank_hist_workspace_floats(a.M, a.N, a.C), device=dev)
    calls = max(a.calls, 50)

    def fused():
        products.products_launch(pred, q, thr, mean, std, quant, prob)

    def composed():
        torch_products(pred, q, thr)

    def fused_hist():
        products.rank_hist_launch(pred, target, w, True, hist, ws)

    def composed_hist():
        torch_rank_hist(pred, target, w)

    us_fused, us_torch = alternate(fused, composed, calls, a.rounds, a.warmup)
    us_hist, us_hist_torch = alternate(fused_hist, composed_hist, calls, a.rounds, a.warmup)
    tq, tp, tm, ts = torch_products(pred, q, thr)
    th = torch_rank_hist(pred, target, w)
    nbytes = 4 * a.N * a.C * (a.M + nq + nt + 2)
    hbytes = 4 * (a.M * a.N * a.C + a.N * a.C + a.N)
    print(json.dumps({
        "tool": "products_bench", "M": a.M, "N": a.N, "C": a.C, "calls": calls, "rounds": a.rounds,
        "products_us": round(us_fused, 1), "products_torch_us": round(us_torch, 1),
        "products_speedup": round(us_torch / us_fused, 2), "products_compulsory_bytes": nbytes,
        "products_fraction_of_8tbs_peak": round(nbytes / (us_fused * 1e-6) / PEAK_BYTES_PER_S, 3),
        "rank_hist_us": round(us_hist, 1), "rank_hist_torch_us": round(us_hist_torch, 1),
        "rank_hist_speedup": round(us_hist_torch / us_hist, 2), "rank_hist_compulsory_bytes": hbytes,
        "rank_hist_fraction_of_8tbs_peak": round(hbytes / (us_hist * 1e-6) / PEAK_BYTES_PER_S, 3),
        "max_abs_diff_vs_torch": {"quantiles": float((quant - tq).abs().max()), "prob": float((prob - tp).abs().max()),
                                  "mean": float((mean - tm).abs().max()), "std": float((std - ts).abs().max()),
                                  "rank_hist": float((hist - th).abs().max())}}), flush=True)


if __name__ == "__main__":
    main()
