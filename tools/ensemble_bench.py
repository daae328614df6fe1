"""Time gwen_ens_crps_f32 (the ensemble CRPS pass, gwen_amd.losses) on device events and print one JSON line.

    python tools/ensemble_bench.py M N C [--grad] [--target-grad] [--alpha A] [--calls K]

Compulsory bytes: the ensemble, the truth and the weights read once (4 (M N C + N C + N + C)), plus the gradient
written (4 M N C with --grad, 4 N C with --target-grad).  The fraction is of the 8 TB/s HBM peak."""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("M", type=int)
    ap.add_argument("N", type=int)
    ap.add_argument("C", type=int)
    ap.add_argument("--grad", action="store_true")
    ap.add_argument("--target-grad", action="store_true")
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_bench needs the MI355X")
    from gwen_amd import losses
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(23)
    pred = torch.randn(a.M, a.N, a.C, device=dev, generator=g)
    target = torch.randn(a.N, a.C, device=dev, generator=g)
    w = torch.rand(a.N, device=dev, generator=g)
    v = torch.rand(a.C, device=dev, generator=g)
    gp = torch.empty_like(pred) if a.grad else None
    gt = torch.empty_like(target) if a.target_grad else None
    loss = torch.empty(1, device=dev)
    scores = torch.empty(3, a.C, device=dev)
    ws = torch.empty(losses.workspace_floats(a.M, a.N, a.C), device=dev)
    coef = losses.pair_coef(a.M, a.alpha) if a.M > 1 or a.alpha == 0 else 0.0

    def call():
        losses.crps_launch(pred, target, w, v, coef, gp, gt, loss, scores, ws)

    for _ in range(a.warmup):
        call()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls = max(a.calls, 100)
    t0.record()
    for _ in range(calls):
        call()
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / calls
    nbytes = 4 * (a.M * a.N * a.C + a.N * a.C + a.N + a.C)
    nbytes += 4 * a.M * a.N * a.C if a.grad else 0
    nbytes += 4 * a.N * a.C if a.target_grad else 0
    print(json.dumps({"tool": "ensemble_bench", "M": a.M, "N": a.N, "C": a.C, "grad": a.grad,
                      "target_grad": a.target_grad, "alpha": a.alpha, "calls": calls, "ms_per_call": round(ms, 4),
                      "compulsory_bytes": nbytes, "tb_per_s": round(nbytes / ms / 1e9, 3),
                      "fraction_of_8tbs_peak": round(nbytes / (ms * 1e-3) / PEAK_BYTES_PER_S, 3),
                      "loss": float(loss)}), flush=True)


if __name__ == "__main__":
    main()
