"""Time the entry points behind gwen_amd.loss_functions (csrc/refloss.hip) on device events, beside the same expressions composed
from torch ops in the same process, and print one JSON line per member count.

    python tools/ref_losses_bench.py [--members 4,8,16,32] [--n 200000] [--c 256] [--window-ms W] [--rounds R]

Shapes: CRPSLoss on [M, 1, 1, N, C] (one sample of N C points), EnsembleVarRegLoss on [1, M, N C] against a [1, 1, N C]
target.  Every figure is the time of one CALL of a C entry point on preallocated buffers by device events -- the pass and
its finishing launch together (two launches per entry; the backward is one), not a single kernel's time from a
profiler.  A bracket is as many back-to-back calls as fill ``--window-ms`` (250 ms; sized from a warm probe), after a
warm-up; per entry the median over ``--rounds`` brackets is ``*_us``, the extremes ``*_us_min`` / ``*_us_max``.  The
fraction of the 8 TB/s HBM peak is by compulsory bytes over the median, with P = N C points --
    forward alone                 4 (M + 1) P        (the ensemble and the target read once)
    with gradient                 4 (2 M + 1) P      (... and grad_pred written; + 4 P with grad_target)
For CRPSLoss "with gradient" is the backward launch, which reads the ensemble again; the var-reg kernel gives value and
gradient in one pass.  ``*_torch_us`` is the torch composition on the same tensors (forward under no_grad; forward and
backward for the gradient rows, against our forward + backward), ``*_speedup`` their ratio."""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
from torch.distributions import Normal  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12


class Timing(float):
    """the median of the brackets in us, with their extremes and the calls per bracket"""
    lo = hi = 0.0
    calls = 0


def _bracket_us(fn, calls: int) -> float:
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls


def timed_us(fn, window_ms: float, rounds: int, warmup: int = 2) -> Timing:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    probe = _bracket_us(fn, 3)
    calls = max(3, math.ceil(window_ms * 1e3 / probe))
    out = [_bracket_us(fn, calls) for _ in range(rounds)]
    t = Timing(statistics.median(out))
    t.lo, t.hi, t.calls = min(out), max(out), calls
    return t


def torch_crps(x, t):
    mu, sigma = torch.mean(x, dim=0), torch.std(x, dim=0) + 1e-6
    return torch.mean((Normal(mu, sigma).cdf(t) - 0.5) ** 2, dim=[1, 2, 3])


def torch_varreg(x, t, alpha):
    return torch.mean(torch.abs(x - t)) - alpha * torch.mean(torch.var(x, dim=1))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", default="4,8,16,32")
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--c", type=int, default=256)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--alpha", type=float, default=0.1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ref_losses_bench needs the MI355X")
    from gwen_amd import loss_functions as LF
    dev = torch.device("cuda:0")
    P = a.n * a.c
    for M in (int(m) for m in a.members.split(",")):
        g = torch.Generator(device=dev).manual_seed(23)
        x = torch.randn(M, P, device=dev, generator=g)
        t = torch.randn(P, device=dev, generator=g)
        gp, gt = torch.empty_like(x), torch.empty_like(t)
        loss, up = torch.empty(1, device=dev), torch.ones(1, device=dev)
        ws = torch.empty(max(LF.gauss_crps_workspace_floats(1, M, P, P), LF.varreg_workspace_floats(1, M, P)), device=dev)
        fwd_bytes, grad_bytes = 4 * (M + 1) * P, 4 * (2 * M + 1) * P
        rec = {"tool": "ref_losses_bench", "M": M, "N": a.n, "C": a.c, "points": P, "window_ms": a.window_ms, "rounds": a.rounds,
               "timing": "per call of the C entry (pass + finish launch), device events"}

        def spread(name, us):
            rec[f"{name}_us"] = round(us, 1)
            rec[f"{name}_us_min"], rec[f"{name}_us_max"] = round(us.lo, 1), round(us.hi, 1)
            rec[f"{name}_calls_per_bracket"] = us.calls

        def put(name, us, nbytes):
            spread(name, us)
            rec[f"{name}_compulsory_bytes"] = nbytes
            rec[f"{name}_fraction_of_8tbs_peak"] = round(nbytes / (us * 1e-6) / PEAK_BYTES_PER_S, 3)

        crps_fwd = timed_us(lambda: LF.gauss_crps_launch(x, t, 1, M, P, P, loss, ws), a.window_ms, a.rounds)
        rec["crps_value"] = float(loss)
        crps_bwd = timed_us(lambda: LF.gauss_crps_bwd_launch(up, x, t, 1, M, P, P, gp, None), a.window_ms, a.rounds)
        crps_bwd_t = timed_us(lambda: LF.gauss_crps_bwd_launch(up, x, t, 1, M, P, P, gp, gt), a.window_ms, a.rounds)
        put("crps_forward", crps_fwd, fwd_bytes)
        put("crps_backward", crps_bwd, grad_bytes)
        put("crps_backward_with_grad_target", crps_bwd_t, grad_bytes + 4 * P)
        var_fwd = timed_us(lambda: LF.varreg_launch(x, t, 1, M, P, True, a.alpha, None, None, loss, ws), a.window_ms, a.rounds)
        rec["varreg_value"] = float(loss)
        var_grad = timed_us(lambda: LF.varreg_launch(x, t, 1, M, P, True, a.alpha, gp, None, loss, ws), a.window_ms, a.rounds)
        var_grad_t = timed_us(lambda: LF.varreg_launch(x, t, 1, M, P, True, a.alpha, gp, gt, loss, ws), a.window_ms, a.rounds)
        put("varreg_forward", var_fwd, fwd_bytes)
        put("varreg_with_gradient", var_grad, grad_bytes)
        put("varreg_with_gradient_and_grad_target", var_grad_t, grad_bytes + 4 * P)
        del gp, gt

        # the torch compositions, same tensors, same process
        x5, t4 = x.view(M, 1, 1, a.n, a.c), t.view(1, 1, a.n, a.c)
        x3, t3 = x.view(1, M, P), t.view(1, 1, P)

        def torch_step(fn, xs):
            xs.grad = None
            fn().sum().backward()

        with torch.no_grad():
            rec["crps_torch_value"] = float(torch_crps(x5, t4))
            rec["varreg_torch_value"] = float(torch_varreg(x3, t3, a.alpha))
            tc_fwd = timed_us(lambda: torch_crps(x5, t4), a.window_ms, a.rounds, warmup=1)
            tv_fwd = timed_us(lambda: torch_varreg(x3, t3, a.alpha), a.window_ms, a.rounds, warmup=1)
        xg = x5.detach().requires_grad_()
        tc_step = timed_us(lambda: torch_step(lambda: torch_crps(xg, t4), xg), a.window_ms, a.rounds, warmup=1)
        xg.grad = None
        xv = x3.detach().requires_grad_()
        tv_step = timed_us(lambda: torch_step(lambda: torch_varreg(xv, t3, a.alpha), xv), a.window_ms, a.rounds, warmup=1)
        xv.grad = None
        for name, us in (("crps_forward_torch", tc_fwd), ("crps_step_torch", tc_step),
                         ("varreg_forward_torch", tv_fwd), ("varreg_step_torch", tv_step)):
            spread(name, us)
        rec.update({"crps_forward_speedup": round(tc_fwd / crps_fwd, 2),
                    "crps_step_us": round(crps_fwd + crps_bwd, 1),
                    "crps_step_speedup": round(tc_step / (crps_fwd + crps_bwd), 2),
                    "varreg_forward_speedup": round(tv_fwd / var_fwd, 2),
                    "varreg_step_speedup": round(tv_step / var_grad, 2)})
        print(json.dumps(rec), flush=True)
        del x, t, x5, t4, x3, t3, xg, xv
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
