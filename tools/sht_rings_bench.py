"""Time the spherical harmonic transforms on an octahedral reduced Gaussian grid (gwen_amd.spectral, csrc/sht.hip) against
the regular Gauss grid of the same latitudes, on device events, print one JSON line and append it to
profiles/sht_rings_bench.jsonl.

    python tools/sht_rings_bench.py [N] [LMAX] [C] [MEMBERS] [--calls K] [--rounds R]

Four transforms in one process, bracket after bracket in turn, the figure of each the median of its brackets:

    reduced   ``SphericalHarmonics.octahedral(N, lmax=LMAX)``                                      (ragged direct sums)
    bluestein the same grid with ``ring_longitude="bluestein"``                                    (one FFT a ring)
    direct    ``SphericalHarmonics(2 N, 4 N + 16, grid="gauss", lmax=LMAX, longitude="direct")``   (the longest ring everywhere)
    fft       the same regular grid with ``longitude="fft"`` (left out where ``4 N + 16`` is not ``2^a 3^b 5^c``)

Four operations, as tools/sht_bench.py: analysis (fp32 coefficients), synthesis, power_spectrum and analysis + backward.
The default is O320, lmax 319, 64 channels, 4 members.  ``work_ratio`` is ``sum_j ring_nlon[j] (M_j + 1) / (nlat nlon
(lmax + 1))``, the reduced grid's share of the regular grid's longitude fma, from the shapes alone;
``lon_kernel_ratio`` sets the two ragged longitude kernels' device times (one profiled call of analysis and of
synthesis) against the regular direct-sum kernels', ``lon_fft_kernel_ratio`` those of the two ragged FFT kernels against
the ragged direct sums' and, where the regular grid has an FFT, against the regular FFT kernels'."""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def bracket(fn, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls * 1e3                                 # us per call


def alternate(fns, calls, rounds, warmup):
    """Median microseconds per call of every function, their brackets taken in turn."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for t, fn in zip(times, fns):
            t.append(bracket(fn, calls))
    return [statistics.median(t) for t in times]


def kernel_times(fns) -> dict:
    """Device microseconds per kernel of csrc/sht.hip over one call of every function; {} where the profiler has none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for fn in fns:
                fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            found = re.search(r"k_v?sht_[a-z_]+", e.key)
            if found:
                total = getattr(e, "device_time_total", None)
                if total is None:
                    total = getattr(e, "cuda_time_total", 0.0)
                out[found.group(0)] = round(out.get(found.group(0), 0.0) + float(total), 1)
        return out
    except Exception as exc:                                                 # the figures are optional, the run is not
        return {"error": repr(exc)[:200]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("N", type=int, nargs="?", default=320)
    ap.add_argument("lmax", type=int, nargs="?", default=None)
    ap.add_argument("C", type=int, nargs="?", default=64)
    ap.add_argument("members", type=int, nargs="?", default=4)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sht_rings_bench needs the MI355X")
    import gwen_amd
    from gwen_amd import spectral
    dev = torch.device("cuda:0")
    nlat, nlon = 2 * a.N, 4 * a.N + 16
    L = a.N - 1 if a.lmax is None else a.lmax
    shs = {"reduced": gwen_amd.SphericalHarmonics.octahedral(a.N, dev, lmax=L),
           "bluestein": gwen_amd.SphericalHarmonics.octahedral(a.N, dev, lmax=L, ring_longitude="bluestein"),
           "direct": gwen_amd.SphericalHarmonics(nlat, nlon, dev, lmax=L, grid="gauss", longitude="direct")}
    if spectral.fft_supported(nlon):
        shs["fft"] = gwen_amd.SphericalHarmonics(nlat, nlon, dev, lmax=L, grid="gauss", longitude="fft")
    modes = list(shs)
    rings = shs["reduced"].ring_nlon
    orders = np.minimum(L, (rings - 1) // 2)
    work_ratio = float((rings * (orders + 1)).sum()) / float(nlat * nlon * (L + 1))
    g = torch.Generator(device=dev).manual_seed(23)
    B, C, T = a.members, a.C, (L + 1) ** 2
    coef = torch.randn(B, T, C, device=dev, generator=g)
    gout = torch.randn(B, T, C, device=dev, generator=g)

    def operations(s):
        x = torch.randn(B, s.rows, C, device=dev, generator=g)
        xg = x.clone().requires_grad_()

        def backward():
            xg.grad = None
            s.analysis(xg).backward(gout)

        return {"analysis": lambda: s.analysis(x), "synthesis": lambda: s.synthesis(coef),
                "power_spectrum": lambda: s.power_spectrum(x), "analysis_backward": backward}

    ops = {m: operations(shs[m]) for m in modes}
    line = {"tool": "sht_rings_bench", "N": a.N, "nlat": nlat, "points": int(rings.sum()), "regular_nlon": nlon,
            "regular_points": nlat * nlon, "lmax": L, "C": C, "members": B, "calls": a.calls, "rounds": a.rounds,
            "truncated_rings": int((orders < L).sum()), "work_ratio": round(work_ratio, 4),
            "point_ratio": round(float(rings.sum()) / (nlat * nlon), 4),
            "bluestein_rings": int(sum(spectral.ring_fft_plan(n)[0] == "bluestein" for n in rings))}
    for name in ("analysis", "synthesis", "power_spectrum", "analysis_backward"):
        times = alternate([ops[m][name] for m in modes], a.calls, a.rounds, a.warmup)
        us = dict(zip(modes, times))
        line[name] = {f"{m}_us": round(us[m], 1) for m in modes}
        line[name]["reduced_over_direct"] = round(us["reduced"] / us["direct"], 3)
        line[name]["bluestein_over_reduced"] = round(us["bluestein"] / us["reduced"], 3)
        if "fft" in us:
            line[name]["reduced_over_fft"] = round(us["reduced"] / us["fft"], 3)
            line[name]["bluestein_over_fft"] = round(us["bluestein"] / us["fft"], 3)
    kernels = {m: kernel_times([ops[m]["analysis"], ops[m]["synthesis"]]) for m in modes}
    line["kernel_us"] = kernels
    pairs = {"fwd": ("k_sht_rings_lon_fwd", "k_sht_lon_fwd"), "inv": ("k_sht_rings_lon_inv", "k_sht_lon_inv")}
    line["lon_kernel_ratio"] = {k: round(kernels["reduced"][r] / kernels["direct"][d], 4) for k, (r, d) in pairs.items()
                                if kernels["reduced"].get(r) and kernels["direct"].get(d)}
    ragged = {"fwd": ("k_sht_rings_lon_fft_fwd", "k_sht_rings_lon_fwd", "k_sht_lon_fft_fwd"),
              "inv": ("k_sht_rings_lon_fft_inv", "k_sht_rings_lon_inv", "k_sht_lon_fft_inv")}
    line["lon_fft_kernel_ratio"] = {}
    for k, (b, r, f) in ragged.items():
        own = kernels["bluestein"].get(b)
        if own and kernels["reduced"].get(r):
            line["lon_fft_kernel_ratio"][f"{k}_over_reduced"] = round(own / kernels["reduced"][r], 4)
        if own and kernels.get("fft", {}).get(f):
            line["lon_fft_kernel_ratio"][f"{k}_over_fft"] = round(own / kernels["fft"][f], 4)
    # the reduced transform of a band-limited field returns its coefficients
    for m in ("reduced", "bluestein"):
        back = shs[m].analysis(shs[m].synthesis(coef))
        line["round_trip_max_abs" if m == "reduced" else "bluestein_round_trip_max_abs"] = float((back - coef).abs().max())
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "sht_rings_bench.jsonl"), "a") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
