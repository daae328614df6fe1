"""Time the spherical harmonic transforms (gwen_amd.spectral, csrc/sht.hip) against the torch composition of the same
outputs, on device events, print one JSON line and append it to profiles/sht_bench.jsonl.

    python tools/sht_bench.py NLAT NLON LMAX C MEMBERS [--grid equiangular] [--calls K] [--rounds R]
                              [--longitude {direct,fft,both}]

``--longitude both`` (the default) times the direct-sum and the FFT longitude stage and the composition in one process,
bracket after bracket in turn, and writes one line per longitude stage (field ``longitude``; the FFT's line also carries
``direct_us``, the other path's time from the same run).

Four operations: analysis (fp32 coefficients), synthesis, power_spectrum (fp64 on the way) and analysis + backward.  The
composition is ``torch.fft.rfft`` along the longitudes and an fp64 ``einsum`` against a Legendre table ``[m, l, lat]`` that
is made on the host outside the timed region (``irfft`` and the transposed einsum for the synthesis).  The two sides
alternate, bracket by bracket, on the same box; the figure of a side is the median of its brackets.

fp64 flops issued by the fused path, per transform: 4 B nlat nlon (lmax + 1) C along the longitudes (two fma per point
and order; with the FFT the nominal 2.5 nlon log2 nlon a ring and channel) and 2 B nlat (lmax + 1)(lmax + 2) C over the latitudes (two fma per latitude and (l, m >= 0)); the fraction
is of the 78.6 TF/s fp64 peak.  Compulsory bytes: the input read, the output written, the fp64 intermediate written and
read; the fraction is of the 8 TB/s HBM peak.  Kernel times per stage come from one profiled call of each operation;
``lon_kernel_fraction_of_8tbs`` sets the longitude kernels' compulsory bytes (x once, the ring once) against them."""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_FP64_FLOPS = 78.6e12
PEAK_BYTES_PER_S = 8.0e12


def legendre_table(sh) -> np.ndarray:
    """fp64 ``[lmax + 1 (m), lmax + 1 (l), nlat]``, zero below the diagonal: the table the composition contracts with."""
    from gwen_amd import spectral
    lat, _ = spectral.quadrature(sh.grid, sh.nlat)
    mu, cl = np.sin(np.deg2rad(lat)), np.cos(np.deg2rad(lat))
    seed = spectral.sectoral_seeds(sh.lmax)
    L = sh.lmax
    p = np.zeros((L + 1, L + 1, sh.nlat))
    for m in range(L + 1):
        p[m, m] = seed[m] * cl ** m
        for l in range(m + 1, L + 1):
            a = np.sqrt((4.0 * l * l - 1.0) / (l * l - m * m))
            b = np.sqrt(((l - 1.0) ** 2 - m * m) / (4.0 * (l - 1.0) ** 2 - 1.0))
            p[m, l] = a * (mu * p[m, l - 1] - (b * p[m, l - 2] if l >= m + 2 else 0.0))
    return p


class Composition:
    """The transforms from torch operators: coefficients as complex ``[B, l, m, C]`` (cos part real, sin part -imag)."""

    def __init__(self, sh, dev):
        from gwen_amd import spectral
        self.sh = sh
        _, w = spectral.quadrature(sh.grid, sh.nlat)
        p = torch.from_numpy(legendre_table(sh)).to(dev)
        self.p = p.to(torch.complex128)
        self.pw = (p * torch.from_numpy(w / sh.nlon).to(dev)).to(torch.complex128)
        # irfft divides by nlon and counts every order m > 0 twice
        self.scale = torch.full((sh.lmax + 1, 1), 0.5 * sh.nlon, dtype=torch.float64, device=dev)
        self.scale[0] = float(sh.nlon)

    def analysis(self, x):
        sh = self.sh
        f = torch.fft.rfft(x.reshape(-1, sh.nlat, sh.nlon, x.shape[-1]).double(), dim=2)[:, :, :sh.lmax + 1]
        return torch.einsum("mlj,bjmc->blmc", self.pw, f)

    def synthesis(self, c):
        sh = self.sh
        g = torch.einsum("mlj,blmc->bjmc", self.p, c)
        full = torch.zeros(g.shape[0], sh.nlat, sh.nlon // 2 + 1, g.shape[-1], dtype=g.dtype, device=g.device)
        full[:, :, :sh.lmax + 1] = g * self.scale
        return torch.fft.irfft(full, n=sh.nlon, dim=2).float().reshape(g.shape[0], sh.nlat * sh.nlon, -1)

    def power(self, x):
        c = self.analysis(x)
        return (c.real ** 2 + c.imag ** 2).sum(2)


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
            if "k_sht_" in e.key:
                name = e.key[e.key.index("k_sht_"):].split("(")[0].split("<")[0].split("I")[0]
                total = getattr(e, "device_time_total", None)
                if total is None:
                    total = getattr(e, "cuda_time_total", 0.0)
                out[name] = round(out.get(name, 0.0) + float(total), 1)
        return out
    except Exception as exc:                                                 # the figures are optional, the run is not
        return {"error": repr(exc)[:200]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("nlat", type=int)
    ap.add_argument("nlon", type=int)
    ap.add_argument("lmax", type=int)
    ap.add_argument("C", type=int)
    ap.add_argument("members", type=int)
    ap.add_argument("--grid", default="equiangular")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--longitude", choices=("direct", "fft", "both"), default="both")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sht_bench needs the MI355X")
    import gwen_amd
    dev = torch.device("cuda:0")
    modes = ["direct", "fft"] if a.longitude == "both" else [a.longitude]
    shs = {m: gwen_amd.SphericalHarmonics(a.nlat, a.nlon, dev, lmax=a.lmax, grid=a.grid, longitude=m) for m in modes}
    sh = shs[modes[-1]]
    comp = Composition(sh, dev)
    g = torch.Generator(device=dev).manual_seed(23)
    B, N, T, L, C = a.members, a.nlat * a.nlon, sh.num_coefficients, sh.lmax, a.C
    x = torch.randn(B, N, C, device=dev, generator=g)
    coef = torch.randn(B, T, C, device=dev, generator=g)
    gout = torch.randn(B, T, C, device=dev, generator=g)
    ccoef = comp.analysis(x)
    cgout = torch.randn_like(ccoef.real).to(ccoef.dtype)
    xc = x.clone().requires_grad_()

    def fused(s):
        xg = x.clone().requires_grad_()

        def backward():
            xg.grad = None
            s.analysis(xg).backward(gout)

        return {"analysis": lambda: s.analysis(x), "synthesis": lambda: s.synthesis(coef),
                "power_spectrum": lambda: s.power_spectrum(x), "analysis_backward": backward}

    def composed_backward():
        xc.grad = None
        comp.analysis(xc).backward(cgout)

    ops = {m: fused(shs[m]) for m in modes}
    composed = {"analysis": lambda: comp.analysis(x), "synthesis": lambda: comp.synthesis(ccoef),
                "power_spectrum": lambda: comp.power(x), "analysis_backward": composed_backward}
    lon_flops = {"direct": 4.0 * B * a.nlat * a.nlon * (L + 1) * C,
                 "fft": 2.5 * a.nlon * math.log2(max(a.nlon, 2)) * B * a.nlat * C}
    lat_flops = 2.0 * B * a.nlat * (L + 1) * (L + 2) * C
    ring_bytes = 8.0 * B * a.nlat * (2 * L + 1) * C
    nbytes = {"analysis": 4.0 * B * N * C + 4.0 * B * T * C + 2 * ring_bytes}
    nbytes["synthesis"] = nbytes["analysis"]
    nbytes["power_spectrum"] = 4.0 * B * N * C + 2 * 8.0 * B * T * C + 8.0 * B * (L + 1) * C + 2 * ring_bytes
    nbytes["analysis_backward"] = 2 * nbytes["analysis"]
    passes = {"analysis": 1, "synthesis": 1, "power_spectrum": 1, "analysis_backward": 2}
    lines = {m: {"tool": "sht_bench", "longitude": m, "grid": a.grid, "nlat": a.nlat, "nlon": a.nlon, "lmax": L, "C": C,
                 "members": B, "calls": a.calls, "rounds": a.rounds, "flops_longitude_stage": lon_flops[m],
                 "flops_latitude_stage": lat_flops} for m in modes}
    for name in composed:
        times = alternate([ops[m][name] for m in modes] + [composed[name]], a.calls, a.rounds, a.warmup)
        us_torch = times[-1]
        for m, us in zip(modes, times):
            flops = passes[name] * (lon_flops[m] + lat_flops)
            lines[m][name] = {"us": round(us, 1), "torch_us": round(us_torch, 1), "speedup": round(us_torch / us, 3),
                              "fraction_of_fp64_peak": round(flops / (us * 1e-6) / PEAK_FP64_FLOPS, 4),
                              "fraction_of_8tbs_peak": round(nbytes[name] / (us * 1e-6) / PEAK_BYTES_PER_S, 4)}
            if m == "fft" and "direct" in modes:
                lines[m][name]["direct_us"] = round(times[0], 1)
                lines[m][name]["fft_over_direct"] = round(us / times[0], 3)
    lon_bytes = 4.0 * B * N * C + ring_bytes                                 # x once, the ring once
    for m in modes:
        kernels = kernel_times([ops[m]["analysis"], ops[m]["synthesis"]])
        lines[m]["kernel_us"] = kernels
        stage = {k: v for k, v in kernels.items() if k.startswith("k_sht_lon") and isinstance(v, float) and v > 0}
        lines[m]["lon_kernel_fraction_of_8tbs"] = {k: round(lon_bytes / (v * 1e-6) / PEAK_BYTES_PER_S, 4)
                                                   for k, v in stage.items()}
    want = comp.analysis(x)
    rows = torch.arange(L + 1, device=dev)
    for mode in modes:
        got = shs[mode].analysis(x, dtype=torch.float64)
        diff = 0.0
        for m in (0, 1, L):                                                  # a few orders against the composition
            r = rows[m:] ** 2 + rows[m:]
            diff = max(diff, float((got[:, r + m] - want[:, m:, m].real).abs().max()),
                       float((got[:, r - m] + want[:, m:, m].imag).abs().max()) if m else 0.0)
        lines[mode]["max_abs_diff_vs_torch"] = diff
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    for mode in modes:
        text = json.dumps(lines[mode])
        print(text, flush=True)
        with open(os.path.join(ROOT, "profiles", "sht_bench.jsonl"), "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
