"""Time the vector spherical harmonic transforms (gwen_amd.spectral, csrc/sht.hip) against the torch composition of the
same outputs, on device events, print one JSON line a shape and append it to profiles/vsht_bench.jsonl.

    python tools/vsht_bench.py                                  the four standard shapes: 721 x 1440 lmax 360 and
                                                                361 x 720 lmax 180, 16 and 64 channels, 4 members
    python tools/vsht_bench.py NLAT NLON LMAX C MEMBERS [--grid equiangular] [--calls K] [--rounds R]
                               [--longitude {direct,fft,both}]

``--longitude both`` (the default) times the direct-sum and the FFT longitude stage and the composition in one process,
bracket after bracket in turn, and writes one line per longitude stage (field ``longitude``; the FFT's line also carries
``direct_us``, the other path's time from the same run).

Four operations: vector_analysis (fp32 coefficients), vector_synthesis, kinetic_energy_spectrum (fp64 on the way) and
vector_analysis + backward.  The composition is ``torch.fft.rfft`` along the longitudes of u and v and fp64 ``einsum``s
against the tables ``m Q`` and ``D`` ``[m, l, lat]`` that are made on the host outside the timed region (``irfft`` and the
transposed einsums for the synthesis).  With z = cos part - i sin part of an order:  vort = D.Fu + i mQ.Fv,
div = i mQ.Fu - D.Fv;  U = -D.psi + i mQ.chi,  V = i mQ.psi + D.chi.  The two sides alternate, bracket by bracket, on the
same box; the figure of a side is the median of its brackets.

fp64 flops issued by the fused path, per transform: 8 B nlat nlon (lmax + 1) C along the longitudes (u and v, two fma per
point and order) and 8 B nlat (lmax + 1)(lmax + 2) C over the latitudes (eight fma per latitude and (l, m >= 0)); the
fraction is of the 78.6 TF/s fp64 peak.  Compulsory bytes: the inputs read, the outputs written, the fp64 intermediate
written and read; the fraction is of the 8 TB/s HBM peak.  Kernel times per stage come from one profiled call of the
analysis and of the synthesis."""
from __future__ import annotations

import argparse
import json
import math
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_FP64_FLOPS = 78.6e12
PEAK_BYTES_PER_S = 8.0e12
STANDARD = [(721, 1440, 360, 16, 4), (721, 1440, 360, 64, 4), (361, 720, 180, 16, 4), (361, 720, 180, 64, 4)]


def vector_tables(sh):
    """fp64 ``(m Q, D)``, ``[lmax + 1 (m), lmax + 1 (l), nlat]`` each, zero below the diagonal."""
    from gwen_amd import spectral
    lat, _ = spectral.quadrature(sh.grid, sh.nlat)
    mu, cl = np.sin(np.deg2rad(lat)), np.cos(np.deg2rad(lat))
    seed = spectral.sectoral_seeds(max(sh.lmax, 1))
    L = sh.lmax
    mq = np.zeros((L + 1, L + 1, sh.nlat))
    d = np.zeros((L + 1, L + 1, sh.nlat))
    for m in range(L + 1):
        mm = max(m, 1)                                          # order 0 walks Pbar_l^1: D_l^0 = sqrt(l (l + 1) / 2) Pbar_l^1
        p1, p2 = seed[mm] * cl ** (m - 1 if m else 1), np.zeros_like(mu)
        for l in range(mm, L + 1):
            if l > mm:
                a = np.sqrt((4.0 * l * l - 1.0) / (l * l - mm * mm))
                b = np.sqrt(((l - 1.0) ** 2 - mm * mm) / (4.0 * (l - 1.0) ** 2 - 1.0))
                p1, p2 = a * (mu * p1 - b * p2), p1
            if m:
                mq[m, l] = m * p1
                d[m, l] = np.sqrt((2.0 * l + 1.0) * (l * l - m * m) / (2.0 * l - 1.0)) * p2 - l * mu * p1
            else:
                d[m, l] = np.sqrt(l * (l + 1.0) / 2.0) * p1
    return mq, d


class Composition:
    """The vector transforms from torch operators: coefficients as complex ``[B, l, m, C]`` (cos part real, sin part
    -imag)."""

    def __init__(self, sh, dev):
        from gwen_amd import spectral
        self.sh = sh
        _, w = spectral.quadrature(sh.grid, sh.nlat)
        mq, d = (torch.from_numpy(t).to(dev) for t in vector_tables(sh))
        wq = torch.from_numpy(w / sh.nlon).to(dev)
        self.q, self.d = (1j * mq).to(torch.complex128), d.to(torch.complex128)          # i m Q, D
        self.qw, self.dw = (1j * mq * wq).to(torch.complex128), (d * wq).to(torch.complex128)
        l = torch.arange(sh.lmax + 1, dtype=torch.float64, device=dev)
        big = l * (l + 1.0)
        self.inv_l = torch.where(big > 0, -1.0 / big.clamp(min=1.0), torch.zeros_like(big))[None, :, None, None]
        self.half_inv_l = -0.5 * self.inv_l[..., 0]
        # irfft divides by nlon and counts every order m > 0 twice
        self.scale = torch.full((sh.lmax + 1, 1), 0.5 * sh.nlon, dtype=torch.float64, device=dev)
        self.scale[0] = float(sh.nlon)

    def _rfft(self, x):
        sh = self.sh
        return torch.fft.rfft(x.reshape(-1, sh.nlat, sh.nlon, x.shape[-1]).double(), dim=2)[:, :, :sh.lmax + 1]

    def _irfft(self, g):
        sh = self.sh
        full = torch.zeros(g.shape[0], sh.nlat, sh.nlon // 2 + 1, g.shape[-1], dtype=g.dtype, device=g.device)
        full[:, :, :sh.lmax + 1] = g * self.scale
        return torch.fft.irfft(full, n=sh.nlon, dim=2).float().reshape(g.shape[0], sh.nlat * sh.nlon, -1)

    def analysis(self, u, v):
        fu, fv = self._rfft(u), self._rfft(v)
        vort = torch.einsum("mlj,bjmc->blmc", self.dw, fu) + torch.einsum("mlj,bjmc->blmc", self.qw, fv)
        div = torch.einsum("mlj,bjmc->blmc", self.qw, fu) - torch.einsum("mlj,bjmc->blmc", self.dw, fv)
        return vort, div

    def synthesis(self, vort, div):
        psi, chi = vort * self.inv_l, div * self.inv_l
        gu = torch.einsum("mlj,blmc->bjmc", self.q, chi) - torch.einsum("mlj,blmc->bjmc", self.d, psi)
        gv = torch.einsum("mlj,blmc->bjmc", self.q, psi) + torch.einsum("mlj,blmc->bjmc", self.d, chi)
        return self._irfft(gu), self._irfft(gv)

    def energy(self, u, v):
        vort, div = self.analysis(u, v)
        return (vort.real ** 2 + vort.imag ** 2 + div.real ** 2 + div.imag ** 2).sum(2) * self.half_inv_l


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
            hit = re.search(r"k_v?sht_(lon|lat)_(fft_)?(fwd|inv)", e.key)
            if hit:
                total = getattr(e, "device_time_total", None)
                if total is None:
                    total = getattr(e, "cuda_time_total", 0.0)
                out[hit.group(0)] = round(out.get(hit.group(0), 0.0) + float(total), 1)
        return out
    except Exception as exc:                                                 # the figures are optional, the run is not
        return {"error": repr(exc)[:200]}


def run(nlat, nlon, lmax, C, members, grid, calls, rounds, warmup, longitude="both") -> list:
    """One line per longitude stage."""
    import gwen_amd
    dev = torch.device("cuda:0")
    modes = ["direct", "fft"] if longitude == "both" else [longitude]
    shs = {m: gwen_amd.SphericalHarmonics(nlat, nlon, dev, lmax=lmax, grid=grid, workspace_bytes=4 << 30, longitude=m)
           for m in modes}
    sh = shs[modes[-1]]
    comp = Composition(sh, dev)
    g = torch.Generator(device=dev).manual_seed(29)
    B, N, T, L = members, nlat * nlon, sh.num_coefficients, sh.lmax
    u, v = torch.randn(B, N, C, device=dev, generator=g), torch.randn(B, N, C, device=dev, generator=g)
    vort, div = torch.randn(B, T, C, device=dev, generator=g), torch.randn(B, T, C, device=dev, generator=g)
    gv, gd = torch.randn(B, T, C, device=dev, generator=g), torch.randn(B, T, C, device=dev, generator=g)
    cvort, cdiv = comp.analysis(u, v)
    cgv, cgd = torch.randn_like(cvort.real).to(cvort.dtype), torch.randn_like(cvort.real).to(cvort.dtype)
    uc, vc = u.clone().requires_grad_(), v.clone().requires_grad_()

    def fused(s):
        ug, vg = u.clone().requires_grad_(), v.clone().requires_grad_()

        def backward():
            ug.grad = vg.grad = None
            torch.autograd.backward(s.vector_analysis(ug, vg), [gv, gd])

        return {"vector_analysis": lambda: s.vector_analysis(u, v),
                "vector_synthesis": lambda: s.vector_synthesis(vort, div),
                "kinetic_energy_spectrum": lambda: s.kinetic_energy_spectrum(u=u, v=v),
                "vector_analysis_backward": backward}

    def composed_backward():
        uc.grad = vc.grad = None
        torch.autograd.backward(comp.analysis(uc, vc), [cgv, cgd])

    ops = {m: fused(shs[m]) for m in modes}
    composed = {"vector_analysis": lambda: comp.analysis(u, v), "vector_synthesis": lambda: comp.synthesis(cvort, cdiv),
                "kinetic_energy_spectrum": lambda: comp.energy(u, v), "vector_analysis_backward": composed_backward}
    lon_flops = {"direct": 8.0 * B * nlat * nlon * (L + 1) * C,
                 "fft": 2 * 2.5 * nlon * math.log2(max(nlon, 2)) * B * nlat * C}
    lat_flops = 8.0 * B * nlat * (L + 1) * (L + 2) * C
    ring_bytes = 2 * 8.0 * B * nlat * (2 * L + 1) * C
    nbytes = {"vector_analysis": 2 * 4.0 * B * N * C + 2 * 4.0 * B * T * C + 2 * ring_bytes}
    nbytes["vector_synthesis"] = nbytes["vector_analysis"]
    nbytes["kinetic_energy_spectrum"] = (2 * 4.0 * B * N * C + 2 * 2 * 8.0 * B * T * C + 4 * 8.0 * B * (L + 1) * C
                                         + 2 * ring_bytes)
    nbytes["vector_analysis_backward"] = 2 * nbytes["vector_analysis"]
    passes = {"vector_analysis": 1, "vector_synthesis": 1, "kinetic_energy_spectrum": 1, "vector_analysis_backward": 2}
    lines = {m: {"tool": "vsht_bench", "longitude": m, "grid": grid, "nlat": nlat, "nlon": nlon, "lmax": L, "C": C,
                 "members": B, "calls": calls, "rounds": rounds, "flops_longitude_stage": lon_flops[m],
                 "flops_latitude_stage": lat_flops, "composition_table_bytes": 4 * comp.q.numel() * 16} for m in modes}
    for name in composed:
        times = alternate([ops[m][name] for m in modes] + [composed[name]], calls, rounds, warmup)
        us_torch = times[-1]
        for m, us in zip(modes, times):
            flops = passes[name] * (lon_flops[m] + lat_flops)
            lines[m][name] = {"us": round(us, 1), "torch_us": round(us_torch, 1), "speedup": round(us_torch / us, 3),
                              "faster": "fused" if us < us_torch else "torch",
                              "fraction_of_fp64_peak": round(flops / (us * 1e-6) / PEAK_FP64_FLOPS, 4),
                              "fraction_of_8tbs_peak": round(nbytes[name] / (us * 1e-6) / PEAK_BYTES_PER_S, 4)}
            if m == "fft" and "direct" in modes:
                lines[m][name]["direct_us"] = round(times[0], 1)
                lines[m][name]["fft_over_direct"] = round(us / times[0], 3)
    rows = torch.arange(L + 1, device=dev)
    for mode in modes:
        lines[mode]["kernel_us"] = kernel_times([ops[mode]["vector_analysis"], ops[mode]["vector_synthesis"]])
        got = shs[mode].vector_analysis(u, v, dtype=torch.float64)
        diff = 0.0
        for m in (0, 1, L):                                                  # a few orders against the composition
            r = rows[max(m, 1):] ** 2 + rows[max(m, 1):]
            for have, want in zip(got, (cvort, cdiv)):
                diff = max(diff, float((have[:, r + m] - want[:, max(m, 1):, m].real).abs().max()),
                           float((have[:, r - m] + want[:, max(m, 1):, m].imag).abs().max()) if m else 0.0)
        lines[mode]["max_abs_diff_vs_torch"] = diff
    return [lines[m] for m in modes]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", type=int, nargs="*", help="NLAT NLON LMAX C MEMBERS; none: the four standard shapes")
    ap.add_argument("--grid", default="equiangular")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--longitude", choices=("direct", "fft", "both"), default="both")
    a = ap.parse_args()
    if len(a.shape) not in (0, 5):
        ap.error("give NLAT NLON LMAX C MEMBERS, or nothing")
    if not torch.cuda.is_available():
        raise SystemExit("vsht_bench needs the MI355X")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    for shape in ([tuple(a.shape)] if a.shape else STANDARD):
        for line in run(*shape, a.grid, a.calls, a.rounds, a.warmup, a.longitude):
            text = json.dumps(line)
            print(text, flush=True)
            with open(os.path.join(ROOT, "profiles", "vsht_bench.jsonl"), "a") as fh:
                fh.write(text + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
