"""Time the spectral convolution of gwen_amd.sfno (csrc/spectral_conv.hip) against the best torch composition of the same
outputs, and one SFNOBlock, on device events; print one JSON line a case and append it to profiles/sfno_bench.jsonl.

    python tools/sfno_bench.py                          the three standard shapes and the block
    python tools/sfno_bench.py LMAX CIN COUT BATCH      one spectral-convolution shape
    options: --precision f16x3|3xbf16  --calls K  --rounds R  --warmup W  --no-block  --longitude direct|fft|both

Spectral convolution: the forward, the gradient in coef and the gradient in the weight, each as microseconds a call and
as a fraction of the 8 TB/s HBM peak by compulsory bytes (the weights once, the coefficients in and out; for the weight
gradient the two coefficient-sized inputs in and the weights out).  The torch composition zero-pads the degrees to
``[L, batch (2 lmax + 1), C]`` with one index_select (a zero row appended), runs one fp32 ``bmm`` against ``W [L, Cin,
Cout]`` and gathers the rows back; the padding and the gather are inside the timed region, the index tables are not.  The
two sides alternate bracket by bracket in one process; a side's figure is the median of its brackets.

Block: one SFNOBlock at 361 x 720, lmax 180, 64 channels, forward (no_grad) and forward + backward, and the same for its
transforms alone (analysis + synthesis; with their adjoints for the backward), whose share of the block is stated.
``--longitude both`` (the default) runs the block on the direct-sum and on the FFT longitude stage of the transforms in
one process, bracket after bracket in turn, and writes one line per stage (field ``longitude``)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12
STANDARD = [(360, 256, 256, 4), (360, 64, 64, 4), (180, 256, 256, 4)]
BLOCK = (361, 720, 180, 64, 2)                     # nlat, nlon, lmax, channels, members


class Composition:
    """The spectral convolution from torch operators: pad the degrees to one length, one bmm, gather back."""

    def __init__(self, lmax, batch, dev):
        L, M, T = lmax + 1, 2 * lmax + 1, (lmax + 1) ** 2
        pad = np.full((L, batch, M), batch * T, dtype=np.int64)                # the appended zero row
        back = np.empty((batch, T), dtype=np.int64)
        for l in range(L):
            m = 2 * l + 1
            rows = np.arange(batch)[:, None] * T + l * l + np.arange(m)[None, :]
            pad[l, :, :m] = rows
            back[:, l * l:(l + 1) ** 2] = (l * batch + np.arange(batch)[:, None]) * M + np.arange(m)[None, :]
        self.pad = torch.from_numpy(pad.reshape(-1)).to(dev)
        self.back = torch.from_numpy(back.reshape(-1)).to(dev)
        self.L, self.rows, self.batch, self.T = L, batch * M, batch, T

    def padded(self, c):
        flat = torch.cat([c.reshape(-1, c.shape[-1]), c.new_zeros(1, c.shape[-1])])
        return flat.index_select(0, self.pad).view(self.L, self.rows, c.shape[-1])

    def forward(self, c, w):
        y = torch.bmm(self.padded(c), w)
        return y.view(-1, w.shape[2]).index_select(0, self.back).view(self.batch, self.T, w.shape[2])

    def grad_coef(self, g, w):
        return self.forward(g, w.transpose(1, 2))

    def grad_weight(self, c, g):
        return torch.bmm(self.padded(c).transpose(1, 2), self.padded(g))


def bracket(fn, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls * 1e3                                   # us per call


def alternate_many(fns, calls, rounds, warmup):
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


def alternate(a, b, calls, rounds, warmup):
    return tuple(alternate_many([a, b], calls, rounds, warmup))


def run_conv(lmax, cin, cout, batch, precision, calls, rounds, warmup) -> dict:
    from gwen_amd import _lib, sfno
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(31)
    T = (lmax + 1) ** 2
    coef = torch.randn(batch, T, cin, device=dev, generator=g)
    grad = torch.randn(batch, T, cout, device=dev, generator=g)
    w = torch.randn(lmax + 1, cin, cout, device=dev, generator=g) * cin ** -0.5
    code = _lib.CONTRACT_NAMES[precision]
    comp = Composition(lmax, batch, dev)
    gw = torch.empty_like(w)

    def fused_grad_weight():
        from gwen_amd.graph import _ptr, _stream
        rc = _lib.lib().gwen_spectral_conv_grad_weight_f32(_ptr(coef), _ptr(grad), _ptr(gw), batch, lmax, cin, cout,
                                                           code, _stream(dev))
        _lib.check(rc, "gwen_spectral_conv_grad_weight_f32")
        return gw

    pairs = {
        "forward": (lambda: sfno._launch(coef, w, batch, lmax, cin, cout, False, code), lambda: comp.forward(coef, w)),
        "grad_coef": (lambda: sfno._launch(grad, w, batch, lmax, cout, cin, True, code),
                      lambda: comp.grad_coef(grad, w)),
        "grad_weight": (fused_grad_weight, lambda: comp.grad_weight(coef, grad)),
    }
    wbytes, cbytes, obytes = 4.0 * w.numel(), 4.0 * coef.numel(), 4.0 * grad.numel()
    nbytes = {"forward": wbytes + cbytes + obytes, "grad_coef": wbytes + cbytes + obytes,
              "grad_weight": wbytes + cbytes + obytes}
    flops = 2.0 * batch * T * cin * cout
    line = {"tool": "sfno_bench", "case": "spectral_conv", "lmax": lmax, "cin": cin, "cout": cout, "batch": batch,
            "precision": precision, "calls": calls, "rounds": rounds, "flops": flops, "compulsory_bytes": nbytes["forward"],
            "padded_rows_over_rows": round((lmax + 1) * (2 * lmax + 1) / T, 3)}
    for name, (fused, composed) in pairs.items():
        us, us_torch = alternate(fused, composed, calls, rounds, warmup)
        line[name] = {"us": round(us, 1), "torch_us": round(us_torch, 1), "speedup": round(us_torch / us, 3),
                      "faster": "fused" if us < us_torch else "torch",
                      "fraction_of_8tbs_peak": round(nbytes[name] / (us * 1e-6) / PEAK_BYTES_PER_S, 4),
                      "tflops": round(flops / (us * 1e-6) / 1e12, 2)}
    ref = comp.forward(coef, w)
    line["max_rel_diff_vs_torch"] = float((pairs["forward"][0]() - ref).abs().max() / ref.abs().max())
    return line


def run_block(nlat, nlon, lmax, channels, members, precision, calls, rounds, warmup, longitude="both") -> list:
    """One line per longitude stage."""
    import gwen_amd
    dev = torch.device("cuda:0")
    modes = ["direct", "fft"] if longitude == "both" else [longitude]
    x = torch.randn(members, nlat * nlon, channels, device=dev, generator=torch.Generator(device=dev).manual_seed(38))
    r = torch.randn_like(x)

    def side(mode):
        sh = gwen_amd.SphericalHarmonics(nlat, nlon, dev, lmax=lmax, workspace_bytes=4 << 30, longitude=mode)
        torch.manual_seed(37)
        block = gwen_amd.SFNOBlock(sh, channels, precision=precision).to(dev)
        xg = x.clone().requires_grad_()
        xt = x.clone().requires_grad_()

        def forward():
            with torch.no_grad():
                return block(x)

        def transforms():
            with torch.no_grad():
                return sh.synthesis(sh.analysis(x))

        def training():
            xg.grad = None
            block.zero_grad(set_to_none=True)
            block(xg).backward(r)

        def transforms_training():
            xt.grad = None
            sh.synthesis(sh.analysis(xt)).backward(r)

        return forward, transforms, training, transforms_training

    sides = [side(m) for m in modes]
    fwd = alternate_many([f for s in sides for f in s[:2]], calls, rounds, warmup)
    trn = alternate_many([f for s in sides for f in s[2:]], calls, rounds, warmup)
    lines = []
    for k, mode in enumerate(modes):
        line = {"tool": "sfno_bench", "case": "sfno_block", "longitude": mode, "nlat": nlat, "nlon": nlon, "lmax": lmax,
                "channels": channels, "members": members, "precision": precision, "calls": calls, "rounds": rounds,
                "forward_us": round(fwd[2 * k], 1), "forward_transforms_us": round(fwd[2 * k + 1], 1),
                "forward_transforms_share": round(fwd[2 * k + 1] / fwd[2 * k], 4),
                "forward_backward_us": round(trn[2 * k], 1), "forward_backward_transforms_us": round(trn[2 * k + 1], 1),
                "forward_backward_transforms_share": round(trn[2 * k + 1] / trn[2 * k], 4)}
        if mode == "fft" and "direct" in modes:
            line["direct_forward_us"], line["direct_forward_backward_us"] = round(fwd[0], 1), round(trn[0], 1)
        lines.append(line)
    return lines


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("shape", type=int, nargs="*", help="LMAX CIN COUT BATCH; none: the standard shapes and the block")
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-block", action="store_true")
    ap.add_argument("--longitude", choices=("direct", "fft", "both"), default="both")
    a = ap.parse_args()
    if len(a.shape) not in (0, 4):
        ap.error("give LMAX CIN COUT BATCH, or nothing")
    if not torch.cuda.is_available():
        raise SystemExit("sfno_bench needs the MI355X")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        with open(os.path.join(ROOT, "profiles", "sfno_bench.jsonl"), "a") as fh:
            fh.write(text + "\n")
        torch.cuda.empty_cache()

    for shape in ([tuple(a.shape)] if a.shape else STANDARD):
        emit(run_conv(*shape, a.precision, a.calls, a.rounds, a.warmup))
    if not a.shape and not a.no_block:
        for line in run_block(*BLOCK, a.precision, max(1, a.calls // 2), a.rounds, 1, a.longitude):
            emit(line)


if __name__ == "__main__":
    main()
