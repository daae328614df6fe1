"""Time gwen_amd.UNet (csrc/conv.hip) in eval mode against the same nn.Module composition run by torch's own convolutions,
on device events, in one process; print one JSON line a configuration and tier and append it to
profiles/unet_bench.jsonl.

    python tools/unet_bench.py            options: --calls K  --rounds R  --warmup W  --size H W  --batch B

Configurations: the reference's (124 -> 1 channels, hidden 1024) and its "simplify" one (1 -> 1), batch 1, on 128 x 128.
ASSUMPTION: the reference's field has 16 384 cells; how that factors into height x cells is not recorded anywhere in this
repository, and 128 x 128 is this tool's choice (``--size`` takes another).

Both tiers ("bf16x6", "3xbf16").  The yardstick is the SAME module object: its Conv2d / ConvTranspose2d / BatchNorm2d
layers called through torch (MIOpen), max_pool2d and bilinear interpolate in between, in the order of the reference's
forward -- in NCHW as the reference runs it, and once more with channels_last memory format.  The sides alternate
bracket by bracket; a side's figure is the median of its brackets.  ``launches`` lists every kernel call of one forward
of the library with its own median time (events around each call, in a pass of its own: the brackets add host gaps, so
their sum exceeds the forward's time).  ``max_rel_diff_vs_torch`` compares the two outputs on the timed input.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

CONFIGS = {"reference": (124, 1, 1024), "simplify": (1, 1, 1024)}


def torch_forward(model, x):
    """The reference's forward from torch operators on the layers of ``model`` (gwen_amd.UNet holds real nn layers)."""
    enc, dec = model.encoder, model.decoder
    feats, v = [], x
    for i in range(4):
        v = F.relu(enc.batch_norm_layers[i](F.max_pool2d(enc.conv_layers[i](v), 2, 2)))
        feats.append(v)
    y = feats[3]
    for k, (bn, skip) in enumerate(((2, feats[2]), (1, feats[1]), (0, feats[0]))):
        y = F.interpolate(dec.conv_transposed_layers[k](y), scale_factor=2, mode="bilinear", align_corners=True)
        y = F.relu(dec.batch_norm_layers[bn](y))
        if y.shape != skip.shape:
            skip = dec.crop(skip, y)
        y = F.relu(torch.cat([skip, y], dim=1))
    y = F.relu(F.interpolate(dec.conv_transposed_layers[3](y), scale_factor=2, mode="bilinear", align_corners=True))
    out = dec.conv_layers[4](y)
    if x.shape[3] != out.shape[3]:
        out = F.pad(out, (x.shape[3] - out.shape[3], 0, 0, 0), mode="replicate")
    return out


def bracket(fn, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls * 1e3                                   # us per call


def alternate_many(fns, calls, rounds, warmup):
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for t, fn in zip(times, fns):
            t.append(bracket(fn, calls))
    return [statistics.median(t) for t in times], [min(t) for t in times]


def per_launch(model, x, rounds):
    """[(call, shape of its input, median us)] of one forward: events around each kernel call of gwen_amd.ops"""
    from gwen_amd import ops
    names = ("conv3x3", "upsample2x", "linear")
    saved = {n: getattr(ops, n) for n in names}
    record = []

    def wrap(name):
        def call(*a, **k):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out = saved[name](*a, **k)
            t1.record()
            tag = name + ("+pool" if k.get("pool") else "") + ("+T" if k.get("transposed") else "")
            record.append((tag, tuple(a[0].shape), tuple(out.shape), t0, t1))
            return out
        return call

    runs = []
    try:
        for n in names:
            setattr(ops, n, wrap(n))
        for _ in range(rounds):
            record.clear()
            with torch.no_grad():
                model(x)
            torch.cuda.synchronize()
            runs.append([(tag, i, o, t0.elapsed_time(t1) * 1e3) for tag, i, o, t0, t1 in record])
    finally:
        for n in names:
            setattr(ops, n, saved[n])
    return [{"call": runs[0][j][0], "in": list(runs[0][j][1]), "out": list(runs[0][j][2]),
             "us": round(statistics.median(r[j][3] for r in runs), 1)} for j in range(len(runs[0]))]


def run(config, precision, size, batch, calls, rounds, warmup) -> dict:
    import gwen_amd
    dev = torch.device("cuda:0")
    cin, cout, hidden = CONFIGS[config]
    torch.manual_seed(41)
    model = gwen_amd.UNet(cin, cout, hidden, precision=precision)
    with torch.no_grad():
        for m in model.modules():                                  # statistics a trained model would carry
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0.0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    model = model.to(dev).eval()
    h, w = size
    x = torch.randn(batch, cin, h, w, device=dev, generator=torch.Generator(device=dev).manual_seed(42))
    x_cl = x.contiguous(memory_format=torch.channels_last)
    model_cl = None
    if cin > 1:
        import copy
        model_cl = copy.deepcopy(model).to(memory_format=torch.channels_last)

    def ours():
        with torch.no_grad():
            return model(x)

    def theirs():
        with torch.no_grad():
            return torch_forward(model, x)

    def theirs_cl():
        with torch.no_grad():
            return torch_forward(model_cl, x_cl)

    fns = [ours, theirs] + ([theirs_cl] if model_cl is not None else [])
    med, best = alternate_many(fns, calls, rounds, warmup)
    ref = theirs()
    diff = float((ours() - ref).abs().max() / ref.abs().max())
    torch_best = min(med[1:])
    line = {"tool": "unet_bench", "config": config, "channels_in": cin, "channels_out": cout, "hidden": hidden,
            "batch": batch, "height": h, "width": w, "mode": "eval", "precision": precision, "calls": calls,
            "rounds": rounds,
            "size_is_an_assumption": f"the reference's field has 16384 cells, its height x width is not recorded; run on "
                                     f"{h} x {w} = {h * w} cells",
            "forward_us": round(med[0], 1), "forward_us_min": round(best[0], 1),
            "torch_nchw_us": round(med[1], 1), "torch_nchw_us_min": round(best[1], 1),
            "torch_channels_last_us": round(med[2], 1) if len(med) > 2 else None,
            "speedup_vs_best_torch": round(torch_best / med[0], 3),
            "faster": "gwen_amd" if med[0] < torch_best else "torch",
            "max_rel_diff_vs_torch": diff, "launches": per_launch(model, x, rounds)}
    return line


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, nargs=2, default=(128, 128))
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--configs", nargs="*", default=list(CONFIGS))
    ap.add_argument("--precisions", nargs="*", default=["bf16x6", "3xbf16"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("unet_bench needs the MI355X")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    for config in a.configs:
        for precision in a.precisions:
            text = json.dumps(run(config, precision, tuple(a.size), a.batch, a.calls, a.rounds, a.warmup))
            print(text, flush=True)
            with open(os.path.join(ROOT, "profiles", "unet_bench.jsonl"), "a") as fh:
                fh.write(text + "\n")
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
