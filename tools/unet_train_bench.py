"""Time one training iteration without the optimiser (forward + MSE + backward) of gwen_amd.UNet(grad=True) against the
same nn.Module composition run by torch's own convolutions, on device events, in one process; print one JSON line a
batch and tier and append it to profiles/unet_train_bench.jsonl.

    python tools/unet_train_bench.py      options: --calls K  --rounds R  --warmup W  --size H W  --batches 1 8
                                                   --time-limit SECONDS

Configuration: the reference's (124 -> 1 channels, hidden 1024) on 128 x 128 (the size is this tool's choice, as in
tools/unet_bench.py), train mode, batch 1 and 8, both tiers.  The yardstick is the SAME module object through torch
(MIOpen) in NCHW and once more in channels_last.  The sides alternate bracket by bracket; a side's figure is the median
of its brackets (7 by default).  Every line also carries
  ``wgrad``: the weight-gradient kernel alone (gwen_conv3x3_grad_weight_f32, reduction included) at the four encoder
      shapes of that batch, median us per launch and its share of the dense bf16 MFMA peak (2.5 PF) counted in SPLIT
      terms: 2 * 9 * Cin * Cout * B H W flops times 6 ("bf16x6") or 3 ("3xbf16") MFMA terms;
  ``held_bytes``: the device memory the recorded forward holds for the backward (allocated after the forward minus
      before it, output included), beside ``inference_bytes``, the same for the no_grad forward's output alone.
``max_rel_diff_of_conv_weight_grads_vs_torch`` compares the two sides' conv weight gradients on the timed (random) input,
relative to each tensor's maximum: an untrained model on noise has no switch margin, so a ReLU or pool that falls the
other way on one side shows here as percents (tests/unet_grad_ref.py, "the margin rule").
The whole run stops with an error after ``--time-limit`` seconds (default 900).
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import signal
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from unet_bench import alternate_many, torch_forward  # noqa: E402

CONFIG = (124, 1, 1024)
PEAK_BF16_FLOPS = 2.5e15


def wgrad_lines(batch, size, precision, rounds, calls):
    from gwen_amd import ops
    cin, _, hidden = CONFIG
    h, w = size
    dev = torch.device("cuda:0")
    out = []
    chans = [(cin, hidden // 8), (hidden // 8, hidden // 4), (hidden // 4, hidden // 2), (hidden // 2, hidden)]
    for i, (ci, co) in enumerate(chans):
        hh, ww = h >> i, w >> i
        g = torch.randn(batch, hh, ww, co, device=dev)
        x = torch.randn(batch, hh, ww, ci, device=dev)
        fn = lambda: ops.conv3x3_grad_weight(g, x, contract=precision)
        (med,), _ = alternate_many([fn], calls, rounds, 2)
        terms = 6 if precision == "bf16x6" else 3
        flops = 2.0 * 9 * ci * co * batch * hh * ww * terms
        tiles, chunks = ops.conv3x3_grad_weight_plan(batch, hh, ww, ci, co)
        out.append({"stage": i, "cin": ci, "cout": co, "height": hh, "width": ww, "channel_tiles": tiles,
                    "pixel_chunks": chunks, "us": round(med, 1),
                    "share_of_bf16_peak_in_split_terms": round(flops / (med * 1e-6) / PEAK_BF16_FLOPS, 4)})
    return out


def held_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    keep = fn()
    torch.cuda.synchronize()
    after = torch.cuda.memory_allocated()
    del keep
    return after - before


def run(precision, size, batch, calls, rounds, warmup) -> dict:
    import gwen_amd
    dev = torch.device("cuda:0")
    cin, cout, hidden = CONFIG
    torch.manual_seed(41)
    model = gwen_amd.UNet(cin, cout, hidden, precision=precision, grad=True).to(dev).train()
    model_cl = copy.deepcopy(model).to(memory_format=torch.channels_last)
    h, w = size
    gen = torch.Generator(device=dev).manual_seed(42)
    x = torch.randn(batch, cin, h, w, device=dev, generator=gen)
    target = torch.randn(batch, cout, h, w, device=dev, generator=gen)
    x_cl = x.contiguous(memory_format=torch.channels_last)

    def step(forward, m, inp):
        def fn():
            for p in m.parameters():
                p.grad = None
            loss = F.mse_loss(forward(inp), target)
            loss.backward()
            return loss
        return fn

    ours = step(model, model, x)
    theirs = step(lambda v: torch_forward(model, v), model, x)
    theirs_cl = step(lambda v: torch_forward(model_cl, v), model_cl, x_cl)
    med, best = alternate_many([ours, theirs, theirs_cl], calls, rounds, warmup)
    torch_best = min(med[1:])
    # the gradients of the two sides on the timed input (train mode: the same batch statistics on both)
    ours()
    mine = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    theirs()
    diff = max(float((mine[k] - p.grad).abs().max() / p.grad.abs().max().clamp_min(1e-30))
               for k, p in model.named_parameters() if p.grad is not None and k in mine and "conv" in k and k.endswith("weight"))
    for p in model.parameters():
        p.grad = None

    def no_grad_forward():
        with torch.no_grad():
            return model(x)

    return {"tool": "unet_train_bench", "channels_in": cin, "channels_out": cout, "hidden": hidden, "batch": batch,
            "height": h, "width": w, "mode": "train", "precision": precision, "calls": calls, "rounds": rounds,
            "step_us": round(med[0], 1), "step_us_min": round(best[0], 1),
            "torch_nchw_us": round(med[1], 1), "torch_nchw_us_min": round(best[1], 1),
            "torch_channels_last_us": round(med[2], 1),
            "speedup_vs_best_torch": round(torch_best / med[0], 3),
            "faster": "gwen_amd" if med[0] < torch_best else "torch",
            "max_rel_diff_of_conv_weight_grads_vs_torch": diff,
            "held_bytes": held_bytes(lambda: model(x)), "inference_bytes": held_bytes(no_grad_forward),
            "wgrad": wgrad_lines(batch, size, precision, rounds, calls)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, nargs=2, default=(128, 128))
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--precisions", nargs="*", default=["bf16x6", "3xbf16"])
    ap.add_argument("--time-limit", type=int, default=900)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("unet_train_bench needs the MI355X")

    def expired(*_):
        raise SystemExit(f"unet_train_bench: over its time limit of {a.time_limit} s")

    signal.signal(signal.SIGALRM, expired)
    signal.alarm(a.time_limit)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    for batch in a.batches:
        for precision in a.precisions:
            text = json.dumps(run(precision, tuple(a.size), batch, a.calls, a.rounds, a.warmup))
            print(text, flush=True)
            with open(os.path.join(ROOT, "profiles", "unet_train_bench.jsonl"), "a") as fh:
                fh.write(text + "\n")
            torch.cuda.empty_cache()
    signal.alarm(0)


if __name__ == "__main__":
    main()
