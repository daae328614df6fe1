"""Writes tests/golden/ref_unet_grads.npz: the gradients of the reference's own U-Net classes, run on the CPU in fp32 and
fp64 -- the numbers the backward of gwen_amd.models_cnn is pinned to (tests/test_unet_grad_host.py,
tests/test_gpu_unet_grad.py).

    python tests/golden/make_ref_unet_grads_golden.py      # needs a checkout of the reference

The reference is loaded as tests/golden/make_ref_unet_golden.py loads it (``load_reference``, the same one-rank gloo
group).  The loss is ``(out * G).sum()`` with a seeded cotangent G.  Results only: the weights, inputs and cotangents
are NOT in the file -- tests/unet_grad_ref.py makes them from seeds (``case_state``, ``case_input``,
``case_cotangent``) -- and nothing of the reference is copied.

Per case ``<name>`` of unet_grad_ref.FIXTURE_CASES and tensor ``<key>`` (a state_dict key the forward reads, or
``input``): ``<name>/g64/<key>``, the fp64 gradient ROUNDED TO FP32 (6e-8 of each element, far under every bound the
tests hold the device to), and ``<name>/err32/<key>`` = max|g32 - g64|, the reference's own fp32 distance from fp64,
taken before that rounding.  Also ``<name>/out64`` (fp64), ``<name>/margin`` (the smallest switch margin of the fp64
run, unet_grad_ref's rule, asserted here to meet unet_grad_ref.MARGIN), ``<name>/unused`` (the keys whose grad stayed
None) and ``torch``, the version that ran it.  Every gradient that is not mathematically zero must have a non-zero
maximum (a dead last ReLU leaves them all zero): asserted.
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import unet_grad_ref as G  # noqa: E402
from make_ref_unet_golden import available, load_reference, SOURCE  # noqa: E402

OUT = G.GOLDEN


def _margins(model, x):
    """the smallest switch margin of one forward of the reference's model (hooks on its pools and ReLUs)"""
    margins, handles = [], []

    def relu_hook(_m, args):
        z = args[0].detach()
        if float(z.min()) < 0.0:                    # (the second ReLU after a concatenation sees no negative value)
            margins.append(G.relu_margin(z))

    def pool_hook(_m, args):
        margins.append(G.pool_margin(args[0]))

    for m in model.modules():
        if isinstance(m, torch.nn.ReLU):
            handles.append(m.register_forward_pre_hook(relu_hook))
        elif isinstance(m, torch.nn.MaxPool2d):
            handles.append(m.register_forward_pre_hook(pool_hook))
    return margins, handles


def _run(ref, name, dtype):
    (b, cin, cout, hidden, h, w), mode, _ = G.CASES[name]
    state = {k: torch.from_numpy(np.asarray(v)) for k, v in G.case_state(name).items()}
    model = ref.UNet(cin, cout, hidden)
    model.load_state_dict(state, strict=True)
    model = model.to(dtype)
    model.train(mode == "train")
    margins, handles = _margins(model, None)
    x = torch.from_numpy(G.case_input(name)).to(dtype).requires_grad_()
    out = model(x)
    for hnd in handles:
        hnd.remove()
    (out * torch.from_numpy(G.case_cotangent(name)).to(dtype)).sum().backward()
    grads = {k: (None if p.grad is None else p.grad.detach().numpy()) for k, p in model.named_parameters()}
    grads["input"] = x.grad.numpy()
    return out.detach().numpy(), grads, min(margins)


def generate() -> dict:
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                                         # one summation order, whatever the machine
    store = tempfile.NamedTemporaryFile(delete=False)
    store.close()
    torch.distributed.init_process_group("gloo", init_method=f"file://{store.name}", rank=0, world_size=1)
    try:
        ref = load_reference()
        out = {"torch": np.array(torch.__version__)}
        for name in G.FIXTURE_CASES:
            meta, mode, _ = G.CASES[name]
            out64, g64, margin = _run(ref, name, torch.float64)
            _, g32, _ = _run(ref, name, torch.float32)
            assert margin >= G.MARGIN[name], f"{name}: margin {margin:.2e} under {G.MARGIN[name]:.0e}: pick another seed"
            out[f"{name}/out64"] = out64
            out[f"{name}/margin"] = np.array(margin)
            out[f"{name}/unused"] = np.array(sorted(k for k, v in g64.items() if v is None))
            assert sorted(k for k, v in g64.items() if v is not None and k != "input") == sorted(G.used_keys(*meta[1:4]))
            for k, v in g64.items():
                if v is None:
                    continue
                if not (mode == "train" and G.zero_in_train(k)):
                    assert np.abs(v).max() > 0.0, f"{name}: the gradient of {k} is dead: pick another seed"
                out[f"{name}/g64/{k}"] = v.astype(np.float32)
                out[f"{name}/err32/{k}"] = np.array(np.abs(g32[k].astype(np.float64) - v).max())
        return out
    finally:
        torch.distributed.destroy_process_group()
        if os.path.exists(store.name):                               # (the store removes its file when the group goes)
            os.unlink(store.name)
        torch.set_num_threads(threads)


if __name__ == "__main__":
    if not available():
        raise SystemExit(f"{SOURCE} not found: set GWEN_REFERENCE to a checkout of the reference")
    arrays = generate()
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT}: {len(G.FIXTURE_CASES)} cases, {os.path.getsize(OUT)} bytes")
    for k, v in arrays.items():
        if k.endswith("/margin"):
            print(k, float(v))
