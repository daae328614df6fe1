"""Writes tests/golden/ref_unet.npz: the reference's own U-Net classes run on the CPU in fp32 and fp64 -- the numbers
gwen_amd.models_cnn is pinned to (tests/test_unet_host.py, tests/test_gpu_unet.py).

    python tests/golden/make_ref_unet_golden.py            # needs a checkout of the reference

The reference's ``src/gwen/models_cnn.py`` is loaded by path (GWEN_REFERENCE, default /root/reference) and run; its
non-torch imports (``mlflow``, ``pytorch_lightning.loggers``, ``gwen.loggers_configs``, ``gwen.utils``) are replaced in
``sys.modules`` by the stand-ins below, and a one-rank gloo group on a temporary file answers ``Decoder.forward``'s
``dist.get_rank()``.  Nothing of the reference is copied: only results it returned are kept.  The weights and inputs are
NOT in the file: tests/unet_ref.py makes them from seeds (``make_state``, ``make_input``), here and in every test, and
they enter the reference through ``load_state_dict(strict=True)``.

Per case ``<name>`` (tests/unet_ref.py::CASES) and mode (``eval``, and ``train`` where the case has it):
``<name>/<mode>/out32`` and ``out64`` -- the fp32 and fp64 forward of the same fp32 input and weights -- and in train mode
``<name>/train/stats64/<key>`` / ``stats32/<key>``, the updated running statistics and ``num_batches_tracked``.  Per case
also ``<name>/keys`` and ``<name>/shapes`` (the reference's ``state_dict``: names, and shapes as text) and
``<name>/meta`` = (B, Cin, Cout, hidden, H, W).  The fp32 numbers depend on the torch build that ran them (``torch``).

In train mode every BatchNorm's batch variance must be at least 1e-3 of its input's mean square (asserted below, per
channel): the fp32 yardstick is then not the luck of a near-degenerate channel.  A seed that fails is replaced in CASES.
"""
from __future__ import annotations

import importlib.util
import logging
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import unet_ref as R  # noqa: E402

OUT = R.GOLDEN
REFERENCE = os.environ.get("GWEN_REFERENCE", "/root/reference")
SOURCE = os.path.join(REFERENCE, "src", "gwen", "models_cnn.py")
MIN_VARIANCE_SHARE = 1e-3


def available() -> bool:
    return os.path.exists(SOURCE)


def load_reference():
    """The reference's module object, with logging-only stand-ins for what it imports beside torch."""
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        return m

    stand_ins = {
        "mlflow": module("mlflow"),
        "pytorch_lightning": module("pytorch_lightning", __path__=[]),
        "pytorch_lightning.loggers": module("pytorch_lightning.loggers", MLFlowLogger=object),
        "gwen": module("gwen", __path__=[]),
        "gwen.loggers_configs": module("gwen.loggers_configs", setup_logger=lambda *a, **k: logging.getLogger("gwen"),
                                       setup_mlflow=lambda *a, **k: (None, None)),
        "gwen.utils": module("gwen.utils", ConvDataset=object),
    }
    saved = {k: sys.modules.get(k) for k in stand_ins}
    sys.modules.update(stand_ins)
    try:
        spec = importlib.util.spec_from_file_location("_gwen_reference_models_cnn", SOURCE)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def _variance_shares(model):
    """hooks that record, per BatchNorm call, min over channels of (batch variance / mean square) of its input"""
    shares, handles = [], []

    def hook(_m, args):
        x = args[0].detach().double()
        var = x.var(dim=(0, 2, 3), unbiased=False)
        ms = x.square().mean(dim=(0, 2, 3))
        shares.append(float((var / ms.clamp_min(1e-300)).min()))

    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            handles.append(m.register_forward_pre_hook(hook))
    return shares, handles


def _run(ref, name, mode, dtype):
    (b, cin, cout, hidden, h, w), _, _, _, _ = R.CASES[name]
    state = {k: torch.from_numpy(np.asarray(v)) for k, v in R.case_state(name).items()}
    model = ref.UNet(cin, cout, hidden)
    model.load_state_dict(state, strict=True)
    model = model.to(dtype)
    model.train(mode == "train")
    shares, handles = _variance_shares(model)
    with torch.no_grad():
        out = model(torch.from_numpy(R.make_input(name)).to(dtype))
    for hnd in handles:
        hnd.remove()
    if mode == "train":
        assert min(shares) >= MIN_VARIANCE_SHARE, \
            f"{name}: a BatchNorm input has batch variance {min(shares):.2e} of its mean square: pick another seed"
    stats = {k: v.detach().numpy() for k, v in model.state_dict().items()
             if k.rsplit(".", 1)[1] in ("running_mean", "running_var", "num_batches_tracked")}
    return out.numpy(), stats, model


def generate() -> dict:
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                                         # one summation order, whatever the machine
    store = tempfile.NamedTemporaryFile(delete=False)
    store.close()
    torch.distributed.init_process_group("gloo", init_method=f"file://{store.name}", rank=0, world_size=1)
    try:
        return _generate(load_reference())
    finally:
        torch.distributed.destroy_process_group()
        if os.path.exists(store.name):                               # (the store removes its file when the group goes)
            os.unlink(store.name)
        torch.set_num_threads(threads)


def _generate(ref) -> dict:
    out = {"torch": np.array(torch.__version__)}
    for name, (meta, _, _, _, _) in R.CASES.items():
        out[f"{name}/meta"] = np.array(meta, np.int64)
        for mode in R.modes(name):
            for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
                y, stats, model = _run(ref, name, mode, dtype)
                out[f"{name}/{mode}/out{tag}"] = y
                if mode == "train":
                    used = {k for k, _, u in R.state_spec(*meta[1:4]) if u}
                    for k, v in stats.items():
                        if k in used:
                            out[f"{name}/train/stats{tag}/{k}"] = v
        sd = model.state_dict()
        out[f"{name}/keys"] = np.array(list(sd))
        out[f"{name}/shapes"] = np.array(["x".join(str(d) for d in v.shape) for v in sd.values()])
    return out


if __name__ == "__main__":
    if not available():
        raise SystemExit(f"{SOURCE} not found: set GWEN_REFERENCE to a checkout of the reference")
    arrays = generate()
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT}: {len(R.CASES)} cases, {os.path.getsize(OUT)} bytes")
