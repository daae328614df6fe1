"""Writes tests/golden/ref_losses.npz (and ref_losses_large.npz, the two cases of 20 000 and 33 000 elements, which
would carry one file past the size a committed file may have): the reference's own loss classes run on the CPU in fp32
and fp64, autograd included -- the numbers gwen_amd.loss_functions is pinned to (tests/test_ref_losses_host.py,
tests/test_gpu_ref_losses.py; tests/ref_losses_ref.py::load_fixtures reads both files as one).

    python tests/golden/make_ref_losses_golden.py            # needs a checkout of the reference

The reference's ``src/gwen/loss_functions.py`` is loaded by path (GWEN_REFERENCE, default /root/reference) and run; its
one non-torch import, ``gwen.loggers_configs`` (which pulls in mlflow and pyprojroot), is replaced in ``sys.modules`` by
the stand-in below.  Nothing of the reference is copied: only the inputs made here and the results it returned are kept.

Per case ``<name>``: the inputs (``x``, ``t``, ``mask``), ``meta`` (``dim`` / ``alpha`` / ``kind``), ``value32`` and
``value64`` (the forward in fp32 and fp64 of the same fp32 inputs), and ``grad32_x`` / ``grad64_x`` / ``grad32_t`` /
``grad64_t`` (autograd of the summed result).  The fp32 numbers depend on the torch build that ran them (``torch``).
"""
from __future__ import annotations

import importlib.util
import logging
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ref_losses.npz")
OUT_LARGE = os.path.join(HERE, "ref_losses_large.npz")
LARGE = ("crps_m8_b4096_s1", "crps_m150_b2")
REFERENCE = os.environ.get("GWEN_REFERENCE", "/root/reference")
SOURCE = os.path.join(REFERENCE, "src", "gwen", "loss_functions.py")
KINDS = ("l1", "mse")


def available() -> bool:
    return os.path.exists(SOURCE)


def load_reference():
    """The reference's module object, with a logging-only ``gwen.loggers_configs``."""
    stand_in = types.ModuleType("gwen.loggers_configs")
    stand_in.setup_logger = lambda *a, **k: logging.getLogger("gwen")
    pkg = types.ModuleType("gwen")
    pkg.__path__ = []
    saved = {k: sys.modules.get(k) for k in ("gwen", "gwen.loggers_configs")}
    sys.modules["gwen"], sys.modules["gwen.loggers_configs"] = pkg, stand_in
    try:
        spec = importlib.util.spec_from_file_location("_gwen_reference_loss_functions", SOURCE)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def crps_inputs():
    """name -> (x fp32 5-D, t fp32 4-D, dim)"""
    cases = {}

    def normal(seed, m, b, rest, loc=0.0):
        g = np.random.default_rng(seed)
        x = loc + g.standard_normal((m, b) + rest)
        t = loc + g.standard_normal((b,) + rest)
        return _f32(x), _f32(t)

    cases["crps_m5_b3"] = (*normal(101, 5, 3, (1, 7, 9)), 0)
    cases["crps_m8_b4096_s1"] = (*normal(102, 8, 4096, (1, 1, 1)), 0)
    cases["crps_m150_b2"] = (*normal(103, 150, 2, (1, 5, 13)), 0)
    cases["crps_m16_offset1000"] = (*normal(104, 16, 2, (1, 8, 8), loc=1000.0), 0)
    # zero spread (identical members) with t != mu and t == mu, among ordinary points
    x, t = normal(105, 6, 2, (1, 4, 6))
    x[:, 0, 0, 0, :] = x[0, 0, 0, 0, :]             # t != mu (t is random)
    x[:, 1, 0, 1, :] = x[0, 1, 0, 1, :]
    t[1, 0, 1, :] = x[0, 1, 0, 1, :]                # t == mu exactly
    x[:, 1, 0, 3, 2] = 0.0
    t[1, 0, 3, 2] = 0.0
    cases["crps_zero_spread"] = (x, t, 0)
    # spread 1e-3: targets near the mean and 5 away (the score saturates at 1/4)
    g = np.random.default_rng(106)
    x = _f32(2.0 + 1e-3 * g.standard_normal((7, 2, 1, 4, 8)))
    t = _f32(2.0 + 1e-3 * g.standard_normal((2, 1, 4, 8)))
    t[:, :, 2:] += 5.0
    t[:, :, 3] -= 10.0
    cases["crps_small_spread"] = (x, t, 0)
    # members on dim 2
    g = np.random.default_rng(107)
    cases["crps_dim2"] = (_f32(g.standard_normal((3, 2, 6, 5, 7))), _f32(g.standard_normal((3, 2, 5, 7))), 2)
    return cases


def varreg_inputs():
    """name -> (x, t, alpha)"""
    cases = {}
    g = np.random.default_rng(201)
    x = _f32(g.standard_normal((3, 5, 7, 9)))
    cases["varreg_broadcast_target"] = (x, _f32(g.standard_normal((3, 1, 7, 9))), 0.1)
    cases["varreg_full_target"] = (x, _f32(g.standard_normal((3, 5, 7, 9))), 0.1)
    cases["varreg_alpha0"] = (x, _f32(g.standard_normal((3, 1, 7, 9))), 0.0)
    t = _f32(g.standard_normal((3, 5, 7, 9)))
    tie = g.random((3, 5, 7, 9)) < 0.3
    t[tie] = x[tie]                                 # exact ties: sign(0) = 0
    cases["varreg_ties"] = (x, t, 0.25)
    cases["varreg_m1_nan"] = (_f32(g.standard_normal((4, 1, 6))), _f32(g.standard_normal((4, 1, 6))), 0.1)
    return cases


def masked_inputs():
    """name -> (x, t, mask (fp32 or bool), kind)"""
    cases = {}
    g = np.random.default_rng(301)
    x, t = _f32(g.standard_normal((3, 5, 7, 9))), _f32(g.standard_normal((3, 5, 7, 9)))
    weights = _f32(g.random((7, 9)))
    flags = g.random((7, 9)) < 0.6
    full = _f32(g.random((3, 5, 7, 9)) * (g.random((3, 5, 7, 9)) < 0.7))
    for kind in KINDS:
        cases[f"masked_{kind}_float_7x9"] = (x, t, weights, kind)
        cases[f"masked_{kind}_bool_7x9"] = (x, t, flags, kind)
        cases[f"masked_{kind}_full"] = (x, t, full, kind)
        cases[f"masked_{kind}_bool_full"] = (x, t, full > 0.5, kind)
        cases[f"masked_{kind}_all_zero"] = (x, t, np.zeros((7, 9), np.float32), kind)
    return cases


def _run(fn, x, t, dtype):
    """value and the autograd of its sum in ``dtype``, from fp32 inputs"""
    xt = torch.from_numpy(x).to(dtype).requires_grad_()
    tt = torch.from_numpy(t).to(dtype).requires_grad_()
    value = fn(xt, tt)
    value.sum().backward()
    return value.detach().numpy(), xt.grad.numpy(), tt.grad.numpy()


def _record(out, name, fn, x, t):
    out[f"{name}/x"], out[f"{name}/t"] = x, t
    for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
        value, gx, gt = _run(fn, x, t, dtype)
        out[f"{name}/value{tag}"], out[f"{name}/grad{tag}_x"], out[f"{name}/grad{tag}_t"] = value, gx, gt


def generate() -> dict:
    """Every array of the fixture file, from the reference's classes."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                                         # one summation order, whatever the machine
    try:
        return _generate(load_reference())
    finally:
        torch.set_num_threads(threads)


def _generate(ref) -> dict:
    out = {"torch": np.array(torch.__version__)}
    for name, (x, t, dim) in crps_inputs().items():
        crit = ref.CRPSLoss()
        _record(out, name, lambda a, b: crit(a, b, dim=dim), x, t)
        out[f"{name}/meta"] = np.array([dim], np.float64)
    for name, (x, t, alpha) in varreg_inputs().items():
        crit = ref.EnsembleVarRegLoss(alpha=alpha)
        _record(out, name, crit, x, t)
        out[f"{name}/meta"] = np.array([alpha], np.float64)
    for name, (x, t, mask, kind) in masked_inputs().items():
        loss_fn = torch.nn.L1Loss(reduction="none") if kind == "l1" else torch.nn.MSELoss(reduction="none")
        crit = ref.MaskedLoss(loss_fn)
        mk = torch.from_numpy(mask)
        _record(out, name, lambda a, b: crit(a, b, mk if mk.dtype == torch.bool else mk.to(a.dtype)), x, t)
        out[f"{name}/mask"] = mask
        out[f"{name}/meta"] = np.array([KINDS.index(kind)], np.float64)
    return out


def case_names(arrays) -> list:
    return sorted({k.split("/")[0] for k in arrays if "/" in k})


def split(arrays) -> tuple:
    """(the arrays of ref_losses.npz, those of ref_losses_large.npz)"""
    large = {k: v for k, v in arrays.items() if k.split("/")[0] in LARGE}
    return {k: v for k, v in arrays.items() if k not in large}, large


if __name__ == "__main__":
    if not available():
        raise SystemExit(f"{SOURCE} not found: set GWEN_REFERENCE to a checkout of the reference")
    arrays = generate()
    for path, part in zip((OUT, OUT_LARGE), split(arrays)):
        np.savez_compressed(path, **part)
        print(f"{path}: {len(case_names(part))} cases, {os.path.getsize(path)} bytes")
