"""fp64 numpy restatement of the three reference losses and their gradients, in the project's own words -- pinned to the
reference's fp64 numbers by tests/test_ref_losses_host.py, and the yardstick of the GPU shapes the fixtures do not hold.

Every function takes the members axis where the kernels do: ``x [A, M, R]``."""
from __future__ import annotations

import math
import os

import numpy as np

try:
    from scipy.special import erf as _erf
except ImportError:                                     # pragma: no cover
    _erf = np.vectorize(math.erf, otypes=[np.float64])

SQRT2 = math.sqrt(2.0)


def gauss_crps(x, t, samples: int):
    """x [A, M, R], t [A, R]; the A R points form ``samples`` runs of equal length.  Returns (loss [samples],
    grad_x, grad_t) with the gradients of ``loss.sum()``."""
    x, t = np.asarray(x, np.float64), np.asarray(t, np.float64)
    a, m, r = x.shape
    mu = x.mean(1)
    dev = x - mu[:, None, :]
    s = np.sqrt((dev * dev).sum(1) / (m - 1))
    sigma = s + 1e-6
    z = (t - mu) / (sigma * SQRT2)
    q = 0.5 * _erf(z)
    per = a * r // samples
    loss = (q * q).reshape(samples, per).mean(1)
    c = (2.0 * q / per) * np.exp(-z * z) / math.sqrt(math.pi)            # d loss.sum() / dz
    grad_t = c / (sigma * SQRT2)
    with np.errstate(divide="ignore", invalid="ignore"):
        ds = np.where(s[:, None, :] == 0.0, 0.0, dev / ((m - 1) * s[:, None, :]))
    grad_x = -grad_t[:, None, :] / m - (c * z / sigma)[:, None, :] * ds
    return loss, grad_x, grad_t


def varreg_l1(x, t, alpha: float):
    """x [A, M, R], t [A, M, R] or [A, 1, R].  Returns (loss, grad_x, grad_t)."""
    x, t = np.asarray(x, np.float64), np.asarray(t, np.float64)
    a, m, r = x.shape
    d = x - t
    mu = x.mean(1, keepdims=True)
    dev = x - mu
    with np.errstate(divide="ignore", invalid="ignore"):
        var = (dev * dev).sum(1) / (m - 1)
        loss = np.abs(d).mean() - alpha * var.mean()
        sg = np.sign(d) / d.size
        grad_x = sg - alpha * (np.float64(2.0) / ((m - 1) * a * r)) * dev
    grad_t = -sg if t.shape[1] == m else -sg.sum(1, keepdims=True)
    return loss, grad_x, grad_t


def masked_mean(x, t, mask, kind: str):
    """x, t of one shape, mask over the trailing dims (or all): sum(l mask) / sum(mask as given)."""
    x, t, mask = np.asarray(x, np.float64), np.asarray(t, np.float64), np.asarray(mask, np.float64)
    d = x - t
    l, dl = (np.abs(d), np.sign(d)) if kind == "l1" else (d * d, 2.0 * d)
    with np.errstate(divide="ignore", invalid="ignore"):
        loss = (l * mask).sum() / mask.sum()
        grad_x = dl * mask / mask.sum()
    return loss, grad_x, -grad_x


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = ("l1", "mse")


def load_fixtures() -> dict:
    """tests/golden/ref_losses.npz and ref_losses_large.npz as one dict of arrays (golden/make_ref_losses_golden.py)."""
    out = {}
    for name in ("ref_losses.npz", "ref_losses_large.npz"):
        with np.load(os.path.join(GOLDEN, name)) as z:
            out.update({k: z[k] for k in z.files})
    return out


def case_names(arrays) -> list:
    return sorted({k.split("/")[0] for k in arrays if "/" in k})


def layout(name: str, arrays):
    """A fixture case as the restatement takes it: (family, x [A, M, R], t, extra) with extra = (samples, dim) for
    ``crps`` (members moved to the middle of [A, M, R] = [1, M, rest]), alpha for ``varreg``, (mask, kind) for
    ``masked``."""
    x, t, meta = arrays[f"{name}/x"], arrays[f"{name}/t"], float(arrays[f"{name}/meta"][0])
    family = name.split("_")[0]
    if family == "crps":
        dim = int(meta)
        xm = np.moveaxis(x, dim, 0)
        return family, xm.reshape(1, xm.shape[0], -1), t.reshape(1, -1), (t.shape[0], dim)
    if family == "varreg":
        return family, x.reshape(x.shape[0], x.shape[1], -1), t.reshape(t.shape[0], t.shape[1], -1), meta
    return family, x, t, (arrays[f"{name}/mask"], KINDS[int(meta)])


def restate(name: str, arrays):
    """(value, grad_x, grad_t) of a fixture case from the restatement, in the fixture's own shapes."""
    family, x, t, extra = layout(name, arrays)
    shape_x, shape_t = arrays[f"{name}/x"].shape, arrays[f"{name}/t"].shape
    if family == "crps":
        samples, dim = extra
        value, gx, gt = gauss_crps(x, t, samples)
        moved = np.moveaxis(np.empty(shape_x), dim, 0).shape
        return value, np.moveaxis(gx.reshape(moved), 0, dim), gt.reshape(shape_t)
    if family == "varreg":
        value, gx, gt = varreg_l1(x, t, extra)
        return value, gx.reshape(shape_x), gt.reshape(shape_t)
    return masked_mean(x, t, *extra)
