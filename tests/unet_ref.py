"""numpy fp64 restatements of the U-Net (gwen_amd.models_cnn) and of its kernels, the weights every U-Net test uses, and
the fixture cases of tests/golden/ref_unet.npz (written by tests/golden/make_ref_unet_golden.py from the reference's own
classes).  Everything here is [B, C, H, W], as the reference's modules are; test_unet_host.py shows that ``forward``
below IS the reference (it reproduces the fixture's fp64 outputs to 1e-12).
"""
from __future__ import annotations

import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_unet.npz")
EPS = 1e-5
MOMENTUM = 0.1

# name -> (B, Cin, Cout, hidden, H, W), train mode too?, weight seed, input seed, flip the sign of some BN weights?
CASES = {
    "aligned": ((2, 3, 2, 64, 32, 48), True, 11, 111, False),
    "one_channel_crop": ((2, 1, 1, 64, 40, 37), True, 12, 112, True),
    "odd_both": ((1, 4, 2, 64, 17, 33), False, 13, 113, False),
    "ref_split": ((2, 124, 1, 128, 16, 16), False, 14, 114, False),
    "ref_width": ((2, 124, 1, 1024, 16, 16), False, 15, 115, False),
    "crop_pads": ((1, 2, 3, 64, 35, 50), False, 16, 116, True),
}


def modes(name):
    return ("eval", "train") if CASES[name][1] else ("eval",)


# ---- the parameter tree --------------------------------------------------------------------------------------------

def state_spec(cin: int, cout: int, hidden: int):
    """[(key, shape, used by the forward?)] in the reference's state_dict order."""
    h = hidden
    convs = [(h // 8, cin, 3, 3), (h // 4, h // 8, 3, 3), (h // 2, h // 4, 3, 3), (h, h // 2, 3, 3), (cout, cout, 1, 1)]
    tconvs = [(h, h // 2, 3, 3), (h, h // 4, 3, 3), (h // 2, h // 8, 3, 3), (h // 4, cout, 3, 3)]
    bns = [h // 8, h // 4, h // 2, h]
    used = {"encoder.": ({0, 1, 2, 3}, set(), {0, 1, 2, 3}), "decoder.": ({4}, {0, 1, 2, 3}, {0, 1, 2}), "": (set(), set(), set())}
    spec = []
    for prefix in ("", "encoder.", "decoder."):
        uc, ut, ub = used[prefix]
        for i, s in enumerate(convs):
            spec.append((f"{prefix}conv_layers.{i}.weight", s, i in uc))
            spec.append((f"{prefix}conv_layers.{i}.bias", (s[0],), i in uc))
        for i, s in enumerate(tconvs):
            spec.append((f"{prefix}conv_transposed_layers.{i}.weight", s, i in ut))
            spec.append((f"{prefix}conv_transposed_layers.{i}.bias", (s[1],), i in ut))
        for i, c in enumerate(bns):
            for leaf in ("weight", "bias", "running_mean", "running_var"):
                spec.append((f"{prefix}batch_norm_layers.{i}.{leaf}", (c,), i in ub))
            spec.append((f"{prefix}batch_norm_layers.{i}.num_batches_tracked", (), i in ub))
    return spec


def make_state(cin: int, cout: int, hidden: int, seed: int, flip: bool = False) -> dict:
    """key -> numpy array (fp32; num_batches_tracked int64) of a whole state_dict, from numpy.random.default_rng(seed),
    one draw per USED tensor in state_dict order: conv weights normal / sqrt(fan_in), biases N(0, 0.1), BN weight
    U(0.5, 1.5) (``flip``: every third one negative), BN bias and running_mean N(0, 0.1), running_var U(0.5, 1.5); the
    tensors the forward never reads are zeros."""
    g = np.random.default_rng(seed)
    state = {}
    for key, shape, used in state_spec(cin, cout, hidden):
        leaf = key.rsplit(".", 1)[1]
        if leaf == "num_batches_tracked":
            state[key] = np.zeros((), np.int64)
        elif not used:
            state[key] = np.zeros(shape, np.float32)
        elif "batch_norm" in key:
            if leaf in ("weight", "running_var"):
                v = g.uniform(0.5, 1.5, shape)
                if leaf == "weight" and flip:
                    v[::3] *= -1.0
            else:
                v = g.normal(0.0, 0.1, shape)
            state[key] = v.astype(np.float32)
        elif leaf == "bias":
            state[key] = g.normal(0.0, 0.1, shape).astype(np.float32)
        else:                                    # Conv2d [Cout, Cin, k, k] and ConvTranspose2d [Cin, Cout, k, k]:
            fan_in = shape[0 if "transposed" in key else 1] * shape[2] * shape[3]        # the contraction's length
            state[key] = (g.standard_normal(shape) / np.sqrt(fan_in)).astype(np.float32)
    return state


def make_input(name: str) -> np.ndarray:
    (b, cin, _, _, h, w), _, _, xseed, _ = CASES[name]
    return np.random.default_rng(xseed).standard_normal((b, cin, h, w)).astype(np.float32)


def case_state(name: str) -> dict:
    (_, cin, cout, hidden, _, _), _, wseed, _, flip = CASES[name]
    return make_state(cin, cout, hidden, wseed, flip)


def load_fixtures() -> dict:
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


# ---- the pieces (fp64) ---------------------------------------------------------------------------------------------

def conv3x3(x, w, b=None, transposed=False):
    """3x3, stride 1, padding 1.  ``transposed``: w is a ConvTranspose2d's [Cin, Cout, 3, 3]."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    if transposed:
        w = w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1]
    B, C, H, W = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    out = np.zeros((B, w.shape[0], H, W))
    for ky in range(3):
        for kx in range(3):
            out += np.tensordot(w[:, :, ky, kx], xp[:, :, ky:ky + H, kx:kx + W], axes=([1], [1])).transpose(1, 0, 2, 3)
    if b is not None:
        out += np.asarray(b, np.float64)[None, :, None, None]
    return out


def pool2x2(x):
    B, C, H, W = x.shape
    return x[:, :, :H // 2 * 2, :W // 2 * 2].reshape(B, C, H // 2, 2, W // 2, 2).max(axis=(3, 5))


def _lerp_axis(n):
    o = np.arange(2 * n, dtype=np.float64)
    src = o * ((n - 1) / (2 * n - 1)) if n > 1 else np.zeros(2)
    i0 = np.minimum(np.floor(src).astype(np.int64), n - 1)
    return i0, np.minimum(i0 + 1, n - 1), src - i0


def upsample2x(x):
    """bilinear, scale 2, align_corners=True"""
    x = np.asarray(x, np.float64)
    y0, y1, ly = _lerp_axis(x.shape[2])
    x0, x1, lx = _lerp_axis(x.shape[3])
    top = x[:, :, y0][:, :, :, x0] * (1 - lx) + x[:, :, y0][:, :, :, x1] * lx
    bot = x[:, :, y1][:, :, :, x0] * (1 - lx) + x[:, :, y1][:, :, :, x1] * lx
    return top * (1 - ly)[:, None] + bot * ly[:, None]


def batch_norm(x, weight, bias, running_mean, running_var, train):
    """(y, new running_mean, new running_var); train: batch statistics, momentum 0.1, unbiased running variance"""
    w, b = np.asarray(weight, np.float64), np.asarray(bias, np.float64)
    rm, rv = np.asarray(running_mean, np.float64), np.asarray(running_var, np.float64)
    if train:
        n = x.shape[0] * x.shape[2] * x.shape[3]
        mean, var = x.mean(axis=(0, 2, 3)), x.var(axis=(0, 2, 3))
        rm = (1 - MOMENTUM) * rm + MOMENTUM * mean
        rv = (1 - MOMENTUM) * rv + MOMENTUM * var * n / (n - 1)
    else:
        mean, var = rm, rv
    y = (x - mean[None, :, None, None]) / np.sqrt(var + EPS)[None, :, None, None] * w[None, :, None, None] \
        + b[None, :, None, None]
    return y, rm, rv


def crop_range(size, target):
    """the reference's Decoder.crop along one axis: an odd difference drops one more element at the start"""
    d = size - target
    return d // 2 + d % 2, size - d // 2


def output_shape(b, cout, h, w):
    """the height floors to a multiple of 16 (four pools, then the crops); the width is padded back on the left"""
    return b, cout, h // 16 * 16, w


def forward(state: dict, x, train: bool = False):
    """(output, {key: updated running statistic}) of the reference's UNet.forward in fp64"""
    x = np.asarray(x, np.float64)
    new = {}

    def bn(prefix, i, v):
        p = f"{prefix}batch_norm_layers.{i}."
        y, rm, rv = batch_norm(v, state[p + "weight"], state[p + "bias"], state[p + "running_mean"],
                               state[p + "running_var"], train)
        if train:
            new[p + "running_mean"], new[p + "running_var"] = rm, rv
            new[p + "num_batches_tracked"] = np.asarray(state[p + "num_batches_tracked"]) + 1
        return y

    feats, v = [], x
    for i in range(4):
        v = conv3x3(v, state[f"encoder.conv_layers.{i}.weight"], state[f"encoder.conv_layers.{i}.bias"])
        v = np.maximum(bn("encoder.", i, pool2x2(v)), 0.0)
        feats.append(v)
    y = feats[3]
    for k, (i_bn, skip) in enumerate(((2, feats[2]), (1, feats[1]), (0, feats[0]))):
        p = f"decoder.conv_transposed_layers.{k}."
        y = upsample2x(conv3x3(y, state[p + "weight"], state[p + "bias"], transposed=True))
        y = np.maximum(bn("decoder.", i_bn, y), 0.0)
        (a0, a1), (b0, b1) = crop_range(skip.shape[2], y.shape[2]), crop_range(skip.shape[3], y.shape[3])
        y = np.maximum(np.concatenate([skip[:, :, a0:a1, b0:b1], y], axis=1), 0.0)
    p = "decoder.conv_transposed_layers.3."
    y = np.maximum(upsample2x(conv3x3(y, state[p + "weight"], state[p + "bias"], transposed=True)), 0.0)
    w4 = np.asarray(state["decoder.conv_layers.4.weight"], np.float64)[:, :, 0, 0]
    out = np.einsum("bchw,oc->bohw", y, w4) + np.asarray(state["decoder.conv_layers.4.bias"], np.float64)[None, :, None, None]
    pad = x.shape[3] - out.shape[3]               # (the decoder's own pad is by 2 x 0: its crops leave nothing over)
    if pad:
        out = np.concatenate([np.repeat(out[:, :, :, :1], pad, axis=3), out], axis=3)
    return out, new
