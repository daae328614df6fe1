"""torch fp64 restatement of the U-Net's forward + backward (gwen_amd.models_cnn with grad=True) from torch's own
functional ops and autograd, the gradient cases of tests/golden/ref_unet_grads.npz (written by
tests/golden/make_ref_unet_grads_golden.py from the reference's own classes), and the margin rule of the whole-model
gradient tests.  test_unet_grad_host.py shows that ``run`` below IS the reference: it reproduces the fixture's fp64
gradients to their fp32 rounding.

The margin rule.  A ReLU or a pool is a switch: if the device's forward and the fp64 yardstick disagree on ONE of them
the gradients differ by percents, and no tolerance may hide that.  So whole-model cases use inputs whose margin exceeds
the forward bound of the tier (10 helpers.LINEAR_TOL[tier]): for a ReLU input z, min|z| / max|z| over the tensor; for a
pool input c, the smallest (largest - second largest) over the windows divided by max|c|.  ``run`` returns the smallest
margin over every switch of the network (the second ReLU after a concatenation is no switch: it acts on non-negative
values and passes exactly what the first one passed).  A condition on the inputs, asserted -- never a filter.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn.functional as F

import unet_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_unet_grads.npz")

# name -> ((B, Cin, Cout, hidden, H, W), mode, seed s): weights unet_ref.make_state(cin, cout, hidden, s, flip=True),
# input default_rng(s + 100).standard_normal, cotangent default_rng(s + 200).standard_normal; the margin each must have
CASES = {
    "train_32": ((2, 3, 2, 64, 32, 32), "train", 1001),
    "eval_odd": ((1, 4, 2, 64, 35, 33), "eval", 1000),
    "eval_split": ((2, 124, 1, 128, 16, 16), "eval", 1003),
    "eval_x3": ((1, 3, 2, 64, 16, 16), "eval", 1002),
}
FIXTURE_CASES = ("train_32", "eval_odd")                 # pinned to the reference's own gradients
MARGIN = {"train_32": 2e-5, "eval_odd": 2e-5, "eval_split": 2e-5, "eval_x3": 2e-4}


def case_state(name):
    (_, cin, cout, hidden, _, _), _, s = CASES[name]
    return R.make_state(cin, cout, hidden, s, flip=True)


def case_input(name):
    (b, cin, _, _, h, w), _, s = CASES[name]
    return np.random.default_rng(s + 100).standard_normal((b, cin, h, w)).astype(np.float32)


def case_cotangent(name):
    (b, _, cout, _, h, w), _, s = CASES[name]
    return np.random.default_rng(s + 200).standard_normal(R.output_shape(b, cout, h, w)).astype(np.float32)


def used_keys(cin, cout, hidden):
    """the parameters the forward reads (running statistics excluded): the tensors that get a gradient"""
    return [k for k, _, used in R.state_spec(cin, cout, hidden)
            if used and k.rsplit(".", 1)[1] in ("weight", "bias")]


def zero_in_train(key):
    """a conv bias in front of a train-mode BatchNorm: its gradient is mathematically zero.  Returns the key of the
    matching BatchNorm's bias (whose gradient gives the scale), or None."""
    enc = {f"encoder.conv_layers.{i}.bias": f"encoder.batch_norm_layers.{i}.bias" for i in range(4)}
    dec = {f"decoder.conv_transposed_layers.{k}.bias": f"decoder.batch_norm_layers.{2 - k}.bias" for k in range(3)}
    return {**enc, **dec}.get(key)


def load_fixtures() -> dict:
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


# ---- the switches ----------------------------------------------------------------------------------------------------

def relu_margin(z):
    a = z.detach().abs()
    return float(a.min() / a.max())


def pool_margin(c):
    c = c.detach()
    b, ch, h, w = c.shape
    win = c[:, :, :h // 2 * 2, :w // 2 * 2].reshape(b, ch, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(b, ch, h // 2, w // 2, 4)
    top = win.topk(2, dim=-1).values
    return float((top[..., 0] - top[..., 1]).min() / c.abs().max())


def relu(z, mask=None):
    """ReLU; ``mask`` (bool, z's shape) replaces the sign test -- the device's own pattern"""
    return F.relu(z) if mask is None else z * mask.to(z.dtype)


def pool(c, argmax=None):
    """2x2 / stride 2 max-pool, floor rule; ``argmax`` (window position 0..3, [B, C, H/2, W/2]) replaces the comparison"""
    if argmax is None:
        return F.max_pool2d(c, 2)
    b, ch, h, w = c.shape
    win = c[:, :, :h // 2 * 2, :w // 2 * 2].reshape(b, ch, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(b, ch, h // 2, w // 2, 4)
    return win.gather(-1, argmax.long().unsqueeze(-1)).squeeze(-1)


def window_position(indices, w):
    """torch's flat max_pool2d indices (into H x W) -> the window position 0..3 in the order (0,0) (0,1) (1,0) (1,1)"""
    return ((indices // w) % 2) * 2 + (indices % w) % 2


# ---- the whole model -------------------------------------------------------------------------------------------------

def run(state: dict, x, cotangent, train: bool, switches: dict = None, dtype=torch.float64):
    """(out, {key or "input": gradient of (out * cotangent).sum()}, smallest margin) of the reference's UNet.forward.
    ``switches``: optional {"relu/<where>": bool mask, "pool/<i>": window positions} that replace the comparisons."""
    switches = switches or {}
    p = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in state.items()
         if k.rsplit(".", 1)[1] in ("weight", "bias")}
    stat = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in state.items()
            if k.rsplit(".", 1)[1] in ("running_mean", "running_var")}
    x = torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True)
    margins = []

    def bn(prefix, i, v):
        q = f"{prefix}batch_norm_layers.{i}."
        return F.batch_norm(v, stat[q + "running_mean"].clone(), stat[q + "running_var"].clone(), p[q + "weight"],
                            p[q + "bias"], training=train, momentum=R.MOMENTUM, eps=R.EPS)

    def act(z, where):
        margins.append(relu_margin(z))
        return relu(z, switches.get("relu/" + where))

    feats, v = [], x
    for i in range(4):
        c = F.conv2d(v, p[f"encoder.conv_layers.{i}.weight"], p[f"encoder.conv_layers.{i}.bias"], padding=1)
        margins.append(pool_margin(c))
        v = act(bn("encoder.", i, pool(c, switches.get(f"pool/{i}"))), f"enc{i}")
        feats.append(v)
    y = feats[3]
    for k, (i_bn, skip) in enumerate(((2, feats[2]), (1, feats[1]), (0, feats[0]))):
        q = f"decoder.conv_transposed_layers.{k}."
        y = F.interpolate(F.conv_transpose2d(y, p[q + "weight"], p[q + "bias"], padding=1), scale_factor=2,
                          mode="bilinear", align_corners=True)
        y = act(bn("decoder.", i_bn, y), f"dec{k}")
        (a0, a1), (b0, b1) = R.crop_range(skip.shape[2], y.shape[2]), R.crop_range(skip.shape[3], y.shape[3])
        y = F.relu(torch.cat([skip[:, :, a0:a1, b0:b1], y], dim=1))
    q = "decoder.conv_transposed_layers.3."
    y = act(F.interpolate(F.conv_transpose2d(y, p[q + "weight"], p[q + "bias"], padding=1), scale_factor=2,
                          mode="bilinear", align_corners=True), "dec3")
    out = F.conv2d(y, p["decoder.conv_layers.4.weight"], p["decoder.conv_layers.4.bias"])
    if x.shape[3] != out.shape[3]:
        out = F.pad(out, (x.shape[3] - out.shape[3], 0, 0, 0), mode="replicate")
    (out * torch.tensor(np.asarray(cotangent), dtype=dtype)).sum().backward()
    grads = {k: v.grad.numpy() for k, v in p.items() if v.grad is not None}
    grads["input"] = x.grad.numpy()
    return out.detach().numpy(), grads, min(margins)


def run_case(name, dtype=torch.float64):
    meta, mode, _ = CASES[name]
    return run(case_state(name), case_input(name), case_cotangent(name), mode == "train", dtype=dtype)


def decoder_inputs(name, seed=2100):
    """positive encoder maps [x1, x2, x3, x4] (what an encoder's ReLUs hand a decoder) for the shapes of a case"""
    (b, _, _, hidden, h, w), _, _ = CASES[name]
    r = np.random.default_rng(seed)
    sizes = [(hidden // 8, h // 2, w // 2), (hidden // 4, h // 4, w // 4), (hidden // 2, h // 8, w // 8),
             (hidden, h // 16, w // 16)]
    return [np.abs(r.standard_normal((b, c, a, d))).astype(np.float32) + 0.1 for c, a, d in sizes]


def run_decoder(state: dict, feats, cotangent=None, cot_seed=2101):
    """(out, the gradients of the four inputs, smallest ReLU margin, cotangent) of the reference's Decoder.forward in
    eval mode, fp64; ``state``: a whole state_dict (its ``decoder.`` part is read)."""
    st = {k[len("decoder."):]: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in state.items()
          if k.startswith("decoder.")}
    ts = [torch.tensor(f, dtype=torch.float64, requires_grad=True) for f in feats]
    y, margins = ts[3], []
    for k, (i_bn, skip) in enumerate(((2, ts[2]), (1, ts[1]), (0, ts[0]))):
        q, n = f"conv_transposed_layers.{k}.", f"batch_norm_layers.{i_bn}."
        y = F.interpolate(F.conv_transpose2d(y, st[q + "weight"], st[q + "bias"], padding=1), scale_factor=2,
                          mode="bilinear", align_corners=True)
        y = F.batch_norm(y, st[n + "running_mean"], st[n + "running_var"], st[n + "weight"], st[n + "bias"], eps=R.EPS)
        margins.append(relu_margin(y))
        (a0, a1), (b0, b1) = R.crop_range(skip.shape[2], y.shape[2]), R.crop_range(skip.shape[3], y.shape[3])
        y = F.relu(torch.cat([skip[:, :, a0:a1, b0:b1], F.relu(y)], dim=1))
    q = "conv_transposed_layers.3."
    y = F.interpolate(F.conv_transpose2d(y, st[q + "weight"], st[q + "bias"], padding=1), scale_factor=2,
                      mode="bilinear", align_corners=True)
    margins.append(relu_margin(y))
    out = F.conv2d(F.relu(y), st["conv_layers.4.weight"], st["conv_layers.4.bias"])
    if cotangent is None:
        cotangent = np.random.default_rng(cot_seed).standard_normal(tuple(out.shape)).astype(np.float32)
    (out * torch.tensor(cotangent, dtype=torch.float64)).sum().backward()
    return out.detach().numpy(), [t.grad.numpy() for t in ts], min(margins), cotangent
