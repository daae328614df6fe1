"""The U-Net kernels (csrc/conv.hip) and gwen_amd.UNet on the GPU, against the fp64 restatement of tests/unet_ref.py and the
reference's own numbers (tests/golden/ref_unet.npz).

Bounds.  Per op: helpers.rel_err <= helpers.LINEAR_TOL[tier], K3's own bound (the conv is the same arithmetic at
K = 9 Cin); the fp32-only kernels (upsample, affine) are held to the tighter of the two, 2e-6: a handful of fp32
roundings, each 6e-8 of the result.  A wrong tap, flip or halo is O(1), so every output channel and the two outermost
pixel rings are also held to 1e-3 of their OWN maximum.  Whole model, default tier: max |out - out64| <=
max(4 max|out32 - out64|, 10 LINEAR_TOL["bf16x6"] max|out64|) -- the reference's own fp32 distance from fp64 on that case
(x 4: the two fp32 summation orders differ), or ten contractions in sequence at the per-contraction bound; "3xbf16":
helpers.REL_TOL.  Every test prints the measured error and its share of the bound.
"""
import functools

import numpy as np
import pytest
import torch

import helpers
import unet_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TIERS = ("bf16x6", "3xbf16")
FP32_TOL = helpers.LINEAR_TOL["bf16x6"]


def _report(what, err, bound):
    print(f"{what}: err {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")


def _nhwc(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))


def _nchw(t):
    return t.detach().cpu().double().numpy().transpose(0, 3, 1, 2)


def _sliced(a_nhwc, left, right, fill):
    """(device buffer [B, H, W, left + C + right] filled with ``fill``, its channel slice holding ``a``)"""
    b, h, w, c = a_nhwc.shape
    buf = torch.full((b, h, w, left + c + right), fill, dtype=torch.float32, device=DEV)
    view = buf[..., left:left + c]
    view.copy_(torch.from_numpy(a_nhwc))
    return buf, view


# (Cin, Cout, H, W, B, transposed, pool, affine, relu, pitched): every channel count, image and batch of the issue, both
# layouts, all eight epilogues (pool on odd sizes with negative scale entries among them), pitched and packed rows
CONV_CASES = [
    (1, 1, 2, 2, 1, False, False, False, False, False),
    (3, 8, 5, 7, 3, True, True, True, True, True),
    (16, 24, 16, 16, 1, False, True, False, False, False),
    (124, 64, 18, 35, 1, True, False, True, False, True),
    (136, 136, 5, 7, 3, False, False, False, True, False),
    (3, 136, 18, 35, 3, False, True, True, False, True),
    (16, 1, 16, 16, 3, True, False, True, True, False),
    (124, 8, 2, 2, 3, False, True, False, True, True),
    (136, 24, 18, 35, 1, True, True, True, True, False),
    (1, 64, 5, 7, 1, False, False, False, False, True),
    # images large enough that a block keeps more than one tile of 16 output channels (the launcher's plan: every
    # case above runs one tile a block): 4, 3 and 2 tiles, with a 16-byte-aligned Cin (vector loads) and without,
    # channel counts that leave the last block a partial group, pool on odd sizes
    (8, 128, 128, 128, 1, False, True, False, False, False),
    (3, 128, 127, 129, 1, True, True, True, True, False),
    (12, 136, 128, 128, 1, False, False, True, False, False),
    (12, 112, 96, 128, 1, True, True, False, True, False),
    (5, 48, 128, 128, 1, False, False, False, False, True),
    (3, 112, 96, 128, 2, False, False, True, True, True),
    (16, 48, 128, 128, 1, True, True, True, False, False),
]
# case index -> (output-channel tiles a block, slices of Cin) the launcher's plan gives it (gwen_conv3x3_plan); the
# first ten: one tile, and two slices from 124 input channels on
CONV_PLAN = {0: (1, 1), 1: (1, 1), 2: (1, 1), 3: (1, 2), 4: (1, 2), 5: (1, 1), 6: (1, 1), 7: (1, 2), 8: (1, 2),
             9: (1, 1), 10: (4, 1), 11: (4, 1), 12: (4, 1), 13: (3, 1), 14: (2, 1), 15: (3, 1), 16: (2, 1)}


def _plan_of(i):
    import ctypes
    from gwen_amd import _lib
    cin, cout, h, w, _, _, pool, *_ = CONV_CASES[i]
    nct, nz = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = _lib.lib().gwen_conv3x3_plan(h, w, cin, cout, _lib.CONV_POOL if pool else 0, ctypes.byref(nct), ctypes.byref(nz))
    assert rc == 0
    return nct.value, nz.value


@functools.lru_cache(maxsize=None)
def _conv_case(i):
    cin, cout, h, w, b, transposed, pool, affine, relu, _ = CONV_CASES[i]
    g = np.random.default_rng(500 + i)
    x = g.standard_normal((b, cin, h, w)).astype(np.float32)
    wshape = (cin, cout, 3, 3) if transposed else (cout, cin, 3, 3)
    wt = (g.standard_normal(wshape) / np.sqrt(9 * cin)).astype(np.float32)
    bias = g.normal(0, 0.1, cout).astype(np.float32)
    scale = g.uniform(0.5, 1.5, cout).astype(np.float32)
    scale[::2] *= -1.0
    shift = g.normal(0, 0.1, cout).astype(np.float32)
    want = R.conv3x3(x, wt, bias, transposed)
    if pool:
        want = R.pool2x2(want)
    if affine:
        want = want * scale.astype(np.float64)[None, :, None, None] + shift.astype(np.float64)[None, :, None, None]
    if relu:
        want = np.maximum(want, 0.0)
    return x, wt, bias, scale, shift, want


def _own_maximum_checks(got, want, what):
    """every output channel and the two outermost pixel rings against their own maximum at 1e-3"""
    diff = np.abs(got - want)
    whole = np.abs(want).max()
    worst = 0.0
    for c in range(want.shape[1]):
        scale = np.abs(want[:, c]).max() or whole
        worst = max(worst, diff[:, c].max() / scale)
    h, w = want.shape[2:]
    for d in range(2):
        if h > 2 * d and w > 2 * d:
            ring = np.zeros((h, w), bool)
            ring[d:h - d, d:w - d] = True
            if h > 2 * d + 2 and w > 2 * d + 2:
                ring[d + 1:h - d - 1, d + 1:w - d - 1] = False
            scale = np.abs(want[:, :, ring]).max() or whole
            worst = max(worst, diff[:, :, ring].max() / scale)
    _report(what + " worst channel / ring", worst, 1e-3)
    assert worst <= 1e-3


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("i", range(len(CONV_CASES)))
def test_conv3x3(i, tier):
    from gwen_amd import ops
    cin, cout, h, w, b, transposed, pool, affine, relu, pitched = CONV_CASES[i]
    assert _plan_of(i) == CONV_PLAN[i]                 # the case runs the kernel instantiation it is here for
    x, wt, bias, scale, shift, want = _conv_case(i)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    out = None
    if pitched:            # NaN all around the input slice: nothing beside the Cin channels may enter; a sentinel around the output
        _, xv = _sliced(_nhwc(x), 2, 3, float("nan"))
        obuf, out = _sliced(np.zeros((b,) + want.shape[2:] + (cout,), np.float32), 1, 2, 7.0)
    else:
        xv = dev(_nhwc(x))
    got = ops.conv3x3(xv, dev(wt), dev(bias), transposed=transposed, pool=pool,
                      affine=(dev(scale), dev(shift)) if affine else None, relu=relu, contract=tier, out=out)
    assert tuple(got.shape) == (b,) + want.shape[2:] + (cout,)
    if pitched:
        assert got.data_ptr() == out.data_ptr()
        assert bool((obuf[..., :1] == 7.0).all()) and bool((obuf[..., 1 + cout:] == 7.0).all())
    got = _nchw(got)
    if want.size == 0:
        return
    err = helpers.rel_err(got, want)
    what = f"conv3x3 {CONV_CASES[i]} {tier}"
    _report(what, err, helpers.LINEAR_TOL[tier])
    assert err <= helpers.LINEAR_TOL[tier]
    _own_maximum_checks(got, want, what)


def test_conv3x3_packed_image_follows_the_weight_version():
    from gwen_amd import ops
    x, wt, bias, *_ = _conv_case(2)
    xv, w, b = (torch.from_numpy(a).to(DEV) for a in (_nhwc(x), wt, bias))
    img = ops.conv3x3_pack(w)
    assert ops.conv3x3_pack(w) is img                              # cached per version
    other = ops.conv3x3_pack(w, contract="3xbf16")
    assert other is not img and other.numel() * 3 == img.numel() * 2
    assert ops.conv3x3_pack(w) is img and ops.conv3x3_pack(w, contract="3xbf16") is other   # two tiers, no repacking
    first = ops.conv3x3(xv, w, b)
    w.mul_(2.0)
    assert ops.conv3x3_pack(w) is not img
    second = ops.conv3x3(xv, w, None)
    want = R.conv3x3(x, 2.0 * wt.astype(np.float64))
    assert helpers.rel_err(_nchw(second), want) <= helpers.LINEAR_TOL["bf16x6"]
    assert not torch.equal(first, second)
    with pytest.raises(ValueError):
        ops.conv3x3(xv[..., :3], w, b)                             # channel count does not match the weight
    with pytest.raises(ValueError):
        ops.conv3x3(xv.permute(0, 3, 1, 2), w, b)                  # not channels-last rows


@pytest.mark.parametrize("epilogue", [False, True])
@pytest.mark.parametrize("size", [(1, 1), (2, 3), (9, 5)])
def test_upsample2x(size, epilogue):
    from gwen_amd import ops
    h, w = size
    b, c = 2, 5
    g = np.random.default_rng(600 + 10 * h + w)
    x = g.standard_normal((b, c, h, w)).astype(np.float32)
    scale = g.uniform(0.5, 1.5, c).astype(np.float32)
    scale[1] *= -1.0
    shift = g.normal(0, 0.1, c).astype(np.float32)
    want = R.upsample2x(x)
    if epilogue:
        want = np.maximum(want * scale.astype(np.float64)[None, :, None, None] + shift.astype(np.float64)[None, :, None, None], 0.0)
    _, xv = _sliced(_nhwc(x), 1, 1, float("nan"))
    obuf, out = _sliced(np.zeros((b, 2 * h, 2 * w, c), np.float32), 3, 2, 7.0)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    got = ops.upsample2x(xv, affine=(dev(scale), dev(shift)) if epilogue else None, relu=epilogue, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert bool((obuf[..., :3] == 7.0).all()) and bool((obuf[..., 3 + c:] == 7.0).all())
    err = helpers.rel_err(_nchw(got), want)
    _report(f"upsample2x {size} epilogue={epilogue}", err, FP32_TOL)
    assert err <= FP32_TOL
    if h == 1:                                                     # both output rows copy the input row
        assert torch.equal(got[:, 0], got[:, 1])
    packed = ops.upsample2x(xv.contiguous(), affine=(dev(scale), dev(shift)) if epilogue else None, relu=epilogue)
    assert torch.equal(packed, got)


@pytest.mark.parametrize("rows", [2, 8, 4099])
def test_channel_stats(rows):
    from gwen_amd import ops
    c = 70                                                         # more than one block of 64 channels
    g = np.random.default_rng(700 + rows)
    x = (0.5 + g.standard_normal((rows, c))).astype(np.float32)
    buf = torch.full((rows, c + 9), float("nan"), dtype=torch.float32, device=DEV)
    view = buf[:, 4:4 + c]
    view.copy_(torch.from_numpy(x))
    mean, var = ops.channel_stats(view)
    assert mean.dtype == torch.float64 and var.dtype == torch.float64
    x64 = x.astype(np.float64)
    for name, got, want in (("mean", mean, x64.mean(0)), ("var", var, x64.var(0))):
        err = helpers.rel_err(got, want)
        _report(f"channel_stats rows={rows} {name}", err, 1e-12)
        assert err <= 1e-12
    again = ops.channel_stats(view)
    assert torch.equal(again[0], mean) and torch.equal(again[1], var)
    v4 = buf.view(1, 1, rows, c + 9)[..., 4:4 + c]                 # the same rows as a channels-last tensor
    m4, _ = ops.channel_stats(v4)
    assert torch.equal(m4, mean)


def test_affine_relu_in_place_on_a_slice():
    from gwen_amd import ops
    g = np.random.default_rng(800)
    x = g.standard_normal((2, 3, 5, 6)).astype(np.float32)         # [B, H, W, C]
    scale, shift = g.uniform(-1.5, 1.5, 6).astype(np.float32), g.normal(0, 0.1, 6).astype(np.float32)
    buf, view = _sliced(x, 2, 1, 7.0)
    ops.affine_relu_(view, torch.from_numpy(scale).to(DEV), torch.from_numpy(shift).to(DEV))
    want = np.maximum(x.astype(np.float64) * scale + shift, 0.0)
    err = helpers.rel_err(view, want)
    _report("affine_relu_", err, FP32_TOL)
    assert err <= FP32_TOL
    assert bool((buf[..., :2] == 7.0).all()) and bool((buf[..., 8:] == 7.0).all())


# ---- the whole model -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fixtures():
    return R.load_fixtures()


def _model(name, precision="bf16x6", train=False):
    import gwen_amd
    (_, cin, cout, hidden, _, _) = R.CASES[name][0]
    model = gwen_amd.UNet(cin, cout, hidden, precision=precision)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in R.case_state(name).items()}, strict=True)
    return model.to(DEV).train(train)


def _model_bound(out32, out64):
    return max(4.0 * np.abs(out32.astype(np.float64) - out64).max(),
               10.0 * helpers.LINEAR_TOL["bf16x6"] * np.abs(out64).max())


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", list(R.CASES))
def test_model_eval(fixtures, name, tier):
    model = _model(name, tier)
    x = torch.from_numpy(R.make_input(name)).to(DEV)
    with torch.no_grad():
        out = model(x)
    out64 = fixtures[f"{name}/eval/out64"]
    assert tuple(out.shape) == out64.shape
    got = out.cpu().double().numpy()
    if tier == "bf16x6":
        err, bound = np.abs(got - out64).max(), _model_bound(fixtures[f"{name}/eval/out32"], out64)
    else:
        err, bound = helpers.rel_err(got, out64), helpers.REL_TOL
    _report(f"UNet eval {name} {tier}", err, bound)
    assert err <= bound


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", [n for n in R.CASES if R.CASES[n][1]])
def test_model_train(fixtures, name, tier):
    model = _model(name, tier, train=True)
    x = torch.from_numpy(R.make_input(name)).to(DEV)
    with torch.no_grad():
        out = model(x)
    out64 = fixtures[f"{name}/train/out64"]
    got = out.cpu().double().numpy()
    assert got.shape == out64.shape
    if tier == "bf16x6":
        err, bound = np.abs(got - out64).max(), _model_bound(fixtures[f"{name}/train/out32"], out64)
    else:
        err, bound = helpers.rel_err(got, out64), helpers.REL_TOL
    _report(f"UNet train {name} {tier}", err, bound)
    assert err <= bound
    sd = model.state_dict()
    prefix = f"{name}/train/stats64/"
    keys = [k[len(prefix):] for k in fixtures if k.startswith(prefix)]
    assert len(keys) == 7 * 3                                      # seven BatchNorms run, three buffers each
    worst = 0.0
    for key in keys:
        want, got = fixtures[prefix + key], sd[key].cpu().numpy()
        if key.endswith("num_batches_tracked"):
            assert int(got) == int(want) == 1
            continue
        if tier == "bf16x6":
            err, bound = np.abs(got - want).max(), _model_bound(fixtures[f"{name}/train/stats32/{key}"], want)
        else:
            err, bound = helpers.rel_err(got, want), helpers.REL_TOL
        worst = max(worst, err / bound)
        assert err <= bound, (key, err, bound)
    _report(f"UNet train {name} {tier} running statistics, worst share of its bound", worst, 1.0)
    for key, v in sd.items():                                      # the BatchNorms the forward never runs stay put
        if "running" in key and key not in keys:
            assert torch.equal(v.cpu(), torch.from_numpy(np.asarray(R.case_state(name)[key]))), key


def test_reproducible_and_contained():
    name = "aligned"
    model = _model(name)
    g = np.random.default_rng(900)
    x = torch.from_numpy(g.standard_normal((3, 3, 32, 48)).astype(np.float32)).to(DEV)
    with torch.no_grad():
        a, b = model(x), model(x)
        assert torch.equal(a, b)                                   # run to run
        alone = model(x[:1].contiguous())
        assert torch.equal(alone[0], a[0])                         # an item's bits do not depend on the batch
        bad = x.clone()
        bad[0, 1, 5, 7] = float("nan")
        c = model(bad)
        assert torch.isnan(c[0]).any()
        assert torch.equal(c[1], a[1]) and torch.equal(c[2], a[2])  # a NaN stays in its item
        # hipGraph replay of the eval forward: the eager bits
        static = x.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model(static)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = model(static)
        static.copy_(x.flip(0))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, model(x.flip(0)))
        static.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, a)


def test_train_forward_is_graph_capturable_after_one_eager_call():
    name = "aligned"
    model = _model(name, train=True)
    x = torch.from_numpy(R.make_input(name)).to(DEV)
    with torch.no_grad():
        first = model(x)                                           # eager: packs the weights
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model(x)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = model(x)
        before = int(model.encoder.batch_norm_layers[0].num_batches_tracked)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(y, first)                                   # batch statistics: the output does not depend on the running ones
    assert int(model.encoder.batch_norm_layers[0].num_batches_tracked) == before + 1
