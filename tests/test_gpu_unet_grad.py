"""The U-Net backward on the GPU (csrc/conv_bwd.hip, gwen_conv3x3_argmax_f32, gwen_amd.UNet(grad=True)): every raw op
against an fp64 yardstick, the whole model against the reference's own gradients (tests/golden/ref_unet_grads.npz) and
against the torch fp64 restatement of tests/unet_grad_ref.py.

Bounds.  Weight gradient: helpers.rel_err <= helpers.GRAD_W_TOL[tier] (the GCN weight gradient's bound: the same split
contraction over rows), and each of the nine taps to 1e-3 of its own maximum (a wrong tap or flip is O(1)).  The fp32
kernels: 2e-6 (a handful of fp32 roundings), their fp64 sums 1e-12, the argmax and the unpool exact.  Data gradient:
adjointness within helpers.LINEAR_TOL[tier].  Whole model: per tensor max|g - g64| <= max(4 err32, 10 GRAD_W_TOL[tier]
max|g64|) -- the reference's own fp32 distance from fp64 (x 4: the two fp32 summation orders differ), or ten
contractions in sequence.  A ReLU or pool that switches differently on the device than in fp64 would move a gradient
by percents, so the raw-op tests hand the yardstick the device's own mask and argmax, and the whole-model cases are
inputs whose switch margin exceeds the tier's forward bound (unet_grad_ref, asserted here): nothing is dropped or
capped.  "3xbf16" in train mode has no whole-model case at a testable size (no seed has the margin): that tier's
train path is pinned by the raw ops.  Every test prints the measured error and its share of the bound.
"""
import functools

import numpy as np
import pytest
import torch

import helpers
import unet_ref as R
import unet_grad_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TIERS = ("bf16x6", "3xbf16")
FP32_TOL = helpers.LINEAR_TOL["bf16x6"]


def _report(what, err, bound):
    print(f"{what}: err {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")


def _nhwc(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))


def _sliced(a_nhwc, left, right, fill):
    """(device buffer [B, H, W, left + C + right] filled with ``fill``, its channel slice holding ``a``)"""
    b, h, w, c = a_nhwc.shape
    buf = torch.full((b, h, w, left + c + right), fill, dtype=torch.float32, device=DEV)
    view = buf[..., left:left + c]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a_nhwc)))
    return buf, view


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- 1. the weight gradient ------------------------------------------------------------------------------------------

# (Cin, Cout, H, W, B, transposed, pitched); the last one is where a chunk holds more than one pixel tile
WGRAD_CASES = [
    (1, 1, 2, 2, 1, False, False),
    (3, 8, 5, 7, 3, True, True),
    (16, 24, 16, 16, 1, False, False),
    (124, 64, 18, 35, 1, True, True),
    (136, 136, 5, 7, 3, False, False),
    (5, 48, 40, 33, 2, False, True),
    (64, 32, 8, 8, 2, True, False),
    (12, 136, 64, 64, 2, False, False),
    (136, 136, 32, 64, 3, False, False),
]
# case -> (channel tiles of 16 x 16 per block, pixel chunks) of gwen_conv3x3_grad_weight_plan: one and several of both
WGRAD_PLAN = {0: (1, 1), 1: (1, 3), 2: (2, 2), 3: (4, 9), 4: (4, 3), 5: (2, 30), 6: (4, 2), 7: (2, 64), 8: (4, 24)}


@functools.lru_cache(maxsize=None)
def _wgrad_case(i):
    cin, cout, h, w, b, transposed, _ = WGRAD_CASES[i]
    r = np.random.default_rng(1500 + i)
    g = r.standard_normal((b, cout, h, w)).astype(np.float32)
    x = r.standard_normal((b, cin, h, w)).astype(np.float32)
    xp = np.pad(x.astype(np.float64), ((0, 0), (0, 0), (1, 1), (1, 1)))
    g64 = g.astype(np.float64)
    want = np.empty((cout, cin, 3, 3))
    for ky in range(3):
        for kx in range(3):
            want[:, :, ky, kx] = np.einsum("bohw,bihw->oi", g64, xp[:, :, ky:ky + h, kx:kx + w], optimize=True)
    if transposed:
        want = np.ascontiguousarray(want.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])
    return g, x, want


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("i", range(len(WGRAD_CASES)))
def test_conv3x3_grad_weight(i, tier):
    from gwen_amd import ops
    cin, cout, h, w, b, transposed, pitched = WGRAD_CASES[i]
    assert ops.conv3x3_grad_weight_plan(b, h, w, cin, cout) == WGRAD_PLAN[i]
    g, x, want = _wgrad_case(i)
    if pitched:                                       # NaN all around both slices: nothing beside them may enter
        _, gv = _sliced(_nhwc(g), 3, 2, float("nan"))
        _, xv = _sliced(_nhwc(x), 2, 3, float("nan"))
    else:
        gv, xv = _dev(_nhwc(g)), _dev(_nhwc(x))
    got = ops.conv3x3_grad_weight(gv, xv, transposed=transposed, contract=tier)
    assert tuple(got.shape) == want.shape
    err = helpers.rel_err(got, want)
    _report(f"conv3x3_grad_weight case {i} {tier}", err, helpers.GRAD_W_TOL[tier])
    gn = got.cpu().double().numpy()
    worst = max(np.abs(gn[:, :, a, c] - want[:, :, a, c]).max() / np.abs(want[:, :, a, c]).max()
                for a in range(3) for c in range(3) if np.abs(want[:, :, a, c]).max() > 0)
    _report(f"conv3x3_grad_weight case {i} {tier} worst tap", worst, 1e-3)
    assert err <= helpers.GRAD_W_TOL[tier]
    assert worst <= 1e-3
    assert torch.equal(ops.conv3x3_grad_weight(gv, xv, transposed=transposed, contract=tier), got)


# ---- 2. the pool's argmax --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("cin", [1, 124])
def test_conv3x3_argmax_rule(cin, tier):
    """A weight that is 1 at the centre tap of one input channel copies that channel: integer inputs of at most 8
    significant bits are exact on both tiers, so planted ties and NaNs meet the comparison itself."""
    from gwen_amd import ops, _lib
    import ctypes
    b, h, w, cout, pick = 2, 9, 11, 3, cin // 2
    r = np.random.default_rng(1600 + cin)
    x = r.integers(-100, 101, (b, cin, h, w)).astype(np.float32)
    ch = x[:, pick]
    ch[0, 0:2, 0:2] = 7.0                                        # a four-way tie: the first wins
    ch[0, 2:4, 2:4] = [[1.0, 5.0], [5.0, 5.0]]                   # a tie of three: (0, 1) wins
    ch[0, 4:6, 0:2] = [[np.nan, 3.0], [200.0, np.nan]]           # the last NaN wins
    ch[1, 0:2, 4:6] = [[9.0, np.nan], [50.0, 60.0]]              # a NaN is not displaced by a larger value
    ch[1, 6:8, 6:8] = [[-5.0, -5.0], [-4.0, -4.0]]
    wt = np.zeros((cout, cin, 3, 3), np.float32)
    wt[:, pick, 1, 1] = [1.0, -1.0, 2.0]
    bias = np.array([0.5, -1.0, 0.0], np.float32)
    scale, shift = np.array([-1.5, 0.5, 1.0], np.float32), np.array([0.25, 0.0, -3.0], np.float32)
    nct, nz = ctypes.c_int(-1), ctypes.c_int(-1)
    assert _lib.lib().gwen_conv3x3_plan(h, w, cin, cout, _lib.CONV_POOL, ctypes.byref(nct), ctypes.byref(nz)) == 0
    assert (nz.value > 1) == (cin == 124)                        # 124 channels take the Cin-split path
    xv, wd, bd = _dev(_nhwc(x)), _dev(wt), _dev(bias)
    for affine, relu in ((None, False), ((_dev(scale), _dev(shift)), True)):
        plain = ops.conv3x3(xv, wd, bd, pool=True, affine=affine, relu=relu, contract=tier)
        out, am, pre = ops.conv3x3(xv, wd, bd, pool=True, affine=affine, relu=relu, contract=tier, argmax=True)
        assert am.dtype == torch.uint8
        assert torch.equal(out.view(torch.int32), plain.view(torch.int32))                   # NaN bits included
        # (a NaN reaches its whole 3 x 3 neighbourhood through the zero taps, on the device as in torch's conv2d)
        conv = torch.nn.functional.conv2d(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(wt.astype(np.float64)),
                                          padding=1)
        pooled, idx = torch.nn.functional.max_pool2d(conv, 2, return_indices=True)
        want_am = G.window_position(idx, w).permute(0, 2, 3, 1).to(torch.uint8)
        assert torch.equal(am.cpu(), want_am)
        want_pre = (pooled + torch.from_numpy(bias.astype(np.float64)).view(1, 3, 1, 1)).permute(0, 2, 3, 1).float()
        assert torch.equal(torch.nan_to_num(pre.cpu(), nan=12345.0), torch.nan_to_num(want_pre, nan=12345.0))
        assert torch.equal(torch.isnan(pre.cpu()), torch.isnan(want_pre))
    with pytest.raises(ValueError, match="argmax needs pool"):
        ops.conv3x3(xv, wd, bd, argmax=True)


# ---- 3. the upsample's adjoint ---------------------------------------------------------------------------------------

def _up_matrix(n):
    """[2n, n] fp64: the bilinear x2 / align_corners map along one axis, from unet_ref._lerp_axis"""
    i0, i1, l = R._lerp_axis(n)
    m = np.zeros((2 * n, n))
    for o in range(2 * n):
        m[o, i0[o]] += 1.0 - l[o]
        m[o, i1[o]] += l[o]
    return m


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("size", [(1, 1), (2, 3), (9, 5)])
def test_upsample2x_backward(size, masked):
    from gwen_amd import ops
    h, w = size
    b, c = 2, 5
    r = np.random.default_rng(1700 + 10 * h + w)
    g = r.standard_normal((b, 2 * h, 2 * w, c)).astype(np.float32)
    y = r.standard_normal((b, 2 * h, 2 * w, c)).astype(np.float32)
    _, gv = _sliced(g, 2, 1, float("nan"))
    _, yv = _sliced(y, 1, 3, float("nan"))
    buf, ov = _sliced(np.zeros((b, h, w, c), np.float32), 2, 2, 7.0)
    got = ops.upsample2x_backward(gv, mask_from=yv if masked else None, out=ov)
    gm = g.astype(np.float64) * ((y > 0) if masked else 1.0)
    want = np.einsum("oh,pw,bopc->bhwc", _up_matrix(h), _up_matrix(w), gm)
    err = helpers.rel_err(got, want)
    _report(f"upsample2x_backward {size} masked={masked}", err, FP32_TOL)
    assert err <= FP32_TOL
    assert bool((buf[..., :2] == 7.0).all()) and bool((buf[..., 2 + c:] == 7.0).all())
    assert torch.equal(ops.upsample2x_backward(gv.contiguous(), mask_from=yv.contiguous() if masked else None), got)
    # <up(x), g> = <x, up^T(g)> with the device's own forward
    x = _dev(r.standard_normal((b, h, w, c)).astype(np.float32))
    lhs = float((ops.upsample2x(x).double() * _dev(g).double()).sum())
    rhs = float((x.double() * ops.upsample2x_backward(_dev(g)).double()).sum())
    scale = float((ops.upsample2x(x).double() * _dev(g).double()).abs().sum())
    _report(f"upsample2x adjointness {size}", abs(lhs - rhs) / scale, FP32_TOL)
    assert abs(lhs - rhs) <= FP32_TOL * scale


# ---- 4. ReLU + BatchNorm backward, unpool ----------------------------------------------------------------------------

@pytest.mark.parametrize("train", [True, False])
def test_norm_relu_backward(train):
    from gwen_amd import ops
    b, h, w, c = 2, 3, 5, 70                                       # more than one block of 64 channels
    r = np.random.default_rng(1800 + train)
    pre = (0.3 + r.standard_normal((b, h, w, c))).astype(np.float32)
    gy = r.standard_normal((b, h, w, c)).astype(np.float32)
    gamma = r.uniform(0.5, 1.5, c).astype(np.float32)
    gamma[::3] *= -1.0
    beta = r.normal(0, 0.1, c).astype(np.float32)
    _, pv = _sliced(pre, 2, 3, float("nan"))
    _, gv = _sliced(gy, 1, 1, float("nan"))
    if train:
        mean, var = ops.channel_stats(pv)
    else:
        mean, var = _dev(r.normal(0, 0.1, c)), _dev(r.uniform(0.5, 1.5, c))
    rstd = torch.rsqrt(var + R.EPS)
    ybuf = torch.full((b, h, w, c + 4), float("nan"), dtype=torch.float32, device=DEV)
    yv = ybuf[..., 2:2 + c]
    yv.copy_(pv)
    s = gamma.astype(np.float64) * rstd.cpu().numpy()
    ops.affine_relu_(yv, _dev(s.astype(np.float32)), _dev((beta - mean.cpu().numpy() * s).astype(np.float32)))
    g_pre, g_gamma, g_beta = ops.norm_relu_backward(gv, yv, pv, _dev(gamma), mean, rstd, train)
    assert g_gamma.dtype == torch.float64 and g_beta.dtype == torch.float64
    # the formulas in fp64, on the device's own y as the mask
    m64, r64, n = mean.cpu().numpy(), rstd.cpu().numpy(), b * h * w
    gz = gy.astype(np.float64) * (yv.cpu().numpy() > 0)
    xh = (pre.astype(np.float64) - m64) * r64
    want_beta, want_gamma = gz.sum((0, 1, 2)), (gz * xh).sum((0, 1, 2))
    want = gamma * r64 * ((gz - want_beta / n - xh * want_gamma / n) if train else gz)
    for name, got, ref, bound in (("g_pre", g_pre, want, FP32_TOL), ("g_weight", g_gamma, want_gamma, 1e-12),
                                  ("g_bias", g_beta, want_beta, 1e-12)):
        err = helpers.rel_err(got, ref)
        _report(f"norm_relu_backward train={train} {name}", err, bound)
        assert err <= bound
    again = ops.norm_relu_backward(gv, yv, pv, _dev(gamma), mean, rstd, train)
    assert all(torch.equal(a, b_) for a, b_ in zip(again, (g_pre, g_gamma, g_beta)))


@pytest.mark.parametrize("size", [(4, 6), (5, 7), (1, 3)])
def test_unpool2x2(size):
    from gwen_amd import ops
    h, w = size
    b, c = 2, 70
    r = np.random.default_rng(1900 + h)
    gp = r.standard_normal((b, h // 2, w // 2, c)).astype(np.float32)
    am = r.integers(0, 4, (b, h // 2, w // 2, c)).astype(np.uint8)
    _, gv = _sliced(gp, 1, 2, float("nan"))
    got = ops.unpool2x2(gv, _dev(am), h, w).cpu().numpy()
    want = np.zeros((b, h, w, c), np.float32)
    for k in range(4):
        want[:, k // 2:h // 2 * 2:2, k % 2:w // 2 * 2:2][am == k] = gp[am == k]
    assert np.array_equal(got, want)                               # zeros in the odd last row / column too


# ---- 5. the data gradient is the convolution with the weight read as the other type ----------------------------------

@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("layer_transposed", [False, True])
@pytest.mark.parametrize("shape", [(124, 64, 18, 35), (3, 8, 5, 7)])
def test_data_gradient_adjointness(shape, layer_transposed, tier):
    from gwen_amd import ops
    cin, cout, h, w = shape
    r = np.random.default_rng(2000 + cin)
    x = _dev(r.standard_normal((2, h, w, cin)).astype(np.float32))
    g = _dev(r.standard_normal((2, h, w, cout)).astype(np.float32))
    wshape = (cin, cout, 3, 3) if layer_transposed else (cout, cin, 3, 3)
    wt = _dev((r.standard_normal(wshape) / np.sqrt(9 * cin)).astype(np.float32))
    y = ops.conv3x3(x, wt, None, transposed=layer_transposed, contract=tier)
    gx = ops.conv3x3(g, wt, None, transposed=not layer_transposed, contract=tier)
    assert tuple(gx.shape) == tuple(x.shape)
    lhs, rhs = float((y.double() * g.double()).sum()), float((x.double() * gx.double()).sum())
    scale = float((y.double() * g.double()).abs().sum())
    _report(f"conv3x3 adjointness {shape} transposed={layer_transposed} {tier}", abs(lhs - rhs) / scale,
            helpers.LINEAR_TOL[tier])
    assert abs(lhs - rhs) <= helpers.LINEAR_TOL[tier] * scale


# ---- 6 / 7. the whole model ------------------------------------------------------------------------------------------

def _model(name, precision="bf16x6", cls="UNet"):
    import gwen_amd
    from gwen_amd import models_cnn
    (_, cin, cout, hidden, _, _), mode, _ = G.CASES[name]
    model = getattr(models_cnn, cls)(cin, cout, hidden, precision=precision, grad=True)
    state = G.case_state(name)
    if cls != "UNet":
        prefix = cls.lower() + "."
        state = {k[len(prefix):]: v for k, v in state.items() if k.startswith(prefix)}
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}, strict=True)
    return model.to(DEV).train(mode == "train")


def _device_grads(name, precision):
    model = _model(name, precision)
    x = _dev(G.case_input(name)).requires_grad_()
    out = model(x)
    assert out.requires_grad
    (out * _dev(G.case_cotangent(name))).sum().backward()
    grads = {k: (None if p.grad is None else p.grad.cpu().double().numpy()) for k, p in model.named_parameters()}
    grads["input"] = x.grad.cpu().double().numpy()
    return out.detach().cpu().double().numpy(), grads


def _check_grads(name, grads, g64, err32, tier):
    (_, cin, cout, hidden, _, _), mode, _ = G.CASES[name]
    worst = 0.0
    for key in G.used_keys(cin, cout, hidden) + ["input"]:
        want = np.asarray(g64[key], np.float64)
        scale_key = G.zero_in_train(key) if mode == "train" else None
        scale = np.abs(np.asarray(g64[scale_key if scale_key else key], np.float64)).max()
        assert scale > 0.0, f"{key}: a dead gradient"              # every gradient that is not mathematically zero lives
        bound = max(4.0 * float(err32.get(key, 0.0)), 10.0 * helpers.GRAD_W_TOL[tier] * scale)
        err = np.abs(grads[key] - want).max()
        print(f"  {name} {tier} {key}: err {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
        worst = max(worst, err / bound)
    _report(f"UNet gradients {name} {tier}, worst share of its bound", worst, 1.0)
    unused = [k for k, v in grads.items() if v is None]
    assert sorted(unused) == sorted(k for k, _, u in R.state_spec(cin, cout, hidden)
                                    if not u and k.rsplit(".", 1)[1] in ("weight", "bias"))
    assert worst <= 1.0


@pytest.fixture(scope="module")
def fixtures():
    return G.load_fixtures()


@pytest.mark.parametrize("name", G.FIXTURE_CASES)
def test_model_gradients_against_the_reference(fixtures, name):
    assert float(fixtures[f"{name}/margin"]) >= G.MARGIN[name] == pytest.approx(10 * helpers.LINEAR_TOL["bf16x6"], rel=1e-12)
    out, grads = _device_grads(name, "bf16x6")
    prefix = f"{name}/g64/"
    g64 = {k[len(prefix):]: v for k, v in fixtures.items() if k.startswith(prefix)}
    err32 = {k[len(f"{name}/err32/"):]: float(v) for k, v in fixtures.items() if k.startswith(f"{name}/err32/")}
    assert np.abs(out - fixtures[f"{name}/out64"]).max() <= G.MARGIN[name] * np.abs(fixtures[f"{name}/out64"]).max()
    _check_grads(name, grads, g64, err32, "bf16x6")


@pytest.mark.parametrize("name,tier", [("eval_split", "bf16x6"), ("eval_x3", "3xbf16")])
def test_model_gradients_against_the_restatement(name, tier):
    _, g64, margin = G.run_case(name)
    assert margin >= G.MARGIN[name] == pytest.approx(10 * helpers.LINEAR_TOL[tier], rel=1e-12)
    _, grads = _device_grads(name, tier)
    _check_grads(name, grads, g64, {}, tier)


def test_decoder_alone_returns_its_four_input_gradients():
    """Decoder(grad=True) on the fp64 encoder maps of the eval_odd case: the gradients of its four inputs against
    torch's own autograd through the restatement's decoder half."""
    name = "eval_odd"
    feats = G.decoder_inputs(name)
    _, want, margin, cot = G.run_decoder(G.case_state(name), feats)
    assert margin >= 10 * helpers.LINEAR_TOL["bf16x6"], margin
    dec = _model(name, cls="Decoder")
    xs = [_dev(f).requires_grad_() for f in feats]
    out = dec(tuple(xs))
    assert tuple(out.shape) == cot.shape
    (out * _dev(cot)).sum().backward()
    bound_share = 0.0
    for i, (x, t) in enumerate(zip(xs, want)):
        scale = float(np.abs(t).max())
        assert scale > 0.0
        err = float(np.abs(x.grad.cpu().double().numpy() - t).max())
        bound = 10.0 * helpers.GRAD_W_TOL["bf16x6"] * scale
        _report(f"Decoder alone, gradient of input {i + 1}", err, bound)
        bound_share = max(bound_share, err / bound)
    assert bound_share <= 1.0


def test_encoder_alone_records_and_matches_the_model():
    """Encoder(grad=True) alone: its four maps carry a graph, and their gradients are the bits the whole model's
    encoder half computes for the same cotangents (the same Functions on the same kernels)."""
    name = "eval_odd"
    enc, model = _model(name, cls="Encoder"), _model(name)
    x = _dev(G.case_input(name))
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    feats = enc(xa)
    assert len(feats) == 4 and all(f.requires_grad for f in feats)
    cots = [_dev(np.random.default_rng(2150 + i).standard_normal(tuple(f.shape)).astype(np.float32))
            for i, f in enumerate(feats)]
    sum((f * c).sum() for f, c in zip(feats, cots)).backward()
    other = model.encoder(xb)
    assert all(torch.equal(f.detach(), o.detach()) for f, o in zip(feats, other))
    sum((f * c).sum() for f, c in zip(other, cots)).backward()
    assert torch.equal(xa.grad, xb.grad) and float(xa.grad.abs().max()) > 0.0
    got = {k: p.grad for k, p in enc.named_parameters()}
    for k, p in model.encoder.named_parameters():
        assert (got[k] is None) == (p.grad is None), k
        assert p.grad is None or torch.equal(got[k], p.grad), k
    assert sum(g is not None for g in got.values()) == 16          # conv 0-3 and BatchNorm 0-3, weight and bias


# ---- 8. behaviour ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["train_32", "eval_odd"])
def test_recorded_forward_has_the_bits_of_the_inference_path(name):
    model, twin = _model(name), _model(name)
    x = _dev(G.case_input(name))
    with torch.no_grad():
        plain = twin(x)
    out = model(x.clone().requires_grad_())
    assert out.requires_grad and not plain.requires_grad
    assert torch.equal(out.detach(), plain)
    for (k, a), (_, b) in zip(model.state_dict().items(), twin.state_dict().items()):
        assert torch.equal(a, b), k                                # running statistics moved alike


def _backward(model, x, cot):
    for p in model.parameters():
        p.grad = None
    xr = x.clone().requires_grad_()
    (model(xr) * cot).sum().backward()
    return [xr.grad] + [p.grad for p in model.parameters() if p.grad is not None]


def test_backward_is_reproducible_and_contained():
    name = "eval_odd"
    model = _model(name)
    (_, cin, cout, _, h, w), _, _ = G.CASES[name]
    r = np.random.default_rng(2200)
    x = _dev(r.standard_normal((3, cin, h, w)).astype(np.float32))
    cot = _dev(r.standard_normal((3,) + R.output_shape(3, cout, h, w)[1:]).astype(np.float32))
    a, b = _backward(model, x, cot), _backward(model, x, cot)
    assert len(a) == 1 + 32 and all(torch.equal(p, q) for p, q in zip(a, b))        # two runs: equal bits
    alone = _backward(model, x[1:2].contiguous(), cot[1:2].contiguous())
    assert torch.equal(alone[0][0], a[0][1])                       # eval: an item's input gradient, alone and in a batch
    bad = x.clone()
    bad[0, 1, 5, 7] = float("nan")
    c = _backward(model, bad, cot)
    assert torch.equal(c[0][1], a[0][1]) and torch.equal(c[0][2], a[0][2])          # a NaN stays in its item
    used = {k for k, _, u in R.state_spec(*G.CASES[name][0][1:4]) if u}
    for k, p in model.named_parameters():
        assert (p.grad is None) == (k not in used), k


def test_train_backward_is_reproducible():
    name = "train_32"
    model = _model(name)
    x, cot = _dev(G.case_input(name)), _dev(G.case_cotangent(name))
    a, b = _backward(model, x, cot), _backward(model, x, cot)
    assert len(a) == 1 + 32 and all(torch.equal(p, q) for p, q in zip(a, b))


def test_forward_follows_an_in_place_weight_update():
    name = "eval_odd"
    model, x = _model(name), _dev(G.case_input(name))
    cot = _dev(G.case_cotangent(name))
    _backward(model, x, cot)
    with torch.no_grad():
        for p in model.parameters():
            if p.grad is not None:
                p.add_(p.grad, alpha=-1e-3)
    fresh = _model(name)
    fresh.load_state_dict(model.state_dict(), strict=True)
    out = model(x.clone().requires_grad_())
    with torch.no_grad():
        assert torch.equal(out.detach(), fresh(x))


@pytest.mark.parametrize("name", ["train_32", "eval_odd"])
def test_forward_and_backward_replay_from_one_graph(name):
    model = _model(name)
    x, cot = _dev(G.case_input(name)), _dev(G.case_cotangent(name))
    eager = _backward(model, x, cot)                               # eager: packs the weights
    static = x.clone().requires_grad_()
    for p in model.parameters():                                   # (the eager gradients stay as they are)
        p.grad = None
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        (model(static) * cot).sum().backward()
    torch.cuda.current_stream().wait_stream(side)
    static.grad = None
    for p in model.parameters():
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        (model(static) * cot).sum().backward()
    with torch.no_grad():
        static.copy_(x.flip(2))
    graph.replay()
    with torch.no_grad():
        static.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    got = [static.grad] + [p.grad for p in model.parameters() if p.grad is not None]
    assert len(got) == len(eager) and all(torch.equal(p, q) for p, q in zip(got, eager))
