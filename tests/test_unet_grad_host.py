"""The U-Net backward without a GPU: the gradient fixture (tests/golden/ref_unet_grads.npz, the reference's own
gradients) against the torch fp64 restatement of tests/unet_grad_ref.py, the margin rule on every whole-model case, the
public surface of ``grad=True``, and the argument checks and plans of the new entry points (they return before any HIP
call)."""
import ctypes

import numpy as np
import pytest
import torch

import helpers
import unet_ref as R
import unet_grad_ref as G


@pytest.fixture(scope="module")
def fixtures():
    return G.load_fixtures()


@pytest.fixture(scope="module")
def runs():
    return {name: G.run_case(name) for name in G.CASES}


@pytest.mark.parametrize("name", G.FIXTURE_CASES)
def test_restatement_reproduces_the_reference_gradients(fixtures, runs, name):
    (_, cin, cout, hidden, _, _), mode, _ = G.CASES[name]
    out, grads, _ = runs[name]
    assert np.abs(out - fixtures[f"{name}/out64"]).max() <= 1e-12 * np.abs(out).max()
    keys = G.used_keys(cin, cout, hidden) + ["input"]
    assert sorted(k[len(name) + 5:] for k in fixtures if k.startswith(f"{name}/g64/")) == sorted(keys)
    for key in keys:
        want = fixtures[f"{name}/g64/{key}"]
        assert want.dtype == np.float32
        scale_key = G.zero_in_train(key) if mode == "train" else None
        if scale_key:                              # mathematically zero: rounding noise of the BatchNorm's scale
            scale = np.abs(fixtures[f"{name}/g64/{scale_key}"]).max()
            assert np.abs(grads[key]).max() <= 1e-12 * scale and np.abs(want).max() <= 1e-12 * scale, key
            continue
        # the fixture is the fp64 gradient rounded to fp32: half an ulp of each element
        slack = 2.0 ** -24 * np.abs(want.astype(np.float64)) + 1e-12 * np.abs(want).max()
        assert (np.abs(grads[key] - want) <= slack).all(), key
        assert float(fixtures[f"{name}/err32/{key}"]) <= 4.5e-6 * np.abs(want).max(), key


@pytest.mark.parametrize("name", list(G.CASES))
def test_margins_meet_the_rule_and_no_gradient_is_dead(fixtures, runs, name):
    (_, cin, cout, hidden, _, _), mode, _ = G.CASES[name]
    tier = "3xbf16" if name == "eval_x3" else "bf16x6"
    assert G.MARGIN[name] == pytest.approx(10 * helpers.LINEAR_TOL[tier], rel=1e-12)
    _, grads, margin = runs[name]
    assert margin >= G.MARGIN[name], (name, margin)
    if name in G.FIXTURE_CASES:
        assert float(fixtures[f"{name}/margin"]) == pytest.approx(margin, rel=1e-6)
        unused = {k for k, _, u in R.state_spec(cin, cout, hidden) if not u and k.rsplit(".", 1)[1] in ("weight", "bias")}
        assert set(fixtures[f"{name}/unused"].tolist()) == unused
    for key in G.used_keys(cin, cout, hidden) + ["input"]:
        if not (mode == "train" and G.zero_in_train(key)):
            assert np.abs(grads[key]).max() > 0.0, key


def test_switches_reproduce_the_comparisons(runs):
    """the restatement with its own masks and argmax handed back in gives its own gradients"""
    name = "eval_x3"
    state, x, cot = G.case_state(name), G.case_input(name), G.case_cotangent(name)
    import torch.nn.functional as F
    t = torch.tensor(x, dtype=torch.float64)
    c = F.conv2d(t, torch.tensor(state["encoder.conv_layers.0.weight"], dtype=torch.float64),
                 torch.tensor(state["encoder.conv_layers.0.bias"], dtype=torch.float64), padding=1)
    pooled, idx = F.max_pool2d(c, 2, return_indices=True)
    pos = G.window_position(idx, c.shape[3])
    assert torch.equal(G.pool(c, pos), pooled)
    _, grads, _ = G.run(state, x, cot, False, switches={"pool/0": pos})
    for k, v in runs[name][1].items():
        assert np.array_equal(v, grads[k]), k


def test_grad_flag_keeps_the_state_dict_and_the_guards():
    import gwen_amd
    plain, rec = gwen_amd.UNet(3, 2, 64), gwen_amd.UNet(3, 2, 64, grad=True)
    assert list(plain.state_dict()) == list(rec.state_dict())
    assert rec.grad and rec.encoder.grad and rec.decoder.grad and not plain.grad and not plain.encoder.grad
    rec3 = gwen_amd.UNet(3, 2, 64, "3xbf16", True)
    assert rec3.precision == rec3.encoder.precision == "3xbf16" and rec3.decoder.grad
    with pytest.raises(RuntimeError, match="HIP device"):
        rec(torch.zeros(1, 3, 16, 16, requires_grad=True))
    with pytest.raises(RuntimeError, match="HIP device"):
        rec.encoder(torch.zeros(1, 3, 16, 16))
    with pytest.raises(RuntimeError, match="backward is not implemented"):
        plain(torch.zeros(1, 3, 16, 16))


# ---- the entry points, before any HIP call -------------------------------------------------------------------------

EINVAL, ERANGE, OK = -1, -2, 0
BF16X6, F32 = 2, 1


def _wgrad_plan(lib, b, h, w, cin, cout):
    tiles, chunks = ctypes.c_int(-1), ctypes.c_int64(-1)
    rc = lib.gwen_conv3x3_grad_weight_plan(b, h, w, cin, cout, ctypes.byref(tiles), ctypes.byref(chunks))
    return rc, tiles.value, chunks.value


def test_grad_weight_plan_and_validation(hip_lib):
    from gwen_amd import _lib
    lib = _lib.lib()
    # (Cin, Cout, H, W, B) of test_gpu_unet_grad.WGRAD_CASES -> (channel tiles per block, pixel chunks)
    plans = {(1, 1, 2, 2, 1): (1, 1), (3, 8, 5, 7, 3): (1, 3), (16, 24, 16, 16, 1): (2, 2), (124, 64, 18, 35, 1): (4, 9),
             (136, 136, 5, 7, 3): (4, 3), (5, 48, 40, 33, 2): (2, 30), (64, 32, 8, 8, 2): (4, 2),
             (12, 136, 64, 64, 2): (2, 64), (136, 136, 32, 64, 3): (4, 24),
             (124, 128, 128, 128, 8): (4, 64), (512, 1024, 8, 8, 1): (4, 1)}
    for (cin, cout, h, w, b), want in plans.items():
        assert _wgrad_plan(lib, b, h, w, cin, cout) == (OK,) + want, (cin, cout, h, w, b)
        ws = lib.gwen_conv3x3_grad_weight_workspace_floats(b, h, w, cin, cout)
        assert ws == (0 if want[1] == 1 else want[1] * 9 * cin * cout)
    assert _wgrad_plan(lib, 0, 8, 8, 4, 4)[0] == EINVAL and _wgrad_plan(lib, 1, 8, 8, 0, 4)[0] == EINVAL
    assert _wgrad_plan(lib, 1, 8, 8, 4, 2049)[0] == EINVAL
    assert lib.gwen_conv3x3_grad_weight_plan(1, 8, 8, 4, 4, None, None) == EINVAL
    assert lib.gwen_conv3x3_grad_weight_workspace_floats(1, 8, 8, 0, 4) == 0
    assert lib.gwen_conv3x3_grad_weight_workspace_floats(0, 8, 8, 4, 4) == 0
    assert lib.gwen_conv3x3_grad_weight_workspace_floats(1 << 20, 64, 64, 4, 4) == -1          # an input of 4 GiB or more
    f = lib.gwen_conv3x3_grad_weight_f32
    one = ctypes.c_void_p(64)                                      # never dereferenced: every call below returns first
    assert f(one, one, one, 1, 8, 8, 0, 4, 4, 4, 0, BF16X6, None, 0, None) == EINVAL           # Cin
    assert f(one, one, one, 1, 8, 8, 4, 4, 3, 4, 0, BF16X6, None, 0, None) == EINVAL           # pitch < Cout
    assert f(one, one, one, 1, 8, 8, 4, 4, 4, 4, 2, BF16X6, None, 0, None) == EINVAL           # transposed
    assert f(one, one, one, 1, 8, 8, 4, 4, 4, 4, 0, F32, None, 0, None) == EINVAL              # not a split contraction
    assert f(one, one, one, -1, 8, 8, 4, 4, 4, 4, 0, BF16X6, None, 0, None) == EINVAL
    assert f(one, one, None, 1, 8, 8, 4, 4, 4, 4, 0, BF16X6, None, 0, None) == EINVAL          # no output
    assert f(one, one, one, 1 << 20, 64, 64, 4, 4, 4, 4, 0, BF16X6, None, 0, None) == ERANGE
    assert f(one, one, one, 1, 1 << 15, 1 << 15, 4, 4, 4, 4, 0, BF16X6, None, 0, None) == ERANGE


def test_argmax_and_small_kernels_validate(hip_lib):
    from gwen_amd import _lib
    lib = _lib.lib()
    one, two, three = ctypes.c_void_p(64), ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21)   # never dereferenced
    f = lib.gwen_conv3x3_argmax_f32
    pool = _lib.CONV_POOL
    args = lambda b, flags, am=one, ldp=4: (one, two, None, None, None, three, b, 8, 8, 4, 4, 4, 4, flags, BF16X6,
                                             None, 0, am, None, ldp, None)
    assert f(*args(1, 0)) == EINVAL                               # argmax without pool
    assert f(*args(1, _lib.CONV_RELU)) == EINVAL
    assert f(*args(1, pool | 8)) == EINVAL                        # a flag that does not exist
    assert f(*args(1, pool, None)) == EINVAL                      # argmax is required
    assert f(*args(0, pool)) == OK                                # an empty batch
    assert f(*args(1 << 26, pool)) == ERANGE                      # 4 GiB
    f = lib.gwen_upsample2x_backward_f32
    assert f(one, None, one, 0, 4, 4, 3, 3, 3, 3, None) == OK
    assert f(one, None, one, 1, 4, 4, 0, 3, 3, 3, None) == EINVAL
    assert f(one, None, one, 1, 4, 4, 3, 2, 3, 3, None) == EINVAL
    assert f(one, one, one, 1, 4, 4, 3, 3, 2, 3, None) == EINVAL  # the mask's pitch
    assert f(one, None, None, 1, 4, 4, 3, 3, 3, 3, None) == EINVAL
    assert f(one, None, one, 1 << 20, 32, 32, 3, 3, 3, 3, None) == ERANGE
    f = lib.gwen_unpool2x2_f32
    assert f(one, one, one, 0, 4, 4, 3, 3, 3, None) == OK
    assert f(one, one, one, 1, 4, 4, 0, 3, 3, None) == EINVAL
    assert f(one, one, one, 1, 4, 4, 3, 2, 3, None) == EINVAL
    assert f(one, None, one, 1, 4, 4, 3, 3, 3, None) == EINVAL
    assert f(one, one, one, 1 << 20, 32, 32, 3, 3, 3, None) == ERANGE
    f = lib.gwen_norm_relu_backward_f32
    tail = lambda rows, c, train: (rows, c, c, c, c, c, train, one, 1 << 20, None)
    eight = tuple(ctypes.c_void_p(4096 * (i + 1)) for i in range(8))
    assert f(*eight, *tail(0, 4, 1)) == EINVAL
    assert f(*eight, *tail(8, 0, 1)) == EINVAL
    assert f(*eight, *tail(8, 4, 2)) == EINVAL
    assert f(*eight, *tail(1 << 30, 4, 0)) == ERANGE
    assert f(*eight[:6], None, eight[7], *tail(8, 4, 1)) == EINVAL
    assert f(*eight, 8, 4, 4, 4, 4, 4, 1, one, 8, None) == -3     # a workspace too short
