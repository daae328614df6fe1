"""The U-Net without a GPU: the fp64 restatement (tests/unet_ref.py) against the reference's own numbers
(tests/golden/ref_unet.npz), and what gwen_amd.UNet promises on the host -- the reference's parameter tree, its
output-shape rule, and its refusals (CPU tensors, calls that would need a backward)."""
import numpy as np
import pytest
import torch

import unet_ref as R


@pytest.fixture(scope="module")
def fixtures():
    return R.load_fixtures()


def _model(name, **kw):
    import gwen_amd
    (_, cin, cout, hidden, _, _) = R.CASES[name][0]
    return gwen_amd.UNet(cin, cout, hidden, **kw)


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_is_the_reference(fixtures, name):
    state, x = R.case_state(name), R.make_input(name)
    for mode in R.modes(name):
        want = fixtures[f"{name}/{mode}/out64"]
        got, new = R.forward(state, x, train=mode == "train")
        assert got.shape == want.shape
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"{name} {mode}: restatement vs the reference's fp64 forward {err:.2e}")
        assert err <= 1e-12
        for key, v in new.items():
            ref = fixtures[f"{name}/train/stats64/{key}"]
            assert np.abs(v - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), key


@pytest.mark.parametrize("name", list(R.CASES))
def test_fixture_cases_are_the_issue_s(fixtures, name):
    meta = tuple(int(v) for v in fixtures[f"{name}/meta"])
    assert meta == R.CASES[name][0]
    b, cin, cout, hidden, h, w = meta
    assert fixtures[f"{name}/eval/out64"].shape == R.output_shape(b, cout, h, w)
    assert fixtures[f"{name}/eval/out64"].dtype == np.float64 and fixtures[f"{name}/eval/out32"].dtype == np.float32
    assert (f"{name}/train/out64" in fixtures) == R.CASES[name][1]


@pytest.mark.parametrize("name", ["aligned", "one_channel_crop", "ref_split"])
def test_state_dict_is_the_reference_s(fixtures, name):
    model = _model(name)
    sd = model.state_dict()
    assert list(sd) == [str(k) for k in fixtures[f"{name}/keys"]]
    assert ["x".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in fixtures[f"{name}/shapes"]]
    meta = R.CASES[name][0]
    assert [(k, tuple(s)) for k, s, _ in R.state_spec(*meta[1:4])] == [(k, tuple(v.shape)) for k, v in sd.items()]
    state = {k: torch.from_numpy(np.asarray(v)) for k, v in R.case_state(name).items()}
    assert model.load_state_dict(state, strict=True).missing_keys == []
    assert torch.equal(model.encoder.conv_layers[0].weight.detach(), state["encoder.conv_layers.0.weight"])


@pytest.mark.parametrize("name", list(R.CASES))
def test_output_shape_rule(fixtures, name):
    import gwen_amd
    b, cin, cout, hidden, h, w = R.CASES[name][0]
    assert (b, cout) + gwen_amd.UNet.output_hw(h, w) == fixtures[f"{name}/eval/out64"].shape
    with pytest.raises(ValueError):
        gwen_amd.UNet.output_hw(15, 64)


def test_crop_rule():
    from gwen_amd.models_cnn import crop_range
    for size in range(2, 40):
        for target in (size, size - 1, size - 2, size - 3):
            if target > 0:
                assert crop_range(size, target) == R.crop_range(size, target)
                lo, hi = crop_range(size, target)
                assert hi - lo == target
    assert crop_range(9, 8) == (1, 9)              # an odd difference drops the FIRST row or column


def test_cpu_input_raises():
    model = _model("aligned").eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="HIP device"):
        model(torch.zeros(1, 3, 16, 16))


def test_call_that_needs_a_backward_raises():
    model = _model("aligned").eval()
    with pytest.raises(RuntimeError, match="backward is not implemented"):
        model(torch.zeros(1, 3, 16, 16))                         # the parameters require grad
    for p in model.parameters():
        p.requires_grad_(False)
    with pytest.raises(RuntimeError, match="backward is not implemented"):
        model(torch.zeros(1, 3, 16, 16, requires_grad=True))
    with pytest.raises(RuntimeError, match="HIP device"):        # nothing requires grad: it runs, and wants a device
        model(torch.zeros(1, 3, 16, 16))


def test_precision_names():
    with pytest.raises(ValueError):
        _model("aligned", precision="fp32")
    assert _model("aligned", precision="3xbf16").encoder.precision == "3xbf16"


def _plan(L, h, w, cin, cout, flags):
    import ctypes
    nct, nz = ctypes.c_int(-1), ctypes.c_int(-1)
    assert L.gwen_conv3x3_plan(h, w, cin, cout, flags, ctypes.byref(nct), ctypes.byref(nz)) == 0
    return nct.value, nz.value


def test_conv_plan_and_workspace_are_one_decision(hip_lib):
    """The launcher and the size function read one plan: a split over Cin (slices > 1) has a workspace size or the call is
    refused -- it never runs without its slabs (B = 8200 of 16 x 16, 128 -> 512, pooled: input and output are each
    about 1 GiB and legal, the two slabs of raw sums would be 8 GiB)."""
    L, POOL = hip_lib, 4
    # the reference configuration's layers on 128 x 128: wide blocks at high resolution, slices at low
    assert _plan(L, 128, 128, 124, 128, POOL) == (4, 1)
    assert _plan(L, 64, 64, 128, 256, POOL) == (2, 1)
    assert _plan(L, 8, 8, 1024, 512, 0) == (1, 8)
    assert _plan(L, 16, 16, 128, 512, POOL) == (1, 2)
    # the shapes tests/test_gpu_unet.py runs for the wider blocks
    assert _plan(L, 127, 129, 3, 128, POOL) == (4, 1) and _plan(L, 128, 128, 12, 136, 0) == (4, 1)
    assert _plan(L, 96, 128, 12, 112, POOL) == (3, 1) and _plan(L, 128, 128, 5, 48, 0) == (2, 1)
    assert L.gwen_conv3x3_plan(0, 8, 16, 16, 0, None, None) == -1
    for b in (1, 8, 4096):
        assert L.gwen_conv3x3_workspace_floats(b, 16, 16, 128, 512, POOL) == 2 * b * 256 * 512
    for b in (4097, 8192, 8200):                        # slabs of 4 GiB and more: no size, and the launcher refuses
        assert L.gwen_conv3x3_workspace_floats(b, 16, 16, 128, 512, POOL) == -1
        x, img, out, ws = 1 << 20, 2 << 20, 3 << 20, 4 << 20      # never dereferenced: refused before any HIP call
        assert L.gwen_conv3x3_f32(x, img, None, None, None, out, b, 16, 16, 128, 512, 128, 512, POOL, 2, None, 0, None) == -2
        assert L.gwen_conv3x3_f32(x, img, None, None, None, out, b, 16, 16, 128, 512, 128, 512, POOL, 2, ws, 1 << 40, None) == -2
    # in range, a split without (enough) workspace is GWEN_ENOSPACE
    assert L.gwen_conv3x3_f32(x, img, None, None, None, out, 8, 16, 16, 128, 512, 128, 512, POOL, 2, None, 0, None) == -3
    assert L.gwen_conv3x3_f32(x, img, None, None, None, out, 8, 16, 16, 128, 512, 128, 512, POOL, 2, ws, 100, None) == -3
    # more pixel tiles than a grid holds (grid.x * 256 threads < 2^32)
    assert L.gwen_conv3x3_f32(x, img, None, None, None, out, 1 << 24, 1, 1, 4, 4, 4, 4, 0, 2, None, 0, None) == -2
    assert L.gwen_conv3x3_f32(x, img, None, None, None, out, 1, 1, 1 << 28, 1, 1, 1, 1, 0, 2, None, 0, None) == -2


def test_entry_points_refuse_before_any_launch(hip_lib):
    L = hip_lib
    assert L.gwen_conv3x3_pack_bytes(124, 1, 2) == 4 * 9 * 1 * 3 * 1024
    assert L.gwen_conv3x3_pack_bytes(32, 16, 0) == 9 * 2 * 1024
    assert L.gwen_conv3x3_pack_bytes(32, 16, 3) == L.gwen_conv3x3_pack_bytes(32, 16, 2)      # f16x3 means bf16x6
    assert L.gwen_conv3x3_pack_bytes(0, 16, 2) == 0 and L.gwen_conv3x3_pack_bytes(16, 2049, 2) == 0
    assert L.gwen_conv3x3_pack_bytes(16, 16, 1) == 0                                          # no fp32-input path
    assert L.gwen_conv3x3_pack_f32(None, 16, 16, 0, 2, None, None) == -1
    assert L.gwen_conv3x3_f32(None, None, None, None, None, None, 1, 4, 4, 16, 16, 8, 16, 0, 2, None, 0, None) == -1   # ldx < Cin
    assert L.gwen_conv3x3_f32(None, None, None, None, None, None, 1, 4, 4, 16, 16, 16, 16, 8, 2, None, 0, None) == -1  # flags
    assert L.gwen_conv3x3_f32(None, None, None, None, None, None, 1, 4, 4, 16, 16, 16, 16, 1, 2, None, 0, None) == -1  # no scale
    assert L.gwen_conv3x3_f32(None, None, None, None, None, None, 0, 4, 4, 16, 16, 16, 16, 0, 2, None, 0, None) == 0   # empty
    assert L.gwen_conv3x3_f32(None, None, None, None, None, None, 1, 1, 5, 16, 16, 16, 16, 4, 2, None, 0, None) == 0   # pooled away
    assert L.gwen_conv3x3_f32(None, None, None, None, None, None, 1, 1 << 15, 1 << 15, 16, 16, 16, 16, 0, 2, None, 0, None) == -2
    # one image's shape decides the cut into blocks and slices of Cin, never the batch
    assert L.gwen_conv3x3_workspace_floats(1, 128, 128, 124, 128, 4) == 0
    assert L.gwen_conv3x3_workspace_floats(1, 8, 8, 1024, 512, 0) == 8 * 64 * 512
    assert L.gwen_conv3x3_workspace_floats(3, 8, 8, 1024, 512, 0) == 3 * 8 * 64 * 512
    assert L.gwen_conv3x3_workspace_floats(1, 2, 2, 124, 8, 4) == 2 * 4 * 8
    assert L.gwen_upsample2x_f32(None, None, None, None, 1, 1 << 13, 1 << 13, 16, 16, 16, 0, None) == -2
    assert L.gwen_upsample2x_f32(None, None, None, None, 1, 4, 4, 16, 16, 8, 0, None) == -1
    assert L.gwen_channel_stats_workspace_bytes(4099, 24) == 129 * 2 * 24 * 8         # chunks of 32 rows
    assert L.gwen_channel_stats_workspace_bytes(0, 24) == 0
    assert L.gwen_channel_stats_f64(None, 0, 8, 8, None, None, None, 0, None) == -1
    assert L.gwen_affine_relu_f32(None, None, None, 0, 8, 8, None) == 0
    assert L.gwen_affine_relu_f32(None, None, None, 4, 8, 4, None) == -1
