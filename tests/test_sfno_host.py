"""gwen_amd.sfno without a device: argument checks, the C entry points' size checks, the documented state_dict, and the
restatement's own rotation equivariance (tests/sfno_ref.py)."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sfno_ref as F  # noqa: E402

from gwen_amd import sfno  # noqa: E402


def transform(lmax=8, nlat=9, nlon=18):
    """What the modules need of a SphericalHarmonics before any launch (the real one needs a device to hold its tables)."""
    return SimpleNamespace(lmax=lmax, nlat=nlat, nlon=nlon, rows=nlat * nlon, num_coefficients=(lmax + 1) ** 2,
                           analysis=None, synthesis=None)


def test_public_surface():
    import gwen_amd
    for name in ("SFNO", "SFNOBlock", "SpectralConv", "spectral_conv", "spectral_conv_supported"):
        assert name in gwen_amd.__all__ and getattr(gwen_amd, name) is getattr(sfno, name)


def test_spectral_conv_checks_shapes_then_dtypes_then_devices():
    w = torch.zeros(9, 16, 32)
    with pytest.raises(ValueError, match="T = 81"):
        sfno.spectral_conv(torch.zeros(2, 80, 16), w)                       # wrong T
    with pytest.raises(ValueError, match="T = 81"):
        sfno.spectral_conv(torch.zeros(2, 81, 32), w)                       # wrong Cin
    with pytest.raises(ValueError):
        sfno.spectral_conv(torch.zeros(2, 81, 16), w, lmax=7)               # weight does not hold lmax + 1 matrices
    with pytest.raises(ValueError, match="multiples of 16"):
        sfno.spectral_conv(torch.zeros(2, 81, 24), torch.zeros(9, 24, 32))
    with pytest.raises(ValueError, match="multiples of 16"):
        sfno.spectral_conv(torch.zeros(1, 1, 16), torch.zeros(1, 16, 528))
    with pytest.raises(ValueError, match="precision"):
        sfno.spectral_conv(torch.zeros(2, 81, 16), w, precision="fp32")
    # a wrong shape AND a wrong dtype AND the CPU: the shape is named first, then the dtype, then the device
    with pytest.raises(ValueError):
        sfno.spectral_conv(torch.zeros(2, 80, 16, dtype=torch.float64), w)
    with pytest.raises(TypeError, match="float32"):
        sfno.spectral_conv(torch.zeros(2, 81, 16, dtype=torch.float64), w)
    with pytest.raises(TypeError, match="float32"):
        sfno.spectral_conv(torch.zeros(2, 81, 16), w.double())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sfno.spectral_conv(torch.zeros(2, 81, 16), w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sfno.spectral_conv(torch.zeros(81, 16), w, precision="3xbf16")


def test_module_argument_checks():
    sh = transform()
    with pytest.raises(ValueError, match="lmax"):
        sfno.SpectralConv(sh, 16, 16, sh_out=transform(lmax=7))
    with pytest.raises(ValueError, match="multiples of 16"):
        sfno.SpectralConv(sh, 16, 40)
    with pytest.raises(ValueError, match="multiples of 16"):
        sfno.SpectralConv(sh, 1024, 16)
    with pytest.raises(ValueError, match="multiples of 16"):
        sfno.SFNO(sh, 3, 2, channels=20, blocks=1)
    with pytest.raises(ValueError, match="precision"):
        sfno.SFNO(sh, 3, 2, channels=16, blocks=1, precision="fp64")
    with pytest.raises(ValueError, match="residual"):
        sfno.SFNO(sh, 2, 3, channels=16, blocks=1, residual=True)
    with pytest.raises(ValueError, match="SphericalHarmonics"):
        sfno.SpectralConv(object(), 16, 16)
    model = sfno.SFNO(sh, 3, 2, channels=16, blocks=1)
    with pytest.raises(ValueError):
        model(torch.zeros(2, sh.rows + 1, 3))
    with pytest.raises(ValueError):
        model(torch.zeros(2, sh.rows, 4))
    with pytest.raises(TypeError, match="float32"):
        model(torch.zeros(2, sh.rows, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(torch.zeros(2, sh.rows, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sfno.SFNOBlock(sh, 16)(torch.zeros(sh.rows, 16))


def test_weight_initialisation_follows_torchs_generator():
    sh = transform(lmax=40)
    torch.manual_seed(5)
    a = sfno.SpectralConv(sh, 64, 32).weight.detach()
    torch.manual_seed(5)
    b = sfno.SpectralConv(sh, 64, 32).weight.detach()
    assert a.shape == (41, 64, 32) and torch.equal(a, b)
    assert abs(float(a.std()) * 8.0 - 1.0) < 0.02 and abs(float(a.mean())) < 1e-3        # std Cin^-1/2 on 84 000 draws


def test_state_dict_is_as_documented():
    sh = transform()
    model = sfno.SFNO(sh, 3, 2, channels=16, blocks=2, mlp_ratio=2)
    want = {"encoder.weight": (16, 3), "encoder.bias": (16,), "decoder.weight": (2, 16), "decoder.bias": (2,)}
    for k in range(2):
        p = f"blocks.{k}."
        want.update({p + "norm1.weight": (16,), p + "norm1.bias": (16,), p + "norm2.weight": (16,), p + "norm2.bias": (16,),
                     p + "conv.weight": (9, 16, 16), p + "skip.weight": (16, 16), p + "mlp.0.weight": (32, 16),
                     p + "mlp.0.bias": (32,), p + "mlp.2.weight": (16, 32), p + "mlp.2.bias": (16,)})
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == want
    bare = sfno.SFNO(sh, 3, 2, channels=16, blocks=1, layer_norm=False).state_dict()
    assert not any("norm" in k for k in bare) and "blocks.0.conv.weight" in bare
    # the fp64 restatement loads it as it is
    ref = F.RefSFNO("gauss", 9, 18, 8, 3, 2, 16, 2)
    ref.load_state_dict({k: v.double() for k, v in model.state_dict().items()}, strict=True)


def test_c_entry_points_refuse_bad_sizes_before_any_hip_call(hip_lib):
    BF16X3, F32, BF16X6, F16X3 = 0, 1, 2, 3

    def both(batch, lmax, cin, cout, contract=BF16X6, tw=0):
        a = hip_lib.gwen_spectral_conv_f32(None, None, None, batch, lmax, cin, cout, tw, contract, None)
        b = hip_lib.gwen_spectral_conv_grad_weight_f32(None, None, None, batch, lmax, cin, cout, contract, None)
        assert a == b
        return a

    assert both(-1, 8, 16, 16) == -1 and both(1, -1, 16, 16) == -1 and both(1, 1024, 16, 16) == -1
    assert both(1, 8, -16, 16) == -1 and both(1, 8, 16, 0) == -1 and both(1, 8, 24, 16) == -1 and both(1, 8, 16, 528) == -1
    assert both(1, 8, 16, 16, contract=F32) == -1 and both(1, 8, 16, 16, contract=4) == -1
    assert both(1, 8, 16, 16, contract=-1) == -1
    assert hip_lib.gwen_spectral_conv_f32(None, None, None, 1, 8, 16, 16, 2, BF16X6, None) == -1      # flag
    assert both(1, 8, 16, 16) == -1                                         # good sizes, null pointers
    assert both(2 ** 31, 8, 16, 16) == -2                                   # a degree's rows pass int32
    for contract in (BF16X3, BF16X6, F16X3):
        assert both(0, 8, 16, 48, contract=contract) == 0                   # nothing to do
    assert both(0, 8, 16, 40) == -1                                         # ... but the sizes are judged first


def test_supported_agrees_with_the_library(hip_lib):
    sizes = [-16, 0, 1, 8, 15, 16, 17, 24, 32, 48, 64, 100, 256, 496, 511, 512, 513, 528, 1024]
    for cin in sizes:
        for cout in sizes:
            want = sfno.spectral_conv_supported(cin, cout)
            assert want == (16 <= cin <= 512 and 16 <= cout <= 512 and cin % 16 == 0 and cout % 16 == 0)
            for contract in (0, 2, 3):
                assert bool(hip_lib.gwen_spectral_conv_supported(cin, cout, contract)) == want, (cin, cout, contract)
            assert hip_lib.gwen_spectral_conv_supported(cin, cout, 1) == 0
    assert hip_lib.gwen_spectral_conv_supported(64, 64, 4) == 0 and hip_lib.gwen_spectral_conv_supported(64, 64, -1) == 0


def test_the_restatement_is_rotation_equivariant_and_a_per_m_weight_is_not():
    """Gauss 12 x 24, lmax 8, 16 -> 48 channels, the field turned by 5 longitudes.  With one matrix a degree the layer
    commutes with the turn up to fp64 rounding (measured 1.6e-15 of max |y|; 1e-12 allows for 81 x 16-term sums 600 times
    over); with a matrix of its own for every (l, m) it does not (measured 2.45 of max |y|: the cos and sin rows of a
    degree mix under a turn, and only a common factor survives that)."""
    grid, nlat, nlon, lmax, cin, cout = "gauss", 12, 24, 8, 16, 48
    rng = np.random.default_rng(7)
    x = rng.standard_normal((2, nlat * nlon, cin))
    w = rng.standard_normal((lmax + 1, cin, cout)) / np.sqrt(cin)
    y = F.layer(x, w, grid, nlat, nlon, lmax)
    y_turned = F.layer(F.roll(x, nlat, nlon, 5), w, grid, nlat, nlon, lmax)
    good = np.abs(y_turned - F.roll(y, nlat, nlon, 5)).max() / np.abs(y).max()
    wm = rng.standard_normal(((lmax + 1) ** 2, cin, cout)) / np.sqrt(cin)
    z = F.layer(x, wm, grid, nlat, nlon, lmax, per_m=True)
    z_turned = F.layer(F.roll(x, nlat, nlon, 5), wm, grid, nlat, nlon, lmax, per_m=True)
    bad = np.abs(z_turned - F.roll(z, nlat, nlon, 5)).max() / np.abs(z).max()
    print(f"equivariance defect: per-degree weight {good:.2e}, per-(l, m) weight {bad:.2e}")
    assert good <= 1e-12
    assert bad >= 0.1


def test_restated_gradients_match_autograd():
    rng = np.random.default_rng(3)
    lmax, cin, cout = 3, 4, 5
    c, w = rng.standard_normal((2, 16, cin)), rng.standard_normal((lmax + 1, cin, cout))
    r = rng.standard_normal((2, 16, cout))
    ct, wt = torch.from_numpy(c).requires_grad_(), torch.from_numpy(w).requires_grad_()
    deg = torch.from_numpy(F.R.degrees(lmax))
    out = torch.einsum("btc,tcd->btd", ct, wt[deg])
    assert np.allclose(out.detach().numpy(), F.spectral_conv(c, w), rtol=0, atol=1e-13)
    (out * torch.from_numpy(r)).sum().backward()
    g_c, g_w = F.spectral_conv_grads(c, w, r)
    assert np.allclose(ct.grad.numpy(), g_c, rtol=0, atol=1e-12) and np.allclose(wt.grad.numpy(), g_w, rtol=0, atol=1e-12)
