"""The longitude FFT of gwen_amd.spectral on the host: which ring lengths it takes, the errors of the ``longitude`` keyword
and of ``gwen_sht_transform`` -- all before any device is touched -- and the convention of the intermediate ring, pinned
against numpy's rfft."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sht_ref as R  # noqa: E402

from gwen_amd import spectral  # noqa: E402

GOOD = [1, 2, 3, 4, 5, 6, 18, 20, 32, 45, 150, 1440, 3645, 4096]
BAD = [0, 7, 14, 4095, 4098, 4100]                      # 4095 = 3^2 5 7 13; the last two are over the limit


def test_fft_supported_lengths():
    assert spectral.LONGITUDE == ("direct", "fft")
    for n in GOOD:
        assert spectral.fft_supported(n) is True, n
    for n in BAD:
        assert spectral.fft_supported(n) is False, n


def test_c_fft_supported_agrees(hip_lib):
    for n in GOOD:
        assert hip_lib.gwen_sht_fft_supported(n) == 1, n
    for n in BAD:
        assert hip_lib.gwen_sht_fft_supported(n) == 0, n


def test_longitude_errors_come_before_any_device():
    for bad in ("FFT", "auto"):
        with pytest.raises(ValueError, match="longitude"):
            spectral.SphericalHarmonics(9, 18, "cpu", grid="gauss", longitude=bad)
    with pytest.raises(ValueError, match="4096.*2, 3 and 5"):
        spectral.SphericalHarmonics(9, 14 * 2, "cpu", grid="gauss", longitude="fft")
    with pytest.raises(ValueError):
        spectral.check_sizes("gauss", 9, 28, None, "fft")
    assert spectral.check_sizes("gauss", 9, 28, None, "direct") == 8 == spectral.check_sizes("gauss", 9, 28, None)
    # good requests reach the device check
    for longitude in spectral.LONGITUDE:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            spectral.SphericalHarmonics(9, 18, "cpu", grid="gauss", longitude=longitude)


def test_transform_refuses_bad_calls_before_any_hip_call(hip_lib):
    from gwen_amd import _lib
    EQ, CEN, GAUSS = 0, 1, 2
    assert hip_lib.gwen_sht_transform(None) == -1

    def old(op, grid, nlat, nlon, lmax, c, batch):
        if op < 2:
            args = (None, 0, None, 0, None, None, None, None, grid, batch, nlat, nlon, lmax, c, None, 0, None)
            return (hip_lib.gwen_sht_analysis, hip_lib.gwen_sht_synthesis)[op](*args)
        args = (None, None, 0, None, None, 0, None, None, None, None, grid, batch, nlat, nlon, lmax, c, 0, None, 0, None)
        return (hip_lib.gwen_sht_vector_analysis, hip_lib.gwen_sht_vector_synthesis)[op - 2](*args)

    def new(op, longitude, grid, nlat, nlon, lmax, c=3, batch=1):
        call = _lib.ShtCall(op=op, longitude=longitude, grid=grid, batch=batch, nlat=nlat, nlon=nlon, lmax=lmax, C=c)
        return hip_lib.gwen_sht_transform(call)

    # the list of test_sht_host.test_c_entry_points_refuse_bad_sizes_before_any_hip_call, with its codes
    sizes = [((EQ, 17, 64, 9), {}, -1), ((CEN, 16, 64, 8), {}, -1), ((GAUSS, 9, 64, 9), {}, -1),
             ((EQ, 17, 16, 8), {}, -1), ((GAUSS, 2048, 4096, 1024), {}, -1), ((3, 17, 32, 4), {}, -1),
             ((-1, 17, 32, 4), {}, -1), ((GAUSS, 9, 18, 8), dict(c=0), -1), ((GAUSS, 9, 18, 8), dict(batch=-1), -1),
             ((GAUSS, 9, 18, 8), {}, -1), ((GAUSS, 9, 18, 8), dict(batch=0), 0),
             ((GAUSS, 2048, 2 ** 21, 8), {}, -2), ((GAUSS, 9, 18, 8), dict(c=2 ** 31), -2)]
    for op in range(4):
        for longitude in (0, 1):
            for geom, kw, code in sizes:
                assert new(op, longitude, *geom, **kw) == code, (op, longitude, geom, kw)
                assert old(op, *geom, kw.get("c", 3), kw.get("batch", 1)) == code, (op, geom, kw)
        assert new(op, 2, GAUSS, 9, 18, 8, batch=0) == -1                  # unknown longitude
        assert new(op, 1, GAUSS, 7, 14, 6, batch=0) == -1                  # no FFT of 14 = 2 . 7 points
        assert new(op, 0, GAUSS, 7, 14, 6, batch=0) == 0
    assert new(4, 0, GAUSS, 9, 18, 8, batch=0) == -1 and new(-1, 1, GAUSS, 9, 18, 8, batch=0) == -1
    assert new(4, 2, GAUSS, 9, 18, 8, batch=0) == -1


@pytest.mark.parametrize("geom", [("gauss", 23, 45, 22), ("equiangular", 17, 32, 8)])
def test_ring_convention_is_rfft(geom):
    """ring[j, lmax + m] = Re rfft(x[j])[m] and ring[j, lmax - m] = -Im rfft(x[j])[m], then the restatement's latitude
    sum: the analysis of tests/sht_ref.py."""
    grid, nlat, nlon, lmax = geom
    rng = np.random.default_rng(31)
    x = rng.standard_normal((2, nlat * nlon, 3))
    spec = np.fft.rfft(x.reshape(2, nlat, nlon, 3), axis=2)[:, :, :lmax + 1]
    ring = np.zeros((2, nlat, 2 * lmax + 1, 3))
    ring[:, :, lmax:] = spec.real
    ring[:, :, :lmax] = -spec.imag[:, :, :0:-1]                           # column lmax - m, m = lmax ... 1
    lat, w = R.latitudes(grid, nlat)
    coef = np.zeros((2, (lmax + 1) ** 2, 3))
    ls = np.arange(lmax + 1)
    for m in range(lmax + 1):
        p = R.legendre(lmax, m, lat) * (w / nlon)[None, :]
        rows = ls[m:] ** 2 + ls[m:]
        coef[:, rows + m] = np.einsum("lj,bjc->blc", p, ring[:, :, lmax + m])
        if m:
            coef[:, rows - m] = np.einsum("lj,bjc->blc", p, ring[:, :, lmax - m])
    assert np.abs(coef - R.analysis(x, *geom)).max() <= 1e-12 * np.abs(x).max()
