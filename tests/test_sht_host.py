"""Spherical harmonics on the host: the quadratures, the numpy restatement (tests/sht_ref.py), the index tables and every
size error of gwen_amd.spectral and of the C entry points -- none of it touches a device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sht_ref as R  # noqa: E402

from gwen_amd import spectral  # noqa: E402


@pytest.mark.parametrize("grid", R.GRIDS)
@pytest.mark.parametrize("nlat", [2, 5, 8, 17, 32])
def test_quadrature_is_exact_to_its_degree(grid, nlat):
    for lat, w in (R.latitudes(grid, nlat), spectral.quadrature(grid, nlat)):
        assert abs(w.sum() - 1.0) <= 1e-14
        assert np.array_equal(lat, -lat[::-1]) and np.array_equal(w, w[::-1]) and (np.diff(lat) > 0).all()
        x = np.sin(np.deg2rad(lat))
        for k in range(R.exact_degree(grid, nlat) + 1):
            want = 0.0 if k % 2 else 1.0 / (k + 1)              # int_{-1}^{1} x^k dx / 2
            assert abs((w * x ** k).sum() - want) <= 1e-12, (grid, nlat, k)


@pytest.mark.parametrize("grid", R.GRIDS)
def test_package_nodes_match_the_restatement_and_latlon_grid(grid):
    import gwen_amd
    lat, w = spectral.quadrature(grid, 12)
    rlat, rw = R.latitudes(grid, 12)
    assert np.allclose(lat, rlat, rtol=0, atol=1e-13) and np.allclose(w, rw, rtol=0, atol=1e-15)
    if grid != "gauss":
        pos, _ = gwen_amd.latlon_grid(12, 7, poles=grid == "equiangular")
        assert np.array_equal(np.rad2deg(np.arcsin(pos[::7, 2])).round(9), lat.round(9))


@pytest.mark.parametrize("grid,nlat,nlon,lmax", [("gauss", 9, 18, 8), ("equiangular", 17, 18, 8),
                                                 ("equiangular-centred", 16, 16, 7)])
def test_restatement_round_trip_at_the_limit(grid, nlat, nlon, lmax):
    assert lmax == R.lmax_limit(grid, nlat) == spectral.max_degree(grid, nlat, nlon)
    rng = np.random.default_rng(5)
    c = rng.standard_normal((2, (lmax + 1) ** 2, 3))
    x = R.synthesis(c, grid, nlat, nlon, lmax)
    back = R.analysis(x, grid, nlat, nlon, lmax)
    assert np.abs(back - c).max() <= 1e-12
    # Parseval and the adjoints of the restatement
    q = R.point_weights(grid, nlat, nlon)
    assert np.allclose(R.power(c, lmax).sum(1), (q[None, :, None] * x * x).sum(1), rtol=1e-12, atol=0)
    g = rng.standard_normal(c.shape)
    h = rng.standard_normal(x.shape)
    assert abs((back * g).sum() - (x * R.analysis_adjoint(g, grid, nlat, nlon, lmax)).sum()) <= 1e-12 * np.abs(g).sum()
    assert abs((x * h).sum() - (c * R.synthesis_adjoint(h, grid, nlat, nlon, lmax)).sum()) <= 1e-12 * np.abs(h).sum()


def test_round_trip_fails_one_degree_above_the_limit():
    rng = np.random.default_rng(6)
    c = rng.standard_normal((1, 10 ** 2, 1))
    back = R.analysis(R.synthesis(c, "equiangular", 17, 20, 9), "equiangular", 17, 20, 9)
    assert np.abs(back - c).max() > 1e-4


@pytest.mark.parametrize("m", [0, 1, 512, 1023])
def test_recurrence_is_orthonormal_at_lmax_1023(m):
    lat, w = R.latitudes("gauss", 1024)
    p = R.legendre(1023, m, lat)
    gram = (p * w[None, :]) @ p.T * (1.0 if m == 0 else 0.5)    # the mean of cos^2 m lon is 1/2
    assert np.abs(gram - np.eye(p.shape[0])).max() <= 1e-10


def test_seeds_are_the_sectoral_recurrence():
    lat = np.array([-61.0, 0.0, 33.0])
    seed = spectral.sectoral_seeds(40)
    for m in (0, 1, 2, 17, 40):
        want = R.legendre(m, m, lat)[0]
        assert np.allclose(seed[m] * np.cos(np.deg2rad(lat)) ** m, want, rtol=1e-13, atol=0)


def test_index_and_degrees_agree():
    lmax = 11
    deg = spectral.degree_index(lmax)
    assert deg.dtype == np.int64 and deg.shape == ((lmax + 1) ** 2,)
    assert np.array_equal(deg, R.degrees(lmax))
    sh = object.__new__(spectral.SphericalHarmonics)
    sh.lmax = lmax
    seen = set()
    for l in range(lmax + 1):
        for m in range(-l, l + 1):
            row = sh.index(l, m)
            assert row == R.index(l, m) and deg[row] == l
            seen.add(row)
    assert seen == set(range((lmax + 1) ** 2))
    for l, m in ((lmax + 1, 0), (3, 4), (3, -4), (-1, 0)):
        with pytest.raises(ValueError):
            sh.index(l, m)


@pytest.mark.parametrize("kwargs", [
    dict(nlat=17, nlon=64, lmax=9, grid="equiangular"),                 # over the Clenshaw-Curtis limit
    dict(nlat=16, nlon=64, lmax=8, grid="equiangular-centred"),         # over Fejer's limit
    dict(nlat=9, nlon=64, lmax=9, grid="gauss"),                        # over the Gauss limit
    dict(nlat=17, nlon=16, lmax=8, grid="equiangular"),                 # nlon < 2 lmax + 1
    dict(nlat=2048, nlon=4096, lmax=1024, grid="gauss"),                # lmax > 1023
    dict(nlat=17, nlon=32, lmax=None, grid="healpix"),                  # unknown grid
    dict(nlat=17, nlon=32, lmax=-1, grid="equiangular"),
    dict(nlat=4096, nlon=32, lmax=4, grid="gauss"),                     # more latitudes than the kernels hold
])
def test_size_errors_come_before_any_device(kwargs):
    # device="cpu" would be the RuntimeError: the sizes are judged first
    with pytest.raises(ValueError):
        spectral.SphericalHarmonics(device="cpu", **kwargs)


def test_defaults_and_the_missing_device():
    assert spectral.check_sizes("equiangular", 721, 1440, None) == 360
    assert spectral.check_sizes("equiangular-centred", 720, 1440, None) == 359
    assert spectral.check_sizes("gauss", 80, 150, None) == 74
    assert spectral.check_sizes("gauss", 2048, 4096, None) == 1023
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spectral.SphericalHarmonics(9, 18, "cpu", grid="gauss")


def test_wrong_row_count_is_a_value_error():
    with pytest.raises(ValueError):
        spectral.check_rows("x", torch.zeros(2, 9 * 18 + 1, 3), 9 * 18, "nlat * nlon")
    with pytest.raises(ValueError):
        spectral.check_rows("x", torch.zeros(9 * 18), 9 * 18, "nlat * nlon")
    with pytest.raises(ValueError):
        spectral.check_rows("x", np.zeros((9 * 18, 3)), 9 * 18, "nlat * nlon")
    spectral.check_rows("x", torch.zeros(4, 2, 9 * 18, 3), 9 * 18, "nlat * nlon")


def test_c_entry_points_refuse_bad_sizes_before_any_hip_call(hip_lib):
    EQ, CEN, GAUSS = 0, 1, 2

    def both(grid, nlat, nlon, lmax, c=3, batch=1):
        args = (None, 0, None, 0, None, None, None, None, grid, batch, nlat, nlon, lmax, c, None, 0, None)
        a, s = hip_lib.gwen_sht_analysis(*args), hip_lib.gwen_sht_synthesis(*args)
        assert a == s
        return a

    assert both(EQ, 17, 64, 9) == -1 and both(CEN, 16, 64, 8) == -1 and both(GAUSS, 9, 64, 9) == -1
    assert both(EQ, 17, 16, 8) == -1                                    # nlon < 2 lmax + 1
    assert both(GAUSS, 2048, 4096, 1024) == -1                          # lmax > 1023
    assert both(3, 17, 32, 4) == -1 and both(-1, 17, 32, 4) == -1       # unknown grid
    assert both(GAUSS, 9, 18, 8, c=0) == -1 and both(GAUSS, 9, 18, 8, batch=-1) == -1
    assert both(GAUSS, 9, 18, 8) == -1                                  # good sizes, null pointers
    assert both(GAUSS, 9, 18, 8, batch=0) == 0                          # nothing to do
    assert both(GAUSS, 2048, 2 ** 21, 8) == -2 and both(GAUSS, 9, 18, 8, c=2 ** 31) == -2
    assert hip_lib.gwen_sht_workspace_bytes(GAUSS, 9, 18, 8, 3) == 9 * 17 * 3 * 8
    assert hip_lib.gwen_sht_workspace_bytes(EQ, 17, 64, 9, 3) == 0
    assert hip_lib.gwen_sht_power_f64(None, None, 1, 8, 3, None) == -1
    assert hip_lib.gwen_sht_power_f64(None, None, 0, 8, 3, None) == 0
    assert hip_lib.gwen_sht_power_f64(None, None, 1, 1024, 3, None) == -1


def test_public_surface():
    import gwen_amd
    assert "SphericalHarmonics" in gwen_amd.__all__ and gwen_amd.SphericalHarmonics is spectral.SphericalHarmonics
