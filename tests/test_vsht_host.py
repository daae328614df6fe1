"""Vector spherical harmonics on the host: the numpy restatement (tests/vsht_ref.py) against its own identities and closed
forms, and every argument error of gwen_amd.spectral's vector methods and of the C entry points that comes before a
device call -- none of it touches a device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sht_ref as R  # noqa: E402
import vsht_ref as V  # noqa: E402

from gwen_amd import spectral  # noqa: E402

# (grid, nlat, nlon, lmax): each at its quadrature's limit; the equiangular grid has both pole rows and an equator row
GEOMS = [("gauss", 9, 18, 8), ("equiangular", 17, 18, 8), ("equiangular-centred", 16, 16, 7)]


def band_limited(geom, seed, b=2, c=3):
    lmax = geom[3]
    rng = np.random.default_rng(seed)
    vort, div = rng.standard_normal((2, b, (lmax + 1) ** 2, c))
    vort[:, 0] = div[:, 0] = 0.0
    return vort, div


@pytest.mark.parametrize("geom", GEOMS, ids=[g[0] for g in GEOMS])
def test_restatement_round_trip_parseval_and_adjoints(geom):
    grid, nlat, nlon, lmax = geom
    vort, div = band_limited(geom, 31)
    u, v = V.vector_synthesis(vort, div, *geom)
    back_vort, back_div = V.vector_analysis(u, v, *geom)
    assert np.abs(back_vort - vort).max() <= 1e-12 and np.abs(back_div - div).max() <= 1e-12
    q = R.point_weights(grid, nlat, nlon)
    energy = V.kinetic_energy(vort, div, lmax)
    assert (energy[:, 0] == 0.0).all()
    assert np.allclose(energy.sum(1), (q[None, :, None] * (u * u + v * v) / 2.0).sum(1), rtol=1e-12, atol=0)
    # <VS(a, b), (U, V)>_q = <(a, b), VA(U, V)> / L
    rng = np.random.default_rng(32)
    U, W = rng.standard_normal((2,) + u.shape)
    av, ad = V.vector_analysis(U, W, *geom)
    inv = np.zeros((lmax + 1) ** 2)
    l = R.degrees(lmax)[1:].astype(np.float64)
    inv[1:] = 1.0 / (l * (l + 1.0))
    lhs = (q[None, :, None] * (u * U + v * W)).sum()
    rhs = ((vort * av + div * ad) * inv[None, :, None]).sum()
    assert abs(lhs - rhs) <= 1e-12 * (np.abs(vort).sum() + np.abs(div).sum())
    # the two adjoints the backward passes use
    g_vort, g_div = rng.standard_normal((2,) + vort.shape)
    h_u, h_v = V.vector_analysis_adjoint(g_vort, g_div, *geom)
    assert abs((av * g_vort + ad * g_div).sum() - (U * h_u + W * h_v).sum()) <= 1e-12 * np.abs(g_vort).sum()
    s_u, s_v = V.vector_synthesis(g_vort, g_div, *geom)
    t_vort, t_div = V.vector_synthesis_adjoint(U, W, *geom)
    assert abs((s_u * U + s_v * W).sum() - (t_vort * g_vort + t_div * g_div).sum()) <= 1e-12 * np.abs(U).sum() * 2
    assert (t_vort[:, 0] == 0).all() and (t_div[:, 0] == 0).all()
    # a missing tensor is zero, and row 0 is read as 0 whatever it holds
    only_u, only_v = V.vector_synthesis(vort, None, *geom)
    zero_u, zero_v = V.vector_synthesis(vort, np.zeros_like(vort), *geom)
    assert np.array_equal(only_u, zero_u) and np.array_equal(only_v, zero_v)
    bad = vort.copy()
    bad[:, 0] = np.nan
    nan_u, nan_v = V.vector_synthesis(bad, None, *geom)
    assert np.array_equal(nan_u, only_u) and np.array_equal(nan_v, only_v)


@pytest.mark.parametrize("geom", GEOMS, ids=[g[0] for g in GEOMS])
def test_restatement_closed_forms(geom):
    grid, nlat, nlon, lmax = geom
    lat, lon = R.latlon(grid, nlat, nlon)
    t = (lmax + 1) ** 2
    # solid-body rotation u = cos lat, v = 0: vort_{1,0} = 2 / sqrt 3 alone
    vort, div = V.vector_analysis(np.cos(lat)[None, :, None], np.zeros((1, lat.size, 1)), *geom)
    want = np.zeros((1, t, 1))
    want[0, R.index(1, 0), 0] = 2.0 / np.sqrt(3.0)
    assert np.abs(vort - want).max() <= 1e-12 and np.abs(div).max() <= 1e-12
    # f = sin lat cos lat cos lon: gradient (-sin lat sin lon, cos 2 lat cos lon)
    c = R.analysis((np.sin(lat) * np.cos(lat) * np.cos(lon))[None, :, None], *geom)
    east, north = V.gradient(c, *geom)
    assert np.abs(east[0, :, 0] + np.sin(lat) * np.sin(lon)).max() <= 1e-12
    assert np.abs(north[0, :, 0] - np.cos(2.0 * lat) * np.cos(lon)).max() <= 1e-12
    # vort_{1,1} = -2 alone: u = sqrt 3 sin lat cos lon, v = -sqrt 3 sin lon, which does not vanish at the poles
    vort = np.zeros((1, t, 1))
    vort[0, R.index(1, 1), 0] = -2.0
    u, v = V.vector_synthesis(vort, None, *geom)
    assert np.abs(u[0, :, 0] - np.sqrt(3.0) * np.sin(lat) * np.cos(lon)).max() <= 1e-12
    assert np.abs(v[0, :, 0] + np.sqrt(3.0) * np.sin(lon)).max() <= 1e-12
    if grid == "equiangular":
        for rows in (slice(0, nlon), slice(-nlon, None)):
            assert abs(abs(lat[rows]) - np.pi / 2.0).max() <= 1e-15
            speed = np.hypot(u[0, rows, 0], v[0, rows, 0])
            assert np.isfinite(speed).all() and np.abs(speed - np.sqrt(3.0)).max() <= 1e-12
    back, none = V.vector_analysis(u, v, *geom)
    assert np.abs(back - vort).max() <= 1e-12 and np.abs(none).max() <= 1e-12


def test_gradient_magnitudes_obey_the_addition_theorem_at_the_poles():
    # sum_m |grad Y_lm|^2 = l (l + 1)(2l + 1) at every point, the poles included: the bound of tests/test_gpu_vsht.py
    lmax = 12
    lat = np.array([-90.0, -37.0, 0.0, 90.0])
    total = np.zeros((lmax + 1, lat.size))
    for m in range(lmax + 1):
        mq, d = V.tables(lmax, m, lat)
        total[m:] += mq * mq + d * d                            # the cos and the sin row of order m together
    l = np.arange(lmax + 1, dtype=np.float64)
    want = (l * (l + 1.0) * (2.0 * l + 1.0))[:, None]
    assert np.abs(total - want).max() <= 1e-12 * want.max()


def bare(nlat=9, nlon=18, lmax=8):
    """A SphericalHarmonics without tables: what the argument checks read, and no device."""
    sh = object.__new__(spectral.SphericalHarmonics)
    sh.nlat, sh.nlon, sh.lmax, sh.grid = nlat, nlon, lmax, "gauss"
    sh.rows, sh.num_coefficients = nlat * nlon, (lmax + 1) ** 2
    sh.device = torch.device("cuda:0")
    return sh


def test_vector_argument_errors_come_in_order_before_any_device_call():
    sh = bare()
    n, t = sh.rows, sh.num_coefficients
    good = torch.zeros(2, n, 3)
    # shapes first
    with pytest.raises(ValueError):
        sh.vector_analysis(torch.zeros(2, n + 1, 3, dtype=torch.float64), good)
    with pytest.raises(ValueError, match="one shape"):
        sh.vector_analysis(good, torch.zeros(2, n, 4))
    with pytest.raises(ValueError, match="one shape"):
        sh.vector_analysis(good, torch.zeros(1, n, 3, dtype=torch.float64))
    with pytest.raises(ValueError):
        sh.vector_analysis(good, None)
    with pytest.raises(ValueError):
        sh.vector_synthesis(torch.zeros(2, t, 3), torch.zeros(2, t + 1, 3))
    with pytest.raises(ValueError):
        sh.vector_synthesis(None, None)
    with pytest.raises(ValueError):
        sh.gradient(torch.zeros(2, t - 1, 3))
    # then dtypes
    with pytest.raises(TypeError):
        sh.vector_analysis(good, good.double())
    with pytest.raises(TypeError):
        sh.vector_analysis(good.double(), good.double())
    with pytest.raises(TypeError):
        sh.vector_synthesis(torch.zeros(2, t, 3), torch.zeros(2, t, 3, dtype=torch.float64))
    with pytest.raises(TypeError):
        sh.vector_synthesis(torch.zeros(2, t, 3, dtype=torch.float16), None)
    with pytest.raises(TypeError):
        sh.gradient(torch.zeros(2, t, 3, dtype=torch.int32))
    # then devices
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sh.vector_analysis(good, good)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sh.vector_synthesis(None, torch.zeros(2, t, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sh.gradient(torch.zeros(2, t, 3))
    # the output dtype is judged after the inputs' devices, as in analysis(): a CPU tensor of a good dtype is the
    # RuntimeError whatever dtype is asked for
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sh.vector_analysis(good, good, dtype=torch.float16)


def test_kinetic_energy_spectrum_takes_exactly_one_pair():
    sh = bare()
    n, t = sh.rows, sh.num_coefficients
    x, c = torch.zeros(n, 2), torch.zeros(t, 2)
    for kwargs in (dict(), dict(u=x), dict(u=x, v=x, vort=c, div=c), dict(u=x, v=x, vort=c), dict(vort=c),
                   dict(u=x, div=c), dict(v=x, vort=c, div=c)):
        with pytest.raises(ValueError, match="exactly one"):
            sh.kinetic_energy_spectrum(**kwargs)
    with pytest.raises(ValueError, match="one shape"):
        sh.kinetic_energy_spectrum(u=x, v=torch.zeros(n, 3))
    with pytest.raises(ValueError):
        sh.kinetic_energy_spectrum(vort=c, div=torch.zeros(t + 1, 2))
    with pytest.raises(TypeError):
        sh.kinetic_energy_spectrum(u=x.double(), v=x.double())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sh.kinetic_energy_spectrum(u=x, v=x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sh.kinetic_energy_spectrum(vort=c, div=c)


def test_vector_c_entry_points_refuse_bad_arguments_before_any_hip_call(hip_lib):
    EQ, CEN, GAUSS = 0, 1, 2

    def both(grid, nlat, nlon, lmax, c=3, batch=1, adjoint=0, f64=0):
        args = (None, None, f64, None, None, 0, None, None, None, None, grid, batch, nlat, nlon, lmax, c, adjoint, None,
                0, None)
        a, s = hip_lib.gwen_sht_vector_analysis(*args), hip_lib.gwen_sht_vector_synthesis(*args)
        assert a == s
        return a

    assert both(EQ, 17, 64, 9) == -1 and both(CEN, 16, 64, 8) == -1 and both(GAUSS, 9, 64, 9) == -1
    assert both(EQ, 17, 16, 8) == -1                                    # nlon < 2 lmax + 1
    assert both(GAUSS, 2048, 4096, 1024) == -1                          # lmax > 1023
    assert both(3, 17, 32, 4) == -1 and both(-1, 17, 32, 4) == -1       # unknown grid
    assert both(GAUSS, 9, 18, 8, c=0) == -1 and both(GAUSS, 9, 18, 8, batch=-1) == -1
    assert both(GAUSS, 9, 18, 8, batch=0, adjoint=2) == -1 and both(GAUSS, 9, 18, 8, batch=0, f64=2) == -1
    assert both(GAUSS, 9, 18, 8) == -1                                  # good sizes, null pointers
    assert both(GAUSS, 9, 18, 8, batch=0) == 0 and both(GAUSS, 9, 18, 8, batch=0, adjoint=1) == 0
    assert both(GAUSS, 2048, 2 ** 21, 8) == -2 and both(GAUSS, 9, 18, 8, c=2 ** 31) == -2
    assert hip_lib.gwen_sht_vector_workspace_bytes(GAUSS, 9, 18, 8, 3) == 2 * 9 * 17 * 3 * 8
    assert hip_lib.gwen_sht_vector_workspace_bytes(GAUSS, 9, 18, 8, 3) == 2 * hip_lib.gwen_sht_workspace_bytes(
        GAUSS, 9, 18, 8, 3)
    assert hip_lib.gwen_sht_vector_workspace_bytes(EQ, 17, 64, 9, 3) == 0
