"""The vector spherical harmonic convention of gwen_amd.spectral restated in numpy fp64 (it imports tests/sht_ref.py for
the grids, the scalar basis and the row order, and nothing of the package).

Unit sphere, u eastward, v northward.  With streamfunction psi and velocity potential chi
    u = -d psi/d lat + (1 / cos lat) d chi/d lon,   v = (1 / cos lat) d psi/d lon + d chi/d lat,
    vort = lap psi,  div = lap chi,  lap Y_lm = -L Y_lm,  L = l (l + 1).
Q_l^m = Pbar_l^m / cos lat and D_l^m = d Pbar_l^m / d lat never divide by cos lat: for m >= 1, Q walks the recurrence of
Pbar from seed[m] cos^(m-1) lat and D_l^m = -l sin lat Q_l^m + sqrt((2l+1)(l^2-m^2)/(2l-1)) Q_{l-1}^m; for m = 0 the Q
term carries the factor m = 0 and D_l^0 = sqrt(l (l + 1) / 2) Pbar_l^1.  grad Y of the cos row (m >= 0) is
(east, north) = (-m Q sin m lon, D cos m lon), of the sin row (m Q cos m lon, D sin m lon); k x grad Y = (-north, east).

    vector_synthesis(vort, div):  psi = -vort / L, chi = -div / L (row 0 read as 0), (u, v) = sum psi k x grad Y + chi grad Y
    vector_analysis(u, v):        div_lm = -sum_p q_p (u, v) . grad Y_lm,  vort_lm = -sum_p q_p (u, v) . (k x grad Y_lm)
    kinetic_energy:               E_l = sum_m (vort_lm^2 + div_lm^2) / (2 L),  E_0 = 0
"""
import numpy as np

import sht_ref as R


def tables(lmax, m, lat_deg):
    """(m Q_l^m, D_l^m) for l = m ... lmax: [lmax + 1 - m, nlat] each."""
    phi = np.deg2rad(np.asarray(lat_deg, dtype=np.float64))
    mu, cl = np.sin(phi), np.cos(phi)
    n = lmax + 1 - m
    if m == 0:
        d = np.zeros((n, mu.size))
        if lmax >= 1:
            l = np.arange(1, lmax + 1, dtype=np.float64)
            d[1:] = np.sqrt(l * (l + 1.0) / 2.0)[:, None] * R.legendre(lmax, 1, lat_deg)
        return np.zeros((n, mu.size)), d
    p = np.ones_like(mu)
    for k in range(1, m + 1):                                   # seed[m] cos^(m-1): the sectoral seed, one cosine short
        p = (np.sqrt(3.0) if k == 1 else np.sqrt((2.0 * k + 1.0) / (2.0 * k))) * (cl if k > 1 else 1.0) * p
    q = np.empty((n, mu.size))
    q[0] = p
    if n > 1:
        q[1] = np.sqrt(2.0 * m + 3.0) * mu * p
    for l in range(m + 2, lmax + 1):
        a = np.sqrt((4.0 * l * l - 1.0) / (l * l - m * m))
        b = np.sqrt(((l - 1.0) ** 2 - m * m) / (4.0 * (l - 1.0) ** 2 - 1.0))
        q[l - m] = a * (mu * q[l - m - 1] - b * q[l - m - 2])
    d = np.empty_like(q)
    d[0] = -m * mu * q[0]
    for l in range(m + 1, lmax + 1):
        d[l - m] = -l * mu * q[l - m] + np.sqrt((2.0 * l + 1.0) * (l * l - m * m) / (2.0 * l - 1.0)) * q[l - m - 1]
    return m * q, d


def _row_scale(lmax, inverse):
    """[T]: 1 / L (inverse) or L per row, 0 on row 0."""
    l = R.degrees(lmax).astype(np.float64)
    big = l * (l + 1.0)
    if not inverse:
        return big
    out = np.zeros_like(big)
    out[1:] = 1.0 / big[1:]
    return out


def vector_analysis(u, v, grid, nlat, nlon, lmax, lat_w=None):
    """u, v [B, nlat * nlon, C] -> (vort, div) [B, (lmax + 1)^2, C].  lat_w [nlat]: the latitude weight, default
    w_j / nlon."""
    lat, w = R.latitudes(grid, nlat)
    lat_w = w / nlon if lat_w is None else np.asarray(lat_w, dtype=np.float64)
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    b, _, ch = u.shape
    u, v = u.reshape(b, nlat, nlon, ch), v.reshape(b, nlat, nlon, ch)
    ct, st = R.twiddles(nlon, lmax)
    uc, us = np.einsum("bjic,im->mbjc", u, ct), np.einsum("bjic,im->mbjc", u, st)
    vc, vs = np.einsum("bjic,im->mbjc", v, ct), np.einsum("bjic,im->mbjc", v, st)
    vort = np.zeros((b, (lmax + 1) ** 2, ch))
    div = np.zeros_like(vort)
    ls = np.arange(lmax + 1)
    for m in range(lmax + 1):
        mq, d = tables(lmax, m, lat)
        mq, d = mq * lat_w[None, :], d * lat_w[None, :]
        rows = ls[m:] ** 2 + ls[m:]
        vort[:, rows + m] = np.einsum("lj,bjc->blc", d, uc[m]) + np.einsum("lj,bjc->blc", mq, vs[m])
        div[:, rows + m] = np.einsum("lj,bjc->blc", mq, us[m]) - np.einsum("lj,bjc->blc", d, vc[m])
        if m:
            vort[:, rows - m] = np.einsum("lj,bjc->blc", d, us[m]) - np.einsum("lj,bjc->blc", mq, vc[m])
            div[:, rows - m] = -np.einsum("lj,bjc->blc", mq, uc[m]) - np.einsum("lj,bjc->blc", d, vs[m])
    vort[:, 0] = 0.0
    div[:, 0] = 0.0
    return vort, div


def _synthesis_of_potentials(psi, chi, grid, nlat, nlon, lmax, lat_w):
    lat, _ = R.latitudes(grid, nlat)
    b, _, ch = psi.shape
    ct, st = R.twiddles(nlon, lmax)
    ls = np.arange(lmax + 1)
    u = np.zeros((b, nlat, nlon, ch))
    v = np.zeros_like(u)
    for m in range(lmax + 1):
        mq, d = tables(lmax, m, lat)
        rows = ls[m:] ** 2 + ls[m:]
        pc, xc = psi[:, rows + m], chi[:, rows + m]
        ps, xs = (psi[:, rows - m], chi[:, rows - m]) if m else (np.zeros_like(pc), np.zeros_like(xc))
        ucos = -np.einsum("lj,blc->bjc", d, pc) + np.einsum("lj,blc->bjc", mq, xs)
        usin = -np.einsum("lj,blc->bjc", d, ps) - np.einsum("lj,blc->bjc", mq, xc)
        vcos = np.einsum("lj,blc->bjc", mq, ps) + np.einsum("lj,blc->bjc", d, xc)
        vsin = -np.einsum("lj,blc->bjc", mq, pc) + np.einsum("lj,blc->bjc", d, xs)
        cm, sm = ct[None, None, :, m, None], st[None, None, :, m, None]
        u += ucos[:, :, None, :] * cm + usin[:, :, None, :] * sm
        v += vcos[:, :, None, :] * cm + vsin[:, :, None, :] * sm
    if lat_w is not None:
        lw = np.asarray(lat_w, dtype=np.float64)[None, :, None, None]
        u, v = u * lw, v * lw
    return u.reshape(b, nlat * nlon, ch), v.reshape(b, nlat * nlon, ch)


def vector_synthesis(vort, div, grid, nlat, nlon, lmax, lat_w=None):
    """vort, div [B, (lmax + 1)^2, C] (either may be None = zero) -> (u, v) [B, nlat * nlon, C].  lat_w [nlat] scales the
    rows of the result (default ones).  Row 0 is read as 0, whatever it holds."""
    some = vort if vort is not None else div
    zero = np.zeros(np.asarray(some).shape)
    inv = _row_scale(lmax, True)[None, :, None]
    pots = []
    for c in (vort, div):
        c = zero if c is None else np.array(c, dtype=np.float64)
        c[:, 0] = 0.0
        pots.append(-c * inv)
    return _synthesis_of_potentials(pots[0], pots[1], grid, nlat, nlon, lmax, lat_w)


def vector_analysis_adjoint(g_vort, g_div, grid, nlat, nlon, lmax):
    """VA^T (g_vort, g_div) = q * VS(L g_vort, L g_div): -> (h_u, h_v) [B, nlat * nlon, C]."""
    _, w = R.latitudes(grid, nlat)
    big = _row_scale(lmax, False)[None, :, None]
    return vector_synthesis(big * np.asarray(g_vort, dtype=np.float64), big * np.asarray(g_div, dtype=np.float64),
                            grid, nlat, nlon, lmax, lat_w=w / nlon)


def vector_synthesis_adjoint(h_u, h_v, grid, nlat, nlon, lmax):
    """VS^T (h_u, h_v) = VA with unit latitude weights, over L (row 0 -> 0): -> (g_vort, g_div) [B, T, C]."""
    vort, div = vector_analysis(h_u, h_v, grid, nlat, nlon, lmax, lat_w=np.ones(nlat))
    inv = _row_scale(lmax, True)[None, :, None]
    return vort * inv, div * inv


def gradient(c, grid, nlat, nlon, lmax):
    """(east, north) of the gradient of the scalar with coefficients c: vector_synthesis(None, -L c)."""
    big = _row_scale(lmax, False)[None, :, None]
    return vector_synthesis(None, -big * np.asarray(c, dtype=np.float64), grid, nlat, nlon, lmax)


def kinetic_energy(vort, div, lmax):
    """E_l = sum_m (vort_lm^2 + div_lm^2) / (2 L), E_0 = 0: [B, T, C] twice -> [B, lmax + 1, C]."""
    s = R.power(vort, lmax) + R.power(div, lmax)
    l = np.arange(lmax + 1, dtype=np.float64)
    inv = np.zeros(lmax + 1)
    inv[1:] = 0.5 / (l[1:] * (l[1:] + 1.0))
    return s * inv[None, :, None]
