"""The spherical harmonic convention of gwen_amd.spectral restated in numpy fp64 (nothing here imports the package).

Grids: rows (lat, lon) row-major, south to north, longitude 2 pi i / nlon; "equiangular" (poles included,
Clenshaw-Curtis), "equiangular-centred" (Fejer's first rule), "gauss" (Gauss-Legendre); latitude weights sum to 1, a point
weighs w_j / nlon.  Basis: real, 4 pi-normalised, Y_{l,m} = Pbar_l^m(sin lat) cos(m lon), Y_{l,-m} = Pbar_l^m sin(m lon);
coefficient row l^2 + l + m.  analysis: c = sum_p q_p Y(p) x_p; synthesis: x_p = sum c Y(p).
"""
import numpy as np

GRIDS = ("equiangular", "equiangular-centred", "gauss")


def latitudes(grid, nlat):
    """(lat_deg [nlat] south to north, w [nlat] summing to 1)."""
    k = np.arange(nlat, dtype=np.float64)
    if grid == "gauss":
        x, w = np.polynomial.legendre.leggauss(nlat)
        x = 0.5 * (x - x[::-1])
        lat = np.rad2deg(np.arcsin(x))
        w = w / 2.0
    elif grid == "equiangular":
        n = nlat - 1
        lat = -90.0 + (180.0 / n) * k
        lat[-1] = 90.0
        lat = 0.5 * (lat - lat[::-1])
        theta = np.pi * k / n                                   # Clenshaw-Curtis on n + 1 points
        j = np.arange(1, n // 2 + 1, dtype=np.float64)
        b = np.where(2 * j == n, 1.0, 2.0)
        w = 1.0 - (b[None, :] / (4.0 * j[None, :] ** 2 - 1.0) * np.cos(2.0 * j[None, :] * theta[:, None])).sum(1)
        cfac = np.full(nlat, 2.0)
        cfac[0] = cfac[-1] = 1.0
        w = cfac / n * w / 2.0
    elif grid == "equiangular-centred":
        lat = -90.0 + (180.0 / nlat) * (k + 0.5)
        lat = 0.5 * (lat - lat[::-1])
        theta = np.pi * (k + 0.5) / nlat                        # Fejer's first rule on nlat points
        j = np.arange(1, nlat // 2 + 1, dtype=np.float64)
        w = 1.0 - 2.0 * (np.cos(2.0 * j[None, :] * theta[:, None]) / (4.0 * j[None, :] ** 2 - 1.0)).sum(1)
        w = w / nlat
    else:
        raise ValueError(grid)
    w = 0.5 * (w + w[::-1])
    return lat, w / w.sum()


def exact_degree(grid, nlat):
    """The highest polynomial degree in sin lat the quadrature integrates exactly."""
    return 2 * nlat - 1 if grid == "gauss" else nlat - 1


def lmax_limit(grid, nlat):
    return nlat - 1 if grid == "gauss" else (nlat - 1) // 2


def legendre(lmax, m, lat_deg):
    """Pbar_l^m(sin lat) for l = m ... lmax: [lmax + 1 - m, nlat], by the plain fp64 recurrence."""
    phi = np.deg2rad(np.asarray(lat_deg, dtype=np.float64))
    mu, cl = np.sin(phi), np.cos(phi)
    p = np.ones_like(mu)
    for k in range(1, m + 1):
        p = (np.sqrt(3.0) if k == 1 else np.sqrt((2.0 * k + 1.0) / (2.0 * k))) * cl * p
    out = np.empty((lmax + 1 - m, mu.size))
    out[0] = p
    if lmax > m:
        out[1] = np.sqrt(2.0 * m + 3.0) * mu * p
    for l in range(m + 2, lmax + 1):
        a = np.sqrt((4.0 * l * l - 1.0) / (l * l - m * m))
        b = np.sqrt(((l - 1.0) ** 2 - m * m) / (4.0 * (l - 1.0) ** 2 - 1.0))
        out[l - m] = a * (mu * out[l - m - 1] - b * out[l - m - 2])
    return out


def index(l, m):
    return l * l + l + m


def degrees(lmax):
    return np.array([l for l in range(lmax + 1) for _ in range(2 * l + 1)], dtype=np.int64)


def twiddles(nlon, lmax):
    """cos, sin of m lon_i, [nlon, lmax + 1] each, the angle reduced exactly: 2 pi ((m i) mod nlon) / nlon."""
    k = (np.arange(nlon)[:, None] * np.arange(lmax + 1)[None, :]) % nlon
    ang = 2.0 * np.pi * k / nlon
    return np.cos(ang), np.sin(ang)


def analysis(x, grid, nlat, nlon, lmax, lat_w=None):
    """x [B, nlat * nlon, C] -> c [B, (lmax + 1)^2, C].  lat_w [nlat]: the latitude weight, default w_j / nlon (ones make
    it the adjoint of the synthesis)."""
    lat, w = latitudes(grid, nlat)
    lat_w = w / nlon if lat_w is None else np.asarray(lat_w, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    b, _, ch = x.shape
    x = x.reshape(b, nlat, nlon, ch)
    ct, st = twiddles(nlon, lmax)
    fc = np.einsum("bjic,im->mbjc", x, ct)
    fs = np.einsum("bjic,im->mbjc", x, st)
    c = np.zeros((b, (lmax + 1) ** 2, ch))
    ls = np.arange(lmax + 1)
    for m in range(lmax + 1):
        p = legendre(lmax, m, lat) * lat_w[None, :]
        rows = ls[m:] ** 2 + ls[m:]
        c[:, rows + m, :] = np.einsum("lj,bjc->blc", p, fc[m])
        if m:
            c[:, rows - m, :] = np.einsum("lj,bjc->blc", p, fs[m])
    return c


def synthesis(c, grid, nlat, nlon, lmax, lat_w=None):
    """c [B, (lmax + 1)^2, C] -> x [B, nlat * nlon, C].  lat_w [nlat] scales the rows of the result (default ones; w_j / nlon
    makes it the adjoint of the analysis)."""
    lat, _ = latitudes(grid, nlat)
    c = np.asarray(c, dtype=np.float64)
    b, _, ch = c.shape
    ct, st = twiddles(nlon, lmax)
    ls = np.arange(lmax + 1)
    x = np.zeros((b, nlat, nlon, ch))
    for m in range(lmax + 1):
        p = legendre(lmax, m, lat)
        rows = ls[m:] ** 2 + ls[m:]
        gc = np.einsum("lj,blc->bjc", p, c[:, rows + m, :])
        x += gc[:, :, None, :] * ct[None, None, :, m, None]
        if m:
            gs = np.einsum("lj,blc->bjc", p, c[:, rows - m, :])
            x += gs[:, :, None, :] * st[None, None, :, m, None]
    if lat_w is not None:
        x *= np.asarray(lat_w, dtype=np.float64)[None, :, None, None]
    return x.reshape(b, nlat * nlon, ch)


def analysis_adjoint(g, grid, nlat, nlon, lmax):
    """A^T g = q * synthesis(g): g [B, T, C] -> [B, nlat * nlon, C]."""
    _, w = latitudes(grid, nlat)
    return synthesis(g, grid, nlat, nlon, lmax, lat_w=w / nlon)


def synthesis_adjoint(h, grid, nlat, nlon, lmax):
    """S^T h = the analysis with unit weights: h [B, nlat * nlon, C] -> [B, T, C]."""
    return analysis(h, grid, nlat, nlon, lmax, lat_w=np.ones(nlat))


def power(c, lmax):
    """S_l = sum_m c_lm^2: c [B, T, C] -> [B, lmax + 1, C]."""
    c = np.asarray(c, dtype=np.float64)
    return np.stack([(c[:, l * l:(l + 1) ** 2, :] ** 2).sum(1) for l in range(lmax + 1)], axis=1)


def point_weights(grid, nlat, nlon):
    _, w = latitudes(grid, nlat)
    return np.repeat(w / nlon, nlon)


def latlon(grid, nlat, nlon):
    """(lat, lon) in radians of every grid row, [nlat * nlon] each."""
    lat, _ = latitudes(grid, nlat)
    lon = 2.0 * np.pi * np.arange(nlon) / nlon
    return np.repeat(np.deg2rad(lat), nlon), np.tile(lon, nlat)
