"""Spherical harmonic transforms and power spectra of fields on a latitude-longitude grid, on the device.

Convention (include/gwen_hip.h, "Spherical harmonic transforms"; tests/sht_ref.py restates it in numpy):

    grid      rows ``(lat, lon)`` row-major, south to north, longitudes ``2 pi i / nlon`` -- the layout of
              ``gridgraph.latlon_grid``.  Three latitude sets, each with quadrature weights ``w_j`` that sum to 1; a grid
              point weighs ``q = w_j / nlon``:
                  "equiangular"          the rows of ``latlon_grid(nlat, nlon, poles=True)``, Clenshaw-Curtis,
                                         exact for ``lmax <= (nlat - 1) // 2``
                  "equiangular-centred"  the rows of ``latlon_grid(nlat, nlon, poles=False)``, Fejer's first rule,
                                         exact for ``lmax <= (nlat - 1) // 2``
                  "gauss"                the ``nlat`` Gauss-Legendre latitudes, exact for ``lmax <= nlat - 1``
              Always ``nlon >= 2 lmax + 1``, ``lmax <= 1023`` and ``nlat <= 2048``; the default ``lmax`` is the largest
              the grid and ``nlon`` allow.
    basis     real, 4 pi-normalised: ``Y_{l,m} = Pbar_l^m(sin lat) cos(m lon)`` for ``m >= 0`` and
              ``Y_{l,-m} = Pbar_l^m(sin lat) sin(m lon)`` for ``m > 0``; the sphere mean of ``Y^2`` is 1.
              ``Pbar_0^0 = 1``, ``Pbar_1^1 = sqrt(3) cos lat``, ``Pbar_m^m = sqrt((2m+1)/(2m)) cos lat Pbar_{m-1}^{m-1}``,
              ``Pbar_{m+1}^m = sqrt(2m+3) sin lat Pbar_m^m`` and ``Pbar_l^m = a (sin lat Pbar_{l-1}^m - b Pbar_{l-2}^m)``
              with ``a = sqrt((4 l^2 - 1) / (l^2 - m^2))``, ``b = sqrt(((l-1)^2 - m^2) / (4 (l-1)^2 - 1))``.
    rows      the coefficient of ``(l, m)`` is row ``l^2 + l + m`` of ``T = (lmax + 1)^2``.
    analysis  ``c_lm = sum_p q_p Y_lm(p) x_p``;  synthesis ``x_p = sum_lm c_lm Y_lm(p)``;  power ``S_l = sum_m c_lm^2``
              (for a band-limited field ``sum_l S_l = sum_p q_p x_p^2``).
    vector    winds are no scalars on the sphere (on a pole row ``u`` and ``v`` turn with the longitude), so they have
              transforms of their own, on the unit sphere, ``u`` eastward and ``v`` northward.  With streamfunction
              ``psi`` and velocity potential ``chi``:
                  ``u = -d psi/d lat + (1/cos lat) d chi/d lon``,  ``v = (1/cos lat) d psi/d lon + d chi/d lat``,
                  ``vort = lap psi``, ``div = lap chi``, ``lap Y_lm = -L Y_lm`` with ``L = l (l + 1)``.
              ``vector_synthesis(vort, div)`` sums ``psi_lm (k x grad Y_lm) + chi_lm grad Y_lm`` with ``psi = -vort / L``,
              ``chi = -div / L`` (row 0 read as 0); ``vector_analysis(u, v)`` gives ``div_lm = -sum_p q_p (u, v) . grad
              Y_lm`` and ``vort_lm = -sum_p q_p (u, v) . (k x grad Y_lm)`` (row 0 is 0), its inverse on band-limited pairs,
              pole rows included.  ``grad Y`` of a cos row is (east, north) = ``(-m Q sin m lon, D cos m lon)``, of a sin
              row ``(m Q cos m lon, D sin m lon)``, with ``Q = Pbar_l^m / cos lat`` and ``D = d Pbar_l^m / d lat`` from
              one recurrence that never divides by ``cos lat`` (include/gwen_hip.h); ``k x grad Y = (-north, east)``.
              Kinetic energy ``E_l = sum_m (vort_lm^2 + div_lm^2) / (2 L)``, ``E_0 = 0``; for a band-limited wind
              ``sum_l E_l = sum_p q_p (u^2 + v^2) / 2``.  ``gradient``, ``laplacian`` and ``inverse_laplacian`` follow.
              Users of a sphere of radius ``a`` scale by ``1/a`` and ``1/a^2``.

Reduced Gaussian grids (``SphericalHarmonics.reduced``, ``SphericalHarmonics.octahedral``; the octahedral ``O96 / O320 /
O640`` and the classic ``N320`` grids of IFS, ERA5 and AIFS) keep everything above and change the rings:

    grid      ``nlat`` Gauss-Legendre latitudes, the nodes and weights ``w_j`` of ``"gauss"``, south to north, and an
              integer vector ``ring_nlon[nlat]``: ring ``j`` holds the longitudes ``2 pi i / ring_nlon[j]``,
              ``i = 0 ... ring_nlon[j] - 1``, starting at longitude 0.  Field rows are ring-major: ring ``j`` starts at row
              ``ring_start[j] = sum_{k<j} ring_nlon[k]`` of ``P = ring_start[nlat]`` points.  A point of ring ``j`` weighs
              ``q = w_j / ring_nlon[j]``; the weights sum to 1.  ``octahedral_nlon(N)`` gives the ``2 N`` ring lengths
              ``4 i + 16``, ``i = 1 ... N``, from each pole to the equator; a classic reduced grid is the user's own list
              (the ``pl`` array of a GRIB file).
    orders    ring ``j`` carries the orders ``m <= M_j = min(lmax, (ring_nlon[j] - 1) // 2)``: the analysis takes the orders
              above ``M_j`` of that ring as zero and the synthesis leaves them out, one masked operator, so the adjoint
              relations of the regular grids hold exactly.  Where every ``ring_nlon[j] >= 2 lmax + 1`` nothing is
              truncated, and rings of one length reproduce ``SphericalHarmonics(nlat, nlon, grid="gauss")`` bit for bit.
    limits    ``nlat <= 2048``, ``lmax <= min(1023, nlat - 1)``, ``max(ring_nlon) >= 2 lmax + 1``, ``P <= 2^31 - 1``.
    accuracy  how well ``analysis(synthesis(c))`` returns ``c`` is a property of the pair (ring lengths, ``lmax``) and not
              of the code: the short polar rings alias what they cannot carry.  A numpy fp64 restatement
              (tests/sht_rings_ref.py) of the round trip of unit-normal coefficients gave, as the largest error,
                  O8, lmax 7: 4e-15     O8, lmax 11 (M_j down to 9): 6e-15     O16, lmax 15: 4e-14
                  O16, lmax 23: 2e-8    O16, lmax 31: 6e-3
              -- round-off at the cubic pairing ``lmax = N - 1`` (the default of ``octahedral``), degrading beyond it.
    longitude ``longitude`` is ``"direct"`` only: octahedral ring lengths mostly have prime factors above 5, which the
              mixed-radix FFT does not take.  The longitude stage of a reduced grid has a keyword of its own,
              ``ring_longitude``: ``"direct"`` (the default) sums as above, ``"bluestein"`` makes every ring of every item
              and channel one fp64 FFT in LDS whatever its length (csrc/sht_fft.h) -- the mixed-radix FFT of
              ``longitude="fft"`` on a ring of ``2^a 3^b 5^c`` points (rings of one such length reproduce
              ``SphericalHarmonics(nlat, nlon, grid="gauss", longitude="fft")`` bit for bit) and elsewhere Bluestein's
              chirp-z convolution on the same stages: with ``n = nlon // 2`` (even rings, and a split step) or ``nlon``,
              ``c_k = exp(-i pi k^2 / n)`` and ``M`` the smallest ``2^a 3^b 5^c >= 2 n - 1``, the ring's DFT is ``c_k``
              times the cyclic convolution of length ``M`` of ``z c`` with ``conj c``, two FFTs of length ``M`` and three
              pointwise products.  ``ring_fft_plan(nlon)`` tells how a ring runs; ``M <= 4096``, so even rings up to 4096
              points and odd ones up to 2048 (any smooth length up to 4096) are taken, ``check_rings`` raising for others.
              Same truncation, same numbers up to rounding, as reproducible and as NaN-tight as ``longitude="fft"``; no
              automatic choice and no fallback.  A regular Gauss grid with an ``nlon`` that ``longitude="fft"`` does not
              take is ``reduced([nlon] * nlat, ..., ring_longitude="bluestein")``.

Everything is accumulated in fp64 by two HIP kernels a transform (csrc/sht.hip): the sums along every latitude ring
against an ``nlon``-entry twiddle table, and a contraction over the latitudes with ``Pbar_l^m`` generated on the fly (the
vector transforms: the ring sums of ``u`` and of ``v``, and one contraction against ``m Q`` and ``D``).  The ring sums
are direct sums (``longitude="direct"``, the default) or, on request (``longitude="fft"``), one fp64 mixed-radix FFT a
ring and channel in LDS (csrc/sht_fft.h) for ``nlon = 2^a 3^b 5^c <= 4096``: the same numbers up to rounding, in
``O(nlon log nlon)`` and not ``O(nlon lmax)``.  There is no automatic choice and no fallback between the two.
Results are bitwise reproducible, whatever the batch and the workspace.  Nodes, weights and tables are made on the host
in fp64 at construction; after it nothing synchronises with the host, so a call can be captured into a hipGraph once it has
run eagerly.  There is no CPU fallback: CPU tensors raise RuntimeError.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

GRIDS = ("equiangular", "equiangular-centred", "gauss")
MAX_LMAX = 1023
MAX_NLAT = 2048
LONGITUDE = ("direct", "fft")
MAX_FFT_NLON = 4096
RING_LONGITUDE = ("direct", "bluestein")
MAX_RING_FFT_POINTS = 4096                 # complex points of a ring's FFT in LDS (kPoints of csrc/sht_fft.h)


def fft_supported(nlon: int) -> bool:
    """Whether ``longitude="fft"`` takes rings of ``nlon`` points: ``1 <= nlon <= 4096`` with no prime factor other than
    2, 3 and 5 (``gwen_sht_fft_supported``)."""
    nlon = int(nlon)
    if not 1 <= nlon <= MAX_FFT_NLON:
        return False
    for f in (2, 3, 5):
        while nlon % f == 0:
            nlon //= f
    return nlon == 1


def ring_fft_plan(nlon: int) -> Tuple[Optional[str], int, int]:
    """``(kind, n, M)``: how ``ring_longitude="bluestein"`` runs a ring of ``nlon`` longitudes (``gwen_sht_ring_fft_plan``).
    ``n`` is the length of the ring's complex FFT, ``nlon // 2`` for an even ``nlon`` (with a split step) and ``nlon`` for
    an odd one.  ``kind`` is ``"mixed"`` where ``fft_supported(nlon)`` -- the radix-4/2/3/5 FFT of ``longitude="fft"``,
    ``M = 0`` -- and ``"bluestein"`` otherwise: a cyclic convolution of length ``M``, the smallest ``2^a 3^b 5^c >= 2 n -
    1``.  ``kind`` is ``None`` where that ``M`` is above 4096: the ring is not supported."""
    nlon = int(nlon)
    if nlon < 1:
        return None, 0, 0
    n = nlon // 2 if nlon % 2 == 0 else nlon
    if fft_supported(nlon):
        return "mixed", n, 0
    m = 2 * n - 1
    while m <= MAX_RING_FFT_POINTS and not fft_supported(m):
        m += 1
    if m > MAX_RING_FFT_POINTS:
        return None, n, 0
    return "bluestein", n, m


def ring_fft_tables(ring_nlon) -> dict:
    """The host tables of ``ring_longitude="bluestein"`` for supported ring lengths, numpy, one set per distinct length
    (include/gwen_hip.h, ``gwen_sht_rings_fft_call``):

        ``plan [nlat, 8]`` int32   ``(kind, n, M, chirp_at, filter_at, conv_at, 0, 0)``, kind 1 mixed, 2 Bluestein
        ``chirp [*, 2]`` fp64      ``c_k = exp(-i pi k^2 / n)``, ``k < n``, the phase index ``k^2 mod 2 n`` in integers
        ``filter [*, 2]`` fp64     ``H = FFT_M(h) / M`` of ``h_k = conj c_k`` wrapped to ``|k| < n``
        ``conv_twiddle [*, 2]``    ``(cos, sin)(2 pi k / M)``, ``k < M``, one table per distinct ``M``
        ``max_points``             the largest ``n`` of a mixed and ``M`` of a Bluestein ring

    Every table has at least one entry, so that its device copy has an address."""
    rings = np.asarray(ring_nlon, dtype=np.int64)
    plan = np.zeros((rings.size, 8), dtype=np.int32)
    chirp, filt, conv = [], [], []
    at = {"chirp": 0, "filter": 0, "conv": 0}
    by_length, by_m = {}, {}
    most = 1
    for j, nlon in enumerate(rings.tolist()):
        kind, n, m = ring_fft_plan(nlon)
        if kind is None:
            raise ValueError(f'ring_longitude="bluestein" does not take ring_nlon[{j}] = {nlon}')
        if kind == "mixed":
            plan[j, :3] = (1, n, 0)
            most = max(most, n)
            continue
        most = max(most, m)
        if nlon not in by_length:
            k = np.arange(n, dtype=np.int64)
            phase = np.pi * ((k * k) % (2 * n)).astype(np.float64) / n
            c = np.cos(phase) - 1j * np.sin(phase)
            h = np.zeros(m, dtype=np.complex128)
            h[:n] = np.conj(c)
            h[m - n + 1:] = np.conj(c[:0:-1])
            if m not in by_m:
                ang = 2.0 * np.pi * np.arange(m, dtype=np.float64) / m
                conv.append(np.stack([np.cos(ang), np.sin(ang)], axis=1))
                by_m[m] = at["conv"]
                at["conv"] += m
            by_length[nlon] = (at["chirp"], at["filter"], by_m[m])
            chirp.append(np.stack([c.real, c.imag], axis=1))
            big = np.fft.fft(h) / m
            filt.append(np.stack([big.real, big.imag], axis=1))
            at["chirp"] += n
            at["filter"] += m
        plan[j, :6] = (2, n, m) + by_length[nlon]
    pad = [np.zeros((1, 2))]
    return {"plan": plan, "chirp": np.concatenate(chirp or pad), "filter": np.concatenate(filt or pad),
            "conv_twiddle": np.concatenate(conv or pad), "max_points": most}


def quadrature(grid: str, nlat: int) -> Tuple[np.ndarray, np.ndarray]:
    """``(lat_deg [nlat], w [nlat])`` of a latitude set, south to north, fp64: the nodes symmetric about the equator to
    the last bit, the weights of ``int_{-1}^{1} f(sin lat) d(sin lat) / 2`` (they sum to 1)."""
    if grid not in GRIDS:
        raise ValueError(f"grid must be one of {GRIDS} (got {grid!r})")
    nlat = int(nlat)
    if nlat < (2 if grid == "equiangular" else 1):
        raise ValueError(f"nlat must be >= {2 if grid == 'equiangular' else 1} on the {grid} grid (got {nlat})")
    k = np.arange(nlat, dtype=np.float64)
    if grid == "gauss":
        x, w = np.polynomial.legendre.leggauss(nlat)
        x = 0.5 * (x - x[::-1])
        lat = np.rad2deg(np.arcsin(x))
    elif grid == "equiangular":
        n = nlat - 1
        lat = -90.0 + (180.0 / n) * k
        lat[-1] = 90.0
        lat = 0.5 * (lat - lat[::-1])
        theta = np.pi * k / n
        w = np.ones(nlat)
        for j in range(1, n // 2 + 1):
            w -= (1.0 if 2 * j == n else 2.0) / (4.0 * j * j - 1.0) * np.cos(2.0 * j * theta)
        w *= 2.0 / n
        w[0] *= 0.5
        w[-1] *= 0.5
    else:
        lat = -90.0 + (180.0 / nlat) * (k + 0.5)
        lat = 0.5 * (lat - lat[::-1])
        theta = np.pi * (k + 0.5) / nlat
        w = np.ones(nlat)
        for j in range(1, nlat // 2 + 1):
            w -= 2.0 / (4.0 * j * j - 1.0) * np.cos(2.0 * j * theta)
        w *= 2.0 / nlat
    w = 0.5 * (w + w[::-1])
    return lat, w / w.sum()


def max_degree(grid: str, nlat: int, nlon: int) -> int:
    """The largest ``lmax`` the quadrature of ``grid`` and ``nlon`` longitudes resolve exactly, at most 1023."""
    if grid not in GRIDS:
        raise ValueError(f"grid must be one of {GRIDS} (got {grid!r})")
    by_lat = nlat - 1 if grid == "gauss" else (nlat - 1) // 2
    return min(by_lat, (nlon - 1) // 2, MAX_LMAX)


def check_sizes(grid: str, nlat: int, nlon: int, lmax: Optional[int], longitude: str = "direct") -> int:
    """``lmax`` (the default filled in) after every size check; ValueError otherwise.  No device is touched."""
    if grid not in GRIDS:
        raise ValueError(f"grid must be one of {GRIDS} (got {grid!r})")
    if longitude not in LONGITUDE:
        raise ValueError(f"longitude must be one of {LONGITUDE} (got {longitude!r})")
    nlat, nlon = int(nlat), int(nlon)
    if longitude == "fft" and not fft_supported(nlon):
        raise ValueError(f'longitude="fft" needs 1 <= nlon <= {MAX_FFT_NLON} with no prime factor other than 2, 3 and 5 '
                         f"(got nlon = {nlon})")
    if nlat < (2 if grid == "equiangular" else 1) or nlon < 1:
        raise ValueError(f"nlat and nlon must be >= 1 (nlat >= 2 with poles); got {nlat}, {nlon}")
    if nlat > MAX_NLAT:
        raise ValueError(f"nlat <= {MAX_NLAT} (got {nlat})")
    if nlat * nlon > 2 ** 31 - 1:
        raise ValueError(f"nlat * nlon = {nlat * nlon} does not fit int32")
    limit = max_degree(grid, nlat, nlon)
    if lmax is None:
        return limit
    lmax = int(lmax)
    if lmax < 0:
        raise ValueError(f"lmax must be >= 0 (got {lmax})")
    if lmax > MAX_LMAX:
        raise ValueError(f"lmax <= {MAX_LMAX}: beyond it the recurrence needs rescaling (got {lmax})")
    if nlon < 2 * lmax + 1:
        raise ValueError(f"nlon >= 2 lmax + 1 = {2 * lmax + 1} (got {nlon})")
    if lmax > limit:
        raise ValueError(f"the {grid} quadrature on {nlat} latitudes is exact up to lmax = "
                         f"{nlat - 1 if grid == 'gauss' else (nlat - 1) // 2} (got {lmax})")
    return lmax


def octahedral_nlon(N: int) -> np.ndarray:
    """int64 ``[2 N]``: the ring lengths of the octahedral reduced Gaussian grid ``O<N>``, south to north -- ``4 i + 16``,
    ``i = 1 ... N``, from each pole to the equator (20 at the poles, ``4 N + 16`` either side of the equator)."""
    N = int(N)
    if N < 1:
        raise ValueError(f"N must be >= 1 (got {N})")
    half = 4 * np.arange(1, N + 1, dtype=np.int64) + 16
    return np.concatenate([half, half[::-1]])


def check_rings(ring_nlon, lmax: int, longitude: str = "direct", ring_longitude: str = "direct") -> np.ndarray:
    """The ring lengths of a reduced grid as an int64 array after every size check (module docstring, "limits");
    ValueError naming the offending value otherwise.  No device is touched."""
    if longitude not in LONGITUDE:
        raise ValueError(f"longitude must be one of {LONGITUDE} (got {longitude!r})")
    if longitude != "direct":
        raise ValueError(f'a reduced grid takes longitude="direct" only: the FFT needs ring lengths 2^a 3^b 5^c '
                         f'(got longitude = {longitude!r}); ring_longitude="bluestein" is the FFT of any ring length')
    if ring_longitude not in RING_LONGITUDE:
        raise ValueError(f"ring_longitude must be one of {RING_LONGITUDE} (got {ring_longitude!r})")
    rings = np.asarray(ring_nlon)
    if rings.ndim != 1 or rings.size < 1:
        raise ValueError(f"ring_nlon must be a list of at least one ring length (got shape {rings.shape})")
    if not np.issubdtype(rings.dtype, np.integer):
        raise ValueError(f"ring_nlon must hold integers (got dtype {rings.dtype})")
    if int(rings.min()) < 1:
        j = int(rings.argmin())
        raise ValueError(f"every ring needs at least one point (ring_nlon[{j}] = {int(rings[j])})")
    nlat, most = rings.size, int(rings.max())
    if nlat > MAX_NLAT:
        raise ValueError(f"nlat <= {MAX_NLAT} (got {nlat} rings)")
    if most > 2 ** 31 - 1:
        raise ValueError(f"max(ring_nlon) = {most} does not fit int32")
    rings = rings.astype(np.int64)
    if int(rings.sum()) > 2 ** 31 - 1:
        raise ValueError(f"sum(ring_nlon) = {int(rings.sum())} does not fit int32")
    if lmax is None:
        raise ValueError("a reduced grid needs lmax")
    lmax = int(lmax)
    if lmax < 0:
        raise ValueError(f"lmax must be >= 0 (got {lmax})")
    if lmax > MAX_LMAX:
        raise ValueError(f"lmax <= {MAX_LMAX}: beyond it the recurrence needs rescaling (got {lmax})")
    if lmax > nlat - 1:
        raise ValueError(f"the gauss quadrature on {nlat} latitudes is exact up to lmax = {nlat - 1} (got {lmax})")
    if most < 2 * lmax + 1:
        raise ValueError(f"max(ring_nlon) >= 2 lmax + 1 = {2 * lmax + 1} (got {most})")
    if ring_longitude == "bluestein":
        for j, n in enumerate(rings.tolist()):
            if ring_fft_plan(n)[0] is None:
                raise ValueError(f'ring_longitude="bluestein" needs a convolution length 2^a 3^b 5^c >= 2 n - 1 of at most '
                                 f"{MAX_RING_FFT_POINTS} (n = nlon / 2 for an even ring): ring_nlon[{j}] = {n} has none")
    return rings


def degree_index(lmax: int) -> np.ndarray:
    """int64 ``[(lmax + 1)^2]``: the degree ``l`` of every coefficient row."""
    return np.repeat(np.arange(lmax + 1, dtype=np.int64), 2 * np.arange(lmax + 1) + 1)


def sectoral_seeds(lmax: int) -> np.ndarray:
    """fp64 ``[lmax + 1]``: ``Pbar_m^m = seed[m] cos^m lat`` -- 1, sqrt(3), then ``seed[m-1] sqrt((2m+1)/(2m))``."""
    seed = np.ones(lmax + 1, dtype=np.float64)
    for m in range(1, lmax + 1):
        seed[m] = np.sqrt(3.0) if m == 1 else np.sqrt((2.0 * m + 1.0) / (2.0 * m)) * seed[m - 1]
    return seed


def check_rows(name: str, t, rows: int, what: str) -> None:
    """ValueError unless ``t`` is a tensor ``[..., rows, C]`` with ``1 <= C < 2^31``."""
    if not isinstance(t, Tensor):
        raise ValueError(f"{name} must be a tensor")
    if t.dim() < 2 or t.shape[-2] != rows:
        raise ValueError(f"{name} must be [..., {what} = {rows}, C], got {tuple(t.shape)}")
    if t.shape[-1] < 1:
        raise ValueError(f"{name} needs at least one channel")
    if t.shape[-1] > 2 ** 31 - 1:
        raise ValueError(f"C = {t.shape[-1]} does not fit int32")


def _check_out_dtype(dtype) -> None:
    if dtype not in (torch.float32, torch.float64):
        raise TypeError(f"gwen_amd: dtype must be float32 or float64 (got {dtype})")


class SphericalHarmonics:
    """The transforms of one grid and truncation (module docstring).  ``workspace_bytes`` bounds the fp64 intermediate
    ``[chunk, nlat, 2 lmax + 1, C]``: the leading axes of a call, flattened into one batch, are cut into chunks that fit
    (one item must: ValueError otherwise); the results do not depend on it.  A vector transform holds the intermediate
    of ``u`` and of ``v``, twice as much an item.  ``longitude`` chooses the longitude stage of every transform of the
    object, the adjoints behind autograd included: ``"direct"`` sums or ``"fft"`` (module docstring; ValueError where
    ``fft_supported(nlon)`` is false).

    ``SphericalHarmonics.reduced(ring_nlon, ...)`` and ``SphericalHarmonics.octahedral(N, ...)`` make the object of a
    reduced Gaussian grid (module docstring): ``grid == "reduced-gauss"``, ``nlon is None``, ``rows`` is the number of
    points and every method below works as it does on a regular grid.  ``ring_nlon`` and ``ring_start`` (numpy int64,
    ``[nlat]`` and ``[nlat + 1]``) are there on every object, constant ``nlon`` on a regular grid; ``ring_longitude`` is
    the longitude stage of a reduced grid (``RING_LONGITUDE``) and ``None`` on a regular one."""

    def __init__(self, nlat: int, nlon: int, device, lmax: Optional[int] = None, grid: str = "equiangular",
                 workspace_bytes: int = 1 << 30, longitude: str = "direct"):
        self.lmax = check_sizes(grid, nlat, nlon, lmax, longitude)
        self.nlat, self.nlon, self.grid, self.longitude = int(nlat), int(nlon), grid, longitude
        self.ring_longitude = None
        self._setup(np.full(self.nlat, self.nlon, dtype=np.int64), device, workspace_bytes)

    @classmethod
    def reduced(cls, ring_nlon, device, lmax: int, workspace_bytes: int = 1 << 30,
                longitude: str = "direct", ring_longitude: str = "direct") -> "SphericalHarmonics":
        """The transforms of the reduced Gaussian grid with ``ring_nlon[j]`` longitudes on Gauss latitude ``j``, south to
        north, truncated at ``lmax`` (module docstring, "Reduced Gaussian grids"; ``check_rings`` has the limits).
        ``ring_longitude`` chooses the longitude stage of every transform of the object: the ``"direct"`` sums or, with
        ``"bluestein"``, one FFT a ring (``ring_fft_plan``)."""
        rings = check_rings(ring_nlon, lmax, longitude, ring_longitude)
        self = cls.__new__(cls)
        self.lmax = int(lmax)
        self.nlat, self.nlon, self.grid, self.longitude = int(rings.size), None, "reduced-gauss", longitude
        self.ring_longitude = ring_longitude
        self._setup(rings, device, workspace_bytes)
        return self

    @classmethod
    def octahedral(cls, N: int, device, lmax: Optional[int] = None, workspace_bytes: int = 1 << 30,
                   longitude: str = "direct", ring_longitude: str = "direct") -> "SphericalHarmonics":
        """``reduced(octahedral_nlon(N), ...)``: the octahedral grid ``O<N>``.  ``lmax`` defaults to ``N - 1``, the cubic
        pairing, at which the round trip of a band-limited field is at round-off."""
        rings = octahedral_nlon(N)
        return cls.reduced(rings, device, int(N) - 1 if lmax is None else lmax, workspace_bytes, longitude,
                           ring_longitude)

    def _setup(self, rings: np.ndarray, device, workspace_bytes: int) -> None:
        """The tables of ``nlat`` rings of ``rings[j]`` longitudes; a regular grid keeps one ring's twiddle table, a
        reduced one holds every ring's end to end."""
        reduced = self.nlon is None
        self.workspace_bytes = int(workspace_bytes)
        if self.workspace_bytes < 1:
            raise ValueError(f"workspace_bytes must be positive (got {workspace_bytes})")
        from .gridgraph import _device
        self.device = _device(device)
        self.ring_nlon = rings
        self.ring_start = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(rings, dtype=np.int64)])
        self.rows = int(self.ring_start[-1])
        self.num_coefficients = (self.lmax + 1) ** 2
        lat, w = quadrature("gauss" if reduced else self.grid, self.nlat)
        self._lat_deg = lat
        phi = np.deg2rad(lat)
        nodes = np.stack([np.sin(phi), np.cos(phi)], axis=1)
        tables = []
        for n in (rings if reduced else rings[:1]):
            i = np.arange(int(n), dtype=np.float64)
            tables.append(np.stack([np.cos(2.0 * np.pi * i / int(n)), np.sin(2.0 * np.pi * i / int(n))], axis=1))
        tw = np.concatenate(tables, axis=0)
        seed = sectoral_seeds(self.lmax)
        dev = self.device
        self._nodes = torch.from_numpy(np.ascontiguousarray(nodes)).to(dev)
        self._twiddle = torch.from_numpy(np.ascontiguousarray(tw)).to(dev)
        self._seed = torch.from_numpy(np.ascontiguousarray(seed)).to(dev)
        self._lat_w = torch.from_numpy(np.ascontiguousarray(w / rings)).to(dev)
        self._weights = torch.from_numpy(np.repeat(w / rings, rings).astype(np.float32)).to(dev)
        if reduced:
            self._ring_nlon = torch.from_numpy(rings.astype(np.int32)).to(dev)
            self._ring_start = torch.from_numpy(self.ring_start).to(dev)
        if self.ring_longitude == "bluestein":
            tables = ring_fft_tables(rings)
            self._ring_fft_points = int(tables.pop("max_points"))
            self._ring_fft = {name: torch.from_numpy(np.ascontiguousarray(t)).to(dev) for name, t in tables.items()}
        self._degrees = torch.from_numpy(degree_index(self.lmax)).to(dev)
        big = (self._degrees * (self._degrees + 1)).to(torch.float64)
        self._lap = -big[:, None]                                # [T, 1]: the Laplacian's factor of every row
        l = torch.arange(self.lmax + 1, dtype=torch.float64, device=dev)
        self._ke_scale = torch.where(l > 0, 0.5 / (l * (l + 1.0)).clamp(min=1.0), torch.zeros_like(l))[:, None]

    # ---- tables -----------------------------------------------------------------------------------------------------
    @property
    def weights(self) -> Tensor:
        """fp32 ``[rows]``: the quadrature weight ``q`` of every grid point (sums to 1) -- the ``node_weights`` of
        ``gwen_amd.losses`` and ``gwen_amd.products``."""
        return self._weights

    @property
    def degrees(self) -> Tensor:
        """int64 ``[T]``: the degree ``l`` of every coefficient row (per-degree weights, filters)."""
        return self._degrees

    @property
    def positions(self) -> np.ndarray:
        """float64 ``[rows, 3]`` unit vectors, the form of ``latlon_grid(...)[0]`` (``grid_pos=``, a ``Regridder`` source
        or target)."""
        from .gridgraph import sphere_points
        if self.nlon is None:
            lat = np.repeat(self._lat_deg, self.ring_nlon)
            lon = np.concatenate([(360.0 / int(n)) * np.arange(int(n), dtype=np.float64) for n in self.ring_nlon])
            return sphere_points(lat, lon)
        lon = (360.0 / self.nlon) * np.arange(self.nlon, dtype=np.float64)
        return sphere_points(self._lat_deg[:, None], lon[None, :])

    def index(self, l: int, m: int) -> int:
        """The coefficient row of ``(l, m)``, ``-l <= m <= l <= lmax``: ``l^2 + l + m``."""
        l, m = int(l), int(m)
        if not 0 <= l <= self.lmax or abs(m) > l:
            raise ValueError(f"need 0 <= l <= {self.lmax} and |m| <= l (got l = {l}, m = {m})")
        return l * l + l + m

    # ---- launches ---------------------------------------------------------------------------------------------------
    def _rows_name(self) -> str:
        """What the row count of a field is called in an error message."""
        return "points" if self.nlon is None else "nlat * nlon"

    def _check(self, name: str, t, rows: int, what: str, dtypes) -> None:
        """Shapes (ValueError), then dtypes (TypeError), then devices (RuntimeError), as ``losses._check``."""
        check_rows(name, t, rows, what)
        if t.dtype not in dtypes:
            raise TypeError(f"gwen_amd: {name} must be {' or '.join(str(d).replace('torch.', '') for d in dtypes)} "
                            f"(got {t.dtype})")
        if not t.is_cuda:
            raise RuntimeError(f"gwen_amd: {name} must live on a HIP device (no CPU fallback)")
        if t.device != self.device:
            raise RuntimeError(f"gwen_amd: {name} is on {t.device}, the transform's tables on {self.device}")

    def _workspace(self, batch: int, c: int, vector: bool = False) -> Tensor:
        from . import _lib
        if self.nlon is None:
            item = int(_lib.lib().gwen_sht_rings_workspace_bytes(int(vector), self.nlat, self.rows,
                                                                 int(self.ring_nlon.max()), self.lmax, c))
        else:
            size = _lib.lib().gwen_sht_vector_workspace_bytes if vector else _lib.lib().gwen_sht_workspace_bytes
            item = int(size(_lib.SHT_GRIDS[self.grid], self.nlat, self.nlon, self.lmax, c))
        if item > self.workspace_bytes:
            raise ValueError(f"workspace_bytes = {self.workspace_bytes} is below one item's intermediate ({item} bytes)")
        items = min(max(batch, 1), self.workspace_bytes // item)
        return torch.empty(items * item // 8, dtype=torch.float64, device=self.device)

    def _launch(self, inverse: bool, src: Tensor, out_rows: int, dtype, weighted: bool) -> Tensor:
        """One transform of ``src [..., rows, C]`` (contiguous) into a new ``[..., out_rows, C]`` of ``dtype``."""
        from . import _lib
        lead, c = src.shape[:-2], src.shape[-1]
        batch = 1
        for s in lead:
            batch *= int(s)
        out = torch.empty(*lead, out_rows, c, dtype=dtype, device=self.device)
        if batch == 0:
            return out
        ws = self._workspace(batch, c)
        self._transform(_lib.SHT_OP_SYNTHESIS if inverse else _lib.SHT_OP_ANALYSIS, (src, None), (out, None), weighted,
                        False, batch, c, ws)
        return out

    def _transform(self, op: int, ins, outs, weighted: bool, adjoint: bool, batch: int, c: int, ws: Tensor) -> None:
        """``gwen_sht_transform`` (``gwen_sht_rings_transform`` on a reduced grid): one of the four transforms with this
        object's tables and longitude stage."""
        from . import _lib

        def ptr(t):                                              # a structure's pointer field takes an int or None
            return None if t is None else t.data_ptr()

        src = ins[0] if ins[0] is not None else ins[1]
        if self.nlon is None:
            rings = _lib.ShtRingsCall(
                op=op, adjoint=int(adjoint), in0=ptr(ins[0]), in1=ptr(ins[1]), in_f64=int(src.dtype == torch.float64),
                out0=ptr(outs[0]), out1=ptr(outs[1]), out_f64=int(outs[0].dtype == torch.float64),
                nodes=ptr(self._nodes), lat_w=ptr(self._lat_w) if weighted else None, twiddle=ptr(self._twiddle),
                seed=ptr(self._seed), ring_nlon=ptr(self._ring_nlon), ring_start=ptr(self._ring_start), batch=batch,
                nlat=self.nlat, points=self.rows, max_nlon=int(self.ring_nlon.max()), lmax=self.lmax, C=c,
                workspace=ptr(ws), workspace_bytes=ws.numel() * 8,
                stream=torch.cuda.current_stream(self.device).cuda_stream)
            if self.ring_longitude == "bluestein":
                t = self._ring_fft
                call = _lib.ShtRingsFftCall(rings=rings, ring_plan=ptr(t["plan"]), chirp=ptr(t["chirp"]),
                                            filter=ptr(t["filter"]), conv_twiddle=ptr(t["conv_twiddle"]),
                                            max_points=self._ring_fft_points)
                with torch.cuda.device(self.device):
                    rc = _lib.lib().gwen_sht_rings_fft_transform(call)
                _lib.check(rc, f"gwen_sht_rings_fft_transform(op={op})")
                return
            with torch.cuda.device(self.device):
                rc = _lib.lib().gwen_sht_rings_transform(rings)
            _lib.check(rc, f"gwen_sht_rings_transform(op={op})")
            return
        call = _lib.ShtCall(
            op=op, longitude=_lib.SHT_LONGITUDE[self.longitude], in0=ptr(ins[0]), in1=ptr(ins[1]),
            in_f64=int(src.dtype == torch.float64), out0=ptr(outs[0]), out1=ptr(outs[1]),
            out_f64=int(outs[0].dtype == torch.float64), nodes=ptr(self._nodes),
            lat_w=ptr(self._lat_w) if weighted else None, twiddle=ptr(self._twiddle), seed=ptr(self._seed),
            grid=_lib.SHT_GRIDS[self.grid], adjoint=int(adjoint), batch=batch, nlat=self.nlat, nlon=self.nlon,
            lmax=self.lmax, C=c, workspace=ptr(ws), workspace_bytes=ws.numel() * 8,
            stream=torch.cuda.current_stream(self.device).cuda_stream)
        with torch.cuda.device(self.device):
            rc = _lib.lib().gwen_sht_transform(call)
        _lib.check(rc, f"gwen_sht_transform(op={op}, longitude={self.longitude!r})")

    def analysis_launch(self, x: Tensor, dtype=torch.float32, weighted: bool = True) -> Tensor:
        """``gwen_sht_analysis`` on a contiguous device tensor, no autograd: with the quadrature weights the analysis,
        without them the adjoint of the synthesis."""
        return self._launch(False, x, self.num_coefficients, dtype, weighted)

    def synthesis_launch(self, c: Tensor, dtype=torch.float32, weighted: bool = False) -> Tensor:
        """``gwen_sht_synthesis`` on a contiguous device tensor, no autograd: without weights the synthesis, with the
        quadrature weights the adjoint of the analysis."""
        return self._launch(True, c, self.rows, dtype, weighted)

    # ---- public transforms ------------------------------------------------------------------------------------------
    def analysis(self, x: Tensor, dtype=torch.float32) -> Tensor:
        """``x [..., nlat * nlon, C]`` fp32 -> coefficients ``[..., T, C]`` in ``dtype`` (float32 or float64, rounded once
        from the fp64 sums).  Differentiable in ``x``."""
        self._check("x", x, self.rows, self._rows_name(), (torch.float32,))
        _check_out_dtype(dtype)
        return _Analysis.apply(x, self, dtype)

    def synthesis(self, c: Tensor, dtype=torch.float32) -> Tensor:
        """Coefficients ``c [..., T, C]`` fp32 or fp64 -> the field ``[..., nlat * nlon, C]`` in ``dtype``.
        Differentiable in ``c``."""
        self._check("c", c, self.num_coefficients, "T", (torch.float32, torch.float64))
        _check_out_dtype(dtype)
        return _Synthesis.apply(c, self, dtype)

    def power_spectrum(self, x: Optional[Tensor] = None, coeffs: Optional[Tensor] = None,
                       dtype=torch.float64) -> Tensor:
        """``[..., lmax + 1, C]``: the power ``S_l`` per degree of the field ``x`` (its coefficients stay fp64 on the
        way) or of given ``coeffs [..., T, C]``.  Not differentiable: the inputs are read detached."""
        from . import _lib
        from .graph import _ptr, _stream
        if (x is None) == (coeffs is None):
            raise ValueError("power_spectrum takes exactly one of x and coeffs")
        if x is not None:
            self._check("x", x, self.rows, self._rows_name(), (torch.float32,))
        else:
            self._check("coeffs", coeffs, self.num_coefficients, "T", (torch.float32, torch.float64))
        _check_out_dtype(dtype)
        if x is not None:
            c64 = self.analysis_launch(x.detach().contiguous(), torch.float64)
        else:
            c64 = coeffs.detach().to(torch.float64).contiguous()
        lead, c = c64.shape[:-2], c64.shape[-1]
        power = torch.empty(*lead, self.lmax + 1, c, dtype=torch.float64, device=self.device)
        batch = power.numel() // ((self.lmax + 1) * c)
        if batch:
            with torch.cuda.device(self.device):
                rc = _lib.lib().gwen_sht_power_f64(_ptr(c64), _ptr(power), batch, self.lmax, c, _stream(self.device))
            _lib.check(rc, "gwen_sht_power_f64")
        return power if dtype == torch.float64 else power.to(dtype)

    # ---- vector harmonics -------------------------------------------------------------------------------------------
    def _check_pair(self, names, pair, rows: int, what: str, dtypes, optional: bool = False) -> None:
        """``_check`` for two tensors of one shape and dtype: every shape, then every dtype, then every device.  With
        ``optional`` one of them (not both) may be None."""
        given = [(n, t) for n, t in zip(names, pair) if not (optional and t is None)]
        if not given:
            raise ValueError(f"at least one of {names[0]} and {names[1]} must be a tensor")
        for n, t in given:
            check_rows(n, t, rows, what)
        if len(given) == 2 and given[0][1].shape != given[1][1].shape:
            raise ValueError(f"{names[0]} and {names[1]} must have one shape, got {tuple(given[0][1].shape)} and "
                             f"{tuple(given[1][1].shape)}")
        for n, t in given:
            if t.dtype not in dtypes:
                raise TypeError(f"gwen_amd: {n} must be {' or '.join(str(d).replace('torch.', '') for d in dtypes)} "
                                f"(got {t.dtype})")
        if len(given) == 2 and given[0][1].dtype != given[1][1].dtype:
            raise TypeError(f"gwen_amd: {names[0]} and {names[1]} must have one dtype, got {given[0][1].dtype} and "
                            f"{given[1][1].dtype}")
        for n, t in given:
            if not t.is_cuda:
                raise RuntimeError(f"gwen_amd: {n} must live on a HIP device (no CPU fallback)")
            if t.device != self.device:
                raise RuntimeError(f"gwen_amd: {n} is on {t.device}, the transform's tables on {self.device}")

    def _vector_launch(self, inverse: bool, a0: Optional[Tensor], a1: Optional[Tensor], out_rows: int, dtype,
                       weighted: bool, adjoint: bool) -> Tuple[Tensor, Tensor]:
        """One vector transform of the contiguous pair ``a0, a1 [..., rows, C]`` (one of them may be None for the
        synthesis) into two new ``[..., out_rows, C]`` of ``dtype``."""
        from . import _lib
        src = a0 if a0 is not None else a1
        lead, c = src.shape[:-2], src.shape[-1]
        batch = 1
        for s in lead:
            batch *= int(s)
        b0 = torch.empty(*lead, out_rows, c, dtype=dtype, device=self.device)
        b1 = torch.empty_like(b0)
        if batch == 0:
            return b0, b1
        ws = self._workspace(batch, c, vector=True)
        self._transform(_lib.SHT_OP_VECTOR_SYNTHESIS if inverse else _lib.SHT_OP_VECTOR_ANALYSIS, (a0, a1), (b0, b1),
                        weighted, adjoint, batch, c, ws)
        return b0, b1

    def vector_analysis_launch(self, u: Tensor, v: Tensor, dtype=torch.float32, weighted: bool = True,
                               adjoint: bool = False) -> Tuple[Tensor, Tensor]:
        """``gwen_sht_vector_analysis`` on contiguous device tensors, no autograd: weighted and plain it is the vector
        analysis; with unit weights and ``adjoint`` (every row over ``L``) the adjoint of the vector synthesis."""
        return self._vector_launch(False, u, v, self.num_coefficients, dtype, weighted, adjoint)

    def vector_synthesis_launch(self, vort: Optional[Tensor], div: Optional[Tensor], dtype=torch.float32,
                                weighted: bool = False, adjoint: bool = False) -> Tuple[Tensor, Tensor]:
        """``gwen_sht_vector_synthesis`` on contiguous device tensors, no autograd: unweighted and plain it is the vector
        synthesis; with the quadrature weights and ``adjoint`` (no division by ``L``) the adjoint of the analysis."""
        return self._vector_launch(True, vort, div, self.rows, dtype, weighted, adjoint)

    def vector_analysis(self, u: Tensor, v: Tensor, dtype=torch.float32) -> Tuple[Tensor, Tensor]:
        """The eastward and northward components ``u, v [..., nlat * nlon, C]`` fp32 -> spectral vorticity and
        divergence ``[..., T, C]`` in ``dtype``; row 0 of both is 0.  Differentiable in ``u`` and ``v``."""
        self._check_pair(("u", "v"), (u, v), self.rows, self._rows_name(), (torch.float32,))
        _check_out_dtype(dtype)
        return _VectorAnalysis.apply(u, v, self, dtype)

    def vector_synthesis(self, vort: Optional[Tensor], div: Optional[Tensor],
                         dtype=torch.float32) -> Tuple[Tensor, Tensor]:
        """Spectral vorticity and divergence ``[..., T, C]`` fp32 or fp64 (one of them may be None: zero) -> the wind
        ``(u, v)``, ``[..., nlat * nlon, C]`` each in ``dtype``.  Row 0 is read as 0.  Differentiable in both."""
        self._check_pair(("vort", "div"), (vort, div), self.num_coefficients, "T", (torch.float32, torch.float64),
                         optional=True)
        _check_out_dtype(dtype)
        return _VectorSynthesis.apply(vort, div, self, dtype)

    def laplacian(self, coeffs: Tensor) -> Tensor:
        """The coefficients of the Laplacian of the scalar with ``coeffs [..., T, C]``: every row times ``-l (l + 1)``."""
        check_rows("coeffs", coeffs, self.num_coefficients, "T")
        return coeffs * self._lap.to(coeffs.dtype)

    def inverse_laplacian(self, coeffs: Tensor) -> Tensor:
        """Every row over ``-l (l + 1)``; row 0 (the mean, which no Laplacian has) becomes 0 whatever it holds."""
        check_rows("coeffs", coeffs, self.num_coefficients, "T")
        lap = self._lap.to(coeffs.dtype)
        return torch.where(lap != 0, coeffs / torch.where(lap != 0, lap, torch.ones_like(lap)), torch.zeros_like(coeffs))

    def gradient(self, coeffs: Tensor, dtype=torch.float32) -> Tuple[Tensor, Tensor]:
        """``(east, north)``, ``[..., nlat * nlon, C]`` each: the horizontal gradient of the scalar with coefficients
        ``coeffs [..., T, C]`` -- ``vector_synthesis(None, laplacian(coeffs))``.  Differentiable in ``coeffs``."""
        self._check("coeffs", coeffs, self.num_coefficients, "T", (torch.float32, torch.float64))
        _check_out_dtype(dtype)
        return self.vector_synthesis(None, self.laplacian(coeffs), dtype)

    def kinetic_energy_spectrum(self, u: Optional[Tensor] = None, v: Optional[Tensor] = None,
                                vort: Optional[Tensor] = None, div: Optional[Tensor] = None,
                                dtype=torch.float64) -> Tensor:
        """``[..., lmax + 1, C]``: ``E_l = sum_m (vort_lm^2 + div_lm^2) / (2 l (l + 1))``, ``E_0 = 0``, of the wind
        ``(u, v)`` (its coefficients stay fp64 on the way) or of given ``(vort, div) [..., T, C]``.  For a band-limited
        wind ``sum_l E_l = sum_p q_p (u^2 + v^2) / 2``.  Not differentiable: the inputs are read detached."""
        from . import _lib
        from .graph import _ptr, _stream
        given = tuple(t is not None for t in (u, v, vort, div))
        if given not in ((True, True, False, False), (False, False, True, True)):
            raise ValueError("kinetic_energy_spectrum takes exactly one of the pairs (u, v) and (vort, div)")
        wind = given[0]
        if wind:
            self._check_pair(("u", "v"), (u, v), self.rows, self._rows_name(), (torch.float32,))
        else:
            self._check_pair(("vort", "div"), (vort, div), self.num_coefficients, "T", (torch.float32, torch.float64))
        _check_out_dtype(dtype)
        if wind:
            pair = self.vector_analysis_launch(u.detach().contiguous(), v.detach().contiguous(), torch.float64)
        else:
            pair = (vort.detach().to(torch.float64).contiguous(), div.detach().to(torch.float64).contiguous())
        lead, c = pair[0].shape[:-2], pair[0].shape[-1]
        power = torch.empty(2, *lead, self.lmax + 1, c, dtype=torch.float64, device=self.device)
        batch = power[0].numel() // ((self.lmax + 1) * c)
        if batch:
            with torch.cuda.device(self.device):
                for k in range(2):
                    rc = _lib.lib().gwen_sht_power_f64(_ptr(pair[k]), _ptr(power[k]), batch, self.lmax, c,
                                                       _stream(self.device))
                    _lib.check(rc, "gwen_sht_power_f64")
        energy = (power[0] + power[1]) * self._ke_scale
        return energy if dtype == torch.float64 else energy.to(dtype)


class _VectorAnalysis(torch.autograd.Function):
    """(vort, div) = VA (u, v); VA^T (g_vort, g_div) = q * VS(L g_vort, L g_div): the synthesis kernels with the
    quadrature weights on the way out and no division by L on the way in."""

    @staticmethod
    def forward(ctx, u: Tensor, v: Tensor, sh: SphericalHarmonics, dtype):
        ctx.sh = sh
        return sh.vector_analysis_launch(u.detach().contiguous(), v.detach().contiguous(), dtype)

    @staticmethod
    def backward(ctx, g_vort, g_div):
        h_u, h_v = ctx.sh.vector_synthesis_launch(g_vort.contiguous(), g_div.contiguous(), torch.float32, weighted=True,
                                                  adjoint=True)
        return h_u, h_v, None, None


class _VectorSynthesis(torch.autograd.Function):
    """(u, v) = VS (vort, div); VS^T (h_u, h_v) = the analysis kernels with unit weights, every row over L."""

    @staticmethod
    def forward(ctx, vort: Optional[Tensor], div: Optional[Tensor], sh: SphericalHarmonics, dtype):
        ctx.sh, ctx.dtype = sh, (vort if vort is not None else div).dtype
        ctx.given = (vort is not None, div is not None)
        return sh.vector_synthesis_launch(None if vort is None else vort.detach().contiguous(),
                                          None if div is None else div.detach().contiguous(), dtype)

    @staticmethod
    def backward(ctx, h_u, h_v):
        g_vort, g_div = ctx.sh.vector_analysis_launch(h_u.contiguous(), h_v.contiguous(), ctx.dtype, weighted=False,
                                                      adjoint=True)
        return g_vort if ctx.given[0] else None, g_div if ctx.given[1] else None, None, None


class _Analysis(torch.autograd.Function):
    """c = A x; A^T g = q * synthesis(g): the synthesis kernels with the quadrature weights on the way out."""

    @staticmethod
    def forward(ctx, x: Tensor, sh: SphericalHarmonics, dtype) -> Tensor:
        ctx.sh = sh
        return sh.analysis_launch(x.detach().contiguous(), dtype)

    @staticmethod
    def backward(ctx, g):
        return ctx.sh.synthesis_launch(g.contiguous(), torch.float32, weighted=True), None, None


class _Synthesis(torch.autograd.Function):
    """x = S c; S^T h = the analysis kernels with unit weights."""

    @staticmethod
    def forward(ctx, c: Tensor, sh: SphericalHarmonics, dtype) -> Tensor:
        ctx.sh, ctx.dtype = sh, c.dtype
        return sh.synthesis_launch(c.detach().contiguous(), dtype)

    @staticmethod
    def backward(ctx, h):
        return ctx.sh.analysis_launch(h.contiguous(), ctx.dtype, weighted=False), None, None
