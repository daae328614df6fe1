"""gwen_amd.spectral with ``longitude="fft"`` on the device against the numpy fp64 restatements (tests/sht_ref.py,
tests/vsht_ref.py): the structure of tests/test_gpu_sht.py, every transform object built with the FFT longitude stage.
No reference value comes from the direct device path.

Bounds, those of tests/test_gpu_sht.py and tests/test_gpu_vsht.py.  An fp64 sum of n terms carries at most n 2^-53 times the
sum of their magnitudes.  Analysis: the point weights sum to 1 and |Y_lm| <= sqrt(2l + 1), so a coefficient's terms sum to at
most sqrt(2l + 1) X with X = max |x|; at 12 000 points and l <= 74 that is 1e-11 X, and the tests allow ten times it,
1e-10 X.  Synthesis: the terms of a point sum to at most S = sum_lm |c_lm| sqrt(2l + 1), hence 1e-10 S.  An fp32 result adds
one rounding, 6e-8 |ref|.  The adjoints are the same sums with other weights: A^T g is a synthesis scaled by the point
weight q, S^T h an analysis whose weights are 1 where the quadrature's sum to 1, so its bound carries the number of
points.  The FFT replaces the nlon-term sum of a ring by log2 nlon levels of butterflies: each level adds a relative
rounding of a few 2^-53 to values bounded by the ring's sum of magnitudes, about 2^-53 log2 nlon <= 1.4e-15 of it -- where
the direct sum's bound carries nlon 2^-53 -- so the FFT path is inside every bound above by the margin the direct path has
or more.  The vector bounds (1e-10 sqrt(L) W, 1e-10 S_v, ...) are derived in tests/test_gpu_vsht.py in the same way.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sht_ref as R  # noqa: E402
import vsht_ref as V  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (grid, nlat, nlon, lmax, C, batch): every radix alone and mixed, half-length (even nlon) and full-length (odd) FFTs, the
# last stored order 2 lmax + 1 = nlon, a ragged channel tile (C = 19), the workload's ring, the longest rings, and the
# degenerate lengths 1 ... 6
SHAPES = [("gauss", 9, 18, 8, 3, 1), ("equiangular", 17, 32, 8, 19, 2), ("equiangular-centred", 12, 20, 5, 1, 1),
          ("gauss", 80, 150, 74, 5, 3), ("gauss", 23, 45, 22, 3, 2), ("gauss", 64, 1440, 63, 2, 1),
          ("gauss", 32, 4096, 31, 1, 1), ("gauss", 32, 3645, 31, 1, 1)]
SHAPES += [("gauss", 4, n, (n - 1) // 2, 2, 1) for n in range(1, 7)]
IDS = [f"{g}-{a}x{b}-l{l}-c{c}-b{n}" for g, a, b, l, c, n in SHAPES]
ID18, ID32, ID20, ID150, ID45, ID1440 = IDS[:6]


@pytest.fixture(scope="module")
def ga(hip_lib):
    import gwen_amd
    return gwen_amd


class Case:
    """One shape: the FFT transform, fp32 inputs on both sides and the restatement's answers, made once."""

    def __init__(self, ga, shape, seed):
        self.grid, self.nlat, self.nlon, self.lmax, self.c, self.batch = shape
        self.geom = (self.grid, self.nlat, self.nlon, self.lmax)
        self.sh = ga.SphericalHarmonics(self.nlat, self.nlon, DEV, lmax=self.lmax, grid=self.grid, longitude="fft")
        assert self.sh.longitude == "fft"
        rng = np.random.default_rng(seed)
        self.n, self.t = self.nlat * self.nlon, (self.lmax + 1) ** 2
        self.x = rng.standard_normal((self.batch, self.n, self.c)).astype(np.float32)
        self.coef = rng.standard_normal((self.batch, self.t, self.c)).astype(np.float32)
        self.ref_coef = R.analysis(self.x, *self.geom)                     # of the fp32 values
        self.ref_x = R.synthesis(self.coef, *self.geom)
        self.band = self.ref_x.astype(np.float32)                           # band-limited up to its rounding
        self.X = float(np.abs(self.x).max())
        amp = np.sqrt(2.0 * R.degrees(self.lmax) + 1.0)
        self.S = (np.abs(self.coef.astype(np.float64)) * amp[None, :, None]).sum(1, keepdims=True)   # [B, 1, C]
        self.q = R.point_weights(self.grid, self.nlat, self.nlon)


_cases = {}


@pytest.fixture(scope="module")
def cases(ga):
    class Lazy:
        def __getitem__(self, case_id):
            if case_id not in _cases:
                _cases[case_id] = Case(ga, SHAPES[IDS.index(case_id)], 300 + IDS.index(case_id))
            return _cases[case_id]
    return Lazy()


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def same_bits(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    view = torch.int32 if a.dtype == torch.float32 else torch.int64
    return bool(torch.equal(a.contiguous().reshape(-1).view(view), b.contiguous().reshape(-1).view(view)))


# ---- 1. analysis ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", IDS)
def test_analysis_against_the_restatement(cases, case_id):
    k = cases[case_id]
    x = dev(k.x)
    c64, c32 = k.sh.analysis(x, dtype=torch.float64), k.sh.analysis(x)
    assert c64.dtype == torch.float64 and c32.dtype == torch.float32
    assert c64.shape == (k.batch, k.t, k.c) == c32.shape
    e64, e32 = np.abs(host(c64) - k.ref_coef), np.abs(host(c32) - k.ref_coef)
    print(f"fft analysis {case_id}: fp64 err {e64.max() / k.X:.2e} X, fp32 err {e32.max():.2e}")
    assert (e64 <= 1e-10 * k.X).all()
    assert (e32 <= 6e-8 * np.abs(k.ref_coef) + 1e-10 * k.X).all()


# ---- 2. synthesis ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", IDS)
def test_synthesis_against_the_restatement(cases, case_id):
    k = cases[case_id]
    c = dev(k.coef)
    x64, x32 = k.sh.synthesis(c, dtype=torch.float64), k.sh.synthesis(c)
    assert x64.dtype == torch.float64 and x32.dtype == torch.float32
    assert x64.shape == (k.batch, k.n, k.c) == x32.shape
    e64, e32 = np.abs(host(x64) - k.ref_x), np.abs(host(x32) - k.ref_x)
    print(f"fft synthesis {case_id}: fp64 err {(e64 / k.S).max():.2e} S, fp32 err {e32.max():.2e}")
    assert (e64 <= 1e-10 * k.S).all()
    assert (e32 <= 6e-8 * np.abs(k.ref_x) + 1e-10 * k.S).all()
    # fp64 coefficients go in as they are
    assert same_bits(k.sh.synthesis(c.double(), dtype=torch.float64), x64)


# ---- 3. closed forms ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", [i for i, s in zip(IDS, SHAPES) if s[3] >= 2])
def test_closed_form_harmonics_land_on_their_rows(cases, case_id):
    k = cases[case_id]
    lat, lon = R.latlon(k.grid, k.nlat, k.nlon)
    s, c = np.sin(lat), np.cos(lat)
    fields = {2: np.sqrt(3.0) * s, 3: np.sqrt(3.0) * c * np.cos(lon), 1: np.sqrt(3.0) * c * np.sin(lon),
              6: np.sqrt(5.0) * (3.0 * s * s - 1.0) / 2.0, 7: np.sqrt(15.0) * s * c * np.cos(lon),
              4: (np.sqrt(15.0) / 2.0) * c * c * np.sin(2.0 * lon)}
    rows = sorted(fields)
    x = dev(np.stack([fields[r] for r in rows], axis=1).astype(np.float32))          # [N, 6]
    got = host(k.sh.analysis(x, dtype=torch.float64))                                 # [T, 6]
    want = np.zeros_like(got)
    for ch, r in enumerate(rows):
        want[r, ch] = 1.0
    assert np.abs(got - want).max() <= 1e-6


# ---- 4. round trip and Parseval -------------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", IDS)
def test_round_trip_and_parseval(cases, case_id):
    k = cases[case_id]
    x = dev(k.band)
    back = k.sh.synthesis(k.sh.analysis(x))
    X = float(np.abs(k.band).max())
    err = float((back - x).abs().max())
    print(f"fft round trip {case_id}: {err / X:.2e} X")
    assert err <= 2e-7 * X
    total = host(k.sh.power_spectrum(x)).sum(1)
    want = (k.q[None, :, None] * k.band.astype(np.float64) ** 2).sum(1)
    assert np.allclose(total, want, rtol=1e-6, atol=0)


# ---- 5. backward ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", IDS)
def test_backward_against_the_restatement_adjoints(cases, case_id):
    k = cases[case_id]
    rng = np.random.default_rng(11)
    n = k.n
    g = rng.standard_normal((k.batch, k.t, k.c))
    h = rng.standard_normal((k.batch, n, k.c))
    amp = np.sqrt(2.0 * R.degrees(k.lmax) + 1.0)
    # analysis: x.grad = q * synthesis(g), fp32
    x = dev(k.x).requires_grad_()
    k.sh.analysis(x, dtype=torch.float64).backward(dev(g))
    want = R.analysis_adjoint(g, *k.geom)
    S = (np.abs(g) * amp[None, :, None]).sum(1, keepdims=True) * k.q[None, :, None]       # [B, N, C]
    assert x.grad.dtype == torch.float32
    assert (np.abs(host(x.grad) - want) <= 6e-8 * np.abs(want) + 1e-10 * S).all()
    # synthesis: c.grad = analysis of h with unit weights, in c's dtype
    H = float(np.abs(h).max())
    want = R.synthesis_adjoint(h, *k.geom)
    c64 = dev(k.coef, torch.float64).requires_grad_()
    k.sh.synthesis(c64, dtype=torch.float64).backward(dev(h))
    assert c64.grad.dtype == torch.float64
    assert (np.abs(host(c64.grad) - want) <= 1e-10 * n * H).all()
    c32 = dev(k.coef).requires_grad_()
    k.sh.synthesis(c32, dtype=torch.float64).backward(dev(h))
    assert c32.grad.dtype == torch.float32
    assert (np.abs(host(c32.grad) - want) <= 6e-8 * np.abs(want) + 1e-10 * n * H).all()


@pytest.mark.parametrize("case_id", IDS)
def test_adjoint_identity_on_fp64_outputs(cases, case_id):
    """<A x, g> = <x, A^T g> and <S c, h> = <c, S^T h>: the two FFT kernels are each other's adjoints up to rounding."""
    k = cases[case_id]
    rng = np.random.default_rng(12)
    x, c = dev(k.x), dev(k.coef, torch.float64)
    g = dev(rng.standard_normal(k.coef.shape))
    h = dev(rng.standard_normal(k.x.shape))
    ax = k.sh.analysis_launch(x, torch.float64)
    atg = k.sh.synthesis_launch(g, torch.float64, weighted=True)
    lhs, rhs = float((ax * g).sum()), float((x.double() * atg).sum())
    assert abs(lhs - rhs) <= 1e-12 * float((ax * g).abs().sum())
    sc = k.sh.synthesis_launch(c, torch.float64)
    sth = k.sh.analysis_launch(h, torch.float64, weighted=False)
    lhs, rhs = float((sc * h).sum()), float((c * sth).sum())
    assert abs(lhs - rhs) <= 1e-12 * float((sc * h).abs().sum())


# ---- 6. vector transforms -------------------------------------------------------------------------------------------

def big_l(lmax):
    l = R.degrees(lmax).astype(np.float64)
    return l * (l + 1.0)


def synthesis_scale(vort, div, lmax):
    """S_v [B, 1, C] of tests/test_gpu_vsht.py."""
    l = R.degrees(lmax).astype(np.float64)
    amp = np.zeros_like(l)
    amp[1:] = np.sqrt((2.0 * l[1:] + 1.0) / (l[1:] * (l[1:] + 1.0)))
    return ((np.abs(vort) + np.abs(div)) * amp[None, :, None]).sum(1, keepdims=True)


@pytest.mark.parametrize("case_id", [ID18, ID32, ID45, ID150])
def test_vector_transforms_against_the_restatement(cases, case_id):
    k = cases[case_id]
    rng = np.random.default_rng(200 + IDS.index(case_id))
    u, v = rng.standard_normal((2, k.batch, k.n, k.c)).astype(np.float32)
    vort, div = rng.standard_normal((2, k.batch, k.t, k.c)).astype(np.float32)
    rootL = np.sqrt(big_l(k.lmax))[None, :, None]
    W = float(np.hypot(u.astype(np.float64), v.astype(np.float64)).max())
    # analysis
    ud, vd = dev(u), dev(v)
    got64, got32 = k.sh.vector_analysis(ud, vd, dtype=torch.float64), k.sh.vector_analysis(ud, vd)
    for g64, g32, ref in zip(got64, got32, V.vector_analysis(u, v, *k.geom)):
        assert g64.dtype == torch.float64 and g32.dtype == torch.float32 and g64.shape == (k.batch, k.t, k.c)
        assert (np.abs(host(g64) - ref) <= 1e-10 * rootL * W).all()
        assert (np.abs(host(g32) - ref) <= 6e-8 * np.abs(ref) + 1e-10 * rootL * W).all()
        assert bool((g64[:, 0] == 0).all()) and bool((g32[:, 0] == 0).all())
    # kinetic energy spectrum: the restatement's spectrum of the device's own coefficients, and Parseval
    energy = k.sh.kinetic_energy_spectrum(u=ud, v=vd)
    assert energy.dtype == torch.float64 and energy.shape == (k.batch, k.lmax + 1, k.c)
    assert same_bits(k.sh.kinetic_energy_spectrum(vort=got64[0], div=got64[1]), energy)
    assert np.allclose(host(energy), V.kinetic_energy(host(got64[0]), host(got64[1]), k.lmax), rtol=1e-13, atol=0)
    # synthesis, one argument None included
    vo, di = dev(vort), dev(div)
    S = synthesis_scale(vort.astype(np.float64), div.astype(np.float64), k.lmax)
    got64, got32 = k.sh.vector_synthesis(vo, di, dtype=torch.float64), k.sh.vector_synthesis(vo, di)
    for g64, g32, ref in zip(got64, got32, V.vector_synthesis(vort, div, *k.geom)):
        assert g64.dtype == torch.float64 and g32.dtype == torch.float32 and g64.shape == (k.batch, k.n, k.c)
        assert (np.abs(host(g64) - ref) <= 1e-10 * S).all()
        assert (np.abs(host(g32) - ref) <= 6e-8 * np.abs(ref) + 1e-10 * S).all()
    band = tuple(t.float() for t in got64)                                      # band-limited up to its rounding
    want = (k.q[None, :, None] * (host(band[0]) ** 2 + host(band[1]) ** 2) / 2.0).sum(1)
    assert np.allclose(host(k.sh.kinetic_energy_spectrum(u=band[0], v=band[1])).sum(1), want, rtol=1e-6, atol=0)
    zero = torch.zeros_like(vo)
    assert same_bits(k.sh.vector_synthesis(vo, None), k.sh.vector_synthesis(vo, zero))
    assert same_bits(k.sh.vector_synthesis(None, di), k.sh.vector_synthesis(zero, di))
    only_div = k.sh.vector_synthesis(None, di, dtype=torch.float64)
    S_div = synthesis_scale(np.zeros_like(div, dtype=np.float64), div.astype(np.float64), k.lmax)
    for got, ref in zip(only_div, V.vector_synthesis(None, div, *k.geom)):
        assert (np.abs(host(got) - ref) <= 1e-10 * S_div).all()
    # gradient
    east, north = k.sh.gradient(vo, dtype=torch.float64)
    lap32 = (-big_l(k.lmax)[None, :, None].astype(np.float32) * vort).astype(np.float64)      # what the device rounds
    want_e, want_n = V.vector_synthesis(None, lap32, *k.geom)
    S_lap = synthesis_scale(np.zeros_like(lap32), lap32, k.lmax)
    assert (np.abs(host(east) - want_e) <= 1e-10 * S_lap).all() and (np.abs(host(north) - want_n) <= 1e-10 * S_lap).all()
    # one backward: (u.grad, v.grad) = q * VS(L g), fp32
    g_vort, g_div = rng.standard_normal((2, k.batch, k.t, k.c))
    ul, vl = dev(u).requires_grad_(), dev(v).requires_grad_()
    torch.autograd.backward(list(k.sh.vector_analysis(ul, vl, dtype=torch.float64)), [dev(g_vort), dev(g_div)])
    want_u, want_v = V.vector_analysis_adjoint(g_vort, g_div, *k.geom)
    l = R.degrees(k.lmax).astype(np.float64)
    amp = np.sqrt(l * (l + 1.0) * (2.0 * l + 1.0))
    S_adj = ((np.abs(g_vort) + np.abs(g_div)) * amp[None, :, None]).sum(1, keepdims=True) * k.q[None, :, None]
    assert ul.grad.dtype == torch.float32 == vl.grad.dtype
    assert (np.abs(host(ul.grad) - want_u) <= 6e-8 * np.abs(want_u) + 1e-10 * S_adj).all()
    assert (np.abs(host(vl.grad) - want_v) <= 6e-8 * np.abs(want_v) + 1e-10 * S_adj).all()


# ---- 7. bitwise reproducibility -------------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", [ID32, ID150, ID1440])
def test_bitwise_reproducible(ga, cases, case_id):
    k = cases[case_id]
    rng = np.random.default_rng(14)
    n, t = k.n, k.t
    x = dev(rng.standard_normal((3, n, k.c)).astype(np.float32))
    c = dev(rng.standard_normal((3, t, k.c)).astype(np.float32))
    item = 8 * k.nlat * (2 * k.lmax + 1) * k.c
    tight = ga.SphericalHarmonics(k.nlat, k.nlon, DEV, lmax=k.lmax, grid=k.grid, workspace_bytes=item, longitude="fft")
    for dtype in (torch.float32, torch.float64):
        a, s, p = k.sh.analysis(x, dtype=dtype), k.sh.synthesis(c, dtype=dtype), k.sh.power_spectrum(x, dtype=dtype)
        assert same_bits(a, k.sh.analysis(x, dtype=dtype)) and same_bits(s, k.sh.synthesis(c, dtype=dtype))
        assert same_bits(p, k.sh.power_spectrum(x, dtype=dtype))
        for i in range(3):
            assert same_bits(a[i], k.sh.analysis(x[i], dtype=dtype))
            assert same_bits(s[i], k.sh.synthesis(c[i], dtype=dtype))
            assert same_bits(p[i], k.sh.power_spectrum(x[i], dtype=dtype))
        assert same_bits(a, tight.analysis(x, dtype=dtype)) and same_bits(s, tight.synthesis(c, dtype=dtype))
        assert same_bits(p, tight.power_spectrum(x, dtype=dtype))
    # leading axes are one batch, and a strided input is made contiguous
    assert same_bits(k.sh.analysis(x.reshape(3, 1, n, k.c))[:, 0], k.sh.analysis(x))
    assert same_bits(k.sh.synthesis(c.reshape(1, 3, t, k.c))[0], k.sh.synthesis(c))
    wide = torch.zeros(3, n, k.c + 2, device=DEV)
    wide[:, :, 1:k.c + 1] = x
    assert same_bits(k.sh.analysis(wide[:, :, 1:k.c + 1]), k.sh.analysis(x))
    with pytest.raises(ValueError):
        ga.SphericalHarmonics(k.nlat, k.nlon, DEV, lmax=k.lmax, grid=k.grid, workspace_bytes=item - 8,
                              longitude="fft").analysis(x)


# ---- 8. a NaN stays in its item and channel -------------------------------------------------------------------------

# channel 2 of 5 sits in the middle of the one (ragged) tile of the 150-longitude shape; of the 19 channels of the
# 32-longitude shape, 7 is in the middle of the first tile and 17 in the ragged last one
@pytest.mark.parametrize("case_id,point,row,channel", [(ID150, 4321, (30, -7), 2), (ID32, 321, (5, -3), 7),
                                                       (ID32, 321, (5, -3), 17)])
def test_nan_containment(cases, case_id, point, row, channel):
    k = cases[case_id]
    x, c = dev(k.x), dev(k.coef)
    clean_a, clean_s, clean_p = k.sh.analysis(x), k.sh.synthesis(c), k.sh.power_spectrum(x)
    x[1, point, channel] = float("nan")
    c[1, k.sh.index(*row), channel] = float("nan")
    a, s, p = k.sh.analysis(x), k.sh.synthesis(c), k.sh.power_spectrum(x)
    for got, clean in ((a, clean_a), (s, clean_s), (p, clean_p)):
        assert not bool(torch.isfinite(got[1, :, channel]).any())
        keep = torch.ones_like(got, dtype=torch.bool)
        keep[1, :, channel] = False
        assert bool(torch.isfinite(got[keep]).all()) and same_bits(got[keep], clean[keep])


# ---- 9. hipGraph capture --------------------------------------------------------------------------------------------

def test_captures_into_a_graph(cases):
    k = cases[ID32]
    rng = np.random.default_rng(15)
    first, second = dev(k.x), dev(rng.standard_normal(k.x.shape).astype(np.float32))
    buf = first.clone()
    k.sh.power_spectrum(buf)
    k.sh.synthesis(k.sh.analysis(buf))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        power = k.sh.power_spectrum(buf)
        back = k.sh.synthesis(k.sh.analysis(buf))
    buf.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(power, k.sh.power_spectrum(second)) and same_bits(back, k.sh.synthesis(k.sh.analysis(second)))
    assert not same_bits(power, k.sh.power_spectrum(first))


# ---- 10. the spectral convolution takes the transform as it is --------------------------------------------------------

def test_spectral_conv_on_the_fft_transform(ga, cases):
    k = cases[ID32]
    torch.manual_seed(16)
    conv = ga.SpectralConv(k.sh, 16, 16).to(DEV)
    x = torch.randn(2, k.n, 16, device=DEV, requires_grad=True)
    out = conv(x)
    want = k.sh.synthesis(ga.spectral_conv(k.sh.analysis(x), conv.weight, k.lmax, conv.precision))
    assert same_bits(out.detach(), want.detach())
    out.square().sum().backward()
    for grad in (x.grad, conv.weight.grad):
        assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
    # the block and the model take the same object
    block = ga.SFNOBlock(k.sh, 16).to(DEV)
    assert bool(torch.isfinite(block(x.detach())).all())


# ---- 11. past 4 GiB -------------------------------------------------------------------------------------------------

def test_input_past_4_gib(ga):
    free, _ = torch.cuda.mem_get_info()
    if free < 16 * 2 ** 30:
        pytest.skip(f"needs 16 GiB of free device memory, {free / 2 ** 30:.1f} GiB are free")
    nlat, nlon, lmax, c, batch = 32, 64, 31, 64, 8200
    sh = ga.SphericalHarmonics(nlat, nlon, DEV, lmax=lmax, grid="gauss", longitude="fft")
    x = torch.empty(batch, nlat * nlon, c, device=DEV)
    assert x.numel() * 4 > 2 ** 32
    block = torch.randn(100, nlat * nlon, c, device=DEV, generator=torch.Generator(device=DEV).manual_seed(16))
    for b0 in range(0, batch, 100):
        x[b0:b0 + 100] = block
    x[-1] = torch.randn(nlat * nlon, c, device=DEV, generator=torch.Generator(device=DEV).manual_seed(17))
    assert 8 * nlat * (2 * lmax + 1) * c * batch > sh.workspace_bytes          # more than one chunk
    coef = sh.analysis(x)
    alone = sh.analysis(x[-1])
    assert bool(torch.isfinite(alone).all()) and float(alone.abs().max()) > 0
    assert same_bits(coef[-1], alone)
    assert same_bits(coef[4100], sh.analysis(x[4100]))
    del coef, x
    torch.cuda.empty_cache()


# ---- 12. the direct path is the default, untouched ------------------------------------------------------------------

@pytest.mark.parametrize("case_id", [ID32, ID150])
def test_direct_is_the_default_and_agrees_to_rounding(ga, cases, case_id):
    k = cases[case_id]
    default = ga.SphericalHarmonics(k.nlat, k.nlon, DEV, lmax=k.lmax, grid=k.grid)
    direct = ga.SphericalHarmonics(k.nlat, k.nlon, DEV, lmax=k.lmax, grid=k.grid, longitude="direct")
    assert default.longitude == "direct" == direct.longitude
    x, c = dev(k.x), dev(k.coef)
    for dtype in (torch.float32, torch.float64):
        assert same_bits(default.analysis(x, dtype=dtype), direct.analysis(x, dtype=dtype))
        assert same_bits(default.synthesis(c, dtype=dtype), direct.synthesis(c, dtype=dtype))
    diff = (direct.analysis(x, dtype=torch.float64) - k.sh.analysis(x, dtype=torch.float64)).abs().max()
    print(f"direct against fft {case_id}: {float(diff) / k.X:.2e} X")
    assert float(diff) <= 2e-10 * k.X


def test_unsupported_length_is_refused_on_the_device(ga):
    with pytest.raises(ValueError, match="2, 3 and 5"):
        ga.SphericalHarmonics(9, 28, DEV, grid="gauss", longitude="fft")
    assert ga.SphericalHarmonics(9, 28, DEV, grid="gauss").longitude == "direct"
