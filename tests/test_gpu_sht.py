"""gwen_amd.spectral on the device against the numpy fp64 restatement (tests/sht_ref.py) and closed-form harmonics.

Bounds.  An fp64 sum of n terms carries at most n 2^-53 times the sum of their magnitudes.  Analysis: the point weights sum
to 1 and |Y_lm| <= sqrt(2l + 1), so a coefficient's terms sum to at most sqrt(2l + 1) X with X = max |x|; at the largest
shape here (12 000 points, l <= 74) that is 1e-11 X, and the tests allow ten times it, 1e-10 X (an fp32 accumulation is
500 times over).  Synthesis: the terms of a point sum to at most S = sum_lm |c_lm| sqrt(2l + 1), hence 1e-10 S.  An fp32
result adds one rounding, 6e-8 |ref|.  The adjoints are the same sums with other weights: A^T g is a synthesis scaled by
the point weight q, S^T h an analysis whose weights are 1 where the quadrature's sum to 1, so its bound carries the
number of points.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sht_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (grid, nlat, nlon, lmax, C, batch)
SHAPES = [("gauss", 9, 18, 8, 3, 1), ("equiangular", 17, 32, 8, 5, 2), ("equiangular-centred", 12, 20, 5, 1, 1),
          ("gauss", 80, 150, 74, 5, 3), ("gauss", 80, 150, 20, 5, 3)]
IDS = [f"{g}-{a}x{b}-l{l}-c{c}-b{n}" for g, a, b, l, c, n in SHAPES]


@pytest.fixture(scope="module")
def ga(hip_lib):
    import gwen_amd
    return gwen_amd


class Case:
    """One shape: the transform, fp32 inputs on both sides and the restatement's answers, made once."""

    def __init__(self, ga, shape, seed):
        self.grid, self.nlat, self.nlon, self.lmax, self.c, self.batch = shape
        self.geom = (self.grid, self.nlat, self.nlon, self.lmax)
        self.sh = ga.SphericalHarmonics(self.nlat, self.nlon, DEV, lmax=self.lmax, grid=self.grid)
        rng = np.random.default_rng(seed)
        n, t = self.nlat * self.nlon, (self.lmax + 1) ** 2
        self.x = rng.standard_normal((self.batch, n, self.c)).astype(np.float32)
        self.coef = rng.standard_normal((self.batch, t, self.c)).astype(np.float32)
        self.ref_coef = R.analysis(self.x, *self.geom)                     # of the fp32 values
        self.ref_x = R.synthesis(self.coef, *self.geom)
        self.band = self.ref_x.astype(np.float32)                           # band-limited up to its rounding
        self.X = float(np.abs(self.x).max())
        amp = np.sqrt(2.0 * R.degrees(self.lmax) + 1.0)
        self.S = (np.abs(self.coef.astype(np.float64)) * amp[None, :, None]).sum(1, keepdims=True)   # [B, 1, C]
        self.q = R.point_weights(self.grid, self.nlat, self.nlon)


@pytest.fixture(scope="module")
def cases(ga):
    return {i: Case(ga, s, 100 + k) for k, (i, s) in enumerate(zip(IDS, SHAPES))}


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def same_bits(a, b):
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
    assert c64.shape == (k.batch, (k.lmax + 1) ** 2, k.c) == c32.shape
    e64, e32 = np.abs(host(c64) - k.ref_coef), np.abs(host(c32) - k.ref_coef)
    print(f"analysis {case_id}: fp64 err {e64.max() / k.X:.2e} X, fp32 err {e32.max():.2e}")
    assert (e64 <= 1e-10 * k.X).all()
    assert (e32 <= 6e-8 * np.abs(k.ref_coef) + 1e-10 * k.X).all()


# ---- 2. synthesis ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", IDS)
def test_synthesis_against_the_restatement(cases, case_id):
    k = cases[case_id]
    c = dev(k.coef)
    x64, x32 = k.sh.synthesis(c, dtype=torch.float64), k.sh.synthesis(c)
    assert x64.dtype == torch.float64 and x32.dtype == torch.float32
    assert x64.shape == (k.batch, k.nlat * k.nlon, k.c) == x32.shape
    e64, e32 = np.abs(host(x64) - k.ref_x), np.abs(host(x32) - k.ref_x)
    print(f"synthesis {case_id}: fp64 err {(e64 / k.S).max():.2e} S, fp32 err {e32.max():.2e}")
    assert (e64 <= 1e-10 * k.S).all()
    assert (e32 <= 6e-8 * np.abs(k.ref_x) + 1e-10 * k.S).all()
    # fp64 coefficients go in as they are
    assert same_bits(k.sh.synthesis(c.double(), dtype=torch.float64), x64)


# ---- 3. closed forms ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", IDS)
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
    assert [k.sh.index(1, 0), k.sh.index(1, 1), k.sh.index(1, -1), k.sh.index(2, 0), k.sh.index(2, 1),
            k.sh.index(2, -2)] == [2, 3, 1, 6, 7, 4]


# ---- 4. round trip and Parseval -------------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", IDS)
def test_round_trip_and_parseval(cases, case_id):
    k = cases[case_id]
    x = dev(k.band)
    back = k.sh.synthesis(k.sh.analysis(x))
    X = float(np.abs(k.band).max())
    err = float((back - x).abs().max())
    print(f"round trip {case_id}: {err / X:.2e} X")
    assert err <= 2e-7 * X
    total = host(k.sh.power_spectrum(x)).sum(1)
    want = (k.q[None, :, None] * k.band.astype(np.float64) ** 2).sum(1)
    assert np.allclose(total, want, rtol=1e-6, atol=0)
    # the tables fit the losses and the filters
    assert k.sh.weights.dtype == torch.float32 and k.sh.weights.shape == (k.nlat * k.nlon,)
    assert np.allclose(host(k.sh.weights), k.q, rtol=1e-7, atol=0)
    assert np.array_equal(k.sh.degrees.cpu().numpy(), R.degrees(k.lmax))
    lat, lon = R.latlon(k.grid, k.nlat, k.nlon)
    pos = k.sh.positions
    assert pos.dtype == np.float64 and pos.shape == (k.nlat * k.nlon, 3)
    assert np.allclose(pos, np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], 1), atol=1e-14)


# ---- 5. a steep spectrum --------------------------------------------------------------------------------------------

def test_steep_spectrum(cases):
    k = cases[IDS[3]]
    assert k.lmax == 74
    rng = np.random.default_rng(7)
    c = rng.standard_normal((1, 75 ** 2, 2)) * (10.0 ** (-R.degrees(74) / 15.0))[None, :, None]
    x32 = R.synthesis(c, *k.geom).astype(np.float32)
    want = R.power(R.analysis(x32, *k.geom), 74)
    got = host(k.sh.power_spectrum(dev(x32)))
    rel = np.abs(got - want) / want
    print(f"steep spectrum: worst relative error {rel.max():.2e} at l = {int(rel.max(2).argmax())}")
    assert (rel <= 1e-4).all()
    # given coefficients, and the fp32 form of the result
    c64 = k.sh.analysis(dev(x32), dtype=torch.float64)
    assert same_bits(k.sh.power_spectrum(coeffs=c64), k.sh.power_spectrum(dev(x32)))
    assert k.sh.power_spectrum(dev(x32), dtype=torch.float32).dtype == torch.float32


# ---- 6. backward ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", IDS)
def test_backward_against_the_restatement_adjoints(cases, case_id):
    k = cases[case_id]
    rng = np.random.default_rng(11)
    n, t = k.nlat * k.nlon, (k.lmax + 1) ** 2
    g = rng.standard_normal((k.batch, t, k.c))
    h = rng.standard_normal((k.batch, n, k.c))
    amp = np.sqrt(2.0 * R.degrees(k.lmax) + 1.0)
    # analysis: x.grad = q * synthesis(g), fp32
    x = dev(k.x).requires_grad_()
    k.sh.analysis(x, dtype=torch.float64).backward(dev(g))
    want = R.analysis_adjoint(g, *k.geom)
    S = (np.abs(g) * amp[None, :, None]).sum(1, keepdims=True) * k.q[None, :, None]       # [B, N, C]
    assert x.grad.dtype == torch.float32
    assert (np.abs(host(x.grad) - want) <= 6e-8 * np.abs(want) + 1e-10 * S).all()
    x32 = dev(k.x).requires_grad_()
    k.sh.analysis(x32).backward(dev(g, torch.float32))
    g32 = g.astype(np.float32).astype(np.float64)
    want32 = R.analysis_adjoint(g32, *k.geom)
    S32 = (np.abs(g32) * amp[None, :, None]).sum(1, keepdims=True) * k.q[None, :, None]
    assert (np.abs(host(x32.grad) - want32) <= 6e-8 * np.abs(want32) + 1e-10 * S32).all()
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


# ---- 7. spectral CRPS -----------------------------------------------------------------------------------------------

def test_spectral_crps_backward(ga, cases):
    k = cases[IDS[1]]
    rng = np.random.default_rng(13)
    n = k.nlat * k.nlon
    pred = dev(rng.standard_normal((4, n, k.c)).astype(np.float32)).requires_grad_()
    target = dev(rng.standard_normal((n, k.c)).astype(np.float32))
    loss = ga.ensemble_crps(k.sh.analysis(pred), k.sh.analysis(target))
    loss.backward()
    coef = k.sh.analysis(pred.detach()).requires_grad_()
    again = ga.ensemble_crps(coef, k.sh.analysis(target))
    again.backward()
    assert same_bits(loss.detach(), again.detach()) and float(loss.detach()) > 0
    assert same_bits(pred.grad, k.sh.synthesis_launch(coef.grad, torch.float32, weighted=True))
    want = R.analysis_adjoint(host(coef.grad), *k.geom)
    amp = np.sqrt(2.0 * R.degrees(k.lmax) + 1.0)
    S = (np.abs(host(coef.grad)) * amp[None, :, None]).sum(1, keepdims=True) * k.q[None, :, None]
    assert (np.abs(host(pred.grad) - want) <= 6e-8 * np.abs(want) + 1e-10 * S).all()
    assert float(pred.grad.abs().max()) > 0


# ---- 8. bitwise reproducibility -------------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", [IDS[1], IDS[3]])
def test_bitwise_reproducible(ga, cases, case_id):
    k = cases[case_id]
    rng = np.random.default_rng(14)
    n, t = k.nlat * k.nlon, (k.lmax + 1) ** 2
    x = dev(rng.standard_normal((3, n, k.c)).astype(np.float32))
    c = dev(rng.standard_normal((3, t, k.c)).astype(np.float32))
    item = 8 * k.nlat * (2 * k.lmax + 1) * k.c
    tight = ga.SphericalHarmonics(k.nlat, k.nlon, DEV, lmax=k.lmax, grid=k.grid, workspace_bytes=item)
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
    wide = torch.zeros(3, n, k.c + 2, device=DEV)
    wide[:, :, 1:k.c + 1] = x
    assert same_bits(k.sh.analysis(wide[:, :, 1:k.c + 1]), k.sh.analysis(x))
    with pytest.raises(ValueError):
        ga.SphericalHarmonics(k.nlat, k.nlon, DEV, lmax=k.lmax, grid=k.grid, workspace_bytes=item - 8).analysis(x)


# ---- 9. a NaN stays in its item and channel -------------------------------------------------------------------------

def test_nan_containment(cases):
    k = cases[IDS[3]]
    x, c = dev(k.x), dev(k.coef)
    clean_a, clean_s, clean_p = k.sh.analysis(x), k.sh.synthesis(c), k.sh.power_spectrum(x)
    x[1, 4321, 2] = float("nan")
    c[1, k.sh.index(30, -7), 2] = float("nan")
    a, s, p = k.sh.analysis(x), k.sh.synthesis(c), k.sh.power_spectrum(x)
    for got, clean in ((a, clean_a), (s, clean_s), (p, clean_p)):
        assert not bool(torch.isfinite(got[1, :, 2]).any())
        keep = torch.ones_like(got, dtype=torch.bool)
        keep[1, :, 2] = False
        assert bool(torch.isfinite(got[keep]).all()) and same_bits(got[keep], clean[keep])


# ---- 10. hipGraph capture -------------------------------------------------------------------------------------------

def test_power_spectrum_captures_into_a_graph(cases):
    k = cases[IDS[1]]
    rng = np.random.default_rng(15)
    first, second = dev(k.x), dev(rng.standard_normal(k.x.shape).astype(np.float32))
    buf = first.clone()
    k.sh.power_spectrum(buf)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = k.sh.power_spectrum(buf)
    buf.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out, k.sh.power_spectrum(second))
    assert not same_bits(out, k.sh.power_spectrum(first))


# ---- 11. past 4 GiB -------------------------------------------------------------------------------------------------

def test_input_past_4_gib(ga):
    free, _ = torch.cuda.mem_get_info()
    if free < 16 * 2 ** 30:
        pytest.skip(f"needs 16 GiB of free device memory, {free / 2 ** 30:.1f} GiB are free")
    nlat, nlon, lmax, c, batch = 32, 64, 31, 64, 8200
    sh = ga.SphericalHarmonics(nlat, nlon, DEV, lmax=lmax, grid="gauss")
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


# ---- the largest latitude count, and the order of the errors ---------------------------------------------------------

def test_most_latitudes(ga):
    grid, nlat, nlon, lmax = "equiangular", 2047, 3, 1
    sh = ga.SphericalHarmonics(nlat, nlon, DEV, lmax=lmax, grid=grid)
    rng = np.random.default_rng(18)
    x = rng.standard_normal((1, nlat * nlon, 2)).astype(np.float32)
    got = host(sh.analysis(dev(x), dtype=torch.float64))
    assert (np.abs(got - R.analysis(x, grid, nlat, nlon, lmax)) <= 1e-10 * np.abs(x).max()).all()


def test_errors_in_the_order_of_the_other_modules(cases):
    k = cases[IDS[0]]
    n = k.nlat * k.nlon
    with pytest.raises(ValueError):
        k.sh.analysis(torch.zeros(n + 1, 3, device=DEV))
    with pytest.raises(ValueError):
        k.sh.synthesis(torch.zeros(n, 3, device=DEV))
    with pytest.raises(ValueError):
        k.sh.analysis(torch.zeros(n + 1, 3, dtype=torch.float64))              # the shape comes first
    with pytest.raises(TypeError):
        k.sh.analysis(torch.zeros(n, 3, dtype=torch.float64))                  # then the dtype
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        k.sh.analysis(torch.zeros(n, 3))                                       # then the device
    with pytest.raises(TypeError):
        k.sh.analysis(torch.zeros(n, 3, device=DEV), dtype=torch.float16)
    with pytest.raises(ValueError):
        k.sh.power_spectrum()
    assert k.sh.analysis(torch.zeros(0, n, 3, device=DEV)).shape == (0, (k.lmax + 1) ** 2, 3)
