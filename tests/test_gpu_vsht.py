"""The vector transforms of gwen_amd.spectral on the device against the numpy fp64 restatement (tests/vsht_ref.py) and
closed-form winds.

Bounds, derived as in tests/test_gpu_sht.py.  An fp64 sum of n terms carries at most n 2^-53 times the sum of their
magnitudes.  The addition theorem gives sum_m |grad Y_lm|^2 = l (l + 1)(2l + 1) at every point (tests/test_vsht_host.py
checks it at the poles), so |grad Y_lm| = |k x grad Y_lm| <= sqrt(L (2l + 1)) with L = l (l + 1), where the scalar file has
|Y_lm| <= sqrt(2l + 1).
  Analysis: the point weights sum to 1, so the terms of vort_lm or div_lm sum to at most sqrt(L (2l + 1)) W with
W = max sqrt(u^2 + v^2).  The scalar file turns sqrt(2l + 1) X at its largest shape (12 000 points, l <= 74) into 1e-11 X
and allows ten times it; the same shape and factor here give 1e-10 sqrt(L) W.  Row 0 is exactly 0.
  Synthesis: psi = -vort / L, so the terms of a point sum to at most S_v = sum_lm (|vort_lm| + |div_lm|) sqrt((2l + 1) / L),
hence 1e-10 S_v.  An fp32 result adds one rounding, 6e-8 |ref|.
  Adjoints: VA^T g = q * VS(L g) is a synthesis of L g scaled by the point weight, bound 1e-10 q sum (|g_vort| + |g_div|)
sqrt(L (2l + 1)); VS^T h = VA_1(h) / L is an analysis whose weights are 1 where the quadrature's sum to 1, over L, bound
1e-10 n H / sqrt(L) with n points and H = max sqrt(h_u^2 + h_v^2).
  Round trip in fp64: the analysis error, plus the analysis of the synthesis error (at most 1e-10 S_v at every point,
against |grad Y_lm| <= sqrt(L (2l + 1))): 1e-10 sqrt(L) (W + sqrt(2l + 1) S_v).
On the CPU the restatement re-applied to its own output stays four orders of magnitude inside these bounds.
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

# (grid, nlat, nlon, lmax, C, batch): the five of tests/test_gpu_sht.py (80 x 150, lmax 74 crosses two latitude tiles and
# three degree tiles, and at m = 10 its last tile holds one degree, so Q_{l-1} crosses a tile edge; the equiangular shapes
# have pole rows and an equator row), two channel tiles, and the smallest grid with poles
SHAPES = [("gauss", 9, 18, 8, 3, 1), ("equiangular", 17, 32, 8, 5, 2), ("equiangular-centred", 12, 20, 5, 1, 1),
          ("gauss", 80, 150, 74, 5, 3), ("gauss", 80, 150, 20, 5, 3), ("gauss", 9, 18, 8, 17, 1),
          ("equiangular", 3, 3, 1, 2, 1)]
IDS = [f"{g}-{a}x{b}-l{l}-c{c}-b{n}" for g, a, b, l, c, n in SHAPES]


@pytest.fixture(scope="module")
def ga(hip_lib):
    import gwen_amd
    return gwen_amd


def big_l(lmax):
    l = R.degrees(lmax).astype(np.float64)
    return l * (l + 1.0)


def synthesis_scale(vort, div, lmax):
    """S_v [B, 1, C]."""
    l = R.degrees(lmax).astype(np.float64)
    amp = np.zeros_like(l)
    amp[1:] = np.sqrt((2.0 * l[1:] + 1.0) / (l[1:] * (l[1:] + 1.0)))
    return ((np.abs(vort) + np.abs(div)) * amp[None, :, None]).sum(1, keepdims=True)


def adjoint_scale(g_vort, g_div, lmax):
    """sum_lm (|g_vort| + |g_div|) sqrt(L (2l + 1)), [B, 1, C]."""
    l = R.degrees(lmax).astype(np.float64)
    amp = np.sqrt(l * (l + 1.0) * (2.0 * l + 1.0))
    return ((np.abs(g_vort) + np.abs(g_div)) * amp[None, :, None]).sum(1, keepdims=True)


class Case:
    """One shape: the transform, fp32 inputs on both sides and the restatement's answers, made once."""

    def __init__(self, ga, shape, seed):
        self.grid, self.nlat, self.nlon, self.lmax, self.c, self.batch = shape
        self.geom = (self.grid, self.nlat, self.nlon, self.lmax)
        self.sh = ga.SphericalHarmonics(self.nlat, self.nlon, DEV, lmax=self.lmax, grid=self.grid)
        rng = np.random.default_rng(seed)
        self.n, self.t = self.nlat * self.nlon, (self.lmax + 1) ** 2
        self.u, self.v = rng.standard_normal((2, self.batch, self.n, self.c)).astype(np.float32)
        self.vort, self.div = rng.standard_normal((2, self.batch, self.t, self.c)).astype(np.float32)
        self.ref_vort, self.ref_div = V.vector_analysis(self.u, self.v, *self.geom)        # of the fp32 values
        self.ref_u, self.ref_v = V.vector_synthesis(self.vort, self.div, *self.geom)
        self.band_u, self.band_v = self.ref_u.astype(np.float32), self.ref_v.astype(np.float32)
        self.W = float(np.hypot(self.u.astype(np.float64), self.v.astype(np.float64)).max())
        self.rootL = np.sqrt(big_l(self.lmax))[None, :, None]
        self.S = synthesis_scale(self.vort.astype(np.float64), self.div.astype(np.float64), self.lmax)
        self.q = R.point_weights(self.grid, self.nlat, self.nlon)


@pytest.fixture(scope="module")
def cases(ga):
    return {i: Case(ga, s, 200 + k) for k, (i, s) in enumerate(zip(IDS, SHAPES))}


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
def test_vector_analysis_against_the_restatement(cases, case_id):
    k = cases[case_id]
    u, v = dev(k.u), dev(k.v)
    got64, got32 = k.sh.vector_analysis(u, v, dtype=torch.float64), k.sh.vector_analysis(u, v)
    for name, g64, g32, ref in (("vort", got64[0], got32[0], k.ref_vort), ("div", got64[1], got32[1], k.ref_div)):
        assert g64.dtype == torch.float64 and g32.dtype == torch.float32
        assert g64.shape == (k.batch, k.t, k.c) == g32.shape
        e64, e32 = np.abs(host(g64) - ref), np.abs(host(g32) - ref)
        worst = (e64[:, 1:] / (k.rootL[:, 1:] * k.W)).max() if k.lmax else 0.0
        print(f"vector analysis {case_id} {name}: fp64 err {worst:.2e} sqrt(L) W, fp32 err {e32.max():.2e}")
        assert (e64 <= 1e-10 * k.rootL * k.W).all()
        assert (e32 <= 6e-8 * np.abs(ref) + 1e-10 * k.rootL * k.W).all()
        assert bool((g64[:, 0] == 0).all()) and bool((g32[:, 0] == 0).all())


# ---- 2. synthesis ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", IDS)
def test_vector_synthesis_against_the_restatement(cases, case_id):
    k = cases[case_id]
    vort, div = dev(k.vort), dev(k.div)
    got64, got32 = k.sh.vector_synthesis(vort, div, dtype=torch.float64), k.sh.vector_synthesis(vort, div)
    for name, g64, g32, ref in (("u", got64[0], got32[0], k.ref_u), ("v", got64[1], got32[1], k.ref_v)):
        assert g64.dtype == torch.float64 and g32.dtype == torch.float32
        assert g64.shape == (k.batch, k.n, k.c) == g32.shape
        e64, e32 = np.abs(host(g64) - ref), np.abs(host(g32) - ref)
        print(f"vector synthesis {case_id} {name}: fp64 err {(e64 / k.S).max():.2e} S_v, fp32 err {e32.max():.2e}")
        assert (e64 <= 1e-10 * k.S).all()
        assert (e32 <= 6e-8 * np.abs(ref) + 1e-10 * k.S).all()
    # fp64 coefficients go in as they are, and a missing tensor is a tensor of zeros
    assert same_bits(k.sh.vector_synthesis(vort.double(), div.double(), dtype=torch.float64), got64)
    zero = torch.zeros_like(vort)
    assert same_bits(k.sh.vector_synthesis(vort, None), k.sh.vector_synthesis(vort, zero))
    assert same_bits(k.sh.vector_synthesis(None, div), k.sh.vector_synthesis(zero, div))


# ---- 3. closed forms ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", IDS)
def test_closed_form_winds(cases, case_id):
    k = cases[case_id]
    lat, lon = R.latlon(k.grid, k.nlat, k.nlon)
    # solid-body rotation u = cos lat, v = 0: vort_{1,0} = 2 / sqrt 3 alone
    u = dev(np.cos(lat)[:, None].astype(np.float32))
    vort, div = k.sh.vector_analysis(u, torch.zeros_like(u), dtype=torch.float64)
    want = np.zeros((k.t, 1))
    want[k.sh.index(1, 0), 0] = 2.0 / np.sqrt(3.0)
    assert np.abs(host(vort) - want).max() <= 1e-6 and np.abs(host(div)).max() <= 1e-6
    # vort_{1,1} = -2 alone: u = sqrt 3 sin lat cos lon, v = -sqrt 3 sin lon, finite and not zero on a pole row
    c = torch.zeros(k.t, 1, device=DEV)
    c[k.sh.index(1, 1), 0] = -2.0
    u, v = k.sh.vector_synthesis(c, None)
    assert np.abs(host(u)[:, 0] - np.sqrt(3.0) * np.sin(lat) * np.cos(lon)).max() <= 1e-6
    assert np.abs(host(v)[:, 0] + np.sqrt(3.0) * np.sin(lon)).max() <= 1e-6
    if k.grid == "equiangular":
        for rows in (slice(0, k.nlon), slice(-k.nlon, None)):
            speed = np.hypot(host(u)[rows, 0], host(v)[rows, 0])
            assert np.isfinite(speed).all() and np.abs(speed - np.sqrt(3.0)).max() <= 1e-6
    # f = sin lat cos lat cos lon: gradient (-sin lat sin lon, cos 2 lat cos lon); f needs degree 2
    if k.lmax >= 2:
        f = dev((np.sin(lat) * np.cos(lat) * np.cos(lon))[:, None].astype(np.float32))
        east, north = k.sh.gradient(k.sh.analysis(f, dtype=torch.float64))
        assert np.abs(host(east)[:, 0] + np.sin(lat) * np.sin(lon)).max() <= 1e-6
        assert np.abs(host(north)[:, 0] - np.cos(2.0 * lat) * np.cos(lon)).max() <= 1e-6


# ---- 4. round trip, Parseval, the spectrum --------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", IDS)
def test_round_trip_of_a_band_limited_pair(cases, case_id):
    k = cases[case_id]
    vort, div = dev(k.vort, torch.float64), dev(k.div, torch.float64)
    u, v = k.sh.vector_synthesis(vort, div, dtype=torch.float64)
    back = k.sh.vector_analysis_launch(u, v, torch.float64)
    W = float(np.hypot(host(u), host(v)).max())
    amp = np.sqrt(2.0 * R.degrees(k.lmax) + 1.0)[None, :, None]
    bound = 1e-10 * k.rootL * (W + amp * k.S)
    for got, src in zip(back, (k.vort, k.div)):
        want = src.astype(np.float64)
        want[:, 0] = 0.0
        err = np.abs(host(got) - want)
        print(f"round trip {case_id}: {err.max():.2e}")
        assert (err <= bound).all()


@pytest.mark.parametrize("case_id", IDS)
def test_parseval_and_the_two_ways_to_the_spectrum(cases, case_id):
    k = cases[case_id]
    u, v = dev(k.band_u), dev(k.band_v)
    energy = k.sh.kinetic_energy_spectrum(u=u, v=v)
    assert energy.dtype == torch.float64 and energy.shape == (k.batch, k.lmax + 1, k.c)
    assert bool((energy[:, 0] == 0).all())
    want = (k.q[None, :, None] * (k.band_u.astype(np.float64) ** 2 + k.band_v.astype(np.float64) ** 2) / 2.0).sum(1)
    assert np.allclose(host(energy).sum(1), want, rtol=1e-6, atol=0)
    vort, div = k.sh.vector_analysis(u, v, dtype=torch.float64)
    assert same_bits(k.sh.kinetic_energy_spectrum(vort=vort, div=div), energy)
    ref = V.kinetic_energy(host(vort), host(div), k.lmax)
    assert np.allclose(host(energy), ref, rtol=1e-13, atol=0)
    e32 = k.sh.kinetic_energy_spectrum(u=u, v=v, dtype=torch.float32)
    assert e32.dtype == torch.float32 and same_bits(e32, energy.float())


# ---- 5. gradient and the Laplacians ---------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", IDS)
def test_gradient_and_laplacians(cases, case_id):
    k = cases[case_id]
    c = dev(k.vort)                                                     # any coefficients
    L = (k.sh.degrees * (k.sh.degrees + 1))[:, None]
    for dtype in (torch.float32, torch.float64):
        got = k.sh.gradient(c, dtype=dtype)
        assert same_bits(got, k.sh.vector_synthesis(None, -L.to(c.dtype) * c, dtype=dtype))
    east, north = k.sh.gradient(c, dtype=torch.float64)
    lap32 = (-big_l(k.lmax)[None, :, None].astype(np.float32) * k.vort).astype(np.float64)   # what the device rounds
    want_e, want_n = V.vector_synthesis(None, lap32, *k.geom)
    S = synthesis_scale(np.zeros_like(lap32), lap32, k.lmax)
    assert (np.abs(host(east) - want_e) <= 1e-10 * S).all() and (np.abs(host(north) - want_n) <= 1e-10 * S).all()
    # laplacian and inverse_laplacian: exact row factors, inverse of each other off row 0, which the inverse zeroes
    c64 = c.double()
    lap = k.sh.laplacian(c64)
    assert lap.dtype == torch.float64 and same_bits(lap, -L.double() * c64)
    assert k.sh.laplacian(c).dtype == torch.float32
    back = k.sh.inverse_laplacian(lap)
    assert bool((back[:, 0] == 0).all())
    assert bool(((back - c64).abs()[:, 1:] <= 4e-16 * c64.abs()[:, 1:]).all())
    poisoned = c64.clone()
    poisoned[:, 0] = float("nan")
    assert same_bits(k.sh.inverse_laplacian(poisoned), k.sh.inverse_laplacian(c64))
    # differentiable: d/dc sum(inverse_laplacian(c)) = -1 / L, 0 on row 0
    leaf = c64.clone().requires_grad_()
    k.sh.inverse_laplacian(leaf).sum().backward()
    want = np.zeros((k.t, 1))
    want[1:, 0] = -1.0 / big_l(k.lmax)[1:]
    assert np.allclose(host(leaf.grad), np.broadcast_to(want[None], leaf.shape), rtol=1e-15, atol=0)


def test_degree_zero_truncation_returns_zeros(ga):
    sh = ga.SphericalHarmonics(4, 5, DEV, lmax=0, grid="gauss")
    x = torch.randn(2, 20, 3, device=DEV)
    for out in sh.vector_analysis(x, x + 1):
        assert out.shape == (2, 1, 3) and bool((out == 0).all())
    c = torch.randn(2, 1, 3, device=DEV)
    for out in sh.vector_synthesis(c, c) + sh.gradient(c):
        assert out.shape == (2, 20, 3) and bool((out == 0).all())
    energy = sh.kinetic_energy_spectrum(u=x, v=x)
    assert energy.shape == (2, 1, 3) and bool((energy == 0).all())


# ---- 6. backward ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", IDS)
def test_backward_against_the_restatement_adjoints(cases, case_id):
    k = cases[case_id]
    rng = np.random.default_rng(21)
    g_vort, g_div = rng.standard_normal((2, k.batch, k.t, k.c))
    h_u, h_v = rng.standard_normal((2, k.batch, k.n, k.c))
    # analysis: (u.grad, v.grad) = q * VS(L g), fp32
    for dtype in (torch.float64, torch.float32):
        gv = g_vort.astype(np.float32).astype(np.float64) if dtype == torch.float32 else g_vort
        gd = g_div.astype(np.float32).astype(np.float64) if dtype == torch.float32 else g_div
        u, v = dev(k.u).requires_grad_(), dev(k.v).requires_grad_()
        vort, div = k.sh.vector_analysis(u, v, dtype=dtype)
        torch.autograd.backward([vort, div], [dev(gv, dtype), dev(gd, dtype)])
        want_u, want_v = V.vector_analysis_adjoint(gv, gd, *k.geom)
        S = adjoint_scale(gv, gd, k.lmax) * k.q[None, :, None]                             # [B, N, C]
        assert u.grad.dtype == torch.float32 == v.grad.dtype
        assert (np.abs(host(u.grad) - want_u) <= 6e-8 * np.abs(want_u) + 1e-10 * S).all()
        assert (np.abs(host(v.grad) - want_v) <= 6e-8 * np.abs(want_v) + 1e-10 * S).all()
    # synthesis: (vort.grad, div.grad) = VA_1(h) / L, in the coefficients' dtype
    H = float(np.hypot(h_u, h_v).max())
    want_vort, want_div = V.vector_synthesis_adjoint(h_u, h_v, *k.geom)
    inv_root = np.zeros(k.t)
    inv_root[1:] = 1.0 / np.sqrt(big_l(k.lmax)[1:])
    bound = 1e-10 * k.n * H * inv_root[None, :, None]
    for dtype in (torch.float64, torch.float32):
        vort, div = dev(k.vort, dtype).requires_grad_(), dev(k.div, dtype).requires_grad_()
        u, v = k.sh.vector_synthesis(vort, div, dtype=torch.float64)
        torch.autograd.backward([u, v], [dev(h_u), dev(h_v)])
        assert vort.grad.dtype == dtype == div.grad.dtype
        rounding = 6e-8 if dtype == torch.float32 else 0.0
        assert (np.abs(host(vort.grad) - want_vort) <= rounding * np.abs(want_vort) + bound).all()
        assert (np.abs(host(div.grad) - want_div) <= rounding * np.abs(want_div) + bound).all()
        assert bool((vort.grad[:, 0] == 0).all()) and bool((div.grad[:, 0] == 0).all())
    # one input missing: the other's gradient is the same, and gradient() reaches its coefficients
    div = dev(k.div, torch.float64).requires_grad_()
    u, v = k.sh.vector_synthesis(None, div, dtype=torch.float64)
    torch.autograd.backward([u, v], [dev(h_u), dev(h_v)])
    assert (np.abs(host(div.grad) - want_div) <= bound).all()
    coef = dev(k.div, torch.float64).requires_grad_()
    east, north = k.sh.gradient(coef, dtype=torch.float64)
    torch.autograd.backward([east, north], [dev(h_u), dev(h_v)])
    want = -big_l(k.lmax)[None, :, None] * want_div                     # the chain through laplacian()
    assert (np.abs(host(coef.grad) - want) <= big_l(k.lmax)[None, :, None] * bound).all()


@pytest.mark.parametrize("case_id", IDS)
def test_adjoint_identities_on_fp64_outputs(cases, case_id):
    k = cases[case_id]
    rng = np.random.default_rng(22)
    u, v = dev(k.u), dev(k.v)
    vort, div = dev(k.vort, torch.float64), dev(k.div, torch.float64)
    g_vort, g_div = dev(rng.standard_normal(k.vort.shape)), dev(rng.standard_normal(k.vort.shape))
    h_u, h_v = dev(rng.standard_normal(k.u.shape)), dev(rng.standard_normal(k.u.shape))
    a_vort, a_div = k.sh.vector_analysis_launch(u, v, torch.float64)
    t_u, t_v = k.sh.vector_synthesis_launch(g_vort, g_div, torch.float64, weighted=True, adjoint=True)
    lhs = float((a_vort * g_vort).sum() + (a_div * g_div).sum())
    rhs = float((u.double() * t_u).sum() + (v.double() * t_v).sum())
    assert abs(lhs - rhs) <= 1e-12 * float((a_vort * g_vort).abs().sum() + (a_div * g_div).abs().sum())
    s_u, s_v = k.sh.vector_synthesis_launch(vort, div, torch.float64)
    t_vort, t_div = k.sh.vector_analysis_launch(h_u, h_v, torch.float64, weighted=False, adjoint=True)
    lhs = float((s_u * h_u).sum() + (s_v * h_v).sum())
    rhs = float((vort * t_vort).sum() + (div * t_div).sum())
    assert abs(lhs - rhs) <= 1e-12 * float((s_u * h_u).abs().sum() + (s_v * h_v).abs().sum())


# ---- 7. spectral CRPS on winds --------------------------------------------------------------------------------------

def test_spectral_crps_on_winds_backward(ga, cases):
    k = cases[IDS[1]]
    rng = np.random.default_rng(23)

    def wind(*lead):
        return dev(rng.standard_normal((*lead, k.n, k.c)).astype(np.float32))

    def stacked(pair):
        return torch.stack(pair, dim=-1).flatten(-2)                    # [..., T, 2 C]

    pred_u, pred_v = wind(4).requires_grad_(), wind(4).requires_grad_()
    target = stacked(k.sh.vector_analysis(wind(), wind()))
    loss = ga.ensemble_crps(stacked(k.sh.vector_analysis(pred_u, pred_v)), target)
    loss.backward()
    coef = stacked(k.sh.vector_analysis(pred_u.detach(), pred_v.detach())).requires_grad_()
    again = ga.ensemble_crps(coef, target)
    again.backward()
    assert same_bits(loss.detach(), again.detach()) and float(loss.detach()) > 0
    g = coef.grad.reshape(4, k.t, k.c, 2)
    g_vort, g_div = g[..., 0].contiguous(), g[..., 1].contiguous()
    assert same_bits((pred_u.grad, pred_v.grad),
                     k.sh.vector_synthesis_launch(g_vort, g_div, torch.float32, weighted=True, adjoint=True))
    want_u, want_v = V.vector_analysis_adjoint(host(g_vort), host(g_div), *k.geom)
    S = adjoint_scale(host(g_vort), host(g_div), k.lmax) * k.q[None, :, None]
    assert (np.abs(host(pred_u.grad) - want_u) <= 6e-8 * np.abs(want_u) + 1e-10 * S).all()
    assert (np.abs(host(pred_v.grad) - want_v) <= 6e-8 * np.abs(want_v) + 1e-10 * S).all()
    assert float(pred_u.grad.abs().max()) > 0 and float(pred_v.grad.abs().max()) > 0


# ---- 8. bitwise reproducibility -------------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", [IDS[1], IDS[3]])
def test_bitwise_reproducible(ga, cases, case_id):
    k = cases[case_id]
    rng = np.random.default_rng(24)
    u, v = (dev(a) for a in rng.standard_normal((2, 3, k.n, k.c)).astype(np.float32))
    vort, div = (dev(a) for a in rng.standard_normal((2, 3, k.t, k.c)).astype(np.float32))
    item = 2 * 8 * k.nlat * (2 * k.lmax + 1) * k.c
    tight = ga.SphericalHarmonics(k.nlat, k.nlon, DEV, lmax=k.lmax, grid=k.grid, workspace_bytes=item)
    for dtype in (torch.float32, torch.float64):
        a, s = k.sh.vector_analysis(u, v, dtype=dtype), k.sh.vector_synthesis(vort, div, dtype=dtype)
        e = k.sh.kinetic_energy_spectrum(u=u, v=v, dtype=dtype)
        assert same_bits(a, k.sh.vector_analysis(u, v, dtype=dtype))
        assert same_bits(s, k.sh.vector_synthesis(vort, div, dtype=dtype))
        assert same_bits(e, k.sh.kinetic_energy_spectrum(u=u, v=v, dtype=dtype))
        for i in range(3):
            assert same_bits([t[i] for t in a], k.sh.vector_analysis(u[i], v[i], dtype=dtype))
            assert same_bits([t[i] for t in s], k.sh.vector_synthesis(vort[i], div[i], dtype=dtype))
            assert same_bits(e[i], k.sh.kinetic_energy_spectrum(u=u[i], v=v[i], dtype=dtype))
        assert same_bits(a, tight.vector_analysis(u, v, dtype=dtype))
        assert same_bits(s, tight.vector_synthesis(vort, div, dtype=dtype))
        assert same_bits(e, tight.kinetic_energy_spectrum(u=u, v=v, dtype=dtype))
    # leading axes are one batch, and a strided input is made contiguous
    a = k.sh.vector_analysis(u, v)
    assert same_bits([t[:, 0] for t in k.sh.vector_analysis(u.reshape(3, 1, k.n, k.c), v.reshape(3, 1, k.n, k.c))], a)
    wide = torch.zeros(3, k.n, 2 * k.c + 2, device=DEV)
    wide[:, :, 1:k.c + 1] = u
    wide[:, :, k.c + 1:2 * k.c + 1] = v
    assert same_bits(k.sh.vector_analysis(wide[:, :, 1:k.c + 1], wide[:, :, k.c + 1:2 * k.c + 1]), a)
    short = ga.SphericalHarmonics(k.nlat, k.nlon, DEV, lmax=k.lmax, grid=k.grid, workspace_bytes=item - 1)
    with pytest.raises(ValueError):
        short.vector_analysis(u, v)
    with pytest.raises(ValueError):
        short.vector_synthesis(vort, div)


# ---- 9. a NaN stays in its item and channel -------------------------------------------------------------------------

def test_nan_containment(cases):
    k = cases[IDS[3]]
    u, v, vort, div = dev(k.u), dev(k.v), dev(k.vort), dev(k.div)
    clean_a, clean_s = k.sh.vector_analysis(u, v), k.sh.vector_synthesis(vort, div)
    clean_e = k.sh.kinetic_energy_spectrum(u=u, v=v)
    # row 0 is read as 0 whatever it holds
    vort[:, 0] = float("nan")
    assert same_bits(k.sh.vector_synthesis(vort, div), clean_s)
    u[1, 4321, 2] = float("nan")
    vort[1, k.sh.index(30, -7), 2] = float("nan")
    a, s, e = k.sh.vector_analysis(u, v), k.sh.vector_synthesis(vort, div), k.sh.kinetic_energy_spectrum(u=u, v=v)
    # every row but row 0, which is 0 by definition, is lost in (item 1, channel 2) and nowhere else
    for got, clean, first in ((a[0], clean_a[0], 1), (a[1], clean_a[1], 1), (s[0], clean_s[0], 0),
                              (s[1], clean_s[1], 0), (e, clean_e, 1)):
        assert not bool(torch.isfinite(got[1, first:, 2]).any())
        assert bool((got[1, :first, 2] == 0).all())
        keep = torch.ones_like(got, dtype=torch.bool)
        keep[1, :, 2] = False
        assert bool(torch.isfinite(got[keep]).all()) and same_bits(got[keep], clean[keep])


# ---- 10. hipGraph capture -------------------------------------------------------------------------------------------

def test_kinetic_energy_spectrum_captures_into_a_graph(cases):
    k = cases[IDS[1]]
    rng = np.random.default_rng(25)
    first = (dev(k.u), dev(k.v))
    second = tuple(dev(rng.standard_normal(k.u.shape).astype(np.float32)) for _ in range(2))
    buf_u, buf_v = first[0].clone(), first[1].clone()
    k.sh.kinetic_energy_spectrum(u=buf_u, v=buf_v)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = k.sh.kinetic_energy_spectrum(u=buf_u, v=buf_v)
    buf_u.copy_(second[0])
    buf_v.copy_(second[1])
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out, k.sh.kinetic_energy_spectrum(u=second[0], v=second[1]))
    assert not same_bits(out, k.sh.kinetic_energy_spectrum(u=first[0], v=first[1]))


# ---- 11. past 4 GiB -------------------------------------------------------------------------------------------------

def test_input_past_4_gib(ga):
    free, _ = torch.cuda.mem_get_info()
    if free < 24 * 2 ** 30:
        pytest.skip(f"needs 24 GiB of free device memory, {free / 2 ** 30:.1f} GiB are free")
    nlat, nlon, lmax, c, batch = 32, 64, 31, 64, 8200
    sh = ga.SphericalHarmonics(nlat, nlon, DEV, lmax=lmax, grid="gauss")
    x = torch.empty(batch, nlat * nlon, c, device=DEV)
    assert x.numel() * 4 > 2 ** 32
    block = torch.randn(100, nlat * nlon, c, device=DEV, generator=torch.Generator(device=DEV).manual_seed(26))
    for b0 in range(0, batch, 100):
        x[b0:b0 + 100] = block
    x[-1] = torch.randn(nlat * nlon, c, device=DEV, generator=torch.Generator(device=DEV).manual_seed(27))
    assert 2 * 8 * nlat * (2 * lmax + 1) * c * batch > sh.workspace_bytes       # more than one chunk
    vort, div = sh.vector_analysis(x, x)                                         # the same tensor as u and as v
    alone = sh.vector_analysis(x[-1], x[-1])
    for got in alone:
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    assert same_bits((vort[-1], div[-1]), alone)
    assert same_bits((vort[4100], div[4100]), sh.vector_analysis(x[4100], x[4100]))
    del vort, div, x
    torch.cuda.empty_cache()


# ---- the largest latitude count, and the order of the errors ---------------------------------------------------------

def test_most_latitudes(ga):
    grid, nlat, nlon, lmax = "equiangular", 2047, 3, 1                  # the largest LDS request of k_vsht_lat_fwd
    sh = ga.SphericalHarmonics(nlat, nlon, DEV, lmax=lmax, grid=grid)
    rng = np.random.default_rng(28)
    u, v = rng.standard_normal((2, 1, nlat * nlon, 2)).astype(np.float32)
    vort, div = sh.vector_analysis(dev(u), dev(v), dtype=torch.float64)
    want_vort, want_div = V.vector_analysis(u, v, grid, nlat, nlon, lmax)
    bound = 1e-10 * np.sqrt(big_l(lmax))[None, :, None] * float(np.hypot(u, v).max())
    assert (np.abs(host(vort) - want_vort) <= bound).all() and (np.abs(host(div) - want_div) <= bound).all()
    c, d = rng.standard_normal((2, 1, 4, 2)).astype(np.float32)
    got_u, got_v = sh.vector_synthesis(dev(c), dev(d), dtype=torch.float64)
    want_u, want_v = V.vector_synthesis(c, d, grid, nlat, nlon, lmax)
    S = synthesis_scale(c.astype(np.float64), d.astype(np.float64), lmax)
    assert (np.abs(host(got_u) - want_u) <= 1e-10 * S).all() and (np.abs(host(got_v) - want_v) <= 1e-10 * S).all()


def test_errors_in_the_order_of_the_other_modules(cases):
    k = cases[IDS[0]]
    n, t = k.n, k.t
    good = torch.zeros(n, 3, device=DEV)
    with pytest.raises(ValueError):
        k.sh.vector_analysis(torch.zeros(n + 1, 3, device=DEV), good)
    with pytest.raises(ValueError):
        k.sh.vector_analysis(good, torch.zeros(n, 4, device=DEV))
    with pytest.raises(ValueError):
        k.sh.vector_synthesis(good, good)
    with pytest.raises(ValueError):
        k.sh.vector_synthesis(None, None)
    with pytest.raises(ValueError):
        k.sh.vector_analysis(torch.zeros(n + 1, 3, dtype=torch.float64), good)            # the shape comes first
    with pytest.raises(TypeError):
        k.sh.vector_analysis(good, torch.zeros(n, 3, dtype=torch.float64))                # then the dtype
    with pytest.raises(TypeError):
        k.sh.vector_synthesis(torch.zeros(t, 3, device=DEV), torch.zeros(t, 3, device=DEV, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        k.sh.vector_analysis(good, torch.zeros(n, 3))                                     # then the device
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        k.sh.gradient(torch.zeros(t, 3))
    with pytest.raises(TypeError):
        k.sh.vector_analysis(good, good, dtype=torch.float16)
    with pytest.raises(ValueError):
        k.sh.kinetic_energy_spectrum(u=good)
    with pytest.raises(ValueError):
        k.sh.kinetic_energy_spectrum(u=good, v=good, vort=torch.zeros(t, 3, device=DEV))
    with pytest.raises(ValueError):
        k.sh.laplacian(good)
    empty = torch.zeros(0, n, 3, device=DEV)
    for out in k.sh.vector_analysis(empty, empty):
        assert out.shape == (0, t, 3)
    for out in k.sh.vector_synthesis(torch.zeros(0, t, 3, device=DEV), None):
        assert out.shape == (0, n, 3)
    assert k.sh.kinetic_energy_spectrum(u=empty, v=empty).shape == (0, k.lmax + 1, 3)
