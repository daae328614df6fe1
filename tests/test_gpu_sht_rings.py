"""gwen_amd.spectral on reduced Gaussian grids, on the device, against the numpy fp64 restatement tests/sht_rings_ref.py.

The geometries are the smallest that reach every edge of the two ragged longitude kernels and of the latitude kernels
behind them: the 16-order wave and the 64-order block (wide: lmax 65), the 16-channel tile of the latitude kernels (wide:
C 17), more than 64 (item, channel) lanes (lanes: 70), truncation on (o8t, irr, wide) and off (o8, lanes, reg), odd, prime
and one-point rings (irr), more than 64 latitudes (wide, reg).

Bounds: those of tests/test_gpu_sht.py and tests/test_gpu_vsht.py, whose headers derive them for 12 000 points and
l <= 74; the largest grid here has 12 000 points and lmax 74 (reg), the others are smaller, and a truncated ring sums
fewer terms, so the derivations carry over: fp64 analysis 1e-10 max |x|, fp64 synthesis 1e-10 S with S = sum_lm |c_lm|
sqrt(2l + 1), one more rounding (6e-8 |ref|) for an fp32 result, and a factor sqrt(l (l + 1)) on the vector transforms.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sht_ref as R  # noqa: E402
import sht_rings_ref as G  # noqa: E402
import vsht_ref as V  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

IRREGULAR = [1, 4, 7, 12, 18, 25, 25, 19, 12, 8, 5, 2]
WIDE = [5 + 4 * min(j, 65 - j) for j in range(66)]
# id -> (ring_nlon, lmax, C, batch)
SHAPES = {"o8": (G.octahedral(8).tolist(), 7, 3, 1), "o8t": (G.octahedral(8).tolist(), 11, 5, 2),
          "irr": (IRREGULAR, 11, 1, 1), "wide": (WIDE, 65, 17, 3), "lanes": (G.octahedral(8).tolist(), 7, 70, 1),
          "reg": ([150] * 80, 74, 5, 3)}
IDS = list(SHAPES)


@pytest.fixture(scope="module")
def ga(hip_lib):
    import gwen_amd
    return gwen_amd


def big_l(lmax):
    l = R.degrees(lmax).astype(np.float64)
    return l * (l + 1.0)


def vector_synthesis_scale(vort, div, lmax):
    """S_v [B, 1, C] of tests/test_gpu_vsht.py."""
    l = R.degrees(lmax).astype(np.float64)
    amp = np.zeros_like(l)
    amp[1:] = np.sqrt((2.0 * l[1:] + 1.0) / (l[1:] * (l[1:] + 1.0)))
    return ((np.abs(vort) + np.abs(div)) * amp[None, :, None]).sum(1, keepdims=True)


class Case:
    """One geometry: the transform, fp32 inputs on both sides and the restatement's answers, made once."""

    def __init__(self, ga, shape, seed):
        self.rings, self.lmax, self.c, self.batch = shape
        self.geom = (self.rings, self.lmax)
        self.sh = ga.SphericalHarmonics.reduced(self.rings, DEV, lmax=self.lmax)
        rng = np.random.default_rng(seed)
        self.n, self.t = int(np.sum(self.rings)), (self.lmax + 1) ** 2
        self.x = rng.standard_normal((self.batch, self.n, self.c)).astype(np.float32)
        self.coef = rng.standard_normal((self.batch, self.t, self.c)).astype(np.float32)
        self.ref_coef = G.analysis(self.x, *self.geom)                      # of the fp32 values
        self.ref_x = G.synthesis(self.coef, *self.geom)
        self.X = float(np.abs(self.x).max())
        self.amp = np.sqrt(2.0 * R.degrees(self.lmax) + 1.0)
        self.S = (np.abs(self.coef.astype(np.float64)) * self.amp[None, :, None]).sum(1, keepdims=True)   # [B, 1, C]
        self.q = G.point_weights(self.rings)


@pytest.fixture(scope="module")
def cases(ga):
    made = {}

    def get(case_id):
        if case_id not in made:
            made[case_id] = Case(ga, SHAPES[case_id], 300 + IDS.index(case_id))
        return made[case_id]
    return get


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


# ---- 1. analysis and synthesis against the restatement ------------------------------------------------------------------

@pytest.mark.parametrize("case_id", IDS)
def test_analysis_against_the_restatement(cases, case_id):
    k = cases(case_id)
    assert k.sh.grid == "reduced-gauss" and k.sh.nlon is None and k.sh.rows == k.n and k.sh.num_coefficients == k.t
    assert k.sh.ring_nlon.dtype == np.int64 and k.sh.ring_nlon.tolist() == list(k.rings)
    assert k.sh.ring_start.dtype == np.int64 and k.sh.ring_start.tolist() == G.geometry(k.rings)[1].tolist()
    x = dev(k.x)
    c64, c32 = k.sh.analysis(x, dtype=torch.float64), k.sh.analysis(x)
    assert c64.dtype == torch.float64 and c32.dtype == torch.float32
    assert c64.shape == (k.batch, k.t, k.c) == c32.shape
    e64, e32 = np.abs(host(c64) - k.ref_coef), np.abs(host(c32) - k.ref_coef)
    print(f"rings analysis {case_id}: fp64 err {e64.max() / k.X:.2e} X, fp32 err {e32.max():.2e}")
    assert (e64 <= 1e-10 * k.X).all()
    assert (e32 <= 6e-8 * np.abs(k.ref_coef) + 1e-10 * k.X).all()


@pytest.mark.parametrize("case_id", IDS)
def test_synthesis_against_the_restatement(cases, case_id):
    k = cases(case_id)
    c = dev(k.coef)
    x64, x32 = k.sh.synthesis(c, dtype=torch.float64), k.sh.synthesis(c)
    assert x64.dtype == torch.float64 and x32.dtype == torch.float32
    assert x64.shape == (k.batch, k.n, k.c) == x32.shape
    e64, e32 = np.abs(host(x64) - k.ref_x), np.abs(host(x32) - k.ref_x)
    print(f"rings synthesis {case_id}: fp64 err {(e64 / k.S).max():.2e} S, fp32 err {e32.max():.2e}")
    assert (e64 <= 1e-10 * k.S).all()
    assert (e32 <= 6e-8 * np.abs(k.ref_x) + 1e-10 * k.S).all()
    assert same_bits(k.sh.synthesis(c.double(), dtype=torch.float64), x64)      # fp64 coefficients go in as they are


# ---- 2. rings of one length are the regular Gauss grid, bit for bit -----------------------------------------------------

@pytest.mark.parametrize("nlat, nlon, lmax, c, batch", [(80, 150, 74, 5, 3), (9, 18, 8, 3, 2)], ids=["reg", "9x18"])
def test_equal_rings_reproduce_the_regular_grid_bit_for_bit(ga, nlat, nlon, lmax, c, batch):
    red = ga.SphericalHarmonics.reduced([nlon] * nlat, DEV, lmax=lmax)
    reg = ga.SphericalHarmonics(nlat, nlon, DEV, lmax=lmax, grid="gauss")
    assert red.rows == reg.rows and np.array_equal(red.ring_nlon, reg.ring_nlon)
    assert np.array_equal(red.ring_start, reg.ring_start) and reg.nlon == nlon and reg.grid == "gauss"
    rng = np.random.default_rng(21)
    x, u, v = (dev(rng.standard_normal((batch, nlat * nlon, c)).astype(np.float32)) for _ in range(3))
    coef = dev(rng.standard_normal((batch, (lmax + 1) ** 2, c)).astype(np.float32))
    assert same_bits(red.analysis(x, dtype=torch.float64), reg.analysis(x, dtype=torch.float64))
    assert same_bits(red.synthesis(coef, dtype=torch.float64), reg.synthesis(coef, dtype=torch.float64))
    assert same_bits(red.vector_analysis(u, v, dtype=torch.float64), reg.vector_analysis(u, v, dtype=torch.float64))
    assert same_bits(red.vector_synthesis(coef, coef.flip(0), dtype=torch.float64),
                     reg.vector_synthesis(coef, coef.flip(0), dtype=torch.float64))
    assert same_bits(red.weights, reg.weights) and np.array_equal(red.positions, reg.positions)


# ---- 3. the orders above M_j are zero, whatever the workspace held ------------------------------------------------------

@pytest.mark.parametrize("case_id, ring, point, visible", [("o8t", 0, 3, False), ("o8t", 15, 19, False),
                                                           ("irr", 0, 0, True), ("irr", 4, 5, True)])
def test_delta_inputs_show_the_truncation(cases, case_id, ring, point, visible):
    """``visible``: whether the truncated orders of this ring would reach the coefficients above the tolerance.  On the
    polar rings of O8 they would not (Pbar_m^m ~ cos^m lat is 1e-9 there, which is why the grid can drop them); there the
    exact zeros of the synthesis below are the check."""
    k = cases(case_id)
    rings, start = G.geometry(k.rings)
    mj = int(G.orders(*k.geom)[ring])
    assert mj < k.lmax
    x = np.zeros((1, k.n, 1), dtype=np.float32)
    x[0, start[ring] + point, 0] = 1.0
    want = G.analysis(x, *k.geom)
    got = host(k.sh.analysis(dev(x), dtype=torch.float64))
    assert (np.abs(got - want) <= 1e-10).all()
    # the sums this ring would add without the truncation: far above the tolerance, and absent
    lat, _ = R.latitudes("gauss", rings.size)
    lon = 2.0 * np.pi * point / rings[ring]
    extra = np.zeros_like(want)
    for m in range(mj + 1, k.lmax + 1):
        p = R.legendre(k.lmax, m, lat)[:, ring] * G.latitude_weights(rings)[ring]
        ls = np.arange(m, k.lmax + 1)
        extra[0, ls * ls + ls + m, 0] = p * np.cos(m * lon)
        extra[0, ls * ls + ls - m, 0] = p * np.sin(m * lon)
    if visible:
        assert np.abs(extra).max() >= 1e-4
        high = np.abs(extra) >= 1e-4
        assert (np.abs(got - (want + extra))[high] >= 0.5e-4).all()
    # the synthesis of coefficients that live on the truncated orders alone leaves this ring at zero
    c = np.zeros((1, k.t, 1))
    for m in range(mj + 1, k.lmax + 1):
        ls = np.arange(m, k.lmax + 1)
        c[0, ls * ls + ls + m, 0] = 1.0
        c[0, ls * ls + ls - m, 0] = -1.0
    back = k.sh.synthesis(dev(c), dtype=torch.float64)
    assert bool((back[0, start[ring]:start[ring + 1]] == 0).all())
    assert (np.abs(host(back) - G.synthesis(c, *k.geom)) <= 1e-10 * (np.abs(c) * k.amp[None, :, None]).sum()).all()


@pytest.mark.parametrize("case_id", ["o8t", "irr"])
def test_a_workspace_full_of_nan_changes_nothing(ga, cases, case_id):
    from gwen_amd import _lib
    k = cases(case_id)
    x, u, v = dev(k.x), dev(k.x * 0.5), dev(k.x[:, ::-1].copy())
    item = 8 * len(k.rings) * (2 * k.lmax + 1) * k.c
    results = []
    for fill in (0.0, float("nan")):
        ws = torch.full((2 * k.batch * item // 8,), fill, dtype=torch.float64, device=DEV)
        coef = torch.empty(k.batch, k.t, k.c, dtype=torch.float64, device=DEV)
        k.sh._transform(_lib.SHT_OP_ANALYSIS, (x, None), (coef, None), True, False, k.batch, k.c, ws)
        ws.fill_(fill)
        vort, div = torch.empty_like(coef), torch.empty_like(coef)
        k.sh._transform(_lib.SHT_OP_VECTOR_ANALYSIS, (u, v), (vort, div), True, False, k.batch, k.c, ws)
        results.append((coef, vort, div))
    assert all(bool(torch.isfinite(t).all()) for t in results[1])
    assert same_bits(results[0], results[1])
    assert same_bits(results[0][0], k.sh.analysis(x, dtype=torch.float64))


# ---- 4. round trip and Parseval -------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [8, 16], ids=["o8", "o16"])
def test_round_trip_and_parseval(ga, n):
    sh = ga.SphericalHarmonics.octahedral(n, DEV)
    assert sh.lmax == n - 1 and sh.nlat == 2 * n and sh.rows == int(G.octahedral(n).sum())
    rng = np.random.default_rng(40 + n)
    c = dev(rng.standard_normal((2, n * n, 3)).astype(np.float32))
    x = sh.synthesis(c)
    back = sh.analysis(x)
    err = float((back - c).abs().max())
    print(f"rings round trip O{n}: {err / float(c.abs().max()):.2e} max |c|")
    assert err <= 1e-6 * float(c.abs().max())
    total = host(sh.power_spectrum(x)).sum(1)
    want = (G.point_weights(G.octahedral(n))[None, :, None] * host(x) ** 2).sum(1)
    assert np.allclose(total, want, rtol=1e-6, atol=0)


# ---- 5. the tables ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", ["o8", "irr", "wide"])
def test_weights_and_positions(cases, case_id):
    k = cases(case_id)
    w = k.sh.weights
    assert w.dtype == torch.float32 and w.shape == (k.n,)
    assert np.allclose(host(w), k.q, rtol=1e-7, atol=0)
    assert abs(float(w.double().sum()) - 1.0) <= 1e-6
    pos = k.sh.positions
    lat, lon = G.latlon(k.rings)
    assert pos.dtype == np.float64 and pos.shape == (k.n, 3)
    assert np.allclose(pos, np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], 1), atol=1e-14)
    assert np.array_equal(k.sh.degrees.cpu().numpy(), R.degrees(k.lmax))
    assert k.sh.index(k.lmax, -k.lmax) == k.lmax ** 2


# ---- 6. backward ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", ["o8t", "wide"])
def test_backward_against_the_restatement_adjoints(cases, case_id):
    k = cases(case_id)
    rng = np.random.default_rng(11)
    g = rng.standard_normal((k.batch, k.t, k.c))
    h = rng.standard_normal((k.batch, k.n, k.c))
    # analysis: x.grad = q * synthesis(g), fp32
    x = dev(k.x).requires_grad_()
    k.sh.analysis(x, dtype=torch.float64).backward(dev(g))
    want = G.analysis_adjoint(g, *k.geom)
    S = (np.abs(g) * k.amp[None, :, None]).sum(1, keepdims=True) * k.q[None, :, None]       # [B, N, C]
    assert x.grad.dtype == torch.float32
    assert (np.abs(host(x.grad) - want) <= 6e-8 * np.abs(want) + 1e-10 * S).all()
    x32 = dev(k.x).requires_grad_()
    k.sh.analysis(x32).backward(dev(g, torch.float32))
    g32 = g.astype(np.float32).astype(np.float64)
    want32 = G.analysis_adjoint(g32, *k.geom)
    S32 = (np.abs(g32) * k.amp[None, :, None]).sum(1, keepdims=True) * k.q[None, :, None]
    assert (np.abs(host(x32.grad) - want32) <= 6e-8 * np.abs(want32) + 1e-10 * S32).all()
    # synthesis: c.grad = analysis of h with unit weights, in c's dtype
    H = float(np.abs(h).max())
    want = G.synthesis_adjoint(h, *k.geom)
    c64 = dev(k.coef, torch.float64).requires_grad_()
    k.sh.synthesis(c64, dtype=torch.float64).backward(dev(h))
    assert c64.grad.dtype == torch.float64
    assert (np.abs(host(c64.grad) - want) <= 1e-10 * k.n * H).all()
    c32 = dev(k.coef).requires_grad_()
    k.sh.synthesis(c32, dtype=torch.float64).backward(dev(h))
    assert c32.grad.dtype == torch.float32
    assert (np.abs(host(c32.grad) - want) <= 6e-8 * np.abs(want) + 1e-10 * k.n * H).all()


@pytest.mark.parametrize("case_id", ["o8t", "wide"])
def test_adjoint_identity_on_fp64_outputs(cases, case_id):
    k = cases(case_id)
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


# ---- 7. vector transforms -------------------------------------------------------------------------------------------

class VectorCase:
    def __init__(self, k, seed):
        rng = np.random.default_rng(seed)
        self.u, self.v = rng.standard_normal((2, k.batch, k.n, k.c)).astype(np.float32)
        self.vort, self.div = rng.standard_normal((2, k.batch, k.t, k.c)).astype(np.float32)
        self.ref_vort, self.ref_div = G.vector_analysis(self.u, self.v, *k.geom)
        self.ref_u, self.ref_v = G.vector_synthesis(self.vort, self.div, *k.geom)
        self.W = float(np.hypot(self.u.astype(np.float64), self.v.astype(np.float64)).max())
        self.rootL = np.sqrt(big_l(k.lmax))[None, :, None]
        self.S = vector_synthesis_scale(self.vort.astype(np.float64), self.div.astype(np.float64), k.lmax)


@pytest.fixture(scope="module")
def vector_cases(cases):
    made = {}

    def get(case_id):
        if case_id not in made:
            made[case_id] = VectorCase(cases(case_id), 500 + IDS.index(case_id))
        return made[case_id]
    return get


@pytest.mark.parametrize("case_id", ["o8t", "wide"])
def test_vector_transforms_against_the_restatement(cases, vector_cases, case_id):
    k, w = cases(case_id), vector_cases(case_id)
    u, v = dev(w.u), dev(w.v)
    got64, got32 = k.sh.vector_analysis(u, v, dtype=torch.float64), k.sh.vector_analysis(u, v)
    for g64, g32, ref in ((got64[0], got32[0], w.ref_vort), (got64[1], got32[1], w.ref_div)):
        assert g64.dtype == torch.float64 and g32.dtype == torch.float32 and g64.shape == (k.batch, k.t, k.c)
        e64, e32 = np.abs(host(g64) - ref), np.abs(host(g32) - ref)
        print(f"rings vector analysis {case_id}: fp64 err {(e64[:, 1:] / (w.rootL[:, 1:] * w.W)).max():.2e} sqrt(L) W")
        assert (e64 <= 1e-10 * w.rootL * w.W).all()
        assert (e32 <= 6e-8 * np.abs(ref) + 1e-10 * w.rootL * w.W).all()
        assert bool((g64[:, 0] == 0).all()) and bool((g32[:, 0] == 0).all())
    vort, div = dev(w.vort), dev(w.div)
    got64, got32 = k.sh.vector_synthesis(vort, div, dtype=torch.float64), k.sh.vector_synthesis(vort, div)
    for g64, g32, ref in ((got64[0], got32[0], w.ref_u), (got64[1], got32[1], w.ref_v)):
        assert g64.dtype == torch.float64 and g32.dtype == torch.float32 and g64.shape == (k.batch, k.n, k.c)
        e64, e32 = np.abs(host(g64) - ref), np.abs(host(g32) - ref)
        print(f"rings vector synthesis {case_id}: fp64 err {(e64 / w.S).max():.2e} S_v")
        assert (e64 <= 1e-10 * w.S).all()
        assert (e32 <= 6e-8 * np.abs(ref) + 1e-10 * w.S).all()
    zero = torch.zeros_like(vort)
    assert same_bits(k.sh.vector_synthesis(vort, None), k.sh.vector_synthesis(vort, zero))


@pytest.mark.parametrize("case_id", ["o8t", "wide"])
def test_gradient_and_kinetic_energy(cases, vector_cases, case_id):
    k, w = cases(case_id), vector_cases(case_id)
    c = dev(k.coef)
    lap32 = (-big_l(k.lmax)[None, :, None].astype(np.float32) * k.coef).astype(np.float64)   # what the device rounds
    east, north = k.sh.gradient(c, dtype=torch.float64)
    assert same_bits((east, north), k.sh.vector_synthesis(None, k.sh.laplacian(c), dtype=torch.float64))
    want_e, want_n = G.vector_synthesis(None, lap32, *k.geom)
    S = vector_synthesis_scale(np.zeros_like(lap32), lap32, k.lmax)
    assert (np.abs(host(east) - want_e) <= 1e-10 * S).all() and (np.abs(host(north) - want_n) <= 1e-10 * S).all()
    c64 = c.double()
    back = k.sh.inverse_laplacian(k.sh.laplacian(c64))
    assert bool((back[:, 0] == 0).all()) and bool(((back - c64).abs()[:, 1:] <= 4e-16 * c64.abs()[:, 1:]).all())
    # the kinetic energy spectrum of a wind, and of its coefficients
    u, v = dev(w.u), dev(w.v)
    energy = k.sh.kinetic_energy_spectrum(u=u, v=v)
    assert energy.dtype == torch.float64 and energy.shape == (k.batch, k.lmax + 1, k.c)
    vort, div = k.sh.vector_analysis(u, v, dtype=torch.float64)
    assert same_bits(k.sh.kinetic_energy_spectrum(vort=vort, div=div), energy)
    assert np.allclose(host(energy), V.kinetic_energy(host(vort), host(div), k.lmax), rtol=1e-13, atol=0)
    want = V.kinetic_energy(w.ref_vort, w.ref_div, k.lmax)
    assert np.allclose(host(energy)[:, 1:], want[:, 1:], rtol=1e-7, atol=0) and bool((energy[:, 0] == 0).all())


# ---- 8. bitwise reproducibility -------------------------------------------------------------------------------------

def test_bitwise_reproducible(ga, cases):
    k = cases("wide")
    rng = np.random.default_rng(14)
    x = dev(rng.standard_normal((3, k.n, k.c)).astype(np.float32))
    c = dev(rng.standard_normal((3, k.t, k.c)).astype(np.float32))
    item = 8 * len(k.rings) * (2 * k.lmax + 1) * k.c
    tight = ga.SphericalHarmonics.reduced(k.rings, DEV, lmax=k.lmax, workspace_bytes=item)
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
    assert same_bits(k.sh.analysis(x.reshape(3, 1, k.n, k.c))[:, 0], k.sh.analysis(x))
    with pytest.raises(ValueError):
        ga.SphericalHarmonics.reduced(k.rings, DEV, lmax=k.lmax, workspace_bytes=item - 8).analysis(x)
    with pytest.raises(ValueError):                                            # a vector transform holds two rings
        tight.vector_analysis(x, x)


# ---- 9. a NaN stays in its item and channel -------------------------------------------------------------------------

def test_nan_containment(cases):
    k = cases("o8t")
    x, c = dev(k.x), dev(k.coef)
    clean_a, clean_s = k.sh.analysis(x), k.sh.synthesis(c)
    x[0, 77, 1] = float("nan")
    c[0, k.sh.index(10, -7), 1] = float("nan")
    a, s = k.sh.analysis(x), k.sh.synthesis(c)
    assert bool(torch.isnan(a[0, :, 1]).any()) and bool(torch.isnan(s[0, :, 1]).any())
    for got, clean in ((a, clean_a), (s, clean_s)):
        keep = torch.ones_like(got, dtype=torch.bool)
        keep[0, :, 1] = False
        assert bool(torch.isfinite(got[keep]).all()) and same_bits(got[keep], clean[keep])


# ---- 10. hipGraph capture -------------------------------------------------------------------------------------------

def test_power_spectrum_captures_into_a_graph(cases):
    k = cases("o8")
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


# ---- 11. spectral CRPS ----------------------------------------------------------------------------------------------

def test_spectral_crps_backward(ga, cases):
    k = cases("o8")
    rng = np.random.default_rng(13)
    pred = dev(rng.standard_normal((4, k.n, k.c)).astype(np.float32)).requires_grad_()
    target = dev(rng.standard_normal((k.n, k.c)).astype(np.float32))
    loss = ga.ensemble_crps(k.sh.analysis(pred), k.sh.analysis(target))
    loss.backward()
    coef = k.sh.analysis(pred.detach()).requires_grad_()
    again = ga.ensemble_crps(coef, k.sh.analysis(target))
    again.backward()
    assert same_bits(loss.detach(), again.detach()) and float(loss.detach()) > 0
    assert same_bits(pred.grad, k.sh.synthesis_launch(coef.grad, torch.float32, weighted=True))
    want = G.analysis_adjoint(host(coef.grad), *k.geom)
    S = (np.abs(host(coef.grad)) * k.amp[None, :, None]).sum(1, keepdims=True) * k.q[None, :, None]
    assert (np.abs(host(pred.grad) - want) <= 6e-8 * np.abs(want) + 1e-10 * S).all()
    assert float(pred.grad.abs().max()) > 0


# ---- 12. the SFNO modules take the object as it is ------------------------------------------------------------------

def test_spectral_conv_and_block_on_an_octahedral_grid(ga):
    from gwen_amd import ops
    from gwen_amd.attention import _ActFunction
    sh = ga.SphericalHarmonics.octahedral(8, DEV)
    torch.manual_seed(11)
    x = torch.randn(2, sh.rows, 16, device=DEV, requires_grad=True)
    conv = ga.SpectralConv(sh, 16, 16).to(DEV)
    y = conv(x)
    want = sh.synthesis(ga.spectral_conv(sh.analysis(x), conv.weight, precision=conv.precision))
    assert y.shape == (2, sh.rows, 16) and same_bits(y.detach(), want.detach())
    block = ga.SFNOBlock(sh, 16).to(DEV)
    out = block(x)
    p = block.precision
    n = ops.layer_norm(x.reshape(-1, 16), block.norm1.weight, block.norm1.bias, block.norm1.eps).view(x.shape)
    h = x + block.conv(n) + ops.linear_autograd(n, block.skip.weight, None, contract=p)
    n2 = ops.layer_norm(h.reshape(-1, 16), block.norm2.weight, block.norm2.bias, block.norm2.eps).view(h.shape)
    t = ops.linear_autograd(n2, block.mlp[0].weight, block.mlp[0].bias, contract=p)
    t = _ActFunction.apply(t.reshape(-1, t.shape[-1]), "silu").view(t.shape)
    want = h + ops.linear_autograd(t, block.mlp[2].weight, block.mlp[2].bias, contract=p)
    assert out.shape == x.shape and same_bits(out.detach(), want.detach())
    (out.square().mean() + y.square().mean()).backward()
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
    for name, q in list(block.named_parameters()) + list(conv.named_parameters()):
        assert q.grad is not None and bool(torch.isfinite(q.grad).all()) and float(q.grad.abs().max()) > 0, name


# ---- 13. past 4 GiB -------------------------------------------------------------------------------------------------

def test_input_past_4_gib(ga):
    free, _ = torch.cuda.mem_get_info()
    if free < 16 * 2 ** 30:
        pytest.skip(f"needs 16 GiB of free device memory, {free / 2 ** 30:.1f} GiB are free")
    lmax, c, batch = 3, 64, 31000
    sh = ga.SphericalHarmonics.octahedral(8, DEV, lmax=lmax)
    x = torch.empty(batch, sh.rows, c, device=DEV)
    assert x.numel() * 4 > 2 ** 32
    block = torch.randn(1000, sh.rows, c, device=DEV, generator=torch.Generator(device=DEV).manual_seed(16))
    for b0 in range(0, batch, 1000):
        x[b0:b0 + 1000] = block
    x[-1] = torch.randn(sh.rows, c, device=DEV, generator=torch.Generator(device=DEV).manual_seed(17))
    assert 8 * sh.nlat * (2 * lmax + 1) * c * batch > sh.workspace_bytes          # more than one chunk
    coef = sh.analysis(x)
    alone = sh.analysis(x[-1])
    assert bool(torch.isfinite(alone).all()) and float(alone.abs().max()) > 0
    assert same_bits(coef[-1], alone)
    assert same_bits(coef[15500], sh.analysis(x[15500]))
    back = sh.synthesis(coef)                                                   # and an output past 4 GiB
    assert same_bits(back[-1], sh.synthesis(alone))
    del coef, x, back
    torch.cuda.empty_cache()


# ---- 14. errors -----------------------------------------------------------------------------------------------------

def test_errors_in_the_order_of_the_regular_grids(ga, cases):
    k = cases("o8")
    n = k.n
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
    with pytest.raises(ValueError):
        k.sh.vector_analysis(torch.zeros(n, 3, device=DEV), torch.zeros(n, 2, device=DEV))
    with pytest.raises(ValueError, match="fft"):
        ga.SphericalHarmonics.reduced(k.rings, DEV, lmax=k.lmax, longitude="fft")
    with pytest.raises(ValueError, match="fft"):
        ga.SphericalHarmonics.octahedral(8, DEV, longitude="fft")
    with pytest.raises(ValueError):
        ga.SphericalHarmonics.reduced(k.rings, DEV, lmax=16)
    assert k.sh.analysis(torch.zeros(0, n, 3, device=DEV)).shape == (0, k.t, 3)
