"""ring_longitude="bluestein" of gwen_amd.spectral on the device: one FFT a ring whatever its length, against the numpy
fp64 restatements tests/sht_rings_ref.py, sht_ref.py and vsht_ref.py -- never against the direct device path, except in
the one test that compares the two.

The geometries are those of tests/test_gpu_sht_rings.py and one more: mixed rings beside the Bluestein rings 28 and 44
(o8), truncation (o8t, irr, wide), the odd prime rings 7 and 19 and the one- and two-point rings (irr), 28 distinct
Bluestein lengths, a ragged channel tile and more than 64 latitudes (wide), several channel tiles a ring (lanes), the
convolution length 4096 in both parities with more than 64 KB of LDS (long), and rings of one 5-smooth length (reg).

Bounds: those of tests/test_gpu_sht_rings.py -- fp64 analysis 1e-10 max |x|, fp64 synthesis 1e-10 S with S = sum_lm
|c_lm| sqrt(2l + 1), one more rounding (6e-8 |ref|) for an fp32 result, a factor sqrt(l (l + 1)) on the vector
transforms.  They carry over: a Bluestein ring replaces a ring's sum of nlon terms by two FFTs and three pointwise
products, a few 2^-53 log2 M of the ring's sum of magnitudes where the direct bound carries nlon 2^-53: on the longest
ring here (4094 points, log2 M = 12) ten times 12 * 2^-53 of 4094 X is 5e-11 X, before the latitude weight w_j / nlon.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sht_ref as R  # noqa: E402
import sht_rings_ref as G  # noqa: E402
from helpers import REL_TOL, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

IRREGULAR = [1, 4, 7, 12, 18, 25, 25, 19, 12, 8, 5, 2]
WIDE = [5 + 4 * min(j, 65 - j) for j in range(66)]
# id -> (ring_nlon, lmax, C, batch)
SHAPES = {"o8": (G.octahedral(8).tolist(), 7, 3, 1), "o8t": (G.octahedral(8).tolist(), 11, 5, 2),
          "irr": (IRREGULAR, 11, 1, 1), "wide": (WIDE, 65, 17, 3), "lanes": (G.octahedral(8).tolist(), 7, 70, 1),
          "long": ([2047, 4088, 4094, 2047], 3, 2, 1), "reg": ([150] * 80, 74, 5, 3)}
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
        self.sh = ga.SphericalHarmonics.reduced(self.rings, DEV, lmax=self.lmax, ring_longitude="bluestein")
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
            made[case_id] = Case(ga, SHAPES[case_id], 700 + IDS.index(case_id))
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
def test_analysis_against_the_restatement(ga, cases, case_id):
    k = cases(case_id)
    assert k.sh.ring_longitude == "bluestein" and k.sh.longitude == "direct" and k.sh.grid == "reduced-gauss"
    kinds = {ga.ring_fft_plan(n)[0] for n in k.rings}
    assert kinds == ({"mixed"} if case_id == "reg" else {"bluestein"} if case_id == "long" else {"mixed", "bluestein"})
    x = dev(k.x)
    c64, c32 = k.sh.analysis(x, dtype=torch.float64), k.sh.analysis(x)
    assert c64.dtype == torch.float64 and c32.dtype == torch.float32
    assert c64.shape == (k.batch, k.t, k.c) == c32.shape
    e64, e32 = np.abs(host(c64) - k.ref_coef), np.abs(host(c32) - k.ref_coef)
    print(f"rings fft analysis {case_id}: fp64 err {e64.max() / k.X:.2e} X, fp32 err {e32.max():.2e}")
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
    print(f"rings fft synthesis {case_id}: fp64 err {(e64 / k.S).max():.2e} S, fp32 err {e32.max():.2e}")
    assert (e64 <= 1e-10 * k.S).all()
    assert (e32 <= 6e-8 * np.abs(k.ref_x) + 1e-10 * k.S).all()
    assert same_bits(k.sh.synthesis(c.double(), dtype=torch.float64), x64)      # fp64 coefficients go in as they are


# ---- 2. rings of one 5-smooth length are the regular Gauss grid with longitude="fft", bit for bit ------------------------

def test_equal_smooth_rings_reproduce_the_regular_fft_bit_for_bit(ga, cases):
    k = cases("reg")
    nlat, nlon = len(k.rings), k.rings[0]
    reg = ga.SphericalHarmonics(nlat, nlon, DEV, lmax=k.lmax, grid="gauss", longitude="fft")
    assert reg.ring_longitude is None and reg.rows == k.sh.rows
    assert ga.SphericalHarmonics(nlat, nlon, DEV, lmax=k.lmax, grid="gauss").ring_longitude is None
    assert ga.SphericalHarmonics.reduced(k.rings, DEV, lmax=k.lmax).ring_longitude == "direct"
    rng = np.random.default_rng(21)
    x, u, v = dev(k.x), dev(rng.standard_normal(k.x.shape).astype(np.float32)), dev(k.x[:, ::-1].copy())
    coef = dev(k.coef)
    assert same_bits(k.sh.analysis(x, dtype=torch.float64), reg.analysis(x, dtype=torch.float64))
    assert same_bits(k.sh.synthesis(coef, dtype=torch.float64), reg.synthesis(coef, dtype=torch.float64))
    assert same_bits(k.sh.vector_analysis(u, v, dtype=torch.float64), reg.vector_analysis(u, v, dtype=torch.float64))
    assert same_bits(k.sh.vector_synthesis(coef, coef.flip(0), dtype=torch.float64),
                     reg.vector_synthesis(coef, coef.flip(0), dtype=torch.float64))


# ---- 3. the orders above M_j are zero, whatever the workspace held ------------------------------------------------------

@pytest.mark.parametrize("case_id", ["o8t", "irr"])
def test_a_workspace_full_of_nan_changes_nothing(cases, case_id):
    from gwen_amd import _lib
    k = cases(case_id)
    assert int(G.orders(*k.geom).min()) < k.lmax
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


def test_the_synthesis_leaves_a_truncated_ring_at_zero(cases):
    k = cases("o8t")
    _, start = G.geometry(k.rings)
    mj = int(G.orders(*k.geom)[0])
    c = np.zeros((1, k.t, 1))
    for m in range(mj + 1, k.lmax + 1):
        ls = np.arange(m, k.lmax + 1)
        c[0, ls * ls + ls + m, 0] = 1.0
        c[0, ls * ls + ls - m, 0] = -1.0
    back = k.sh.synthesis(dev(c), dtype=torch.float64)
    assert bool((back[0, start[0]:start[1]] == 0).all()) and float(back.abs().max()) > 0
    assert (np.abs(host(back) - G.synthesis(c, *k.geom)) <= 1e-10 * (np.abs(c) * k.amp[None, :, None]).sum()).all()


# ---- 4. vector transforms -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", ["o8", "wide"])
def test_vector_transforms_against_the_restatement(cases, case_id):
    k = cases(case_id)
    rng = np.random.default_rng(900 + IDS.index(case_id))
    u, v = rng.standard_normal((2, k.batch, k.n, k.c)).astype(np.float32)
    vort, div = rng.standard_normal((2, k.batch, k.t, k.c)).astype(np.float32)
    W = float(np.hypot(u.astype(np.float64), v.astype(np.float64)).max())
    rootL = np.sqrt(big_l(k.lmax))[None, :, None]
    got64, got32 = k.sh.vector_analysis(dev(u), dev(v), dtype=torch.float64), k.sh.vector_analysis(dev(u), dev(v))
    for g64, g32, ref in zip(got64, got32, G.vector_analysis(u, v, *k.geom)):
        assert g64.dtype == torch.float64 and g32.dtype == torch.float32 and g64.shape == (k.batch, k.t, k.c)
        e64, e32 = np.abs(host(g64) - ref), np.abs(host(g32) - ref)
        print(f"rings fft vector analysis {case_id}: fp64 err {(e64[:, 1:] / (rootL[:, 1:] * W)).max():.2e} sqrt(L) W")
        assert (e64 <= 1e-10 * rootL * W).all()
        assert (e32 <= 6e-8 * np.abs(ref) + 1e-10 * rootL * W).all()
        assert bool((g64[:, 0] == 0).all()) and bool((g32[:, 0] == 0).all())
    S = vector_synthesis_scale(vort.astype(np.float64), div.astype(np.float64), k.lmax)
    got64 = k.sh.vector_synthesis(dev(vort), dev(div), dtype=torch.float64)
    got32 = k.sh.vector_synthesis(dev(vort), dev(div))
    for g64, g32, ref in zip(got64, got32, G.vector_synthesis(vort, div, *k.geom)):
        assert g64.dtype == torch.float64 and g32.dtype == torch.float32 and g64.shape == (k.batch, k.n, k.c)
        e64, e32 = np.abs(host(g64) - ref), np.abs(host(g32) - ref)
        print(f"rings fft vector synthesis {case_id}: fp64 err {(e64 / S).max():.2e} S_v")
        assert (e64 <= 1e-10 * S).all()
        assert (e32 <= 6e-8 * np.abs(ref) + 1e-10 * S).all()


# ---- 5. backward: the adjoint identities through autograd -----------------------------------------------------------

@pytest.mark.parametrize("case_id", ["o8", "irr"])
def test_adjoint_identities_through_autograd(cases, case_id):
    """<A x, g> = <x, A^T g> and <S c, h> = <c, S^T h> with the transposes that autograd returns; fp64 outputs and an fp64
    c, so that the two sides differ by the rounding of the sums (1e-12 of the sum of magnitudes, as
    tests/test_gpu_sht_rings.py) and, for x, by the one fp32 rounding of x.grad."""
    k = cases(case_id)
    rng = np.random.default_rng(12)
    g, h = dev(rng.standard_normal(k.coef.shape)), dev(rng.standard_normal(k.x.shape))
    x = dev(k.x).requires_grad_()
    ax = k.sh.analysis(x, dtype=torch.float64)
    ax.backward(g)
    lhs, rhs = float((ax.detach() * g).sum()), float((x.detach().double() * x.grad.double()).sum())
    terms = float((x.detach().double() * x.grad.double()).abs().sum())
    print(f"rings fft adjoint {case_id}: analysis {abs(lhs - rhs) / terms:.1e} of the terms")
    assert x.grad.dtype == torch.float32 and abs(lhs - rhs) <= 6e-8 * terms + 1e-12 * float((ax.detach() * g).abs().sum())
    atg = k.sh.synthesis_launch(g, torch.float64, weighted=True)                # the same transpose, unrounded
    assert abs(lhs - float((x.detach().double() * atg).sum())) <= 1e-12 * float((ax.detach() * g).abs().sum())
    assert same_bits(x.grad, atg.float())
    c = dev(k.coef, torch.float64).requires_grad_()
    sc = k.sh.synthesis(c, dtype=torch.float64)
    sc.backward(h)
    lhs, rhs = float((sc.detach() * h).sum()), float((c.detach() * c.grad).sum())
    assert c.grad.dtype == torch.float64 and abs(lhs - rhs) <= 1e-12 * float((sc.detach() * h).abs().sum())
    # and against the restatement's adjoints
    want = G.synthesis_adjoint(host(h), *k.geom)
    assert (np.abs(host(c.grad) - want) <= 1e-10 * k.n * float(h.abs().max())).all()
    want = G.analysis_adjoint(host(g), *k.geom)
    S = (np.abs(host(g)) * k.amp[None, :, None]).sum(1, keepdims=True) * k.q[None, :, None]
    assert (np.abs(host(x.grad) - want) <= 6e-8 * np.abs(want) + 1e-10 * S).all()


# ---- 6. bitwise reproducibility -------------------------------------------------------------------------------------

def test_bitwise_reproducible(ga, cases):
    k = cases("wide")
    rng = np.random.default_rng(14)
    x = dev(rng.standard_normal((3, k.n, k.c)).astype(np.float32))
    c = dev(rng.standard_normal((3, k.t, k.c)).astype(np.float32))
    item = 8 * len(k.rings) * (2 * k.lmax + 1) * k.c
    tight = ga.SphericalHarmonics.reduced(k.rings, DEV, lmax=k.lmax, workspace_bytes=item, ring_longitude="bluestein")
    for dtype in (torch.float32, torch.float64):
        a, s, p = k.sh.analysis(x, dtype=dtype), k.sh.synthesis(c, dtype=dtype), k.sh.power_spectrum(x, dtype=dtype)
        assert same_bits(a, k.sh.analysis(x, dtype=dtype)) and same_bits(s, k.sh.synthesis(c, dtype=dtype))
        for i in range(3):
            assert same_bits(a[i], k.sh.analysis(x[i], dtype=dtype))
            assert same_bits(s[i], k.sh.synthesis(c[i], dtype=dtype))
            assert same_bits(p[i], k.sh.power_spectrum(x[i], dtype=dtype))
        assert same_bits(a, tight.analysis(x, dtype=dtype)) and same_bits(s, tight.synthesis(c, dtype=dtype))
        assert same_bits(p, tight.power_spectrum(x, dtype=dtype))
    # a channel's bits do not depend on who shares its tile
    assert same_bits(k.sh.analysis(x[..., 3:4].contiguous(), dtype=torch.float64),
                     k.sh.analysis(x, dtype=torch.float64)[..., 3:4])


# ---- 7. a NaN stays in its item and channel -------------------------------------------------------------------------

def test_nan_containment(cases):
    k = cases("o8t")
    x, c = dev(k.x), dev(k.coef)
    clean_a, clean_s = k.sh.analysis(x), k.sh.synthesis(c)
    _, start = G.geometry(k.rings)
    x[0, int(start[2]) + 5, 1] = float("nan")                                    # on the Bluestein ring of 28 points
    c[0, k.sh.index(10, -7), 1] = float("nan")
    a, s = k.sh.analysis(x), k.sh.synthesis(c)
    assert bool(torch.isnan(a[0, :, 1]).any()) and bool(torch.isnan(s[0, :, 1]).any())
    for got, clean in ((a, clean_a), (s, clean_s)):
        keep = torch.ones_like(got, dtype=torch.bool)
        keep[0, :, 1] = False
        assert bool(torch.isfinite(got[keep]).all()) and same_bits(got[keep], clean[keep])


def test_nan_containment_on_o8(cases):
    k = cases("o8")
    x = dev(np.concatenate([k.x, k.x[:, ::-1]], 0))                              # two items
    clean = k.sh.analysis(x, dtype=torch.float64)
    _, start = G.geometry(k.rings)
    x[1, int(start[6]) + 9, 2] = float("nan")                                    # on the Bluestein ring of 44 points
    got = k.sh.analysis(x, dtype=torch.float64)
    keep = torch.ones_like(got, dtype=torch.bool)
    keep[1, :, 2] = False
    assert bool(torch.isnan(got[1, :, 2]).any())
    assert bool(torch.isfinite(got[keep]).all()) and same_bits(got[keep], clean[keep])


# ---- 8. hipGraph capture --------------------------------------------------------------------------------------------

def test_transforms_capture_into_a_graph(cases):
    k = cases("o8")
    rng = np.random.default_rng(15)
    first, second = dev(k.x), dev(rng.standard_normal(k.x.shape).astype(np.float32))
    buf = first.clone()
    eager = k.sh.synthesis(k.sh.analysis(second, dtype=torch.float64))
    k.sh.synthesis(k.sh.analysis(buf, dtype=torch.float64))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = k.sh.synthesis(k.sh.analysis(buf, dtype=torch.float64))
    buf.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(out, eager)
    assert not same_bits(out, k.sh.synthesis(k.sh.analysis(first, dtype=torch.float64)))


# ---- 9. the SFNO modules take the object as it is -----------------------------------------------------------------------

def test_sfno_block_agrees_with_the_direct_object(ga, cases):
    k = cases("o8")
    direct = ga.SphericalHarmonics.reduced(k.rings, DEV, lmax=k.lmax)
    torch.manual_seed(11)
    block = ga.SFNOBlock(k.sh, 16).to(DEV)
    twin = ga.SFNOBlock(direct, 16).to(DEV)
    twin.load_state_dict(block.state_dict())
    x = torch.randn(2, k.n, 16, device=DEV)
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    out, want = block(xa), twin(xb)
    out.square().mean().backward()
    want.square().mean().backward()
    errs = {"forward": rel_err(out.detach(), want.detach()), "x": rel_err(xa.grad, xb.grad)}
    theirs = dict(twin.named_parameters())
    for name, p in block.named_parameters():
        assert p.grad is not None and float(p.grad.abs().max()) > 0, name
        errs[name] = rel_err(p.grad, theirs[name].grad)
    print(f"SFNO block, bluestein against direct: {errs}")
    assert all(v <= REL_TOL for v in errs.values()), errs


# ---- 10. the two longitude stages of one grid -------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", ["o8t", "wide"])
def test_direct_against_bluestein(ga, cases, case_id):
    """Both within 1e-10 of the restatement, so within 2e-10 of each other."""
    k = cases(case_id)
    direct = ga.SphericalHarmonics.reduced(k.rings, DEV, lmax=k.lmax, ring_longitude="direct")
    x, c = dev(k.x), dev(k.coef)
    ea = (k.sh.analysis(x, dtype=torch.float64) - direct.analysis(x, dtype=torch.float64)).abs()
    es = (k.sh.synthesis(c, dtype=torch.float64) - direct.synthesis(c, dtype=torch.float64)).abs()
    print(f"rings fft against direct {case_id}: analysis {float(ea.max()) / k.X:.2e} X, synthesis "
          f"{(host(es) / k.S).max():.2e} S")
    assert float(ea.max()) <= 2e-10 * k.X and (host(es) <= 2e-10 * k.S).all()
    assert same_bits(k.sh.weights, direct.weights) and np.array_equal(k.sh.positions, direct.positions)
