"""Ensemble products and rank histogram on the MI355X (gwen_ens_products_f32 / gwen_ens_rank_hist_f32 through
gwen_amd.products) against the fp64 restatements of tests/products_ref.py.

The quantile bound is derived, not measured: |got - ref| <= 2^-16 max(|s[lo]|, |s[lo + 1]|) per element (pos is rounded
once in fp32: at most 63 * 2^-24 on frac, times a gap of at most twice the larger magnitude, plus three roundings of the
interpolation).  The weighted histogram bound is that of sequential fp32 accumulation of at most N terms:
N 2^-24 ref + N 2^-24 2^-24 sum(w) per bin.  Every case prints the largest error it saw and appends it to the file named
by GWEN_PRODUCTS_ACCURACY when that is set (profiles/products_accuracy.jsonl is such a run)."""
import functools
import json
import os

import pytest
import torch

import products_ref as ref
from helpers import SEED

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Q = (0.0, 0.05, 0.1, 0.25, 1.0 / 3.0, 0.5, 0.9, 0.99, 1.0)
N_OF_C = {1: 1500, 3: 700, 4: 600, 7: 300, 64: 61, 260: 9}


@pytest.fixture(scope="module")
def ga(hip_lib):
    import gwen_amd
    return gwen_amd


def _record(**kw):
    line = json.dumps(kw)
    print(line)
    if os.environ.get("GWEN_PRODUCTS_ACCURACY"):
        with open(os.environ["GWEN_PRODUCTS_ACCURACY"], "a") as fh:
            fh.write(line + "\n")


def _quantised(t):
    return torch.clamp(torch.round(t * 2) / 2, -2, 2)


@functools.lru_cache(maxsize=None)
def _ensemble(m, n, c, kind="offset100"):
    """The inputs of a case, made once on the host and never changed."""
    g = torch.Generator().manual_seed(SEED + 1000 * m + 7 * c + n)
    if kind == "offset100":
        return 100.0 + 3.0 * torch.randn(m, n, c, generator=g)
    if kind == "quantised":
        return _quantised(torch.randn(m, n, c, generator=g))
    if kind == "offset1e4":
        return 1e4 + 0.01 * torch.randn(m, n, c, generator=g)
    return torch.randn(m, n, c, generator=g)


def _worst_rel(got, want):
    """max |got - want| / |want|; where want is 0 (four equal members at 1e4 happen) got must be 0 too: inf if not."""
    got = got.double().cpu()
    err = (got - want).abs() / want.abs()
    err = torch.where(want == 0, torch.where(got == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))), err)
    return float(err.max())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---- 1. quantile parity ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64])
@pytest.mark.parametrize("c", [1, 3, 4, 7, 64, 260])
def test_quantile_parity(ga, m, c):
    n = N_OF_C[c]
    x = _ensemble(m, n, c)
    got = ga.ensemble_quantiles(x.to(DEV), Q).double().cpu()
    want, lo, hi = ref.quantile_parts(x, Q)
    mag = torch.maximum(lo.abs(), hi.abs())
    worst = float(((got - want).abs() / mag).max())
    _record(test="quantile_parity", M=m, N=n, C=c, max_err_over_magnitude=worst, bound=2.0 ** -16)
    assert got.shape == (len(Q), n, c)
    assert bool(((got - want).abs() <= 2.0 ** -16 * mag).all()), worst


# ---- 2. exact cases, bitwise -------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 2, 3, 5, 8, 9, 17, 33, 64])
@pytest.mark.parametrize("c", [3, 8])
def test_exact_quantiles_are_bitwise(ga, m, c):
    x = _ensemble(m, 500, c).to(DEV)
    got = ga.ensemble_quantiles(x, (0.0, 0.5, 1.0))
    assert _same_bits(got[0], x.amin(0)) and _same_bits(got[2], x.amax(0))
    if m % 2 == 1:
        assert _same_bits(got[1], torch.median(x, 0).values)
    if m == 1:
        every = ga.ensemble_quantiles(x, Q)
        assert all(_same_bits(every[j], x[0]) for j in range(len(Q)))


@pytest.mark.parametrize("m", [2, 5, 16, 33, 64])
def test_equal_members_give_that_value_and_zero_spread(ga, m):
    one = _ensemble(1, 400, 6)[0].to(DEV)
    x = one.unsqueeze(0).repeat(m, 1, 1)
    out = ga.ensemble_products(x, quantiles=Q, mean=True, std=True)
    assert all(_same_bits(out["quantiles"][j], one) for j in range(len(Q)))
    assert _same_bits(out["mean"], one)
    assert torch.count_nonzero(out["std"]) == 0 and not torch.isnan(out["std"]).any()


# ---- 3. exceedance -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 3, 4, 8, 17, 33, 64])
@pytest.mark.parametrize("c", [4, 7])
@pytest.mark.parametrize("t", [1, 3])
def test_exceedance_counts(ga, m, c, t):
    x = _ensemble(m, 400, c, "quantised")
    g = torch.Generator().manual_seed(m + c + t)
    for thr in (_quantised(torch.randn(t, generator=g)), _quantised(torch.randn(t, c, generator=g))):
        got = ga.exceedance_probability(x.to(DEV), thr.to(DEV)).cpu()
        want = (ref.exceedance_counts(x, thr) / m).float()                 # count / M, rounded once
        ulp = torch.nextafter(want, torch.full_like(want, 2.0)) - want
        assert got.shape == (t, 400, c)
        assert bool(((got - want).abs() <= ulp).all())
        assert _same_bits(got, ga.exceedance_probability(x.to(DEV), thr.tolist()).cpu())   # a sequence, converted


def test_exceedance_is_strict(ga):
    x = torch.full((6, 300, 5), 1.5, device=DEV)
    assert torch.count_nonzero(ga.exceedance_probability(x, (1.5,))) == 0
    assert bool((ga.exceedance_probability(x, (1.25,)) == 1).all())
    per_channel = torch.tensor([[1.5, 1.0, 1.5, 2.0, 1.5]], device=DEV)
    got = ga.exceedance_probability(x, per_channel)[0, 0].cpu()
    assert got.tolist() == [0.0, 1.0, 0.0, 0.0, 0.0]


# ---- 4. mean / std at a large offset -----------------------------------------------------------------------------

@pytest.mark.parametrize("m", [4, 16, 32])
@pytest.mark.parametrize("c", [8, 6])
def test_mean_std_do_not_cancel_at_large_offsets(ga, m, c):
    x = _ensemble(m, 2000, c, "offset1e4")
    out = ga.ensemble_products(x.to(DEV), mean=True, std=True)
    want_mean, want_std = ref.mean_std(x)
    errs = _worst_rel(out["mean"], want_mean), _worst_rel(out["std"], want_std)
    _record(test="mean_std_offset_1e4", M=m, C=c, mean_rel_err=errs[0], std_rel_err=errs[1], bound=1e-5)
    assert set(out) == {"mean", "std"}
    assert errs[0] <= 1e-5 and errs[1] <= 1e-5, errs


def test_std_of_one_member_is_nan(ga):
    out = ga.ensemble_products(_ensemble(1, 100, 4).to(DEV), mean=True, std=True)
    assert torch.isnan(out["std"]).all() and _same_bits(out["mean"].cpu(), _ensemble(1, 100, 4)[0])


# ---- 5. non-finite containment -----------------------------------------------------------------------------------

@pytest.mark.parametrize("m,c", [(3, 4), (8, 7), (17, 4), (40, 3)])
def test_a_nan_member_stays_in_its_point(ga, m, c):
    clean = _ensemble(m, 300, c)
    dirty = clean.clone()
    dirty[m // 2, 123, c - 1] = float("nan")
    thr = (99.0, 101.0)
    a = ga.ensemble_products(clean.to(DEV), quantiles=Q, thresholds=thr, mean=True, std=True)
    b = ga.ensemble_products(dirty.to(DEV), quantiles=Q, thresholds=thr, mean=True, std=True)
    assert torch.isnan(b["quantiles"][:, 123, c - 1]).all()
    assert torch.isnan(b["mean"][123, c - 1]) and torch.isnan(b["std"][123, c - 1])
    want = ref.exceedance_counts(dirty, thr)[:, 123, c - 1] / m             # the NaN does not exceed
    assert torch.allclose(b["prob"][:, 123, c - 1].double().cpu(), want, rtol=1e-6, atol=0)
    for key in ("quantiles", "prob", "mean", "std"):
        x, y = a[key].clone(), b[key].clone()
        x[..., 123, c - 1] = 0
        y[..., 123, c - 1] = 0
        assert _same_bits(x, y), key


@pytest.mark.parametrize("m", [3, 9, 33])
def test_infinite_members_come_back_as_extremes(ga, m):
    x = _ensemble(m, 200, 4).clone()
    x[0, 5, 1] = float("inf")
    x[m - 1, 6, 2] = -float("inf")
    x[:, 7, 3] = float("inf")
    got = ga.ensemble_quantiles(x.to(DEV), (0.0, 1.0)).cpu()
    assert _same_bits(got[0], x.amin(0)) and _same_bits(got[1], x.amax(0))
    assert got[1, 5, 1] == float("inf") and got[0, 6, 2] == -float("inf") and got[0, 7, 3] == float("inf")


# ---- 6. the two paths agree --------------------------------------------------------------------------------------

def _offset_by_one_float(t):
    """The same values in a buffer that is 4-byte aligned only."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


@pytest.mark.parametrize("m,n,c", [(4, 600, 8), (5, 20000, 8), (16, 300, 64), (8, 1, 4), (33, 1, 4), (9, 50, 260)])
def test_aligned_and_unaligned_paths_give_the_same_bits(ga, m, n, c):
    g = torch.Generator().manual_seed(n)
    x = _ensemble(m, n, c, "quantised").to(DEV)
    y = _quantised(torch.randn(n, c, generator=g)).to(DEV)
    w = torch.rand(n, generator=g).to(DEV)
    thr = torch.tensor([[-0.5], [0.0], [1.0]]).repeat(1, c).to(DEV)
    xo, yo, wo = _offset_by_one_float(x), _offset_by_one_float(y), _offset_by_one_float(w)
    for kw in (dict(thresholds=thr, mean=True, std=True), dict(thresholds=(0.5,), std=True), dict(mean=True),
               dict(quantiles=Q, thresholds=thr, mean=True, std=True)):
        a, b = ga.ensemble_products(x, **kw), ga.ensemble_products(xo, **kw)
        assert set(a) == set(b) and all(_same_bits(a[k], b[k]) for k in a), kw
    # the sort-free outputs do not depend on whether quantiles ride along (another kernel instantiation)
    a = ga.ensemble_products(x, thresholds=thr, mean=True, std=True)
    b = ga.ensemble_products(x, quantiles=Q, thresholds=thr, mean=True, std=True)
    assert all(_same_bits(a[k], b[k]) for k in a)
    for normalize in (False, True):
        assert _same_bits(ga.rank_histogram(x, y, w, normalize=normalize),
                          ga.rank_histogram(xo, yo, wo, normalize=normalize))


def test_products_of_many_node_chunks(ga):
    x = _ensemble(5, 20000, 8)
    out = ga.ensemble_products(x.to(DEV), quantiles=Q, thresholds=(100.0,), mean=True, std=True)
    want, lo, hi = ref.quantile_parts(x, Q)
    assert bool(((out["quantiles"].double().cpu() - want).abs() <= 2.0 ** -16 * torch.maximum(lo.abs(), hi.abs())).all())
    assert torch.equal(out["prob"].cpu(), ref.exceedance_counts(x, (100.0,)).float() / 5)   # rounded once, in fp32
    mean, std = ref.mean_std(x)
    assert _worst_rel(out["mean"], mean) <= 1e-5 and _worst_rel(out["std"], std) <= 1e-5


# ---- 7. rank histogram -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 2, 8, 17, 64])
@pytest.mark.parametrize("c", [3, 8])
def test_rank_histogram_counts_exactly(ga, m, c):
    g = torch.Generator().manual_seed(m * 10 + c)
    x, y = _ensemble(m, 4000, c, "randn"), torch.randn(4000, c, generator=g)
    assert not bool((x == y).any())                                         # tie-free
    got = ga.rank_histogram(x.to(DEV), y.to(DEV), normalize=False)
    want = ref.rank_histogram(x, y)
    assert got.shape == (c, m + 1) and got.dtype == torch.float32
    assert torch.equal(got.double().cpu(), want) and float(want.sum()) == 4000 * c
    norm = ga.rank_histogram(x.to(DEV), y.to(DEV))
    assert float((norm.double().sum(1) - 1).abs().max()) <= 1e-6
    assert float((norm.double().cpu() - want / 4000).abs().max()) <= 1e-6


@pytest.mark.parametrize("m", [1, 3, 8, 17, 33, 64])
@pytest.mark.parametrize("kind", ["randn", "quantised"])
def test_rank_histogram_weighted_and_tied(ga, m, kind):
    n, c = 4000, 6
    g = torch.Generator().manual_seed(m)
    x = _ensemble(m, n, c, kind)
    y = torch.randn(n, c, generator=g)
    y = _quantised(y) if kind == "quantised" else y
    w = torch.rand(n, generator=g)
    got = ga.rank_histogram(x.to(DEV), y.to(DEV), w.to(DEV), normalize=False).double().cpu()
    want = ref.rank_histogram(x, y, w)
    eps = n * 2.0 ** -24
    bound = eps * want + eps * 2.0 ** -24 * float(w.double().sum())
    worst = float(((got - want).abs() / bound).max())
    _record(test="rank_histogram_weighted", M=m, N=n, C=c, data=kind, max_abs_err=float((got - want).abs().max()),
            max_err_over_bound=worst)
    assert bool(((got - want).abs() <= bound).all()), worst
    norm = ga.rank_histogram(x.to(DEV), y.to(DEV), w.to(DEV)).double().cpu()
    assert float((norm.sum(1) - 1).abs().max()) <= 1e-6
    assert float((norm - want / want.sum(1, keepdim=True)).abs().max()) <= 1e-6


def test_rank_histogram_bool_mask_selects_points(ga):
    g = torch.Generator().manual_seed(5)
    n = 3000
    mask = torch.rand(n, generator=g) > 0.5
    # tie-free: the bins are integers, the masked run equals the run on the selected points exactly
    x, y = _ensemble(6, n, 8, "randn"), torch.randn(n, 8, generator=g)
    got = ga.rank_histogram(x.to(DEV), y.to(DEV), mask.to(DEV), normalize=False)
    want = ga.rank_histogram(x[:, mask].to(DEV), y[mask].to(DEV), normalize=False)
    assert torch.equal(got, want) and torch.equal(got.double().cpu(), ref.rank_histogram(x[:, mask], y[mask]))
    # with ties the shares are fractions and the two runs sum them in another order
    x, y = _ensemble(6, n, 8, "quantised"), _quantised(torch.randn(n, 8, generator=g))
    got = ga.rank_histogram(x.to(DEV), y.to(DEV), mask.to(DEV), normalize=False).double().cpu()
    want = ref.rank_histogram(x[:, mask], y[mask])
    eps = n * 2.0 ** -24
    assert bool(((got - want).abs() <= eps * want + eps * 2.0 ** -24 * float(mask.sum())).all())


def test_rank_histogram_skips_nan_points(ga):
    g = torch.Generator().manual_seed(9)
    x, y = _ensemble(8, 2000, 4, "randn").clone(), torch.randn(2000, 4, generator=g)
    y[10, 0] = float("nan")
    y[11, 3] = float("nan")
    x[3, 12, 1] = float("nan")
    got = ga.rank_histogram(x.to(DEV), y.to(DEV), normalize=False).double().cpu()
    assert torch.equal(got, ref.rank_histogram(x, y))
    assert got.sum(1).tolist() == [1999.0, 1999.0, 2000.0, 1999.0]
    # a channel that counted nothing: zeros, and NaN once normalised
    y[:, 2] = float("nan")
    assert torch.count_nonzero(ga.rank_histogram(x.to(DEV), y.to(DEV), normalize=False)[2]) == 0
    norm = ga.rank_histogram(x.to(DEV), y.to(DEV))
    assert torch.isnan(norm[2]).all() and not torch.isnan(norm[[0, 1, 3]]).any()


@pytest.mark.parametrize("m,n,c", [(8, 4000, 8), (17, 5000, 3), (64, 3000, 260)])
def test_two_runs_are_bitwise_equal(ga, m, n, c):
    g = torch.Generator().manual_seed(c)
    x = _ensemble(m, n, c, "quantised").to(DEV)
    y, w = _quantised(torch.randn(n, c, generator=g)).to(DEV), torch.rand(n, generator=g).to(DEV)
    assert _same_bits(ga.rank_histogram(x, y, w), ga.rank_histogram(x, y, w))
    a = ga.ensemble_products(x, quantiles=Q, thresholds=(0.0,), mean=True, std=True)
    b = ga.ensemble_products(x, quantiles=Q, thresholds=(0.0,), mean=True, std=True)
    assert all(_same_bits(a[k], b[k]) for k in a)


# ---- 8. graph capture --------------------------------------------------------------------------------------------

def test_products_capture_into_a_graph(ga):
    m, n, c = 8, 700, 12
    first, second = _ensemble(m, n, c).to(DEV), _ensemble(m, n, c + 1)[:, :, :c].contiguous().to(DEV)
    q = torch.tensor(Q, device=DEV)
    thr = torch.tensor([[99.0] * c, [101.0] * c], device=DEV)
    buf = first.clone()
    kw = dict(quantiles=q, thresholds=thr, mean=True, std=True)
    ga.ensemble_products(buf, **kw)                                          # warm: the library, the occupancy query
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ga.ensemble_products(buf, **kw)
    buf.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    eager = ga.ensemble_products(second, **kw)
    assert all(_same_bits(out[k], eager[k]) for k in eager)
    assert not _same_bits(out["mean"], ga.ensemble_products(first, mean=True)["mean"])


def test_rank_histogram_captures_into_a_graph(ga):
    m, n, c = 9, 3000, 5
    g = torch.Generator().manual_seed(1)
    x1, x2 = _ensemble(m, n, c, "randn").to(DEV), _ensemble(m, n, c, "quantised").to(DEV)
    y1, y2 = torch.randn(n, c, generator=g).to(DEV), _quantised(torch.randn(n, c, generator=g)).to(DEV)
    w = torch.rand(n, generator=g).to(DEV)
    bx, by = x1.clone(), y1.clone()
    ga.rank_histogram(bx, by, w)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ga.rank_histogram(bx, by, w)
    bx.copy_(x2)
    by.copy_(y2)
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(out, ga.rank_histogram(x2, y2, w))
    assert not _same_bits(out, ga.rank_histogram(x1, y1, w))


# ---- 9. one realistic size, once ---------------------------------------------------------------------------------

def test_realistic_size(ga):
    m, n, c = 8, 20 * 100 * 100, 16                                          # the faces of the nu = 100 mesh
    g = torch.Generator(device=DEV).manual_seed(SEED)
    x = 100.0 + 3.0 * torch.randn(m, n, c, device=DEV, generator=g)
    y = 100.0 + 3.0 * torch.randn(n, c, device=DEV, generator=g)
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(SEED))[:2000].sort().values
    out = ga.ensemble_products(x, quantiles=Q, thresholds=(100.0, 103.0), mean=True, std=True)
    xs, ys = x[:, rows.to(DEV)].cpu(), y[rows.to(DEV)].cpu()
    want, lo, hi = ref.quantile_parts(xs, Q)
    got = out["quantiles"][:, rows.to(DEV)].double().cpu()
    assert bool(((got - want).abs() <= 2.0 ** -16 * torch.maximum(lo.abs(), hi.abs())).all())
    assert torch.equal(out["prob"][:, rows.to(DEV)].cpu(), ref.exceedance_counts(xs, (100.0, 103.0)).float() / 8)   # k / 8: exact
    mean, std = ref.mean_std(xs)
    assert _worst_rel(out["mean"][rows.to(DEV)], mean) <= 1e-5 and _worst_rel(out["std"][rows.to(DEV)], std) <= 1e-5
    # the histogram of the sampled rows through the full-size launch (a bool mask), and every point counted once
    mask = torch.zeros(n, dtype=torch.bool)
    mask[rows] = True
    sampled = ga.rank_histogram(x, y, mask.to(DEV), normalize=False).double().cpu()
    assert torch.equal(sampled, ref.rank_histogram(xs, ys))
    full = ga.rank_histogram(x, y, normalize=False).double().cpu()
    assert full.sum(1).tolist() == [float(n)] * c
    flat = ga.rank_histogram(x, y).double().cpu()                            # x, y from one law: a flat histogram
    assert float((flat - 1.0 / (m + 1)).abs().max()) <= 6.0 * (1.0 / (m + 1) / n) ** 0.5
