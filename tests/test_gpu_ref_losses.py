"""gwen_amd.loss_functions on the MI355X: the reference's fp64 numbers (tests/golden/ref_losses*.npz), block and sample
geometry against the fp64 restatement (tests/ref_losses_ref.py), bitwise properties, and the forecaster end to end.

The bound of every comparison, per array:  max(4 max|ref32 - ref64|, 16 * 2^-24 * max|ref64|)  -- four times the error
of the reference's own fp32 run (another summation order, another erf), with a floor for the arrays on which that run
lands on its fp64 value.  For the fixtures ref32 is the recorded CPU run; for the larger shapes it is the reference's
expression in torch fp32 on the device (``torch_crps`` / ``torch_varreg`` / ``torch_masked`` below).  Each case's
measured error is printed beside its bound and appended to the file named by GWEN_REF_LOSSES_ACCURACY when that is set
(profiles/ref_losses_accuracy.jsonl is such a run)."""
import json
import os

import numpy as np
import pytest
import torch
from torch import nn
from torch.distributions import Normal

import large_ref as L
import ref_losses_ref as R
from helpers import SEED, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIX = R.load_fixtures()
NAMES = R.case_names(FIX)


@pytest.fixture(scope="module")
def lf(hip_lib):
    from gwen_amd import loss_functions
    return loss_functions


def _np(t) -> np.ndarray:
    return t.detach().double().cpu().numpy()


def bound(ref32, ref64) -> float:
    ref32, ref64 = np.asarray(ref32, np.float64), np.asarray(ref64, np.float64)
    ok = ~np.isnan(ref64)
    if not ok.any():
        return 0.0
    return max(4.0 * float(np.abs(ref32[ok] - ref64[ok]).max()), 16.0 * 2.0 ** -24 * float(np.abs(ref64[ok]).max()))


def check(test, case, what, got, ref32, ref64):
    """``got`` against ``ref64`` within ``bound(ref32, ref64)``, NaN exactly where ref64 is; prints and records."""
    got, ref64 = np.asarray(got, np.float64).reshape(np.shape(ref64)), np.asarray(ref64, np.float64)
    same_nan = bool(np.array_equal(np.isnan(got), np.isnan(ref64)))
    ok = ~np.isnan(ref64) & ~np.isnan(got)
    err = float(np.abs(got[ok] - ref64[ok]).max()) if ok.any() else 0.0
    b = bound(np.asarray(ref32, np.float64).reshape(ref64.shape), ref64)
    line = json.dumps({"test": test, "case": case, "array": what, "max_abs_err": err, "bound": b,
                       "max_abs_ref64": float(np.abs(ref64[~np.isnan(ref64)]).max()) if ok.any() else None,
                       "nan_where_reference_is": same_nan})
    print(line)
    if os.environ.get("GWEN_REF_LOSSES_ACCURACY"):
        with open(os.environ["GWEN_REF_LOSSES_ACCURACY"], "a") as fh:
            fh.write(line + "\n")
    return same_nan and err <= b, line


def check_all(test, case, got, ref32, ref64):
    bad = []
    for what, g, a, b in zip(("value", "grad_x", "grad_t"), got, ref32, ref64):
        ok, line = check(test, case, what, g, a, b)
        if not ok:
            bad.append(line)
    assert not bad, "\n".join(bad)


def run(crit, x, t, *args, **kw):
    """(value, grad_x, grad_t) of ``crit(x, t, ...)`` summed, on the device; x and t are left as they are."""
    xd, td = x.detach().requires_grad_(), t.detach().requires_grad_()
    value = crit(xd, td, *args, **kw)
    gx, gt = torch.autograd.grad(value.sum(), (xd, td))
    return value.detach(), gx, gt


# the reference's expressions, composed from torch ops (fp32 on the device: ref32 of the larger shapes)
def torch_crps(x, t, dim=0):
    mu, sigma = torch.mean(x, dim=dim), torch.std(x, dim=dim) + 1e-6
    return torch.mean((Normal(mu, sigma).cdf(t) - 0.5) ** 2, dim=[1, 2, 3])


def torch_varreg(alpha):
    return lambda x, t: torch.mean(torch.abs(x - t)) - alpha * torch.mean(torch.var(x, dim=1))


def torch_masked(loss_fn, mask):
    return lambda x, t: torch.sum(loss_fn(x, t) * mask) / torch.sum(mask)


def _loss_fn(kind):
    return nn.L1Loss(reduction="none") if kind == "l1" else nn.MSELoss(reduction="none")


# ---- the fixtures: every case, value and both gradients -------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_fixture_case_matches_the_reference_fp64(lf, name):
    x, t = torch.from_numpy(FIX[f"{name}/x"]).to(DEV), torch.from_numpy(FIX[f"{name}/t"]).to(DEV)
    meta, family = float(FIX[f"{name}/meta"][0]), name.split("_")[0]
    if family == "crps":
        got = run(lf.CRPSLoss(), x, t, dim=int(meta))
    elif family == "varreg":
        got = run(lf.EnsembleVarRegLoss(alpha=meta), x, t)
    else:
        mask = torch.from_numpy(FIX[f"{name}/mask"]).to(DEV)
        got = run(lf.MaskedLoss(_loss_fn(R.KINDS[int(meta)])), x, t, mask)
    check_all("fixture", name, [_np(g) for g in got],
              [FIX[f"{name}/{k}"] for k in ("value32", "grad32_x", "grad32_t")],
              [FIX[f"{name}/{k}"] for k in ("value64", "grad64_x", "grad64_t")])


def test_zero_spread_points_follow_the_s_equals_zero_rule(lf):
    """Fixture ``crps_zero_spread``: the reference's own fp32 run does not find s == 0 at the identical-member points
    (its mean of equal members is rounded), so the case's bound is wide there.  Directly: at those points the value
    and both gradients are the fp64 reference's within the floor alone, 16 * 2^-24 of the array's largest value --
    ds/dx_i = 0 where s == 0, and the shifted mean keeps s == 0 exact."""
    name = "crps_zero_spread"
    x, t = FIX[f"{name}/x"], FIX[f"{name}/t"]
    flat = (x == x[:1]).all(0)                           # [B, 1, H, W]: every member equal
    assert 10 <= int(flat.sum()) < flat.size
    value, gx, gt = run(lf.CRPSLoss(), torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV))
    gx, gt = _np(gx), _np(gt)
    want_x, want_t = FIX[f"{name}/grad64_x"], FIX[f"{name}/grad64_t"]
    floor_x = 16.0 * 2.0 ** -24 * float(np.abs(want_x).max())
    floor_t = 16.0 * 2.0 ** -24 * float(np.abs(want_t).max())
    err_x = float(np.abs(gx - want_x)[:, flat].max())
    err_t = float(np.abs(gt - want_t)[flat].max())
    print(f"zero-spread points: grad_x err {err_x:.2e} (floor {floor_x:.2e}), grad_t err {err_t:.2e} (floor {floor_t:.2e})")
    assert err_x <= floor_x and err_t <= floor_t
    assert np.all(want_x[:, flat] == 0.0) and np.all(gx[:, flat] == 0.0)        # the reference's autograd returns 0 there
    want_v = FIX[f"{name}/value64"]
    assert float(np.abs(_np(value) - want_v).max()) <= 16.0 * 2.0 ** -24 * float(np.abs(want_v).max())


# ---- block and sample geometry against the restatement ------------------------------------------------------------------

def _crps_inputs(m, b, s, seed, spread=1.0):
    g = torch.Generator().manual_seed(SEED + seed)
    x = (spread * torch.randn(m, b, 1, 1, s, generator=g) + 0.3).to(DEV)
    t = torch.randn(b, 1, 1, s, generator=g).to(DEV)
    return x, t


def _offset_copy(t):
    """the same values 4 bytes further: off the 16-byte path"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


CRPS_GEOMETRY = [
    (4, 7, 10007),       # a prime S: samples straddle blocks; R = 70 049 is off the 16-byte path
    (4, 1, 70001),       # one sample over 69 blocks
    (4, 5000, 3),        # 341 samples per block, every third one split between two
    (2, 3, 205), (3, 3, 205), (64, 3, 205), (256, 3, 205),       # the member buckets: 8, 32 and the re-reading path
    (8, 6, 2048),        # the 16-byte path, samples of two whole blocks
    (5, 40, 100),        # the 16-byte path, short samples
    (33, 5, 1500),       # 16-byte path above 32 members, samples across a block boundary
    (9, 2, 5000),        # 16-byte path, the sample boundary inside the tenth block
]


@pytest.mark.parametrize("m,b,s", CRPS_GEOMETRY)
def test_crps_geometry(lf, m, b, s):
    x, t = _crps_inputs(m, b, s, seed=m + s)
    got = run(lf.CRPSLoss(), x, t)
    ref32 = run(torch_crps, x, t)
    want = R.gauss_crps(_np(x).reshape(1, m, b * s), _np(t).reshape(1, b * s), b)
    check_all("crps_geometry", f"M{m}_B{b}_S{s}", [_np(g) for g in got], [_np(g) for g in ref32], want)
    # the same bits from buffers 4 bytes off the 16-byte path, and from a second call
    for again in (run(lf.CRPSLoss(), _offset_copy(x), _offset_copy(t)), run(lf.CRPSLoss(), x, t)):
        for a, c in zip(got, again):
            assert torch.equal(a, c)


@pytest.mark.parametrize("r", [70001, 70004])
@pytest.mark.parametrize("broadcast", [True, False])
def test_varreg_geometry(lf, r, broadcast):
    g = torch.Generator().manual_seed(SEED + r)
    x = torch.randn(2, 5, r, generator=g).to(DEV)
    t = torch.randn(2, 1 if broadcast else 5, r, generator=g).to(DEV)
    t[0, 0, :100] = x[0, 0, :100]                       # ties
    crit = lf.EnsembleVarRegLoss(alpha=0.3)
    got = run(crit, x, t)
    ref32 = run(torch_varreg(0.3), x, t)
    want = R.varreg_l1(_np(x), _np(t), 0.3)
    check_all("varreg_geometry", f"R{r}_{'broadcast' if broadcast else 'full'}", [_np(g) for g in got],
              [_np(g) for g in ref32], want)
    for again in (run(crit, _offset_copy(x), _offset_copy(t)), run(crit, x, t)):
        for a, c in zip(got, again):
            assert torch.equal(a, c)


@pytest.mark.parametrize("m", [1, 2, 9, 33, 40])
def test_varreg_member_buckets(lf, m):
    g = torch.Generator().manual_seed(SEED + m)
    x, t = torch.randn(3, m, 7, 9, generator=g).to(DEV), torch.randn(3, 1, 7, 9, generator=g).to(DEV)
    got = run(lf.EnsembleVarRegLoss(alpha=0.1), x, t)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                 # torch.var of one member warns, and returns NaN
        ref32 = run(torch_varreg(0.1), x, t)
    want = R.varreg_l1(_np(x).reshape(3, m, 63), _np(t).reshape(3, 1, 63), 0.1)
    check_all("varreg_members", f"M{m}", [_np(g) for g in got], [_np(g) for g in ref32], want)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("r", [70001, 70004])
@pytest.mark.parametrize("full", [False, True])
def test_masked_geometry(lf, kind, r, full):
    g = torch.Generator().manual_seed(SEED + r)
    x, t = torch.randn(3, r, generator=g).to(DEV), torch.randn(3, r, generator=g).to(DEV)
    mask = (torch.rand((3, r) if full else (r,), generator=g) * (torch.rand((3, r) if full else (r,), generator=g) < 0.7)).to(DEV)
    crit = lf.MaskedLoss(_loss_fn(kind))
    got = run(crit, x, t, mask)
    ref32 = run(torch_masked(_loss_fn(kind), mask), x, t)
    want = R.masked_mean(_np(x), _np(t), _np(mask), kind)
    check_all("masked_geometry", f"{kind}_R{r}_{'full' if full else 'row'}", [_np(g) for g in got],
              [_np(g) for g in ref32], want)
    for again in (run(crit, _offset_copy(x), _offset_copy(t), _offset_copy(mask)), run(crit, x, t, mask)):
        for a, c in zip(got, again):
            assert torch.equal(a, c)
    # a bool mask is its float image; leading ones on the mask change nothing
    flags = mask > 0.4
    a = run(crit, x, t, flags)
    for u, v in zip(a, run(crit, x, t, flags.float())):
        assert torch.equal(u, v)
    for u, v in zip(got, run(crit, x, t, mask.unsqueeze(0) if not full else mask)):
        assert torch.equal(u, v)


def test_masked_other_loss_fn_is_the_same_expression_on_the_device(lf):
    g = torch.Generator().manual_seed(SEED)
    x, t = torch.randn(3, 5, 7, 9, generator=g).to(DEV), torch.randn(3, 5, 7, 9, generator=g).to(DEV)
    mask = torch.rand(7, 9, generator=g).to(DEV)
    fn = nn.SmoothL1Loss(reduction="none")
    got = run(lf.MaskedLoss(fn), x, t, mask)
    want = run(torch_masked(fn, mask), x, t)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    # a mask that broadcasts from the middle ([5, 1, 9]) keeps the reference's "sum of the mask as given"
    mid = torch.rand(5, 1, 9, generator=g).to(DEV)
    got = run(lf.MaskedLoss(_loss_fn("l1")), x, t, mid)
    want = run(torch_masked(_loss_fn("l1"), mid), x, t)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


# ---- bitwise properties -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [1, 2, 4, -2])
def test_crps_dim_is_bitwise_the_movedim_result(lf, dim):
    g = torch.Generator().manual_seed(SEED + 10 + dim)
    x = torch.randn(6, 6, 6, 6, 6, generator=g).to(DEV)
    t = torch.randn(6, 6, 6, 6, generator=g).to(DEV)
    crit = lf.CRPSLoss()
    value, gx, gt = run(crit, x, t, dim=dim)
    moved = x.movedim(dim, 0).contiguous()
    v0, gx0, gt0 = run(crit, moved, t, dim=0)
    assert value.shape == (6,)
    assert torch.equal(value, v0) and torch.equal(gx.movedim(dim, 0), gx0) and torch.equal(gt, gt0)


@pytest.mark.parametrize("shape,dim", [((5, 7, 3, 20, 25), 1),      # samples of 1500 points across block boundaries
                                       ((5, 1, 7, 20, 75), 2),      # a singleton axis in front of the members
                                       ((5, 1, 1, 7, 1500), 3),     # two of them
                                       ((3, 1, 9, 4, 5), -3)])
def test_crps_dim_read_in_place_is_bitwise_the_movedim_result(lf, shape, dim):
    """The shapes ``_crps_layout`` serves as [A, M, R] without a copy (S divides R): the kernel reads ``outputs`` as it
    lies, and the bits are those of the members-first copy."""
    g = torch.Generator().manual_seed(SEED + 20 + dim)
    assert lf._crps_layout(shape, dim % 5)[0]
    rest = tuple(n for i, n in enumerate(shape) if i != dim % 5)
    x, t = torch.randn(*shape, generator=g).to(DEV), torch.randn(*rest, generator=g).to(DEV)
    crit = lf.CRPSLoss()
    value, gx, gt = run(crit, x, t, dim=dim)
    v0, gx0, gt0 = run(crit, x.movedim(dim, 0).contiguous(), t, dim=0)
    assert value.shape == (shape[0],)
    assert torch.equal(value, v0) and torch.equal(gx.movedim(dim, 0), gx0) and torch.equal(gt, gt0)
    want = R.gauss_crps(_np(x.movedim(dim, 0)).reshape(1, shape[dim], -1), _np(t).reshape(1, -1), shape[0])
    ref32 = run(lambda a, b: torch_crps(a, b, dim=dim), x, t)
    check_all("crps_dim_in_place", f"{shape}_dim{dim}", [_np(value), _np(gx.movedim(dim, 0)), _np(gt)],
              [_np(ref32[0]), _np(ref32[1].movedim(dim, 0)), _np(ref32[2])], want)


def test_gradients_are_once_differentiable_and_only_what_is_asked(lf):
    g = torch.Generator().manual_seed(SEED + 3)
    x, t = torch.randn(4, 2, 1, 5, 7, generator=g).to(DEV), torch.randn(2, 1, 5, 7, generator=g).to(DEV)
    mask = torch.ones(7, device=DEV)
    for crit, args in ((lf.CRPSLoss(), ()), (lf.EnsembleVarRegLoss(), ()), (lf.MaskedLoss(_loss_fn("mse")), (mask,))):
        tt = t if isinstance(crit, lf.CRPSLoss) else torch.randn_like(x)
        xs = x.clone().requires_grad_()
        (gx,) = torch.autograd.grad(crit(xs, tt, *args).sum(), xs, create_graph=True)
        # a second derivative is refused, never computed from the saved gradient as if it were a constant: the
        # gradient comes back without a graph, or -- with an upstream gradient that carries one -- the node raises
        with pytest.raises(RuntimeError, match="once_differentiable|does not require grad"):
            gx.sum().backward()
        # the gradient of the target alone is the one of the full step
        full = run(crit, x, tt, *args)
        ts = tt.clone().requires_grad_()
        (gt,) = torch.autograd.grad(crit(x, ts, *args).sum(), ts)
        assert torch.equal(gt, full[2])


@pytest.mark.parametrize("b,s", [(6, 3000), (300, 20)])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_crps_non_finite_point_stays_in_its_sample(lf, b, s, bad):
    x, t = _crps_inputs(4, b, s, seed=5)
    crit = lf.CRPSLoss()
    clean = crit(x, t)
    k = b // 2
    xb = x.clone()
    xb[2, k, 0, 0, s - 1] = bad                          # the sample's last point: next to sample k + 1
    tb = t.clone()
    tb[k, 0, 0, 0] = bad                                 # ... and its first, in the target
    for xs, ts in ((xb, t), (x, tb)):
        got = crit(xs, ts)
        finite = torch.isfinite(got)
        if bad != bad or xs is xb:                       # (an infinite target is a cdf of 0 or 1: finite, 1/4 at most)
            assert not bool(finite[k])
        keep = torch.ones(b, dtype=torch.bool, device=DEV)
        keep[k] = False
        assert torch.equal(got[keep], clean[keep])


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_scalar_losses_turn_non_finite(lf, bad):
    g = torch.Generator().manual_seed(SEED)
    x, t = torch.randn(3, 5, 2000, generator=g).to(DEV), torch.randn(3, 5, 2000, generator=g).to(DEV)
    x[1, 2, 1777] = bad
    assert not bool(torch.isfinite(lf.EnsembleVarRegLoss()(x, t)))
    for kind in R.KINDS:
        assert not bool(torch.isfinite(lf.MaskedLoss(_loss_fn(kind))(x, t, torch.ones(2000, device=DEV))))


def _steps(lf):
    g = torch.Generator().manual_seed(SEED + 77)
    x5, t4 = torch.randn(5, 3, 2, 30, 41, generator=g).to(DEV), torch.randn(3, 2, 30, 41, generator=g).to(DEV)
    x3, t3 = torch.randn(3, 5, 4001, generator=g).to(DEV), torch.randn(3, 1, 4001, generator=g).to(DEV)
    tm = torch.randn(3, 5, 4001, generator=g).to(DEV)
    mask = torch.rand(4001, generator=g).to(DEV)
    crps, var, masked = lf.CRPSLoss(), lf.EnsembleVarRegLoss(0.2), lf.MaskedLoss(_loss_fn("mse"))
    return [(lambda x, t: crps(x, t), x5, t4), (var, x3, t3), (lambda x, t: masked(x, t, mask), x3, tm)]


def test_two_calls_and_a_replayed_hipgraph_give_the_same_bits(lf):
    for crit, x, t in _steps(lf):
        eager = run(crit, x, t)
        for a, b in zip(eager, run(crit, x, t)):
            assert torch.equal(a, b)
        xs, ts = x.clone().requires_grad_(), t.clone().requires_grad_()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                torch.autograd.grad(crit(xs, ts).sum(), (xs, ts))
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph):
            value = crit(xs, ts)
            gx, gt = torch.autograd.grad(value.sum(), (xs, ts))
        for _ in range(2):
            for out in (value, gx, gt):
                out.detach().fill_(float("nan"))
            gph.replay()
            torch.cuda.synchronize()
            for a, b in zip(eager, (value.detach(), gx, gt)):
                assert torch.equal(a, b)
        del gph


# ---- address range -------------------------------------------------------------------------------------------------------

def test_crps_forward_past_2_31_elements(lf):
    """M R = 2 * 4096 * 262 145 elements, 8.6 GB: every member plane is a block of S = 4096 points repeated (four whole
    tiles, so every sample is summed in the same order), the target likewise.  Every sample is bitwise the first, and
    the first matches fp64.  Member 1's plane lies past 2^32 bytes, its end past element 2^31."""
    L.start(DEV)
    m, s, b = 2, 4096, 262_145
    r = s * b
    assert m * r > L.ELEMS31 and m * r * 4 > 2 * L.BYTES32
    g = torch.Generator().manual_seed(SEED + 31)
    base, tb = torch.randn(m, s, generator=g).to(DEV), torch.randn(s, generator=g).to(DEV)
    pred = torch.empty(m, b, 1, 1, s, dtype=torch.float32, device=DEV)
    for i in range(m):
        pred[i].view(r, 1).copy_(L.periodic(base[i].view(s, 1), r))
    target = L.periodic(tb.view(s, 1), r).view(b, 1, 1, s)
    ptrs = L.nan_blocks(DEV, (b,))
    crit = lf.CRPSLoss()
    with torch.no_grad():
        loss = crit(pred, target)
    L.assert_fresh(ptrs, loss)
    assert loss.shape == (b,)
    small = crit(base.view(m, 1, 1, 1, s), tb.view(1, 1, 1, s))
    assert torch.equal(loss, small.expand(b)), int((loss != small).nonzero()[0])
    ref32 = torch_crps(base.view(m, 1, 1, 1, s), tb.view(1, 1, 1, s))
    want = R.gauss_crps(_np(base).reshape(1, m, s), _np(tb).reshape(1, s), 1)[0]
    ok, line = check("address_range", f"M{m}_B{b}_S{s}", "value", _np(loss[:1]), _np(ref32), want)
    assert ok, line
    with torch.no_grad():
        assert torch.equal(crit(pred, target), loss)
    assert torch.equal(pred[:, 0, 0, 0], base) and torch.equal(pred[:, -1, 0, 0], base)
    del pred, target, loss
    L.finish(DEV, "Gaussian CRPS")


# ---- end to end ----------------------------------------------------------------------------------------------------------

def test_forecaster_trains_on_crps_loss(lf, hip_lib):
    """InteractionForecaster, 64 channels, the nu = 10 mesh, 4 members: CRPSLoss of the [M, 1, 1, N, C] view
    backpropagates, and the parameter gradients are those of the torch composition on the device (the tolerance of
    tests/test_gpu_ensemble_losses.py::test_forecaster_crps_gradients_match_reference)."""
    import gwen_amd
    from gwen_amd.forecaster import InteractionForecaster
    mesh = gwen_amd.geodesic_mesh(10, reorder="hilbert")
    torch.manual_seed(SEED)
    model = InteractionForecaster(6, 64, 2).to(DEV)
    graphs = model.prepare(mesh, DEV)
    nf = mesh.faces.shape[0]
    x0 = torch.randn(nf, 6, device=DEV)
    xm = x0.unsqueeze(0) + 0.1 * torch.randn(4, nf, 6, device=DEV)
    y = torch.randn(nf, 6, device=DEV)
    crit = lf.CRPSLoss()
    out = model(xm, graphs)
    crit(out.view(4, 1, 1, nf, 6), y.view(1, 1, nf, 6)).sum().backward()
    got = {k: p.grad.clone() for k, p in model.named_parameters()}
    assert all(torch.isfinite(v).all() and float(v.abs().max()) > 0 for v in got.values())
    model.zero_grad()
    out = model(xm, graphs)
    torch_crps(out.view(4, 1, 1, nf, 6), y.view(1, 1, nf, 6)).sum().backward()
    for k, p in model.named_parameters():
        err = rel_err(got[k], p.grad)
        print(f"{k}: rel err {err:.2e}")
        assert err <= 1e-5, k
