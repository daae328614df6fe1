"""Ensemble CRPS on the MI355X (gwen_ens_crps_f32 through gwen_amd.losses) against the fp64 pairwise reference."""
import numpy as np
import pytest
import torch

from ensemble_ref import crps_points, pair_coef, reference
from helpers import SEED, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ga(hip_lib):
    import gwen_amd
    return gwen_amd


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float(((a - b).abs() / b.abs().clamp_min(1e-30)).max())


def _check(ga, m, n, c, alpha, weighted, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, n, c, generator=g) * 0.7 + 0.3
    y = torch.randn(n, c, generator=g)
    w = torch.rand(n, generator=g) if weighted else None
    v = torch.rand(c, generator=g) + 0.1 if weighted else None
    xd = x.to(DEV).requires_grad_()
    yd = y.to(DEV).requires_grad_()
    loss = ga.ensemble_crps(xd, yd, None if w is None else w.to(DEV), None if v is None else v.to(DEV), alpha)
    loss.backward()
    sc = ga.ensemble_scores(x.to(DEV), y.to(DEV), None if w is None else w.to(DEV), alpha)
    xr, yr = x.double().requires_grad_(), y.double().requires_grad_()
    want, wsc = reference(xr, yr, w, v, alpha)
    want.backward()
    assert _rel(loss.detach(), want.detach()) <= 1e-5
    assert _rel(sc["crps"], wsc[0].detach()) <= 1e-5
    assert _rel(sc["rmse"], wsc[1].detach().sqrt()) <= 1e-5
    assert _rel(sc["spread"], wsc[2].detach().sqrt()) <= 1e-5
    assert rel_err(xd.grad, xr.grad) <= 2e-6
    assert rel_err(yd.grad, yr.grad) <= 2e-6


@pytest.mark.parametrize("m", [2, 3, 4, 5, 8, 16, 31, 32, 33, 64])
@pytest.mark.parametrize("c", [1, 3, 6, 64, 256])
def test_parity_members_by_channels(ga, m, c):
    n = {1: 2000, 3: 700, 6: 500, 64: 61, 256: 17}[c]
    _check(ga, m, n, c, 1.0, weighted=(m + c) % 2 == 0, seed=SEED + m * 1000 + c)


@pytest.mark.parametrize("m,n,c,alpha,weighted", [(4, 1, 8, 0.95, True), (5, 20000, 8, 0.0, True),
                                                    (32, 3001, 4, 0.95, False), (17, 257, 12, 0.0, True),
                                                    (9, 5000, 6, 0.95, True), (64, 100, 6, 0.0, False)])
def test_parity_sizes_and_alphas(ga, m, n, c, alpha, weighted):
    _check(ga, m, n, c, alpha, weighted, seed=SEED + n)


@pytest.mark.parametrize("m", [3, 8, 16, 32, 64])
@pytest.mark.parametrize("c", [4, 6])
def test_ties_match_autograd_with_sign_zero(ga, m, c):
    g = torch.Generator().manual_seed(m)
    q = lambda t: torch.clamp(torch.round(t * 2) / 2, -2, 2)                      # noqa: E731
    x, y = q(torch.randn(m, 300, c, generator=g)), q(torch.randn(300, c, generator=g))
    xd = x.to(DEV).requires_grad_()
    yd = y.to(DEV).requires_grad_()
    ga.ensemble_crps(xd, yd, alpha=0.95).backward()
    xr, yr = x.double().requires_grad_(), y.double().requires_grad_()
    reference(xr, yr, alpha=0.95)[0].backward()
    assert rel_err(xd.grad, xr.grad) <= 2e-6
    assert rel_err(yd.grad, yr.grad) <= 2e-6


@pytest.mark.parametrize("m", [4, 16, 32])
def test_no_cancellation_at_large_offsets(ga, m):
    g = torch.Generator().manual_seed(m)
    x = 1e4 + 0.01 * torch.randn(m, 2000, 8, generator=g)
    y = 1e4 + 0.01 * torch.randn(2000, 8, generator=g)
    sc = ga.ensemble_scores(x.to(DEV), y.to(DEV))
    want = crps_points(x.double(), y.double()).mean(0)                            # fp64 of the same fp32 inputs
    assert _rel(sc["crps"], want) <= 1e-5


def test_known_answers(ga):
    y = torch.randn(500, 8, device=DEV)
    x = y.unsqueeze(0).repeat(5, 1, 1).requires_grad_()
    loss = ga.ensemble_crps(x, y)
    loss.backward()
    assert float(loss.detach()) == 0.0 and torch.count_nonzero(x.grad) == 0
    # M = 2: fair CRPS = (|a - y| + |b - y|) / 2 - |a - b| / 2
    a, b, t = torch.randn(3, 300, 4, device=DEV).unbind(0)
    got = ga.ensemble_scores(torch.stack([a, b]), t)["crps"].double().cpu()
    want = (((a - t).abs() + (b - t).abs()) / 2 - (a - b).abs() / 2).double().mean(0).cpu()
    assert _rel(got, want) <= 1e-5
    # alpha = 0 with one member: the mean |x - y|; spread NaN
    sc = ga.ensemble_scores(a.unsqueeze(0), t, alpha=0.0)
    assert _rel(sc["crps"], (a - t).abs().double().mean(0)) <= 1e-5
    assert torch.isnan(sc["spread"]).all()
    # zero weights: NaN
    z = ga.ensemble_crps(torch.stack([a, b]), t, node_weights=torch.zeros(300, device=DEV))
    assert torch.isnan(z)


def test_bool_mask_weights(ga):
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(6, 400, 8, generator=g), torch.randn(400, 8, generator=g)
    mask = torch.rand(400, generator=g) > 0.5
    got = ga.ensemble_crps(x.to(DEV), y.to(DEV), node_weights=mask.to(DEV))
    want = ga.ensemble_crps(x[:, mask].to(DEV), y[mask].to(DEV))
    assert _rel(got, want.double()) <= 1e-5


def test_wrong_dtype_on_device(ga):
    with pytest.raises(TypeError):
        ga.ensemble_crps(torch.randn(4, 10, 8, device=DEV, dtype=torch.float64), torch.randn(10, 8, device=DEV))


@pytest.mark.parametrize("m,c", [(4, 8), (16, 6), (32, 8), (64, 3)])
def test_two_calls_are_bitwise_equal(ga, m, c):
    g = torch.Generator().manual_seed(m)
    x = torch.randn(m, 3000, c, generator=g).to(DEV)
    y = torch.randn(3000, c, generator=g).to(DEV)
    w = torch.rand(3000, generator=g).to(DEV)
    outs = []
    for _ in range(2):
        xd, yd = x.clone().requires_grad_(), y.clone().requires_grad_()
        loss = ga.ensemble_crps(xd, yd, w, alpha=0.95)
        loss.backward()
        sc = ga.ensemble_scores(x, y, w)
        outs.append((loss.detach(), sc["crps"], sc["rmse"], sc["spread"], xd.grad, yd.grad))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def _forecaster(ga):
    from gwen_amd.forecaster import InteractionForecaster
    m = ga.geodesic_mesh(4, reorder="hilbert")
    torch.manual_seed(SEED)
    model = InteractionForecaster(6, 32, 2).to(DEV)
    graphs = model.prepare(m, DEV)
    nf = m.faces.shape[0]
    x0 = torch.randn(nf, 6, device=DEV)
    xm = x0.unsqueeze(0) + 0.1 * torch.randn(4, nf, 6, device=DEV)
    y = torch.randn(nf, 6, device=DEV)
    return m, model, graphs, xm, y


def test_forecaster_members_backpropagate(ga):
    """The members axis of the forecaster trains: [4, N_grid, 6] through the block-diagonal graphs."""
    m, model, graphs, xm, y = _forecaster(ga)
    out = model(xm.clone().requires_grad_(), graphs)
    out.square().mean().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    # member i's gradient is that of member i alone
    model.zero_grad()
    xi = xm[1].clone().requires_grad_()
    model(xi, graphs).square().sum().backward()
    want = {k: p.grad.clone() for k, p in model.named_parameters()}
    model.zero_grad()
    xb = xm.clone()
    out = model(xb, graphs)
    (out[1].square().sum()).backward()
    for k, p in model.named_parameters():
        assert rel_err(p.grad, want[k]) <= 1e-4, k


def test_forecaster_crps_gradients_match_reference(ga):
    m, model, graphs, xm, y = _forecaster(ga)
    areas = torch.from_numpy(m.face_areas()).float()
    crit = ga.EnsembleCRPSLoss(node_weights=areas).to(DEV)
    out = model(xm, graphs)
    crit(out, y).backward()
    got = {k: p.grad.clone() for k, p in model.named_parameters()}
    model.zero_grad()
    out = model(xm, graphs)
    ref = reference(out, y, areas.to(DEV))[0]
    ref.float().backward()
    for k, p in model.named_parameters():
        assert rel_err(got[k], p.grad) <= 1e-5, k


def test_forecaster_crps_step_replays_from_a_hipgraph(ga):
    m, model, graphs, xm, y = _forecaster(ga)
    crit = ga.EnsembleCRPSLoss(node_weights=m.face_areas()).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=3e-3, fused=True, capturable=True)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = crit(model(xm, graphs), y)
        loss.backward()
        opt.step()
        return loss

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gph = torch.cuda.CUDAGraph()
    opt.zero_grad(set_to_none=True)
    with torch.cuda.graph(gph):
        loss = crit(model(xm, graphs), y)
        loss.backward()
        opt.step()
    gph.replay()
    torch.cuda.synchronize()
    first = float(loss.detach())
    for _ in range(20):
        gph.replay()
    torch.cuda.synchronize()
    assert float(loss.detach()) < first


def test_scores_of_ensemble_forecast(ga):
    from gwen_amd.forecaster import ensemble_forecast
    m, model, graphs, xm, y = _forecaster(ga)
    model.eval()
    out = ensemble_forecast(model, graphs, xm, 2, 4, gather=False)
    areas = torch.from_numpy(m.face_areas()).float()
    sc = ga.ensemble_scores(out, y, areas.to(DEV))
    _, want = reference(out.detach().cpu(), y.cpu(), areas)
    assert _rel(sc["crps"], want[0]) <= 1e-5
    assert _rel(sc["rmse"], want[1].sqrt()) <= 1e-5
    assert _rel(sc["spread"], want[2].sqrt()) <= 1e-5
