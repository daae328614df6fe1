"""K6's fp32-class tier ("f16x3": gwen_mlp2_contract_f32 / gwen_mlp2_bwd_contract_f32 with GWEN_CONTRACT_F16X3) and its
plumbing through InteractionNet.precision and InteractionForecaster.set_precision, against the fp64 oracle
(oracle/interaction_oracle.py).  The default tier ("3xbf16") through the new entry point is gwen_mlp2_f32 bit for bit."""
import numpy as np
import pytest
import torch

from helpers import SEED, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 2e-6            # the fp32-class tier: forward
GRAD_TOL = 1e-5       # ... and its gradients


@pytest.fixture(scope="module")
def ga(hip_lib):
    import gwen_amd
    return gwen_amd


def _row_err(got, want) -> float:
    """the largest per-row max |got - want| / max |want| (a row of zeros: absolute)"""
    g, w = got.double().cpu(), want.double().cpu()
    scale = w.abs().amax(dim=1).clamp(min=1e-300)
    err = (g - w).abs().amax(dim=1)
    return float(torch.where(w.abs().amax(dim=1) > 0, err / scale, err).max())


def _want(a, w1, w2, b1, b2, act, tab1=None, idx1=None, tab2=None, idx2=None, res=None):
    from oracle import interaction_oracle as IO
    pre = a.double() @ w1.double().t()
    if tab1 is not None:
        pre = pre + (tab1.double()[idx1.long()] if idx1 is not None else tab1.double())
    if tab2 is not None:
        pre = pre + tab2.double()[idx2.long()]
    if b1 is not None:
        pre = pre + b1.double()
    y = IO.act_fn(act)(pre) @ w2.double().t()
    if b2 is not None:
        y = y + b2.double()
    return y if res is None else res.double() + y


def _raw_mlp2_f32(a, w1, w2, b2, g1, idx1, g2, idx2, b1, res, act):
    """gwen_mlp2_f32 itself (the pre-existing entry point), no graph"""
    from gwen_amd import _lib
    from gwen_amd.graph import _ptr, _stream
    from gwen_amd.interaction import _ACT
    L = _lib.lib()
    rows, f = a.shape
    out = torch.empty_like(a)
    nws = int(L.gwen_mlp2_workspace_bytes(f))
    ws = torch.empty(nws, dtype=torch.uint8, device=a.device) if nws > 0 else None
    rc = L.gwen_mlp2_f32(_ptr(a), _ptr(w1), _ptr(g1), _ptr(idx1), 0 if g1 is None else g1.size(0),
                         0 if g1 is None else g1.stride(0), _ptr(g2), _ptr(idx2), 0 if g2 is None else g2.size(0),
                         0 if g2 is None else g2.stride(0), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(res), _ptr(out), rows, f,
                         _ACT[act], None, None, 0, None, 0, 0, _ptr(ws), nws, _stream(a.device))
    _lib.check(rc, "gwen_mlp2_f32")
    return out


@pytest.mark.parametrize("tables", ["none", "g1", "g1g2"])
@pytest.mark.parametrize("act", ["none", "relu", "silu"])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("F", [32, 64, 128, 256])
def test_mlp2_f16x3_vs_oracle(ga, F, rows, act, tables):
    from gwen_amd.interaction import mlp2
    g = torch.Generator().manual_seed(SEED + 7 * F + rows)
    a = torch.randn(rows, F, generator=g)
    w1 = torch.randn(F, F, generator=g) / F ** 0.5
    w2 = torch.randn(F, F, generator=g) / F ** 0.5
    b1, b2 = torch.randn(F, generator=g), torch.randn(F, generator=g)
    t1, t2 = torch.randn(17, F, generator=g), torch.randn(29, F, generator=g)
    i1 = torch.randint(0, 17, (rows,), generator=g, dtype=torch.int32)
    i2 = torch.randint(0, 29, (rows,), generator=g, dtype=torch.int32)
    kw = {}
    if tables != "none":
        kw.update(g1=t1, idx1=i1)
    if tables == "g1g2":
        kw.update(g2=t2, idx2=i2)
    want = _want(a, w1, w2, b1, b2, act, kw.get("g1"), kw.get("idx1"), kw.get("g2"), kw.get("idx2"), res=a)
    dv = {k: v.to(DEV) for k, v in kw.items()}
    ad = a.to(DEV)
    args = (ad, w1.to(DEV), w2.to(DEV), b2.to(DEV))
    got, _ = mlp2(*args, b1=b1.to(DEV), res=ad, act=act, contract="f16x3", **dv)
    again, _ = mlp2(*args, b1=b1.to(DEV), res=ad, act=act, contract="f16x3", **dv)
    lo, _ = mlp2(*args, b1=b1.to(DEV), res=ad, act=act, contract="3xbf16", **dv)
    raw = _raw_mlp2_f32(*args, dv.get("g1"), dv.get("idx1"), dv.get("g2"), dv.get("idx2"), b1.to(DEV), ad, act)
    err, err_lo = rel_err(got, want), rel_err(lo, want)
    assert err <= TOL, (err, err_lo)
    assert torch.equal(got, again)
    assert torch.equal(lo, raw)                       # the default tier through the new entry point: the old bits
    if rows == 1000:
        assert err <= err_lo / 4, (err, err_lo)       # the new path really runs


def _graphs(ga):
    from gwen_amd import g2m
    from gwen_amd.mesh import complete_graph
    m = ga.geodesic_mesh(6)
    a, b = g2m.grid_mesh_edges(m)
    n, nf = m.num_nodes, m.faces.shape[0]
    return {
        "mesh": (n, n, torch.from_numpy(m.edge_index)),
        "g2m": (nf, n, torch.from_numpy(a)),
        "m2g": (n, nf, torch.from_numpy(b)),
        "K125": (125, 125, torch.from_numpy(complete_graph(125))),
        "empty": (5, 7, torch.zeros(2, 0, dtype=torch.long)),
        "one_edge": (3, 3, torch.tensor([[2], [1]])),
    }


def _net(F, act="silu", aggr="sum", precision="f16x3", seed=SEED):
    from gwen_amd.interaction import InteractionNet
    torch.manual_seed(seed)
    net = InteractionNet(F, act, aggr, precision=precision)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
    return net


@pytest.mark.parametrize("aggr", ["sum", "mean"])
@pytest.mark.parametrize("name", ["mesh", "g2m", "m2g", "K125", "empty", "one_edge"])
@pytest.mark.parametrize("F", [32, 64, 128, 256])
def test_block_f16x3_vs_oracle(ga, F, name, aggr):
    from gwen_amd.interaction import interaction_graph
    from oracle import interaction_oracle as IO
    ns, nd, ei = _graphs(ga)[name]
    net = _net(F, "silu", aggr)
    g = torch.Generator().manual_seed(SEED + 1)
    xs = torch.randn(ns, F, generator=g)
    xd = xs if name in ("mesh", "K125", "one_edge") else torch.randn(nd, F, generator=g)
    e = torch.randn(ei.size(1), F, generator=g)
    sd = {k: v.double() for k, v in net.state_dict().items()}
    want_x, want_e = IO.interaction(xs.double(), xd.double(), e.double(), ei, sd, "silu", aggr)
    graph = interaction_graph(ei.to(DEV), ns, nd)
    net = net.to(DEV)
    xs_d = xs.to(DEV)
    xd_d = xs_d if xd is xs else xd.to(DEV)
    with torch.no_grad():
        got_x, got_e = net(xs_d, xd_d, graph.sort_edges(e.to(DEV)), graph)
        again_x, again_e = net(xs_d, xd_d, graph.sort_edges(e.to(DEV)), graph)
    assert rel_err(got_x, want_x) <= TOL
    assert rel_err(graph.unsort_edges(got_e), want_e) <= TOL
    assert torch.equal(got_x, again_x) and torch.equal(got_e, again_e)


def _scaled_case(F, case, g):
    """(a, w1, w2, b1, b2, g1, idx1, g2, idx2, res, act) for one of the range cases"""
    rows = 300
    a = torch.randn(rows, F, generator=g)
    w1 = torch.randn(F, F, generator=g) / F ** 0.5
    w2 = torch.randn(F, F, generator=g) / F ** 0.5
    p2 = lambda k: torch.tensor(2.0, dtype=torch.float64) ** k                               # noqa: E731
    pick = lambda n, ks: torch.tensor(ks, dtype=torch.float64)[torch.randint(0, len(ks), (n,), generator=g)]  # noqa
    none = dict(b1=None, b2=None, g1=None, idx1=None, g2=None, idx2=None, res=None, act="silu")
    if case == "rows_2^60":                   # rows of magnitude 2^60, 2^-60 and 1 side by side; no biases
        a = (a.double() * p2(pick(rows, [60.0, -60.0, 0.0])).view(-1, 1)).float()
        return a, w1, w2, none
    if case == "wcols_2^40":                  # W output columns of magnitude 2^40, 2^-40 and 1
        w1 = (w1.double() * p2(pick(F, [40.0, -40.0, 0.0])).view(-1, 1)).float()
        w2 = (w2.double() * p2(pick(F, [40.0, -40.0, 0.0])).view(-1, 1)).float()
        return a, w1, w2, none
    t1, t2 = torch.randn(31, F, generator=g), torch.randn(37, F, generator=g)
    i1 = torch.randint(0, 31, (rows,), generator=g, dtype=torch.int32)
    i2 = torch.randint(0, 37, (rows,), generator=g, dtype=torch.int32)
    full = dict(b1=torch.randn(F, generator=g), b2=torch.randn(F, generator=g), g1=t1, idx1=i1, g2=t2, idx2=i2, res=a,
                act="silu")
    if case == "zero_rows":                   # every third row all zero (the addends and the residual remain)
        a[::3] = 0
        full["res"] = a
        return a, w1, w2, full
    if case in ("addend_2^40_larger", "addend_2^40_smaller"):
        s = p2(40.0 if case.endswith("larger") else -40.0)
        full.update(g1=(t1.double() * s).float(), g2=(t2.double() * s).float(), b1=None, b2=None, res=None)
        return a, w1, w2, full
    if case == "tiny_a_large_addend":         # A W1^T ~ 2^-120 below the addend (both scales large, addend ~1)
        a = (a.double() * p2(-100.0)).float()
        w1 = (w1.double() * p2(-20.0)).float()
        full.update(b2=None, res=None)
        return a, w1, w2, full
    if case == "silu_to_zero":                # pre ~ -12: SiLU's hidden rows ~ -7e-5, scaled by their own row scale
        # (not further out: the kernel's fp32 SiLU, x / (1 + 2^(-x log2 e)), loses ~|x| 2^-24 relative to the rounding of
        #  its argument -- 2.1e-6 at x = -30 on both tiers -- which is the activation's error, not the contraction's)
        a = a * 0.01
        return a, w1, w2, dict(none, b1=torch.full((F,), -12.0))
    raise ValueError(case)


CASES = ["rows_2^60", "wcols_2^40", "zero_rows", "addend_2^40_larger", "addend_2^40_smaller", "tiny_a_large_addend",
         "silu_to_zero"]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("F", [32, 64, 128, 256])
def test_mlp2_f16x3_range_per_row(ga, F, case):
    from gwen_amd.interaction import mlp2
    g = torch.Generator().manual_seed(SEED + F)
    a, w1, w2, kw = _scaled_case(F, case, g)
    want = _want(a, w1, w2, kw["b1"], kw["b2"], kw["act"], kw["g1"], kw["idx1"], kw["g2"], kw["idx2"], kw["res"])
    dv = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    if dv["res"] is not None:
        dv["res"] = a.to(DEV) if kw["res"] is a else dv["res"]
    got, _ = mlp2(a.to(DEV), w1.to(DEV), w2.to(DEV), dv.pop("b2"), contract="f16x3", **dv)
    assert torch.isfinite(got).all()
    assert _row_err(got, want) <= TOL


@pytest.mark.parametrize("F", [32, 64, 128, 256])
def test_mlp2_f16x3_non_finite_rows_stay_contained(ga, F):
    from gwen_amd.interaction import mlp2
    g = torch.Generator().manual_seed(SEED + 3 * F)
    rows = 200
    a = torch.randn(rows, F, generator=g)
    w1 = torch.randn(F, F, generator=g) / F ** 0.5
    w2 = torch.randn(F, F, generator=g) / F ** 0.5
    b1, b2 = torch.randn(F, generator=g), torch.randn(F, generator=g)
    bad = [0, 17, 64, 130, 199]
    a[0, 3], a[17, F - 1], a[64, 0], a[130, 5], a[199, 7] = float("inf"), float("-inf"), float("nan"), float("inf"), \
        float("nan")
    good = torch.ones(rows, dtype=torch.bool)
    good[bad] = False
    want = _want(a[good], w1, w2, b1, b2, "silu", res=a[good])
    got, _ = mlp2(a.to(DEV), w1.to(DEV), w2.to(DEV), b2.to(DEV), b1=b1.to(DEV), res=a.to(DEV), act="silu",
                  contract="f16x3")
    got = got.cpu()
    assert torch.isfinite(got[good]).all()
    assert _row_err(got[good], want) <= TOL
    assert not torch.isfinite(got[~good]).all(dim=1).any()          # a non-finite row does not come out finite


@pytest.mark.parametrize("F", [64, 256])
def test_members_bitwise_equal_to_single_launch(ga, F):
    """Per-row scales: a member of a block-diagonal batched launch is, bit for bit, the member launched alone."""
    from gwen_amd.interaction import interaction_graph
    members = 4
    m = ga.geodesic_mesh(20, reorder="hilbert")
    n = m.num_nodes
    graph = interaction_graph(torch.from_numpy(m.edge_index).to(DEV), n, n)
    gb = graph.batched(members)
    E = graph.num_edges
    net = _net(F).to(DEV)
    g = torch.Generator().manual_seed(SEED)
    xs = [torch.randn(n, F, generator=g).to(DEV) * (4.0 ** k) for k in range(members)]
    es = [torch.randn(E, F, generator=g).to(DEV) * (0.25 ** k) for k in range(members)]
    with torch.no_grad():
        xb = torch.cat(xs)
        bx, be = net(xb, xb, torch.cat(es), gb)
        for k in range(members):
            sx, se = net(xs[k], xs[k], es[k], graph)
            assert torch.equal(bx[k * n:(k + 1) * n], sx)
            assert torch.equal(be[k * E:(k + 1) * E], se)


@pytest.mark.parametrize("bip", [False, True])
@pytest.mark.parametrize("aggr", ["sum", "mean"])
@pytest.mark.parametrize("F", [32, 64, 128, 256])
def test_block_backward_f16x3_vs_oracle_autograd(ga, F, aggr, bip):
    from gwen_amd.interaction import interaction_graph
    from oracle import interaction_oracle as IO
    rng = np.random.default_rng(177 + F)
    ns, nd, e_ = (150, 210, 1300) if bip else (180, 180, 1100)
    src, dst = rng.integers(0, ns, size=e_), rng.integers(0, nd, size=e_)
    ei = torch.from_numpy(np.stack([src, dst]).astype(np.int64))
    net = _net(F, "silu", aggr, seed=SEED + F)
    g = torch.Generator().manual_seed(SEED)
    xs, xd, ef = torch.randn(ns, F, generator=g), torch.randn(nd, F, generator=g), torch.randn(e_, F, generator=g)
    gxo, geo = torch.randn(nd, F, generator=g), torch.randn(e_, F, generator=g)
    sd = {k: v.double().clone().requires_grad_() for k, v in net.state_dict().items()}
    xs64, xd64, ef64 = xs.double().requires_grad_(), xd.double().requires_grad_(), ef.double().requires_grad_()
    wx, we = IO.interaction(xd64 if not bip else xs64, xd64, ef64, ei, sd, "silu", aggr)
    (wx * gxo.double()).sum().add((we * geo.double()).sum()).backward()
    graph = interaction_graph(ei.to(DEV), ns, nd)
    net = net.to(DEV)
    xsd, xdd = xs.to(DEV).requires_grad_(), xd.to(DEV).requires_grad_()
    efd = graph.sort_edges(ef.to(DEV)).detach().requires_grad_()

    def run():
        for t in [xdd, efd, xsd] + list(net.parameters()):
            t.grad = None
        gx, ge = net(xdd if not bip else xsd, xdd, efd, graph)
        ((gx * gxo.to(DEV)).sum() + (ge * graph.sort_edges(geo.to(DEV))).sum()).backward()
        return gx.detach(), [t.grad.clone() for t in ([xdd, efd] + ([xsd] if bip else []) + list(net.parameters()))]

    gx, first = run()
    assert rel_err(gx, wx.detach()) <= TOL
    assert rel_err(xdd.grad, xd64.grad) <= GRAD_TOL
    if bip:
        assert rel_err(xsd.grad, xs64.grad) <= GRAD_TOL
    assert rel_err(graph.unsort_edges(efd.grad), ef64.grad) <= GRAD_TOL
    for k, p in net.named_parameters():
        assert rel_err(p.grad, sd[k].grad) <= GRAD_TOL, k
    _, again = run()
    assert all(torch.equal(a, b) for a, b in zip(first, again))


def _forecaster_case(ga, C, H, steps=2):
    from gwen_amd import g2m
    from gwen_amd.forecaster import InteractionForecaster, edge_features
    from oracle import interaction_oracle as IO
    m = ga.geodesic_mesh(5)
    torch.manual_seed(SEED + H)
    model = InteractionForecaster(C, H, steps)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
    a, b = g2m.grid_mesh_edges(m)
    cell = m.pos[m.faces].mean(axis=1)
    cell /= np.linalg.norm(cell, axis=1, keepdims=True)
    f = [torch.from_numpy(x).double() for x in (edge_features(cell, m.pos, a), edge_features(m.pos, m.pos, m.edge_index),
                                                 edge_features(m.pos, cell, b))]
    sd = {k: v.double() for k, v in model.state_dict().items()}
    x0 = torch.randn(m.faces.shape[0], C, generator=torch.Generator().manual_seed(SEED))
    want = IO.forecaster_step(sd, x0.double(), torch.from_numpy(m.pos.astype(np.float32)).double(), torch.from_numpy(a),
                              torch.from_numpy(m.edge_index), torch.from_numpy(b), *f, steps)
    return m, model, x0, want


@pytest.mark.parametrize("C,H", [(8, 64), (8, 256)])
def test_forecaster_f16x3_step_vs_oracle(ga, C, H):
    from gwen_amd.forecaster import InteractionForecaster
    m, model, x0, want = _forecaster_case(ga, C, H)
    graphs = InteractionForecaster.prepare(m, DEV)
    model = model.to(DEV)
    assert model.set_precision("f16x3") is model
    with torch.no_grad():
        got = model(x0.to(DEV), graphs)
        model.set_precision("3xbf16")
        lo = model(x0.to(DEV), graphs)
    err, err_lo = rel_err(got, want), rel_err(lo, want)
    assert err <= 1e-6, (err, err_lo)
    assert err <= err_lo / 3, (err, err_lo)


@pytest.mark.parametrize("precision", ["3xbf16", "f16x3"])
def test_forecaster_graphed_step_equals_eager(ga, precision):
    from gwen_amd.forecaster import GraphedStep, InteractionForecaster, ensemble_forecast
    m = ga.geodesic_mesh(5)
    torch.manual_seed(SEED)
    model = InteractionForecaster(8, 64, 2, precision=precision).to(DEV).eval()
    graphs = model.prepare(m, DEV)
    x = torch.randn(m.faces.shape[0], 8, device=DEV)
    with torch.no_grad():
        eager = model(x, graphs)
        step = GraphedStep(model, graphs, x)
        model.set_precision("f16x3" if precision == "3xbf16" else "3xbf16")    # capture time decides
        replayed = step(x).clone()
        model.set_precision(precision)
    assert torch.equal(replayed, eager)
    xm = torch.randn(3, m.faces.shape[0], 8, device=DEV)
    a = ensemble_forecast(model, graphs, xm, 2, 3, graphed=True)
    b = ensemble_forecast(model, graphs, xm, 2, 3, graphed=False)
    assert torch.equal(a, b)
