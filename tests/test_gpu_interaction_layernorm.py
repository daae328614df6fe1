"""The InteractionNet block with a LayerNorm behind both MLPs (``layer_norm=True``): K6 with LayerNorm fused (where
gwen_mlp2_ln_supported says an instantiation exists) and unfused (every other width, and forced), the row kernels of csrc/layernorm.hip, the block's backward and the forecaster,
against an fp64 restatement written HERE on top of oracle.interaction_oracle.mlp2 / act_fn and
torch.nn.functional.layer_norm -- never against the library."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from helpers import REL_TOL, SEED, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_TOL = {"3xbf16": REL_TOL, "f16x3": 2e-6}      # the tiers' forward bounds (the project's contract; f16x3's TOL)
GRAD_TOL = {"3xbf16": 1e-4, "f16x3": 1e-5}        # ... and their gradient bounds
TIERS = ["3xbf16", "f16x3"]
WIDTHS = [32, 64, 128, 256]


@pytest.fixture(scope="module")
def ga(hip_lib):
    import gwen_amd
    return gwen_amd


# ---- the fp64 restatement ---------------------------------------------------------------------------------------------
def ln64(m, gamma, beta, eps=1e-5):
    return TF.layer_norm(m, (m.size(-1),), gamma, beta, eps)


def block64(x_src, x_dst, e, ei, p, act="silu", aggr="sum", eps=1e-5, parts=False):
    """m_e = LN_edge(MLP_e([e, x_s, x_d])); agg = sum / mean; e' = e + m_e; x' = x + LN_node(MLP_n([x, agg]))"""
    from oracle import interaction_oracle as IO
    s, d = ei[0], ei[1]
    pre = IO.mlp2(torch.cat([e, x_src[s], x_dst[d]], dim=1), p["edge_mlp.0.weight"], p["edge_mlp.0.bias"],
                  p["edge_mlp.2.weight"], p["edge_mlp.2.bias"], act)
    m = ln64(pre, p["edge_norm.weight"], p["edge_norm.bias"], eps)
    agg = torch.zeros(x_dst.size(0), m.size(1), dtype=m.dtype).index_add_(0, d, m)
    if aggr == "mean":
        deg = torch.zeros(x_dst.size(0), dtype=m.dtype).index_add_(0, d, torch.ones(d.numel(), dtype=m.dtype))
        agg = agg / deg.clamp(min=1).view(-1, 1)
    y = IO.mlp2(torch.cat([x_dst, agg], dim=1), p["node_mlp.0.weight"], p["node_mlp.0.bias"], p["node_mlp.2.weight"],
                p["node_mlp.2.bias"], act)
    x_new = x_dst + ln64(y, p["node_norm.weight"], p["node_norm.bias"], eps)
    return (x_new, e + m, agg, pre) if parts else (x_new, e + m)


def forecaster64(sd, grid_x, mesh_pos, g2m, mesh_ei, m2g, f_g2m, f_mesh, f_m2g, steps, act="silu", aggr="sum"):
    sub = lambda prefix: {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}      # noqa: E731
    lin = lambda x, name: x @ sd[name + ".weight"].t() + sd[name + ".bias"]                       # noqa: E731
    vg, vm = lin(grid_x, "grid_embed"), lin(mesh_pos, "mesh_embed")
    e_g2m, e_m, e_m2g = lin(f_g2m, "g2m_edge_embed"), lin(f_mesh, "mesh_edge_embed"), lin(f_m2g, "m2g_edge_embed")
    vm, _ = block64(vg, vm, e_g2m, g2m, sub("encoder."), act, aggr)
    for k in range(steps):
        vm, e_m = block64(vm, vm, e_m, mesh_ei, sub(f"processor.{k}."), act, aggr)
    vg, _ = block64(vm, vg, e_m2g, m2g, sub("decoder."), act, aggr)
    return grid_x + lin(vg, "readout")


def _graphs(ga):                      # the six graphs of test_gpu_interaction_precision.py::_graphs
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


def _net(F, aggr="sum", precision="f16x3", seed=SEED, act="silu", plain_norm=False):
    """biases ~ 0.1 N(0,1), gamma ~ 1 + 0.1 N(0,1), beta ~ 0.1 N(0,1)"""
    from gwen_amd.interaction import InteractionNet
    torch.manual_seed(seed)
    net = InteractionNet(F, act, aggr, precision=precision, layer_norm=True)
    with torch.no_grad():
        for k, p in net.named_parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
                if k.endswith("norm.weight"):
                    p.add_(1.0)
        if plain_norm:
            for n in (net.edge_norm, net.node_norm):
                n.weight.fill_(1.0)
                n.bias.zero_()
    return net


def _inputs(name, ns, nd, ei, F, seed=SEED + 1):
    g = torch.Generator().manual_seed(seed)
    xs = torch.randn(ns, F, generator=g)
    xd = xs if name in ("mesh", "K125", "one_edge") else torch.randn(nd, F, generator=g)
    e = torch.randn(ei.size(1), F, generator=g)
    return xs, xd, e


def _row_err(got, want) -> float:
    """the largest per-row max |got - want| / max |want|"""
    g, w = got.double().cpu(), want.double().cpu()
    return float(((g - w).abs().amax(dim=1) / w.abs().amax(dim=1).clamp(min=1e-300)).max())


# ---- block forward ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aggr", ["sum", "mean"])
@pytest.mark.parametrize("name", ["mesh", "g2m", "m2g", "K125", "empty", "one_edge"])
@pytest.mark.parametrize("precision", TIERS)
@pytest.mark.parametrize("F", WIDTHS)
def test_block_forward_vs_fp64(ga, F, precision, name, aggr):
    from gwen_amd.interaction import interaction_graph
    ns, nd, ei = _graphs(ga)[name]
    net = _net(F, aggr, precision)
    xs, xd, e = _inputs(name, ns, nd, ei, F)
    sd = {k: v.double() for k, v in net.state_dict().items()}
    want_x, want_e = block64(xs.double(), xd.double(), e.double(), ei, sd, "silu", aggr)
    graph = interaction_graph(ei.to(DEV), ns, nd)
    net = net.to(DEV)
    xs_d = xs.to(DEV)
    xd_d = xs_d if xd is xs else xd.to(DEV)
    with torch.no_grad():
        got_x, got_e = net(xs_d, xd_d, graph.sort_edges(e.to(DEV)), graph)
        again_x, again_e = net(xs_d, xd_d, graph.sort_edges(e.to(DEV)), graph)
        only_x, none_e = net(xs_d, xd_d, graph.sort_edges(e.to(DEV)), graph, update_edges=False)
    ex, ee = rel_err(got_x, want_x), rel_err(graph.unsort_edges(got_e), want_e)
    print(json.dumps({"test": "block_forward", "F": F, "precision": precision, "graph": name, "aggr": aggr,
                      "err_x": ex, "err_e": ee}))
    assert ex <= FWD_TOL[precision]
    assert ee <= FWD_TOL[precision]
    assert torch.equal(got_x, again_x) and torch.equal(got_e, again_e)
    assert none_e is None and torch.equal(only_x, got_x)


# ---- the conditioning case: rows 1000 + N(0,1) --------------------------------------------------------------------------
@pytest.mark.parametrize("precision", TIERS)
@pytest.mark.parametrize("F", [64, 256])
def test_mlp2_layer_norm_rows_with_a_large_mean(ga, F, precision):
    """Pre-norm rows ~ 1000 + N(0,1): tells the deviations form of the variance from E[m^2] - mu^2.  The yardstick is the
    library's K6 WITHOUT LayerNorm on the same tier followed by torch's fp32 layer_norm on the device; the new result's
    per-row error against fp64 must be at most 4 x the yardstick's (a different summation order of <= 256 terms)."""
    from gwen_amd.interaction import mlp2
    from oracle import interaction_oracle as IO
    g = torch.Generator().manual_seed(SEED + F)
    rows = 1000
    a = torch.randn(rows, F, generator=g)
    w1 = torch.randn(F, F, generator=g) / F ** 0.5
    b1 = torch.randn(F, generator=g) * 0.1
    h = IO.act_fn("silu")(a.double() @ w1.double().t() + b1.double())
    w2 = torch.randn(F, F, generator=g)
    w2 = (w2.double() / (h @ w2.double().t()).std()).float()            # the row's spread is about 1
    b2 = torch.full((F,), 1000.0)
    gamma = 1 + 0.1 * torch.randn(F, generator=g)
    beta = 0.1 * torch.randn(F, generator=g)
    m64 = IO.mlp2(a.double(), w1.double(), b1.double(), w2.double(), b2.double(), "silu")
    assert 0.5 < float(m64.std(dim=1).mean()) < 2.0 and abs(float(m64.mean()) - 1000.0) < 1.0
    want = ln64(m64, gamma.double(), beta.double())
    d = lambda t: t.to(DEV)                                                                      # noqa: E731
    pre, _ = mlp2(d(a), d(w1), d(w2), d(b2), b1=d(b1), act="silu", contract=precision)
    yard = TF.layer_norm(pre, (F,), d(gamma), d(beta), 1e-5)
    got, _ = mlp2(d(a), d(w1), d(w2), d(b2), b1=d(b1), act="silu", contract=precision, ln_weight=d(gamma),
                  ln_bias=d(beta))
    err, err_yard = _row_err(got, want), _row_err(yard, want)
    print(json.dumps({"test": "conditioning", "F": F, "precision": precision, "route": "mlp2 (no block shape: unfused)",
                      "err": err, "err_yardstick": err_yard}))
    assert err <= 4 * err_yard, (err, err_yard)
    # the block's two launch shapes (the fused instantiations at these widths), same rows
    t1 = torch.zeros(rows, F)
    i1 = torch.arange(rows, dtype=torch.int32)
    res = torch.zeros(rows, F)                                         # (zero: out is LN(m) itself, nothing re-rounded)
    node, _ = mlp2(d(a), d(w1), d(w2), d(b2), g1=d(t1), b1=d(b1), res=d(res), act="silu", contract=precision,
                   ln_weight=d(gamma), ln_bias=d(beta))
    err_node = _row_err(node, want)
    from gwen_amd.interaction import interaction_graph
    ei = torch.stack([torch.arange(rows), torch.arange(rows)])
    graph = interaction_graph(ei.to(DEV), rows, rows)                  # one edge per target: stored order = edge order
    ad = d(a)
    edge, agg = mlp2(ad, d(w1), d(w2), d(b2), g1=d(t1), idx1=d(i1), g2=d(t1), idx2=d(i1), b1=d(b1), res=ad, act="silu",
                     graph=graph, contract=precision, ln_weight=d(gamma), ln_bias=d(beta))
    err_edge = _row_err(agg, want)
    print(json.dumps({"test": "conditioning", "F": F, "precision": precision, "route": "block shapes",
                      "err_node": err_node, "err_edge_agg": err_edge, "err_yardstick": err_yard}))
    assert err_edge <= 4 * err_yard, (err_edge, err_yard)           # (one edge per target: agg is LN(m) itself)
    assert err_node <= 4 * err_yard, (err_node, err_yard)
    assert rel_err(edge, a.double() + agg.double().cpu()) <= 1e-6     # e' = e + m: one fp32 rounding of the sum (2^-24)


# ---- closed forms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aggr", ["sum", "mean"])
@pytest.mark.parametrize("precision", TIERS)
@pytest.mark.parametrize("F", WIDTHS)
def test_zero_second_layer_gives_beta(ga, F, precision, aggr):
    """W2 = 0, b2 = 0.5 in every column: every pre-norm row is constant, so every message is exactly beta."""
    from gwen_amd.interaction import interaction_graph, mlp2
    ns, nd, ei = _graphs(ga)["g2m"]
    ei = ei[:, ei[1] != 3]                                    # target 3 loses its in-edges
    net = _net(F, aggr, precision)
    with torch.no_grad():
        net.edge_mlp[2].weight.zero_()
        net.edge_mlp[2].bias.fill_(0.5)
    net = net.to(DEV)
    graph = interaction_graph(ei.to(DEV), ns, nd)
    xs, xd, e = (t.to(DEV) for t in _inputs("g2m", ns, nd, ei, F))
    beta = net.edge_norm.bias.detach()
    with torch.no_grad():
        _, e_new = net(xs, xd, e, graph)
        p = net._weight_blocks()
        from gwen_amd import ops
        ps = ops.linear(xs, p[2][:F], None, exact=False)
        pd = ops.linear(xd, p[2][F:2 * F], p[3][F:2 * F], exact=False)
        _, agg = mlp2(e, p[0], net.edge_mlp[2].weight, net.edge_mlp[2].bias, g1=ps, idx1=graph.src, g2=pd,
                      idx2=graph.dst, res=e, act="silu", graph=graph, mean=aggr == "mean", contract=precision,
                      **net._ln("edge"))
    assert torch.equal(e_new, e + beta)
    deg = graph.degree()
    want = (deg if aggr == "sum" else (deg > 0).float()) * beta.view(1, -1)
    assert float(deg[3]) == 0 and torch.equal(agg[3], torch.zeros_like(agg[3]))      # no in-edges: 0, not beta
    assert float((agg - want).abs().max()) <= 1e-6


@pytest.mark.parametrize("precision", TIERS)
@pytest.mark.parametrize("F", WIDTHS)
def test_plain_norm_rows_have_mean_zero_and_the_stated_power(ga, F, precision):
    """gamma = 1, beta = 0: every row of e' - e has mean 0 and mean square var / (var + eps); agg = sum of e' - e."""
    from gwen_amd.interaction import interaction_graph, mlp2
    from gwen_amd import ops
    ns, nd, ei = _graphs(ga)["mesh"]
    net = _net(F, "sum", precision, plain_norm=True)
    xs, xd, e = _inputs("mesh", ns, nd, ei, F)
    sd = {k: v.double() for k, v in net.state_dict().items()}
    _, _, _, pre64 = block64(xs.double(), xs.double(), e.double(), ei, sd, parts=True)
    var = pre64.var(dim=1, unbiased=False)
    net = net.to(DEV)
    graph = interaction_graph(ei.to(DEV), ns, nd)
    xd_, ed_ = xs.to(DEV), graph.sort_edges(e.to(DEV))
    with torch.no_grad():
        p = net._weight_blocks()
        proj = ops.linear(xd_, p[2], p[3], exact=False) if precision == "3xbf16" else \
            ops.linear(xd_, p[2], p[3], contract=precision)
        e_new, agg = mlp2(ed_, p[0], net.edge_mlp[2].weight, net.edge_mlp[2].bias, g1=proj[:, :F], idx1=graph.src,
                          g2=proj[:, F:2 * F], idx2=graph.dst, res=ed_, act="silu", graph=graph, contract=precision,
                          **net._ln("edge"))
    m = graph.unsort_edges(e_new - ed_).double().cpu()
    assert float(m.mean(dim=1).abs().max()) <= 1e-4
    assert float((m.square().mean(dim=1) - var / (var + 1e-5)).abs().max()) <= 1e-3
    msg = (e_new - ed_).double().cpu()
    want = torch.zeros(nd, F, dtype=torch.float64).index_add_(0, graph.dst.long().cpu(), msg)
    assert rel_err(agg, want) <= 1e-6


# ---- routes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aggr", ["sum", "mean"])
@pytest.mark.parametrize("precision", TIERS)
@pytest.mark.parametrize("F", [64, 256])
def test_fused_and_unfused_routes_agree(ga, F, precision, aggr, monkeypatch):
    from gwen_amd import _lib, interaction
    code = interaction.MLP2_CONTRACTS[precision]
    fused = [bool(_lib.lib().gwen_mlp2_ln_supported(F, code, s)) for s in (_lib.MLP2_LN_EDGE, _lib.MLP2_LN_NODE)]
    if not any(fused):
        return                                        # this width ships the unfused route only: nothing to compare
    ns, nd, ei = _graphs(ga)["g2m"]
    net = _net(F, aggr, precision)
    xs, xd, e = _inputs("g2m", ns, nd, ei, F)
    sd = {k: v.double() for k, v in net.state_dict().items()}
    want_x, want_e = block64(xs.double(), xd.double(), e.double(), ei, sd, "silu", aggr)
    graph = interaction.interaction_graph(ei.to(DEV), ns, nd)
    net = net.to(DEV)
    args = (xs.to(DEV), xd.to(DEV), graph.sort_edges(e.to(DEV)), graph)
    with torch.no_grad():
        fx, fe = net(*args)
        monkeypatch.setattr(interaction, "_LN_FORCE_UNFUSED", True)
        ux, ue = net(*args)
    for got_x, got_e in ((fx, fe), (ux, ue)):
        assert rel_err(got_x, want_x) <= FWD_TOL[precision]
        assert rel_err(graph.unsort_edges(got_e), want_e) <= FWD_TOL[precision]
    if precision == "f16x3":
        assert rel_err(fx, ux) <= 2e-6 and rel_err(fe, ue) <= 2e-6


@pytest.mark.parametrize("precision", TIERS)
@pytest.mark.parametrize("F", WIDTHS)
def test_new_entry_without_layer_norm_is_the_old_entry(ga, F, precision):
    """mlp2 (which calls gwen_mlp2_ln_f32) with gamma = beta = None is gwen_mlp2_contract_f32 bit for bit."""
    from gwen_amd import _lib
    from gwen_amd.graph import _ptr, _stream
    from gwen_amd.interaction import _ACT, MLP2_CONTRACTS, interaction_graph, mlp2
    ns, nd, ei = _graphs(ga)["g2m"]
    graph = interaction_graph(ei.to(DEV), ns, nd)
    g = torch.Generator().manual_seed(SEED + F)
    rows = graph.num_edges
    a = torch.randn(rows, F, generator=g).to(DEV)
    w1, w2 = (torch.randn(F, F, generator=g) / F ** 0.5).to(DEV), (torch.randn(F, F, generator=g) / F ** 0.5).to(DEV)
    b1, b2 = torch.randn(F, generator=g).to(DEV), torch.randn(F, generator=g).to(DEV)
    t1, t2 = torch.randn(ns, F, generator=g).to(DEV), torch.randn(nd, F, generator=g).to(DEV)
    got, got_agg = mlp2(a, w1, w2, b2, g1=t1, idx1=graph.src, g2=t2, idx2=graph.dst, b1=b1, res=a, act="silu", graph=graph,
                        contract=precision)
    L = _lib.lib()
    code = MLP2_CONTRACTS[precision]
    out, agg = torch.empty_like(a), torch.empty(nd, F, device=DEV)
    tile_row, n_tiles = graph.tiles(int(L.gwen_mlp2_rows(F)))
    nws = int(L.gwen_mlp2_contract_workspace_bytes(F, code))
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV) if nws > 0 else None
    rc = L.gwen_mlp2_contract_f32(_ptr(a), _ptr(w1), _ptr(t1), _ptr(graph.src), ns, F, _ptr(t2), _ptr(graph.dst), nd, F,
                                  _ptr(b1), _ptr(w2), _ptr(b2), _ptr(a), _ptr(out), rows, F, _ACT["silu"],
                                  _ptr(graph.rowptr), _ptr(tile_row), n_tiles, _ptr(agg), nd, 0, code, _ptr(ws), nws,
                                  _stream(a.device))
    _lib.check(rc, "gwen_mlp2_contract_f32")
    assert torch.equal(got, out) and torch.equal(got_agg, agg)


def test_mlp2_refuses_a_wrong_dtype(ga):
    from gwen_amd.interaction import mlp2
    a, w = torch.zeros(4, 64, device=DEV), torch.zeros(64, 64, device=DEV)
    with pytest.raises(TypeError):
        mlp2(a, w, w, ln_weight=torch.ones(64, device=DEV, dtype=torch.float64), ln_bias=torch.zeros(64, device=DEV))
    with pytest.raises(RuntimeError):
        mlp2(a, w, w, ln_weight=torch.ones(64, device=DEV), ln_bias=torch.zeros(64))


# ---- members / capture ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", TIERS)
@pytest.mark.parametrize("F", [64, 256])
def test_members_bitwise_equal_to_single_launches(ga, F, precision):
    from gwen_amd.interaction import interaction_graph
    members = 3
    m = ga.geodesic_mesh(12, reorder="hilbert")
    n = m.num_nodes
    graph = interaction_graph(torch.from_numpy(m.edge_index).to(DEV), n, n)
    gb = graph.batched(members)
    E = graph.num_edges
    net = _net(F, "sum", precision).to(DEV)
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


@pytest.mark.parametrize("noise_channels", [0, 16])
@pytest.mark.parametrize("precision", TIERS)
def test_graphed_step_equals_eager(ga, precision, noise_channels):
    from gwen_amd import noise
    from gwen_amd.forecaster import GraphedStep, InteractionForecaster, ensemble_forecast
    m = ga.geodesic_mesh(5)
    torch.manual_seed(SEED)
    model = InteractionForecaster(8, 64, 2, precision=precision, noise_channels=noise_channels, layer_norm=True)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "norm" in k:
                p.add_(0.1 * torch.randn_like(p))
        if noise_channels:
            model.noise_embed.weight.normal_(0, 0.3)
    model = model.to(DEV).eval()
    graphs = model.prepare(m, DEV)
    x = torch.randn(m.faces.shape[0], 8, device=DEV)
    mk = (lambda: {"noise": noise.NoiseStream(SEED, DEV, draw=2)}) if noise_channels else (lambda: {})   # noqa: E731
    with torch.no_grad():
        eager = model(x, graphs, **mk())
        replayed = GraphedStep(model, graphs, x, **mk())(x).clone()
        plain = model(x, graphs)
    assert torch.equal(replayed, eager)
    assert bool(noise_channels) != torch.equal(plain, eager)            # the noise really is in the step
    xm = torch.randn(3, m.faces.shape[0], 8, device=DEV)
    a = ensemble_forecast(model, graphs, xm, 2, 3, graphed=True, **mk())
    b = ensemble_forecast(model, graphs, xm, 2, 3, graphed=False, **mk())
    c = torch.stack(model.rollout(xm[1], graphs, 2, graphed=True)[-1:])[0] if not noise_channels else None
    assert torch.equal(a, b)
    if c is not None:
        assert torch.equal(c, a[1])


# ---- non-finite containment -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", TIERS)
@pytest.mark.parametrize("F", WIDTHS)
def test_a_nan_edge_row_stays_with_its_edge_and_target(ga, F, precision):
    from gwen_amd.interaction import interaction_graph
    ns, nd, ei = _graphs(ga)["g2m"]
    net = _net(F, "sum", precision).to(DEV)
    graph = interaction_graph(ei.to(DEV), ns, nd)
    xs, xd, e = (t.to(DEV) for t in _inputs("g2m", ns, nd, ei, F))
    bad = 777
    e[bad, 5] = float("nan")
    tgt = int(graph.dst[bad])
    with torch.no_grad():
        x_new, e_new = net(xs, xd, e, graph)
    ok_e = torch.isfinite(e_new).all(dim=1)
    ok_x = torch.isfinite(x_new).all(dim=1)
    assert not ok_e[bad] and int((~ok_e).sum()) == 1
    assert not ok_x[tgt] and int((~ok_x).sum()) == 1


# ---- backward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge_out", [True, False])
@pytest.mark.parametrize("bip", [False, True])
@pytest.mark.parametrize("aggr", ["sum", "mean"])
@pytest.mark.parametrize("precision", TIERS)
@pytest.mark.parametrize("F", WIDTHS)
def test_block_backward_vs_fp64_autograd(ga, F, precision, aggr, bip, edge_out):
    from gwen_amd.interaction import interaction_graph
    rng = np.random.default_rng(177 + F)
    ns, nd, e_ = (150, 210, 1300) if bip else (180, 180, 1100)
    src, dst = rng.integers(0, ns, size=e_), rng.integers(0, nd, size=e_)
    ei = torch.from_numpy(np.stack([src, dst]).astype(np.int64))
    net = _net(F, aggr, precision, seed=SEED + F)
    g = torch.Generator().manual_seed(SEED)
    xs, xd, ef = torch.randn(ns, F, generator=g), torch.randn(nd, F, generator=g), torch.randn(e_, F, generator=g)
    gxo, geo = torch.randn(nd, F, generator=g), torch.randn(e_, F, generator=g)
    sd = {k: v.double().clone().requires_grad_() for k, v in net.state_dict().items()}
    assert len(sd) == 12
    xs64, xd64, ef64 = xs.double().requires_grad_(), xd.double().requires_grad_(), ef.double().requires_grad_()
    wx, we = block64(xd64 if not bip else xs64, xd64, ef64, ei, sd, "silu", aggr)
    loss = (wx * gxo.double()).sum()
    if edge_out:
        loss = loss + (we * geo.double()).sum()
    loss.backward()
    graph = interaction_graph(ei.to(DEV), ns, nd)
    net = net.to(DEV)
    xsd, xdd = xs.to(DEV).requires_grad_(), xd.to(DEV).requires_grad_()
    efd = graph.sort_edges(ef.to(DEV)).detach().requires_grad_()

    def run():
        for t in [xdd, efd, xsd] + list(net.parameters()):
            t.grad = None
        gx, ge = net(xdd if not bip else xsd, xdd, efd, graph, update_edges=edge_out)
        out = (gx * gxo.to(DEV)).sum()
        if edge_out:
            out = out + (ge * graph.sort_edges(geo.to(DEV))).sum()
        out.backward()
        return gx.detach(), [t.grad.clone() for t in ([xdd, efd] + ([xsd] if bip else []) + list(net.parameters()))]

    gx, first = run()
    tol = GRAD_TOL[precision]
    errs = {"x_dst": rel_err(xdd.grad, xd64.grad), "e": rel_err(graph.unsort_edges(efd.grad), ef64.grad)}
    if bip:
        errs["x_src"] = rel_err(xsd.grad, xs64.grad)
    for k, p in net.named_parameters():
        errs[k] = rel_err(p.grad, sd[k].grad)
    print(json.dumps({"test": "block_backward", "F": F, "precision": precision, "aggr": aggr, "bip": bip,
                      "edge_out": edge_out, "fwd": rel_err(gx, wx.detach()), "worst": max(errs.values())}))
    assert rel_err(gx, wx.detach()) <= FWD_TOL[precision]
    assert len(errs) == 12 + (3 if bip else 2)
    for k, v in errs.items():
        assert v <= tol, (k, v)
    _, again = run()
    assert all(torch.equal(a, b) for a, b in zip(first, again))


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("rows", [1, 63, 1000])
@pytest.mark.parametrize("F", [4, 36, 64, 256, 1000])
def test_layer_norm_op_vs_fp64(ga, F, rows, with_res):
    g = torch.Generator().manual_seed(SEED + F + rows)
    x = torch.randn(rows, F, generator=g) * 2 + 0.5
    gamma, beta = 1 + 0.1 * torch.randn(F, generator=g), 0.1 * torch.randn(F, generator=g)
    res = torch.randn(rows, F, generator=g) if with_res else None
    go = torch.randn(rows, F, generator=g)
    t64 = [t.double().requires_grad_() for t in (x, gamma, beta)] + ([res.double().requires_grad_()] if with_res else [])
    want = ln64(t64[0], t64[1], t64[2]) + (t64[3] if with_res else 0)
    (want * go.double()).sum().backward()
    td = [t.to(DEV).requires_grad_() for t in (x, gamma, beta)] + ([res.to(DEV).requires_grad_()] if with_res else [])

    def run():
        for t in td:
            t.grad = None
        out = ga.ops.layer_norm(td[0], td[1], td[2], 1e-5, td[3] if with_res else None)
        (out * go.to(DEV)).sum().backward()
        return [out.detach()] + [t.grad.clone() for t in td]

    first, again = run(), run()
    assert rel_err(first[0], want.detach()) <= 1e-6
    for got, t in zip(first[1:], t64):
        assert rel_err(got, t.grad) <= 1e-5
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    with torch.no_grad():
        assert torch.equal(ga.ops.layer_norm(td[0], td[1], td[2], 1e-5, td[3] if with_res else None), first[0])


def test_layer_norm_rows_per_target_sums(ga):
    """The row kernel's aggregate is of LN(x) -- not of out -- in stored order, mean or sum; empty targets get 0."""
    from gwen_amd import ops
    g = torch.Generator().manual_seed(SEED)
    F, deg = 128, [3, 0, 1, 130, 0, 7]
    rowptr = torch.tensor([0] + list(np.cumsum(deg)), dtype=torch.int32)
    rows = int(rowptr[-1])
    x, res = torch.randn(rows, F, generator=g), torch.randn(rows, F, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(F, generator=g), 0.1 * torch.randn(F, generator=g)
    y = ln64(x.double(), gamma.double(), beta.double())
    dst = torch.repeat_interleave(torch.arange(len(deg)), torch.tensor(deg))
    want = torch.zeros(len(deg), F, dtype=torch.float64).index_add_(0, dst, y)
    d = lambda t: t.to(DEV)                                                                      # noqa: E731
    for mean in (False, True):
        out, agg = ops.layer_norm_rows(d(x), d(gamma), d(beta), 1e-5, d(res), d(rowptr), len(deg), mean)
        w = want / torch.tensor(deg, dtype=torch.float64).clamp(min=1).view(-1, 1) if mean else want
        assert rel_err(out, res.double() + y) <= 1e-6 and rel_err(agg, w) <= 1e-6
        assert torch.equal(agg[1], torch.zeros(F, device=DEV)) and torch.equal(agg[4], torch.zeros(F, device=DEV))
        none, agg2 = ops.layer_norm_rows(d(x), d(gamma), d(beta), 1e-5, None, d(rowptr), len(deg), mean, want_out=False)
        assert none is None and torch.equal(agg2, agg)


# ---- forecaster -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", TIERS)
@pytest.mark.parametrize("H", [64, 256])
def test_forecaster_step_vs_fp64(ga, H, precision):
    from gwen_amd import g2m
    from gwen_amd.forecaster import InteractionForecaster, edge_features
    C, steps = 8, 2
    m = ga.geodesic_mesh(10)
    torch.manual_seed(SEED + H)
    model = InteractionForecaster(C, H, steps, precision=precision, layer_norm=True)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
                if k.endswith("norm.weight"):
                    p.add_(1.0)
    a, b = g2m.grid_mesh_edges(m)
    cell = m.pos[m.faces].mean(axis=1)
    cell /= np.linalg.norm(cell, axis=1, keepdims=True)
    f = [torch.from_numpy(x).double() for x in (edge_features(cell, m.pos, a), edge_features(m.pos, m.pos, m.edge_index),
                                                 edge_features(m.pos, cell, b))]
    sd = {k: v.double() for k, v in model.state_dict().items()}
    x0 = torch.randn(m.faces.shape[0], C, generator=torch.Generator().manual_seed(SEED))
    want = forecaster64(sd, x0.double(), torch.from_numpy(m.pos.astype(np.float32)).double(), torch.from_numpy(a),
                        torch.from_numpy(m.edge_index), torch.from_numpy(b), *f, steps)
    graphs = InteractionForecaster.prepare(m, DEV)
    model = model.to(DEV)
    with torch.no_grad():
        got = model(x0.to(DEV), graphs)
    err = rel_err(got, want)
    print(json.dumps({"test": "forecaster_step", "H": H, "precision": precision, "err": err}))
    assert err <= FWD_TOL[precision]


@pytest.mark.parametrize("H", [64, 256])
def test_forecaster_trains_with_crps(ga, H):
    from gwen_amd.forecaster import InteractionForecaster
    m = ga.geodesic_mesh(4, reorder="hilbert")
    torch.manual_seed(SEED)
    model = InteractionForecaster(6, H, 2, layer_norm=True).to(DEV)
    graphs = model.prepare(m, DEV)
    nf = m.faces.shape[0]
    xm = torch.randn(1, nf, 6, device=DEV) + 0.1 * torch.randn(4, nf, 6, device=DEV)
    y = torch.randn(nf, 6, device=DEV)
    crit = ga.EnsembleCRPSLoss(node_weights=m.face_areas()).to(DEV)
    out = model(model(xm, graphs), graphs)                    # two steps
    loss = crit(out, y)
    loss.backward()
    assert torch.isfinite(loss)
    names = [k for k, _ in model.named_parameters()]
    assert sum("norm" in k for k in names) == 4 * 4
    for k, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        if "norm" in k:
            assert float(p.grad.abs().max()) > 0, k
