"""Edge attention (csrc/attention.hip), the GraphTransformer block and the forecaster with processor="transformer" on
the GPU, against the fp64 restatement of tests/test_attention.py -- never against the library.  BUILD-DEFINED, PARITY
UNPINNED.

Bounds.  Bare op (tests 1-5): the error against fp64 must be at most max(floor, 4 x the error of the SAME restatement
evaluated in fp32 by torch on the CPU on the same inputs), floor = 2e-6 for the forward and 1e-5 for gradients (the
project's fp32-class bounds), both PER ROW (``row_err``: no row hides behind the tensor's largest one); only the gradients
of the large-logit case (test 3) use the whole-tensor ``helpers.rel_err``, the per-row measure being ill-conditioned on
saturated softmaxes.  Blocks and forecaster (tests 7-8): the tiers' contract -- forward 1e-4 / 2e-6, gradients 1e-4 / 1e-5
on "3xbf16" / "f16x3", whole-tensor rel_err.  Every case prints its figures as one JSON line before it asserts, and
appends it to the file named by GWEN_ATTENTION_ACCURACY when that is set (profiles/attention_accuracy.jsonl is such a
run's file)."""
import json
import os

import numpy as np
import pytest
import torch

from test_attention import (FWD_FLOOR, GRAD_FLOOR, YARD, attention_ref, block_ref, forecaster_ref, row_err)
from helpers import REL_TOL, SEED, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_TOL = {"3xbf16": REL_TOL, "f16x3": 2e-6}
GRAD_TOL = {"3xbf16": 1e-4, "f16x3": 1e-5}
TIERS = ["3xbf16", "f16x3"]
NAMES = ["mesh", "g2m", "m2g", "K125", "empty", "one_edge"]
FH = [(32, 8), (64, 4), (64, 16), (128, 8), (256, 8), (256, 1)]          # D / 4 = 1, 4, 1, 4, 8 and 64 lanes a head


@pytest.fixture(scope="module")
def ga(hip_lib):
    import gwen_amd
    return gwen_amd


_CACHE = {}


def _graph(ga, name):
    """(num_src, num_dst, edge_index on the CPU, EdgeGraph) of one of the six graphs of
    test_gpu_interaction_layernorm.py::_graphs, built once"""
    if not _CACHE:
        from gwen_amd import g2m
        from gwen_amd.interaction import interaction_graph
        from gwen_amd.mesh import complete_graph
        m = ga.geodesic_mesh(6)
        a, b = g2m.grid_mesh_edges(m)
        n, nf = m.num_nodes, m.faces.shape[0]
        raw = {"mesh": (n, n, torch.from_numpy(m.edge_index)), "g2m": (nf, n, torch.from_numpy(a)),
               "m2g": (n, nf, torch.from_numpy(b)), "K125": (125, 125, torch.from_numpy(complete_graph(125))),
               "empty": (5, 7, torch.zeros(2, 0, dtype=torch.long)), "one_edge": (3, 3, torch.tensor([[2], [1]]))}
        # m2g restricted: targets 1 mod 3 lose their in-edges, targets 0 mod 3 keep ONE, sources 0 mod 5 lose their out-edges
        s, d = raw["m2g"][2]
        first = torch.ones_like(d, dtype=torch.bool)
        order = torch.sort(d, stable=True).indices
        first[order[1:]] = d[order[1:]] != d[order[:-1]]
        keep = (s % 5 != 0) & ((d % 3 == 2) | ((d % 3 == 0) & first))
        raw["m2g_cut"] = (n, nf, raw["m2g"][2][:, keep].contiguous())
        for k, (ns, nd, ei) in raw.items():
            _CACHE[k] = (ns, nd, ei, interaction_graph(ei.to(DEV), ns, nd))
    return _CACHE[name]


def _inputs(ns, nd, e, F, seed=SEED + 1, q_scale=1.0):
    g = torch.Generator().manual_seed(seed + F)
    return (q_scale * torch.randn(nd, F, generator=g), torch.randn(ns, F, generator=g), torch.randn(ns, F, generator=g),
            torch.randn(e, F, generator=g), torch.randn(nd, F, generator=g))


def _log(**kw):
    line = json.dumps({"test": "attention_" + kw.pop("test"), **kw})
    print(line)
    if os.environ.get("GWEN_ATTENTION_ACCURACY"):
        with open(os.environ["GWEN_ATTENTION_ACCURACY"], "a") as fh:
            fh.write(line + "\n")


def _bound(err, yard, floor, what):
    assert err <= max(floor, YARD * yard), (what, err, yard)


def _ref_forward(q, k, v, ei, H, ee):
    want = attention_ref(q.double(), k.double(), v.double(), ei[0], ei[1], H, None if ee is None else ee.double())
    return want, attention_ref(q, k, v, ei[0], ei[1], H, ee)


def _ref_backward(q, k, v, ei, H, ee, w, dtype):
    """gradients of sum(out * w) in ``dtype`` on the CPU: (gq, gk, gv, gee or None)"""
    ts = [t.to(dtype).clone().requires_grad_(True) for t in (q, k, v)] + \
        ([] if ee is None else [ee.to(dtype).clone().requires_grad_(True)])
    out = attention_ref(ts[0], ts[1], ts[2], ei[0], ei[1], H, None if ee is None else ts[3])
    (out * w.to(dtype)).sum().backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad                   # noqa: E731  (no edges: no graph)
    return [zero(t) for t in ts] + ([None] if ee is None else [])


def _gpu_backward(ga, graph, q, k, v, H, ee, w, stacked=False):
    """(out, gq, gk, gv, gee in EDGE_INDEX order or None) of the library; ``stacked``: through edge_attention_kv"""
    d = lambda t: t.to(DEV).clone().requires_grad_(True)                                  # noqa: E731
    qd = d(q)
    eed = None if ee is None else graph.sort_edges(ee.to(DEV)).clone().requires_grad_(True)
    if stacked:
        kv = d(torch.cat([k, v], dim=1))
        out = ga.edge_attention_kv(qd, kv, graph, H, eed)
    else:
        kd, vd = d(k), d(v)
        out = ga.edge_attention(qd, kd, vd, graph, H, eed)
    (out * w.to(DEV)).sum().backward()
    F = q.size(1)
    gk, gv = (kv.grad[:, :F], kv.grad[:, F:]) if stacked else (kd.grad, vd.grad)
    return out.detach(), qd.grad, gk, gv, None if ee is None else graph.unsort_edges(eed.grad)


# ---- 1. forward -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_ee", [False, True])
@pytest.mark.parametrize("F,H", FH)
@pytest.mark.parametrize("name", NAMES)
def test_forward_vs_fp64(ga, name, F, H, with_ee):
    ns, nd, ei, graph = _graph(ga, name)
    q, k, v, ee, _ = _inputs(ns, nd, ei.size(1), F)
    ee = ee if with_ee else None
    want, yard = _ref_forward(q, k, v, ei, H, ee)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    eed = None if ee is None else graph.sort_edges(ee.to(DEV))
    with torch.no_grad():
        got = ga.edge_attention(qd, kd, vd, graph, H, eed)
        kv = torch.cat([kd, vd], dim=1)
        wide = torch.cat([torch.full_like(qd, 7.0), qd, torch.full_like(qd, -7.0)], dim=1)     # q as a column block too
        blocks = ga.edge_attention(wide[:, F:2 * F], kv[:, :F], kv[:, F:], graph, H, eed)
        stacked = ga.edge_attention_kv(qd, kv, graph, H, eed)
    assert got.shape == (nd, F) and torch.equal(got, blocks) and torch.equal(got, stacked)
    err, err_y = row_err(got, want), row_err(yard, want)
    _log(test="forward", graph=name, F=F, H=H, ee=with_ee, err_gpu=err, err_cpu_fp32=err_y)
    _bound(err, err_y, FWD_FLOOR, "out")


def test_argument_errors(ga):
    ns, nd, ei, graph = _graph(ga, "g2m")
    q, k, v, ee, _ = (t.to(DEV) for t in _inputs(ns, nd, ei.size(1), 64))
    with pytest.raises(ValueError):
        ga.edge_attention(q, k, v, graph, 3)
    with pytest.raises(ValueError):
        ga.edge_attention(q, k[:-1], v, graph, 4)
    with pytest.raises(ValueError):
        ga.edge_attention(q, k, v, graph, 4, ee[:-1])
    with pytest.raises(ValueError):
        ga.edge_attention(q, torch.cat([k, v], 1)[:, 2:66], v, graph, 4)              # rows not 16-byte aligned
    with pytest.raises(ValueError):
        ga.edge_attention(q, k.t().contiguous().t(), v, graph, 4, ee)                 # column stride != 1
    pad = torch.cat([ee.reshape(-1), ee.new_zeros(4)])
    with pytest.raises(ValueError):
        ga.edge_attention(q, k, v, graph, 4, pad[2:2 + ee.numel()].view_as(ee))     # ee not 16-byte aligned
    with pytest.raises(TypeError):
        ga.edge_attention(q, k.double(), v, graph, 4)
    with pytest.raises(RuntimeError):
        ga.edge_attention(q, k.cpu(), v, graph, 4)


# ---- 2. closed forms on the device ------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,H", [(32, 8), (256, 1)])
@pytest.mark.parametrize("name", NAMES + ["m2g_cut"])
def test_zero_keys_give_the_in_edge_mean(ga, name, F, H):
    ns, nd, ei, graph = _graph(ga, name)
    q, _, v, _, _ = _inputs(ns, nd, ei.size(1), F)
    k = torch.zeros(ns, F)
    deg = torch.zeros(nd, dtype=torch.float64).index_add_(0, ei[1], torch.ones(ei.size(1), dtype=torch.float64))
    mean = torch.zeros(nd, F, dtype=torch.float64).index_add_(0, ei[1], v.double()[ei[0]]) / deg.clamp(min=1).view(-1, 1)
    yard = attention_ref(q, k, v, ei[0], ei[1], H)
    with torch.no_grad():
        got = ga.edge_attention(q.to(DEV), k.to(DEV), v.to(DEV), graph, H)
    err, err_y = row_err(got, mean), row_err(yard, mean)
    _log(test="zero_keys", graph=name, F=F, H=H, err_gpu=err, err_cpu_fp32=err_y)
    _bound(err, err_y, FWD_FLOOR, "mean of v")


@pytest.mark.parametrize("F,H", [(32, 8), (64, 4), (256, 1)])
@pytest.mark.parametrize("name", ["one_edge", "m2g_cut", "empty"])
def test_degree_one_and_degree_zero_are_exact(ga, name, F, H):
    """one in-edge: p is exactly 1, out bitwise v[s] + ee[e]; no in-edge: out and gq exactly 0; a source without
    out-edges: gk = gv = 0 exactly"""
    ns, nd, ei, graph = _graph(ga, name)
    q, k, v, ee, w = _inputs(ns, nd, ei.size(1), F)
    out, gq, gk, gv, gee = _gpu_backward(ga, graph, q, k, v, H, ee, w)
    deg = torch.bincount(ei[1], minlength=nd)
    outdeg = torch.bincount(ei[0], minlength=ns)
    one = (deg[ei[1]] == 1).nonzero().view(-1)                      # the edges into degree-1 targets
    if name != "empty":
        assert one.numel() > 0
    assert torch.equal(out.cpu()[ei[1][one]], v[ei[0][one]] + ee[one])
    none = deg == 0
    assert name == "one_edge" or int(none.sum()) > 0
    assert float(out.cpu()[none].abs().max()) == 0.0 and float(gq.cpu()[none].abs().max()) == 0.0
    lone = outdeg == 0
    assert int(lone.sum()) > 0
    assert float(gk.cpu()[lone].abs().max()) == 0.0 and float(gv.cpu()[lone].abs().max()) == 0.0
    assert all(bool(torch.isfinite(t).all()) for t in (out, gq, gk, gv, gee))


# ---- 3. large logits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,H", [(64, 4), (256, 8)])
@pytest.mark.parametrize("name", ["mesh", "g2m", "K125"])
def test_large_logits(ga, name, F, H):
    """q = 30 N(0,1): logits of +-200 .. +-300, past expf's overflow at 88.7"""
    ns, nd, ei, graph = _graph(ga, name)
    q, k, v, ee, w = _inputs(ns, nd, ei.size(1), F, q_scale=30.0)
    want, sc, _ = attention_ref(q.double(), k.double(), v.double(), ei[0], ei[1], H, ee.double(), parts=True)
    assert float(sc.abs().max()) > 150.0
    yard = attention_ref(q, k, v, ei[0], ei[1], H, ee)
    out, *grads = _gpu_backward(ga, graph, q, k, v, H, ee, w)
    assert all(bool(torch.isfinite(t).all()) for t in (out, *grads))
    err, err_y = row_err(out, want), row_err(yard, want)
    _log(test="large_logits_forward", graph=name, F=F, H=H, max_logit=float(sc.abs().max()), err_gpu=err,
         err_cpu_fp32=err_y)
    _bound(err, err_y, FWD_FLOOR, "out")
    g64 = _ref_backward(q, k, v, ei, H, ee, w, torch.float64)
    g32 = _ref_backward(q, k, v, ei, H, ee, w, torch.float32)
    for what, got, w64, w32 in zip(("gq", "gk", "gv", "gee"), grads, g64, g32):
        err, err_y = rel_err(got, w64), rel_err(w32, w64)
        _log(test="large_logits_grad", graph=name, F=F, H=H, grad=what, err_gpu=err, err_cpu_fp32=err_y)
        _bound(err, err_y, GRAD_FLOOR, what)


# ---- 4. the running maximum ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,H", [(32, 1), (64, 1), (256, 1)])
@pytest.mark.parametrize("where", ["first", "last", "equal"])
def test_running_maximum_rescales(ga, where, F, H):
    """One target with 9 in-edges (an odd count: the pair loop's tail), H = 1 so that the row has ONE largest logit:
    the same edges permuted so that the largest is the FIRST stored edge (every later edge is scaled down against it), the
    LAST (every earlier partial sum is rescaled at the end), or all logits equal.  Logits in the tens."""
    from gwen_amd.interaction import interaction_graph
    n = 9
    q, k, v, ee, _ = _inputs(n, 2, n, F, seed=SEED + 7, q_scale=10.0)
    if where == "equal":
        k = k[:1].expand(n, F).contiguous()
        ee = ee[:1].expand(n, F).contiguous()
    sc = attention_ref(q.double(), k.double(), v.double(), torch.arange(n), torch.zeros(n, dtype=torch.long), H,
                       ee.double(), parts=True)[1][:, 0]
    top = int(sc.argmax())
    rest = [i for i in range(n) if i != top]
    perm = torch.tensor({"first": [top] + rest, "last": rest + [top], "equal": list(range(n))}[where])
    ei = torch.stack([perm, torch.zeros(n, dtype=torch.long)])             # edge j: source perm[j], edge term ee[perm[j]]
    eo = ee[perm]
    graph = interaction_graph(ei.to(DEV), n, 2)
    stored = graph.src.cpu().long()
    if where == "first":
        assert int(stored[0]) == top
    elif where == "last":
        assert int(stored[-1]) == top
    else:
        assert float(sc.max() - sc.min()) == 0.0
    want, yard = _ref_forward(q, k, v, ei, H, eo)
    with torch.no_grad():
        got = ga.edge_attention(q.to(DEV), k.to(DEV), v.to(DEV), graph, H, graph.sort_edges(eo.to(DEV)))
    err, err_y = row_err(got, want), row_err(yard, want)
    _log(test="running_max", where=where, F=F, H=H, spread=float(sc.max() - sc.min()), err_gpu=err, err_cpu_fp32=err_y)
    _bound(err, err_y, FWD_FLOOR, "out")
    assert float(got[1].abs().max()) == 0.0


# ---- 5. backward --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_ee", [False, True])
@pytest.mark.parametrize("F,H", [(32, 8), (64, 4), (256, 8)])
@pytest.mark.parametrize("name", NAMES)
def test_backward_vs_fp64_autograd(ga, name, F, H, with_ee):
    ns, nd, ei, graph = _graph(ga, name)
    q, k, v, ee, w = _inputs(ns, nd, ei.size(1), F)
    ee = ee if with_ee else None
    g64 = _ref_backward(q, k, v, ei, H, ee, w, torch.float64)
    g32 = _ref_backward(q, k, v, ei, H, ee, w, torch.float32)
    out, *grads = _gpu_backward(ga, graph, q, k, v, H, ee, w)
    out2, *grads2 = _gpu_backward(ga, graph, q, k, v, H, ee, w, stacked=True)      # gk | gv in ONE [Ns, 2F] array
    assert torch.equal(out, out2)
    for what, got, got2, w64, w32 in zip(("gq", "gk", "gv", "gee"), grads, grads2, g64, g32):
        if w64 is None:
            assert got is None and got2 is None
            continue
        assert got.shape == w64.shape and torch.equal(got, got2), what
        err, err_y = row_err(got, w64), row_err(w32, w64)
        _log(test="backward", graph=name, F=F, H=H, ee=with_ee, grad=what, err_gpu=err, err_cpu_fp32=err_y)
        _bound(err, err_y, GRAD_FLOOR, what)


# ---- 6. determinism and batching ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,H", [(64, 4), (256, 8)])
def test_batched_members_are_bitwise_the_members_alone(ga, F, H):
    ns, nd, ei, graph = _graph(ga, "mesh")
    members = 4
    gb = graph.batched(members)
    ins = [_inputs(ns, nd, ei.size(1), F, seed=SEED + 10 * m) for m in range(members)]
    alone = [_gpu_backward(ga, graph, q, k, v, H, ee, w) for q, k, v, ee, w in ins]
    again = _gpu_backward(ga, graph, *ins[1][:3], H, *ins[1][3:])
    assert all(torch.equal(a, b) for a, b in zip(alone[1], again))                  # two runs: bitwise equal
    cat = [torch.cat([m[i] for m in ins], dim=0) for i in range(5)]
    # (stored order of the batched graph = the members' stored orders one after the other)
    d = lambda t: t.to(DEV).clone().requires_grad_(True)                                  # noqa: E731
    qd, kd, vd = d(cat[0]), d(cat[1]), d(cat[2])
    eed = torch.cat([graph.sort_edges(m[3].to(DEV)) for m in ins], dim=0).requires_grad_(True)
    out = ga.edge_attention(qd, kd, vd, gb, H, eed)
    (out * cat[4].to(DEV)).sum().backward()
    e = ei.size(1)
    for m in range(members):
        o, gq, gk, gv, gee = alone[m]
        assert torch.equal(out[m * nd:(m + 1) * nd], o)
        assert torch.equal(qd.grad[m * nd:(m + 1) * nd], gq)
        assert torch.equal(kd.grad[m * ns:(m + 1) * ns], gk) and torch.equal(vd.grad[m * ns:(m + 1) * ns], gv)
        assert torch.equal(graph.unsort_edges(eed.grad[m * e:(m + 1) * e]), gee)


# ---- 7. the block ---------------------------------------------------------------------------------------------------------
def _block(F, heads, precision, seed=SEED):
    from gwen_amd import GraphTransformer
    torch.manual_seed(seed)
    net = GraphTransformer(F, heads, precision=precision)
    with torch.no_grad():
        for k, p in net.named_parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
                if k in ("norm1.weight", "norm2.weight"):
                    p.add_(1.0)
    return net


@pytest.mark.parametrize("precision", TIERS)
@pytest.mark.parametrize("F", [64, 256])
@pytest.mark.parametrize("name", ["mesh", "g2m", "K125"])
def test_block_forward_and_gradients_vs_fp64(ga, name, F, precision):
    heads = 8
    ns, nd, ei, graph = _graph(ga, name)
    same = ns == nd
    net = _block(F, heads, precision)
    g = torch.Generator().manual_seed(SEED + 3)
    xs = torch.randn(ns, F, generator=g)
    xd = xs if same else torch.randn(nd, F, generator=g)
    e = torch.randn(ei.size(1), F, generator=g)
    w = torch.randn(nd, F, generator=g)
    # fp64
    p64 = {k: v.double().clone().requires_grad_(True) for k, v in net.state_dict().items()}
    xs64 = xs.double().requires_grad_(True)
    xd64 = xs64 if same else xd.double().requires_grad_(True)
    e64 = e.double().requires_grad_(True)
    want = block_ref(xs64, xd64, e64, ei[0], ei[1], p64, heads, same=same)
    (want * w.double()).sum().backward()
    # library
    net = net.to(DEV)
    xsd = xs.to(DEV).requires_grad_(True)
    xdd = xsd if same else xd.to(DEV).requires_grad_(True)
    ed = graph.sort_edges(e.to(DEV)).requires_grad_(True)
    got, e_back = net(xsd, xdd, ed, graph)
    assert e_back is ed
    (got * w.to(DEV)).sum().backward()
    with torch.no_grad():
        plain, _ = net(xsd.detach(), xdd.detach(), ed.detach(), graph, update_edges=False)      # the one-launch feed-forward
        pre, _ = net(xsd.detach(), xdd.detach(), ed.detach(), graph, ee=net.edge_term(ed.detach()))
    assert torch.equal(plain, pre)                                  # ee= precomputed: the inline path, bitwise
    want = want.detach()
    errs = {"x_train": rel_err(got.detach(), want), "x_eval": rel_err(plain, want)}
    gerrs = {"x_src": rel_err(xsd.grad, xs64.grad), "e": rel_err(graph.unsort_edges(ed.grad), e64.grad)}
    if not same:
        gerrs["x_dst"] = rel_err(xdd.grad, xd64.grad)
    for k, p in net.named_parameters():
        assert p.grad is not None, k
        gerrs[k] = rel_err(p.grad, p64[k].grad)
    _log(test="block", graph=name, F=F, precision=precision, **errs, grad_max=max(gerrs.values()),
         grad_worst=max(gerrs, key=gerrs.get))
    for k, v in errs.items():
        assert v <= FWD_TOL[precision], (k, v)
    for k, v in gerrs.items():
        assert v <= GRAD_TOL[precision], (k, v)


# ---- 8. the forecaster ------------------------------------------------------------------------------------------------------
def _forecaster(ga, precision="3xbf16", noise_channels=0):
    from gwen_amd.forecaster import InteractionForecaster
    torch.manual_seed(SEED + 64)
    model = InteractionForecaster(8, 64, 2, precision=precision, processor="transformer", heads=4,
                                  noise_channels=noise_channels)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
                if k.endswith(("norm1.weight", "norm2.weight")):
                    p.add_(1.0)
        if noise_channels:
            model.noise_embed.weight.normal_(0, 0.1)
    return model


def _forecaster_fp64_inputs(ga, m):
    from gwen_amd import g2m
    from gwen_amd.forecaster import edge_features
    a, b = g2m.grid_mesh_edges(m)
    cell = m.pos[m.faces].mean(axis=1)
    cell /= np.linalg.norm(cell, axis=1, keepdims=True)
    f = [torch.from_numpy(x).double() for x in (edge_features(cell, m.pos, a), edge_features(m.pos, m.pos, m.edge_index),
                                                 edge_features(m.pos, cell, b))]
    return (torch.from_numpy(m.pos.astype(np.float32)).double(), torch.from_numpy(a), torch.from_numpy(m.edge_index),
            torch.from_numpy(b), *f)


@pytest.mark.parametrize("precision", TIERS)
def test_forecaster_step_and_training_step_vs_fp64(ga, precision):
    m = ga.geodesic_mesh(6)
    model = _forecaster(ga, precision)
    g = torch.Generator().manual_seed(SEED)
    x0 = torch.randn(m.faces.shape[0], 8, generator=g)
    w = torch.randn(m.faces.shape[0], 8, generator=g)
    sd = {k: v.double().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    want = forecaster_ref(sd, x0.double(), *_forecaster_fp64_inputs(ga, m), 2, 4)
    (want * w.double()).sum().backward()
    want = want.detach()
    graphs = model.prepare(m, DEV)
    model = model.to(DEV)
    with torch.no_grad():
        got = model(x0.to(DEV), graphs)
    err = rel_err(got, want)
    _log(test="forecaster_step", precision=precision, err=err)
    assert err <= FWD_TOL[precision]
    out = model(x0.to(DEV), graphs)                               # one training step
    loss = (out * w.to(DEV)).sum()
    loss.backward()
    assert rel_err(out.detach(), want) <= FWD_TOL[precision]
    gerrs = {}
    for k, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        gerrs[k] = rel_err(p.grad, sd[k].grad)
    _log(test="forecaster_grad", precision=precision, grad_max=max(gerrs.values()), grad_worst=max(gerrs, key=gerrs.get))
    for k, v in gerrs.items():
        assert v <= GRAD_TOL[precision], (k, v)


def test_forecaster_rollouts_members_and_noise(ga):
    m = ga.geodesic_mesh(6)
    model = _forecaster(ga, noise_channels=16).to(DEV)
    graphs = model.prepare(m, DEV)
    nf = m.faces.shape[0]
    xm = torch.randn(4, nf, 8, generator=torch.Generator().manual_seed(SEED + 5)).to(DEV)
    eager = model.rollout(xm[0], graphs, 3)
    graphed = model.rollout(xm[0], graphs, 3, graphed=True)
    assert len(eager) == 3 and all(torch.equal(a, b) for a, b in zip(eager, graphed))
    assert all(bool(torch.isfinite(t).all()) for t in eager) and not torch.equal(eager[0], eager[1])
    with torch.no_grad():
        batched = model(xm, graphs)                               # 4 members: one launch set
        for k in range(4):
            assert torch.equal(batched[k], model(xm[k], graphs)), k
    ens = ga.forecaster.ensemble_forecast(model, graphs, xm, 2, 4, gather=False)
    one = ga.forecaster.ensemble_forecast(model, graphs, xm, 2, 4, gather=False, batched=False, graphed=False)
    assert torch.equal(ens, one)
    runs = []
    for graphed_ in (False, True, False):
        st = ga.NoiseStream(SEED, DEV, draw=5)
        runs.append(model.rollout(xm.reshape(-1, 8), graphs.batched(4), 2, graphed=graphed_, noise=st))
        assert st.draw == 7
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1])) and all(torch.equal(a, b) for a, b in zip(runs[0], runs[2]))
    quiet = model.rollout(xm.reshape(-1, 8), graphs.batched(4), 2)
    assert not torch.equal(quiet[1], runs[0][1])                  # (the noise term is there)


# ---- 9. past 4 GiB ------------------------------------------------------------------------------------------------------------
def test_past_4_gib(ga):
    """nu = 100 hilbert mesh x 8 block-diagonal members, F = 256, H = 8, with ee: ee and gee hold 4.9 GB each (> 2^32
    bytes), the stacked k | v and its gradient 1.6 GB.  Three base members cycled over the eight: every member's forward
    and backward rows are bitwise those of its base member run alone (whose arrays all stay below 2^32 bytes), and base
    member 0 is held against fp64 on a 2 000-target sample: out, gq and the gee rows of the sample's in-edges."""
    from gwen_amd.interaction import interaction_graph
    F, H, members = 256, 8, 8
    m = ga.geodesic_mesh(100, reorder="hilbert")
    ei = torch.from_numpy(m.edge_index).to(DEV)
    n = m.num_nodes
    graph = interaction_graph(ei, n, n)
    e = graph.num_edges
    assert members * e * F * 4 > 2 ** 32 and e * F * 4 < 2 ** 32
    gen = torch.Generator(DEV).manual_seed(SEED)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=gen)                             # noqa: E731
    bases = [(rn(n, F), rn(n, 2 * F), rn(e, F), rn(n, F)) for _ in range(3)]               # q, [k | v], ee (stored order), w
    alone = []
    for q, kv, ee, w in bases:
        qd, kvd, eed = (t.clone().requires_grad_(True) for t in (q, kv, ee))
        out = ga.edge_attention_kv(qd, kvd, graph, H, eed)
        (out * w).sum().backward()
        alone.append((out.detach(), qd.grad, kvd.grad, eed.grad))
    cyc = lambda i: torch.cat([bases[k % 3][i] for k in range(members)], dim=0)            # noqa: E731
    qd, kvd, eed = (cyc(i).requires_grad_(True) for i in range(3))
    w = cyc(3)
    gb = graph.batched(members)
    out = ga.edge_attention_kv(qd, kvd, gb, H, eed)
    (out * w).sum().backward()
    del w
    assert eed.grad.numel() * 4 > 2 ** 32
    for k in range(members):
        o, gq, gkv, gee = alone[k % 3]
        assert torch.equal(out[k * n:(k + 1) * n], o), k
        assert torch.equal(qd.grad[k * n:(k + 1) * n], gq), k
        assert torch.equal(kvd.grad[k * n:(k + 1) * n], gkv), k
        assert torch.equal(eed.grad[k * e:(k + 1) * e], gee), k
    # base member 0 against fp64 on a sample of targets: the sub-problem of their in-edges
    pick = torch.randperm(n, generator=torch.Generator().manual_seed(SEED))[:2000].sort().values.to(DEV)
    mask = torch.zeros(n, dtype=torch.bool, device=DEV).index_fill_(0, pick, True)
    es = mask[graph.dst.long()].nonzero().view(-1)                                          # stored edges into the sample
    srcs, inv = torch.unique(graph.src.long()[es], return_inverse=True)
    local = torch.full((n,), -1, dtype=torch.long, device=DEV).index_copy_(0, pick, torch.arange(2000, device=DEV))
    q, kv, ee, w = bases[0]
    sub = [t.cpu() for t in (q[pick], kv[srcs, :F], kv[srcs, F:], ee[es], w[pick])]
    sei = torch.stack([inv.cpu(), local[graph.dst.long()[es]].cpu()])
    want, yard = _ref_forward(*sub[:3], sei, H, sub[3])
    g64 = _ref_backward(*sub[:3], sei, H, sub[3], sub[4], torch.float64)
    g32 = _ref_backward(*sub[:3], sei, H, sub[3], sub[4], torch.float32)
    o, gq, _, gee = alone[0]
    err, err_y = row_err(o[pick], want), row_err(yard, want)
    _log(test="past_4gib_forward", err_gpu=err, err_cpu_fp32=err_y)
    _bound(err, err_y, FWD_FLOOR, "out")
    for what, got, i in (("gq", gq[pick], 0), ("gee", gee[es], 3)):
        err, err_y = row_err(got, g64[i]), row_err(g32[i], g64[i])
        _log(test="past_4gib_grad", grad=what, err_gpu=err, err_cpu_fp32=err_y)
        _bound(err, err_y, GRAD_FLOOR, what)
