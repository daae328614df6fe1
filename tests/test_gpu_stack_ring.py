"""The stack launcher's activation buffers are a ring of three (csrc/forward.hip, kRing): no launch stores over the rows
the launch before it read.  Which buffer a launch writes changes no value, so the whole stack must stay BIT FOR BIT the
chain of per-layer calls it issues -- on the c2 model's six launches and on a stack deep enough to go round the ring
more than twice -- for 1 and 3 members, and stay so from run to run.  The launcher must keep inside the scratch it asks
for (NaN guard behind it) and refuse one float less."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import SEED

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096                                   # floats behind the scratch and behind every output
ENOSPACE = -3


@pytest.fixture(scope="module")
def ga(hip_lib):
    import gwen_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return gwen_amd


_graphs = {}


def _graph(ga, nu):
    if nu not in _graphs:
        m = ga.geodesic_mesh(nu)
        g = ga.prepare_graph(torch.from_numpy(np.ascontiguousarray(m.edge_index.astype(np.int64))).to(DEV), m.num_nodes)
        assert g.num_nodes == 10 * nu * nu + 2 and g.grouped()[0] is None and g.entries() == 7
        _graphs[nu] = g
    return _graphs[nu]


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _guarded(shape):
    numel = int(np.prod(shape))
    buf = torch.full((numel + GUARD,), float("nan"), device=DEV)
    return buf[:numel].view(shape), buf[numel:]


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _inputs(n, members, fin):
    g = torch.Generator().manual_seed(SEED + 131 * fin + members)
    x = torch.randn(members, n, fin, generator=g)
    return (x[0] if members == 1 else x).contiguous().to(DEV)


def _layer(g, x, w, b, relu, contract):
    from gwen_amd import _lib
    _, gc, gv = g.grouped()
    m = 1 if x.dim() == 2 else x.size(0)
    n, fin, fout = g.num_nodes, w.size(1), w.size(0)
    out, guard = _guarded((*x.shape[:-1], fout))
    rc = _lib.lib().gwen_gcn_layer_tuned3_f32(None, _p(gc), _p(gv), _p(x), _p(w), _p(b), _p(out), n, fin, fout, fin, fout,
                                              m, n * fin, n * fout, int(relu), contract, 7, 0, 0, 0, None, 0, _st())
    assert rc == 0
    assert torch.isnan(guard).all()
    return out


def _chain(g, x, w1, w2, b, relu, pre, contract):
    from gwen_amd import _lib
    _, gc, gv = g.grouped()
    m = 1 if x.dim() == 2 else x.size(0)
    n, fin = g.num_nodes, x.size(-1)
    f1 = 0 if w1 is None else w1.size(0)
    f2 = 0 if w2 is None else w2.size(0)
    fw = f2 or f1 or fin
    out, guard = _guarded((*x.shape[:-1], fw))
    rc = _lib.lib().gwen_gcn_chain_tuned3_f32(None, _p(gc), _p(gv), _p(x), _p(w1), _p(w2), _p(b), _p(out), n, fin, f1, f2,
                                              int(pre), int(relu), m, n * fin, n * fw, contract, 7, 0, 0, 0, None, None, 0,
                                              _st())
    assert rc == 0
    assert torch.isnan(guard).all()
    return out


def _launcher(ga, g, plan, x, short=0):
    """gwen_gnn_forward_entries_f32 on a scratch of exactly the floats it asks for (less `short`), NaN guards behind the
    scratch and behind the output; returns (rc, out, kinds)."""
    from gwen_amd import _lib
    L = _lib.lib()
    n, desc, nl = g.num_nodes, plan.desc, len(plan.desc)
    members = 1 if x.dim() == 2 else x.size(0)
    _, gc, gv = g.grouped()
    gd = _lib.GraphDesc()
    gd.N = n
    gd.rowptr, gd.col, gd.val = g.rowptr.data_ptr(), g.col.data_ptr(), g.val.data_ptr()
    gd.g_rowptr, gd.g_col, gd.g_val = 0, gc.data_ptr(), gv.data_ptr()
    ns = int(L.gwen_gnn_forward_scratch_floats(n, members, desc, nl))
    assert ns > 0
    scratch, sguard = _guarded((ns - short,))
    out, oguard = _guarded((*x.shape[:-1], desc[nl - 1].fout))
    ev = ga.KernelEvents(2 * nl)
    rc = L.gwen_gnn_forward_entries_f32(C.byref(gd), desc, nl, _p(x), _p(out), _p(scratch), scratch.numel(), members,
                                        _st(), ev._ev, ev.info, ev.max_launches, C.byref(ev.n), None, 7)
    torch.cuda.synchronize()
    assert torch.isnan(sguard).all(), "written behind the scratch"
    assert torch.isnan(oguard).all(), "written behind the output"
    return rc, out, ([k for k, *_ in ev.durations()] if rc == 0 else None)


def _c2(ga):
    torch.manual_seed(SEED)
    model = ga.GNNModel(ga.GNNConfig(1, 1, 64, 64, 64)).to(DEV)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
    return model


@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("nu", [8, 12])
def test_c2_stack_equals_its_per_layer_calls(ga, nu, members):
    from gwen_amd import _lib
    g = _graph(ga, nu)
    model = _c2(ga)
    plan = ga.StackForward(model.stack(), g)
    desc, nl = plan.desc, len(plan.desc)
    assert [(d.fin, d.fout) for d in desc] == [(64, 64), (64, 32), (32, 16), (16, 32), (32, 64), (64, 64)]
    x = _inputs(g.num_nodes, members, 64)
    W = [plan._keep[3 * i] for i in range(nl)]
    B = [plan._keep[3 * i + 1] for i in range(nl)]
    c = [_lib.dense_contract(d.contract) for d in desc]
    relu = [bool(d.relu) for d in desc]
    h = _chain(g, x, W[0], W[1], B[0], relu[0], False, c[0])                   # layer 0 + layer 1's projection
    h = _chain(g, h, W[2], None, B[1], relu[1], True, c[2])                    # layer 1's gather + layer 2's projection
    h = _chain(g, h, None, None, B[2], relu[2], True, _lib.CONTRACT_BF16X3)    # layer 2's gather
    for i in (3, 4, 5):
        h = _layer(g, h, W[i], B[i], relu[i], c[i])
    assert torch.isfinite(h).all()

    ev = ga.KernelEvents(12)
    got = plan.run(x, events=ev).clone()
    assert [k for k, *_ in ev.durations()] == ["chain"] * 3 + ["layer"] * 3
    assert _same_bits(got, h)
    assert _same_bits(plan.run(x), h)                                          # and again: nothing is left behind
    rc, out, kinds = _launcher(ga, g, plan, x)
    assert rc == 0 and kinds == ["chain"] * 3 + ["layer"] * 3
    assert _same_bits(out, h)
    assert _launcher(ga, g, plan, x, short=1)[0] == ENOSPACE


@pytest.mark.parametrize("members", [1, 3])
def test_deep_stack_goes_round_the_ring(ga, members):
    """Eight 16 -> 16 layers (K4 launches; 16 channels keep the small-graph kernel out): seven intermediate buffers on a
    ring of three."""
    from gwen_amd import _lib
    g = _graph(ga, 8)
    gen = torch.Generator().manual_seed(SEED + 5)
    layers = [((torch.randn(16, 16, generator=gen) / 4).to(DEV), (torch.randn(16, generator=gen) * 0.1).to(DEV), i < 7,
               "auto") for i in range(8)]
    plan = ga.StackForward(layers, g)
    x = _inputs(g.num_nodes, members, 16)
    h = x
    for (w, b, relu, _), d in zip(layers, plan.desc):
        h = _layer(g, h, w, b, relu, _lib.dense_contract(d.contract))
    assert torch.isfinite(h).all()
    rc, out, kinds = _launcher(ga, g, plan, x)
    assert rc == 0 and kinds == ["layer"] * 8
    assert _same_bits(out, h)
    assert _same_bits(plan.run(x), h) and _same_bits(plan.run(x), h)
    assert _launcher(ga, g, plan, x, short=1)[0] == ENOSPACE
