"""Entries-per-group specialisation of the grouped gather (gather_rows.h, GE): on a uniform layout whose rows all hold
at most 7 stored entries K4 / K5 skip the group's last slot.  The skipped term is fma(0, v, acc), so for finite inputs
entries = 7 must equal entries = 8 value for value (``torch.equal``; only the sign of an exact zero may differ, which
``torch.equal`` does not see)."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import SEED

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WIDTHS = (16, 32, 64)


@pytest.fixture(scope="module")
def ga(hip_lib):
    import gwen_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return gwen_amd


def _ring(n):
    i = np.arange(n)
    return np.stack([np.concatenate([i, i]), np.concatenate([(i + 1) % n, (i - 1) % n])]).astype(np.int64)


def _graph(ga, name):
    """(edge_index [2, E] int64 numpy, N).  mesh / mesh-hilbert: nu = 4, N = 162, rows of 6 and 7 entries."""
    if name.startswith("mesh"):
        m = ga.geodesic_mesh(4, reorder="hilbert" if name == "mesh-hilbert" else None)
        return m.edge_index.astype(np.int64), m.num_nodes
    if name == "ring":
        return _ring(50), 50                       # 3 entries per row
    if name == "ring17":
        return _ring(17), 17                       # one full 16-row tile plus one row
    if name == "single":
        return np.zeros((2, 0), dtype=np.int64), 1
    raise KeyError(name)


def _prepare(ga, ei, n):
    return ga.prepare_graph(torch.from_numpy(np.ascontiguousarray(ei)).to(DEV), n)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _layer(g, x, w, b, relu, contract, entries):
    from gwen_amd import _lib
    gr, gc, gv = g.grouped()
    m = 1 if x.dim() == 2 else x.size(0)
    n, fin, fout = g.num_nodes, w.size(1), w.size(0)
    out = torch.full((*x.shape[:-1], fout), float("nan"), device=DEV)
    rc = _lib.lib().gwen_gcn_layer_entries_f32(_p(gr), _p(gc), _p(gv), _p(x), _p(w), _p(b), _p(out), n, fin, fout, fin,
                                               fout, m, n * fin, n * fout, int(relu), contract, entries, _st())
    assert rc == 0
    return out


def _chain(g, x, w1, w2, b, relu, pre, contract, entries):
    from gwen_amd import _lib
    gr, gc, gv = g.grouped()
    m = 1 if x.dim() == 2 else x.size(0)
    n, fin = g.num_nodes, x.size(-1)
    f1 = 0 if w1 is None else w1.size(0)
    f2 = 0 if w2 is None else w2.size(0)
    fw = f2 or f1 or fin
    out = torch.full((*x.shape[:-1], fw), float("nan"), device=DEV)
    rc = _lib.lib().gwen_gcn_chain_entries_f32(_p(gr), _p(gc), _p(gv), _p(x), _p(w1), _p(w2), _p(b), _p(out), n, fin, f1,
                                               f2, int(pre), int(relu), m, n * fin, n * fw, contract, entries, _st())
    assert rc == 0
    return out


def _inputs(n, members, fin, seed=SEED):
    g = torch.Generator().manual_seed(seed + 131 * fin + members)
    x = torch.randn(members, n, fin, generator=g)
    return (x[0] if members == 1 else x).contiguous().to(DEV)


def _params(fin, fout, seed=0):
    g = torch.Generator().manual_seed(SEED + 7 * fin + fout + seed)
    return (torch.randn(fout, fin, generator=g) / fin ** 0.5).to(DEV), (torch.randn(fout, generator=g) * 0.1).to(DEV)


SEVEN = ["mesh", "mesh-hilbert", "ring", "ring17", "single"]


@pytest.mark.parametrize("name", SEVEN)
def test_bound_is_detected(ga, name):
    ei, n = _graph(ga, name)
    g = _prepare(ga, ei, n)
    lens = np.diff(g.rowptr.cpu().numpy())
    assert lens.max() <= 7
    if name.startswith("mesh"):
        assert n == 162 and sorted(set(lens.tolist())) == [6, 7]
    assert g.grouped()[0] is None and g.entries() == 7
    from gwen_amd import _lib
    out = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert _lib.lib().gwen_gcn_max_entries(_p(g.rowptr), n, _p(out), _st()) == 0
    assert int(out.item()) == int(lens.max())


def test_bound_of_many_rows(ga):
    """More rows than the reduction's one block has threads, the longest row far from either end."""
    from gwen_amd import _lib
    n = 5000
    lens = np.full(n, 3, dtype=np.int32)
    lens[3777] = 11
    rowptr = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)).to(DEV)
    out = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert _lib.lib().gwen_gcn_max_entries(_p(rowptr), n, _p(out), _st()) == 0
    assert int(out.item()) == 11


@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("name", SEVEN)
def test_k4_seven_equals_eight(ga, name, members):
    """K4 on bf16x3 / bf16x6 / fp32-MFMA, every width pair, bias and ReLU on and off."""
    from gwen_amd import _lib
    ei, n = _graph(ga, name)
    g = _prepare(ga, ei, n)
    assert g.entries() == 7
    for fin in WIDTHS:
        x = _inputs(n, members, fin)
        for fout in WIDTHS:
            w, b = _params(fin, fout)
            for contract in (_lib.CONTRACT_BF16X3, _lib.CONTRACT_BF16X6, _lib.CONTRACT_F32):
                for on in (True, False):
                    a7 = _layer(g, x, w, b if on else None, on, contract, 7)
                    a8 = _layer(g, x, w, b if on else None, on, contract, 8)
                    assert torch.isfinite(a8).all()
                    assert torch.equal(a7, a8), (fin, fout, contract, on)


@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("name", SEVEN)
def test_k5_seven_equals_eight(ga, name, members):
    """K5 in its three forms (layer + chained projection; activation-first + projection; activation-first alone) on
    both splits."""
    from gwen_amd import _lib
    L = _lib.lib()
    ei, n = _graph(ga, name)
    g = _prepare(ga, ei, n)
    assert g.entries() == 7
    ran = 0
    for contract in (_lib.CONTRACT_BF16X3, _lib.CONTRACT_BF16X6):
        for fin in WIDTHS:
            x = _inputs(n, members, fin)
            bpre = (torch.randn(fin, generator=torch.Generator().manual_seed(SEED + fin)) * 0.1).to(DEV)
            for on in (True, False):
                a7 = _chain(g, x, None, None, bpre if on else None, on, True, contract, 7)
                a8 = _chain(g, x, None, None, bpre if on else None, on, True, contract, 8)
                assert torch.isfinite(a8).all() and torch.equal(a7, a8), ("gather", fin, on)
                ran += 1
                for f1 in WIDTHS:
                    w1, b1 = _params(fin, f1)
                    if L.gwen_gcn_chain_supported(fin, f1, 0, 1, contract):
                        a7 = _chain(g, x, w1, None, bpre if on else None, on, True, contract, 7)
                        a8 = _chain(g, x, w1, None, bpre if on else None, on, True, contract, 8)
                        assert torch.isfinite(a8).all() and torch.equal(a7, a8), ("pre", fin, f1, on)
                        ran += 1
                    for f2 in WIDTHS:
                        if f2 < f1 and L.gwen_gcn_chain_supported(fin, f1, f2, 0, contract):
                            w2, _ = _params(f1, f2, seed=1)
                            a7 = _chain(g, x, w1, w2, b1 if on else None, on, False, contract, 7)
                            a8 = _chain(g, x, w1, w2, b1 if on else None, on, False, contract, 8)
                            assert torch.isfinite(a8).all() and torch.equal(a7, a8), ("chain", fin, f1, f2, on)
                            ran += 1
    assert ran >= 2 * 2 * 3 * (1 + 3 + 3)            # every form ran at every gathered width


def test_row_of_eight_keeps_whole_groups(ga):
    """One extra edge into a 7-entry row: the layout is still uniform, the bound is 8, nothing is skipped."""
    from gwen_amd import _lib, ops
    ei, n = _graph(ga, "mesh")
    g0 = _prepare(ga, ei, n)
    lens = np.diff(g0.rowptr.cpu().numpy())
    dst = int(np.nonzero(lens == 7)[0][0])
    nbrs = set(ei[0][ei[1] == dst].tolist()) | {dst}
    src = next(v for v in range(n) if v not in nbrs)
    ei8 = np.concatenate([ei, np.array([[src], [dst]], dtype=np.int64)], axis=1)
    g = _prepare(ga, ei8, n)
    lens8 = np.diff(g.rowptr.cpu().numpy())
    assert lens8.max() == 8 and (lens8 == 8).sum() == 1
    assert g.grouped()[0] is None and g.entries() == 8
    x, (w, b) = _inputs(n, 1, 64), _params(64, 64)
    got = ops.layer_fused(g, x, w, b, relu=True, contract="bf16x6")
    assert torch.equal(got, _layer(g, x, w, b, True, _lib.CONTRACT_BF16X6, 8))
    # the 8th entry counts: against the layer's own arithmetic on the plain CSR (K2, then the fp32-class K3)
    want = ops.linear(ops.propagate(g, x), w, b, True, contract="bf16x6")
    assert (got - want).abs().max() <= 2e-5 * want.abs().max()
    without = ops.layer_fused(g0, x, w, b, relu=True, contract="bf16x6")
    assert not torch.equal(got[dst], without[dst])


def test_non_uniform_layout_is_unchanged(ga):
    """A row above 8 entries: the layout has a row pointer, the bound is above 7, and entries = 7 changes nothing."""
    from gwen_amd import _lib
    ei, n = _graph(ga, "mesh")
    hub = np.stack([np.arange(20, 32), np.full(12, 5)]).astype(np.int64)
    g = _prepare(ga, np.concatenate([ei, hub], axis=1), n)
    assert np.diff(g.rowptr.cpu().numpy()).max() > 8
    assert g.grouped()[0] is not None and g.entries() == 8
    x, (w, b) = _inputs(n, 1, 32), _params(32, 64)
    for contract in (_lib.CONTRACT_BF16X3, _lib.CONTRACT_BF16X6):
        assert torch.equal(_layer(g, x, w, b, True, contract, 7), _layer(g, x, w, b, True, contract, 8))
        assert torch.equal(_chain(g, x, None, None, None, True, True, contract, 7),
                           _chain(g, x, None, None, None, True, True, contract, 8))


def test_empty_graph(ga):
    from gwen_amd import _lib
    L = _lib.lib()
    for entries in (7, 8):
        assert L.gwen_gcn_layer_entries_f32(None, None, None, None, None, None, None, 0, 16, 16, 16, 16, 1, 0, 0, 1, 0,
                                            entries, _st()) == 0
        assert L.gwen_gcn_chain_entries_f32(None, None, None, None, None, None, None, None, 0, 16, 0, 0, 1, 1, 1, 0, 0, 0,
                                            entries, _st()) == 0
    out = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    rowptr = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert L.gwen_gcn_max_entries(_p(rowptr), 0, _p(out), _st()) == 0
    assert int(out.item()) == 0


@pytest.mark.parametrize("name", ["mesh", "mesh-hilbert"])
def test_stack_launcher_with_detected_bound(ga, name):
    """gwen_gnn_forward_entries_f32 with the graph's bound == the per-layer calls it issues, bit for bit; the launches
    of GNNModel(64, 64) are still 3 chained + 3 plain fused kernels.  (dense = NULL: on 162 nodes the launcher would
    otherwise take the small-graph kernel.)"""
    from gwen_amd import _lib
    L = _lib.lib()
    ei, n = _graph(ga, name)
    g = _prepare(ga, ei, n)
    entries = g.entries()
    assert entries == 7
    torch.manual_seed(SEED)
    model = ga.GNNModel(ga.GNNConfig(1, 1, 64, 64, 64)).to(DEV)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
    plan = ga.StackForward(model.stack(), g)
    desc, nl = plan.desc, len(plan.desc)
    assert [(d.fin, d.fout) for d in desc] == [(64, 64), (64, 32), (32, 16), (16, 32), (32, 64), (64, 64)]
    gr, gc, gv = g.grouped()
    gd = _lib.GraphDesc()
    gd.N = n
    gd.rowptr, gd.col, gd.val = g.rowptr.data_ptr(), g.col.data_ptr(), g.val.data_ptr()
    gd.g_rowptr, gd.g_col, gd.g_val = 0, gc.data_ptr(), gv.data_ptr()
    x = _inputs(n, 1, 64)
    ns = int(L.gwen_gnn_forward_scratch_floats(n, 1, desc, nl))
    scratch = torch.empty(max(ns, 4), device=DEV)
    ev = ga.KernelEvents(12)
    outs = []
    for e in (entries, 8):
        out = torch.full((n, 64), float("nan"), device=DEV)
        rc = L.gwen_gnn_forward_entries_f32(C.byref(gd), desc, nl, _p(x), _p(out), _p(scratch), scratch.numel(), 1, _st(),
                                            ev._ev, ev.info, ev.max_launches, C.byref(ev.n), None, e)
        assert rc == 0
        assert sorted(k for k, *_ in ev.durations()) == ["chain"] * 3 + ["layer"] * 3
        outs.append(out)
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])

    W = [plan._keep[3 * i] for i in range(nl)]
    B = [plan._keep[3 * i + 1] for i in range(nl)]
    c = [_lib.dense_contract(d.contract) for d in desc]
    relu = [bool(d.relu) for d in desc]
    h = _chain(g, x, W[0], W[1], B[0], relu[0], False, c[0], entries)          # layer 0 + layer 1's projection
    h = _chain(g, h, W[2], None, B[1], relu[1], True, c[2], entries)           # layer 1's gather + layer 2's projection
    h = _chain(g, h, None, None, B[2], relu[2], True, _lib.CONTRACT_BF16X3, entries)
    for i in (3, 4, 5):
        h = _layer(g, h, W[i], B[i], relu[i], c[i], entries)
    assert torch.equal(outs[0], h)
