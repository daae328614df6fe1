"""Gather depth of K4 / K5 (gather_rows.h, D): with depth = 2 a wave keeps the row loads of two passes in flight.  It is a
scheduling choice -- every output element is still the fma chain over the row's stored slots in slot order -- so
depth = 2 must equal depth = 1 bit for bit (``torch.equal``), at every forced block size (which sets the number of
passes per wave: 1, 2, 3, 4, 6, 7, 8 -- the odd counts end the two-buffer loop in its peeled form), on partial blocks,
on the non-uniform layout (long rows, empty rows, the null group) and for several members.  Outputs are pre-filled
with NaN and followed by a NaN guard: every row < N must be written, nothing behind the last row may be."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import SEED

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WIDTHS = (16, 32, 64)
GUARD = 4096                                   # floats behind the last row
EINVAL = -1
# block_rows a width accepts (0 = the library's choice): whole gather passes of 1024 / Fin rows
LAYER_ROWS = {64: (0, 64, 96, 112, 128), 32: (0, 64, 96, 128), 16: (0, 64, 128)}
CHAIN_ROWS = {64: (0, 64, 96, 112), 32: (0, 64, 96), 16: (0, 64)}
GRAPHS = ["mesh3", "mesh10", "mesh10-hilbert", "ring65", "random"]
# (bias, relu)
FLAGS = [(True, True), (False, False), (True, False), (False, True)]


@pytest.fixture(scope="module")
def ga(hip_lib):
    import gwen_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return gwen_amd


_graphs = {}


def _graph(ga, name):
    """The prepared graph, built once per module.  mesh3: N = 92 (one partial block, N below every block size);
    mesh10 / mesh10-hilbert: N = 1 002 (many blocks, the last one partial); ring65: N = 64 + 1; random: 300 rows of
    0 .. 40 entries with raw weights (non-uniform layout, entries = 8)."""
    if name in _graphs:
        return _graphs[name]
    if name.startswith("mesh"):
        m = ga.geodesic_mesh(3 if name == "mesh3" else 10, reorder="hilbert" if name.endswith("hilbert") else None)
        g = ga.prepare_graph(torch.from_numpy(np.ascontiguousarray(m.edge_index.astype(np.int64))).to(DEV), m.num_nodes)
        assert g.num_nodes == (92 if name == "mesh3" else 1002)
        assert g.grouped()[0] is None and g.entries() == 7
    elif name == "ring65":
        i = np.arange(65)
        ei = np.stack([np.concatenate([i, i]), np.concatenate([(i + 1) % 65, (i - 1) % 65])]).astype(np.int64)
        g = ga.prepare_graph(torch.from_numpy(ei).to(DEV), 65)
        assert g.grouped()[0] is None and g.entries() == 7
    elif name == "random":
        rng = np.random.default_rng(SEED)
        n = 300
        deg = rng.integers(0, 41, size=n)
        deg[[0, 17, 63, 64, 299]] = 0                       # empty rows, at block and pass boundaries too
        deg[[1, 65, 298]] = 40
        dst = np.repeat(np.arange(n), deg)
        src = np.concatenate([rng.choice(n, size=d, replace=False) for d in deg]) if deg.sum() else dst
        w = torch.from_numpy(rng.standard_normal(dst.size).astype(np.float32)).to(DEV)
        g = ga.prepare_graph(torch.from_numpy(np.stack([src, dst]).astype(np.int64)).to(DEV), n, w,
                             add_self_loops=False, normalize=False)
        lens = np.diff(g.rowptr.cpu().numpy())
        assert lens.min() == 0 and lens.max() == 40
        assert g.grouped()[0] is not None and g.entries() == 8
    else:
        raise KeyError(name)
    _graphs[name] = g
    return g


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _out(shape):
    """(view of `shape`, its guard): one NaN-filled allocation, the guard right behind the last row."""
    numel = int(np.prod(shape))
    buf = torch.full((numel + GUARD,), float("nan"), device=DEV)
    return buf[:numel].view(shape), buf[numel:]


def _whole(out, guard, what):
    assert torch.isfinite(out).all(), ("a row < N was not written", what)
    assert torch.isnan(guard).all(), ("written behind the last row", what)


def _layer(g, x, w, b, relu, contract, depth, rows, expect=0):
    from gwen_amd import _lib
    gr, gc, gv = g.grouped()
    m = 1 if x.dim() == 2 else x.size(0)
    n, fin, fout = g.num_nodes, w.size(1), w.size(0)
    out, guard = _out((*x.shape[:-1], fout))
    rc = _lib.lib().gwen_gcn_layer_tuned_f32(_p(gr), _p(gc), _p(gv), _p(x), _p(w), _p(b), _p(out), n, fin, fout, fin,
                                             fout, m, n * fin, n * fout, int(relu), contract, g.entries(), depth, rows,
                                             _st())
    assert rc == expect, (rc, fin, fout, contract, depth, rows)
    return out, guard


def _chain(g, x, w1, w2, b, relu, pre, contract, depth, rows, expect=0):
    from gwen_amd import _lib
    gr, gc, gv = g.grouped()
    m = 1 if x.dim() == 2 else x.size(0)
    n, fin = g.num_nodes, x.size(-1)
    f1 = 0 if w1 is None else w1.size(0)
    f2 = 0 if w2 is None else w2.size(0)
    fw = f2 or f1 or fin
    out, guard = _out((*x.shape[:-1], fw))
    rc = _lib.lib().gwen_gcn_chain_tuned_f32(_p(gr), _p(gc), _p(gv), _p(x), _p(w1), _p(w2), _p(b), _p(out), n, fin, f1,
                                             f2, int(pre), int(relu), m, n * fin, n * fw, contract, g.entries(), depth,
                                             rows, _st())
    assert rc == expect, (rc, fin, f1, f2, pre, contract, depth, rows)
    return out, guard


def _inputs(n, members, fin, seed=SEED):
    g = torch.Generator().manual_seed(seed + 131 * fin + members)
    x = torch.randn(members, n, fin, generator=g)
    return (x[0] if members == 1 else x).contiguous().to(DEV)


def _params(fin, fout, seed=0):
    g = torch.Generator().manual_seed(SEED + 7 * fin + fout + seed)
    return (torch.randn(fout, fin, generator=g) / fin ** 0.5).to(DEV), (torch.randn(fout, generator=g) * 0.1).to(DEV)


@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("name", GRAPHS)
def test_k4_depth_two_equals_depth_one(ga, name, members):
    """k_layer at all nine width pairs on bf16x3 / bf16x6 / fp32, every valid block size, bias and ReLU on and off."""
    from gwen_amd import _lib
    g = _graph(ga, name)
    n = g.num_nodes
    for fin in WIDTHS:
        x = _inputs(n, members, fin)
        for fout in WIDTHS:
            w, b = _params(fin, fout)
            for contract in (_lib.CONTRACT_BF16X3, _lib.CONTRACT_BF16X6, _lib.CONTRACT_F32):
                for rows in LAYER_ROWS[fin]:
                    for bias, relu in (FLAGS if rows in (0, 112, 96) else FLAGS[:2]):
                        what = (name, members, fin, fout, contract, rows, bias, relu)
                        one, g1 = _layer(g, x, w, b if bias else None, relu, contract, 1, rows)
                        two, g2 = _layer(g, x, w, b if bias else None, relu, contract, 2, rows)
                        _whole(one, g1, what)
                        _whole(two, g2, what)
                        assert torch.equal(one, two), what


# (fin, f1, f2, pre): the chained forms of the c2 model and its neighbours, the activation-first forms, the plain gather
CHAIN_FORMS = [(64, 64, 32, False), (64, 64, 16, False), (64, 32, 16, False),
               (32, 16, 0, True), (16, 32, 0, True), (64, 64, 0, True),
               (16, 0, 0, True), (32, 0, 0, True), (64, 0, 0, True)]


@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("name", GRAPHS)
def test_k5_depth_two_equals_depth_one(ga, name, members):
    """k_chain in its chained and activation-first forms and k_gather, on both splits, every valid block size."""
    from gwen_amd import _lib
    g = _graph(ga, name)
    n = g.num_nodes
    for fin, f1, f2, pre in CHAIN_FORMS:
        x = _inputs(n, members, fin)
        w1 = _params(fin, f1)[0] if f1 else None
        w2 = _params(f1, f2, seed=1)[0] if f2 else None
        bvec = (torch.randn(fin if pre else f1, generator=torch.Generator().manual_seed(SEED + fin + f1)) * 0.1).to(DEV)
        for contract in (_lib.CONTRACT_BF16X3, _lib.CONTRACT_BF16X6):
            assert _lib.lib().gwen_gcn_chain_supported(fin, f1, f2, int(pre), contract)
            for rows in (CHAIN_ROWS[fin] if f1 else (0, 1024 // fin)):
                for bias, relu in (FLAGS if rows in (0, 112, 96) else FLAGS[:2]):
                    what = (name, members, fin, f1, f2, pre, contract, rows, bias, relu)
                    one, g1 = _chain(g, x, w1, w2, bvec if bias else None, relu, pre, contract, 1, rows)
                    two, g2 = _chain(g, x, w1, w2, bvec if bias else None, relu, pre, contract, 2, rows)
                    _whole(one, g1, what)
                    _whole(two, g2, what)
                    assert torch.equal(one, two), what


def test_block_rows_change_no_value(ga):
    """Every forced block size gives the values of the library's own choice (one mesh, the c2 widths)."""
    from gwen_amd import _lib
    g = _graph(ga, "mesh10-hilbert")
    n = g.num_nodes
    for fin, fout in ((64, 64), (32, 64), (16, 32)):
        x, (w, b) = _inputs(n, 1, fin), _params(fin, fout)
        want, _ = _layer(g, x, w, b, True, _lib.CONTRACT_BF16X6, 1, 0)
        for rows in LAYER_ROWS[fin][1:]:
            for depth in (1, 2):
                assert torch.equal(_layer(g, x, w, b, True, _lib.CONTRACT_BF16X6, depth, rows)[0], want), (fin, rows, depth)
    x = _inputs(n, 1, 64)
    w1, b1 = _params(64, 64)
    w2 = _params(64, 32, seed=1)[0]
    want, _ = _chain(g, x, w1, w2, b1, True, False, _lib.CONTRACT_BF16X6, 1, 0)
    for rows in CHAIN_ROWS[64][1:]:
        for depth in (1, 2):
            assert torch.equal(_chain(g, x, w1, w2, b1, True, False, _lib.CONTRACT_BF16X6, depth, rows)[0], want), (rows, depth)


def test_arguments_are_checked(ga):
    from gwen_amd import _lib
    g = _graph(ga, "mesh3")
    n = g.num_nodes
    x64, x32, x16 = _inputs(n, 1, 64), _inputs(n, 1, 32), _inputs(n, 1, 16)
    w, b = _params(64, 64)
    w2 = _params(64, 32, seed=1)[0]
    c = _lib.CONTRACT_BF16X3
    for depth in (-1, 3, 7):
        _layer(g, x64, w, b, True, c, depth, 0, expect=EINVAL)
        _chain(g, x64, w, w2, b, True, False, c, depth, 0, expect=EINVAL)
        _chain(g, x64, None, None, None, True, True, c, depth, 0, expect=EINVAL)
    for rows in (-64, 1, 16, 32, 80, 100, 256):
        _layer(g, x64, w, b, True, c, 1, rows, expect=EINVAL)
        _chain(g, x64, w, w2, b, True, False, c, 1, rows, expect=EINVAL)
    _chain(g, x64, w, w2, b, True, False, c, 1, 128, expect=EINVAL)          # K5: 64 / 96 / 112
    w3264, w1632 = _params(32, 64)[0], _params(16, 32)[0]
    _layer(g, x32, w3264, None, True, c, 2, 112, expect=EINVAL)              # 112 is no multiple of 32 rows
    _layer(g, x16, w1632, None, True, c, 2, 96, expect=EINVAL)               # 96 / 112: no multiple of 64 rows
    _layer(g, x16, w1632, None, True, c, 2, 112, expect=EINVAL)
    _chain(g, x32, _params(32, 16)[0], None, None, True, True, c, 2, 112, expect=EINVAL)
    _chain(g, x16, None, None, None, True, True, c, 2, 32, expect=EINVAL)    # the plain gather: 1024 / Fin rows only
    # a refused call writes nothing
    out, guard = _layer(g, x64, w, b, True, c, 3, 0, expect=EINVAL)
    assert torch.isnan(out).all() and torch.isnan(guard).all()


def test_depth_zero_is_the_table(ga):
    """depth = 0 runs the depth the library names (1 or 2 on a uniform layout; always 1 with a row pointer), and the
    entries-only entry points are depth = 0, block_rows = 0."""
    from gwen_amd import _lib
    L = _lib.lib()
    g = _graph(ga, "mesh10")
    n = g.num_nodes
    gr, gc, gv = g.grouped()
    for fin in WIDTHS:
        x = _inputs(n, 1, fin)
        for fout in WIDTHS:
            w, b = _params(fin, fout)
            for contract in (_lib.CONTRACT_BF16X3, _lib.CONTRACT_BF16X6, _lib.CONTRACT_F32):
                named = L.gwen_gcn_layer_depth(fin, fout, contract)
                assert named in (1, 2)
                auto, ga_ = _layer(g, x, w, b, True, contract, 0, 0)
                _whole(auto, ga_, (fin, fout, contract))
                assert torch.equal(auto, _layer(g, x, w, b, True, contract, named, 0)[0])
                plain = torch.full_like(auto, float("nan"))
                assert L.gwen_gcn_layer_entries_f32(_p(gr), _p(gc), _p(gv), _p(x), _p(w), _p(b), _p(plain), n, fin, fout,
                                                    fin, fout, 1, n * fin, n * fout, 1, contract, g.entries(), _st()) == 0
                assert torch.equal(auto, plain)
    for fin, f1, f2, pre in CHAIN_FORMS:
        for contract in (_lib.CONTRACT_BF16X3, _lib.CONTRACT_BF16X6):
            named = L.gwen_gcn_chain_depth(fin, f1, f2, int(pre), contract)
            assert named in (1, 2)
            x = _inputs(n, 1, fin)
            w1 = _params(fin, f1)[0] if f1 else None
            w2 = _params(f1, f2, seed=1)[0] if f2 else None
            auto, ga_ = _chain(g, x, w1, w2, None, True, pre, contract, 0, 0)
            _whole(auto, ga_, (fin, f1, f2, pre, contract))
            assert torch.equal(auto, _chain(g, x, w1, w2, None, True, pre, contract, named, 0)[0])
    assert L.gwen_gcn_layer_depth(128, 128, 0) == 1 and L.gwen_gcn_layer_depth(48, 64, 0) == 0
    assert L.gwen_gcn_chain_depth(128, 128, 0, 1, 0) == 1 and L.gwen_gcn_chain_depth(64, 32, 64, 0, 0) == 0


def test_ops_take_depth_and_block_rows(ga):
    from gwen_amd import ops
    g = _graph(ga, "mesh10-hilbert")
    x, (w, b) = _inputs(g.num_nodes, 1, 64), _params(64, 64)
    w2 = _params(64, 32, seed=1)[0]
    want = ops.layer(g, x, w, b, relu=True, contract="bf16x6")
    assert torch.equal(want, ops.layer_fused(g, x, w, b, relu=True, contract="bf16x6", depth=2, block_rows=112))
    want = ops.chain(g, x, w, w2, b, True, False, contract="bf16x6")
    assert torch.equal(want, ops.chain(g, x, w, w2, b, True, False, contract="bf16x6", depth=2, block_rows=96))
    want = ops.chain(g, x, None, None, b, True, True)
    assert torch.equal(want, ops.chain(g, x, None, None, b, True, True, depth=2, block_rows=16))
    with pytest.raises(Exception):
        ops.layer(g, x, w, b, depth=5)


def test_stack_on_the_c2_widths(ga):
    """StackForward of GNNModel(64, 64) on the nu = 10 mesh: the same six launches as before (3 chained + 3 plain fused
    kernels), and bit for bit the chain of single-kernel calls at depth = 1 -- whatever depths the library ships."""
    from gwen_amd import _lib
    g = _graph(ga, "mesh10-hilbert")
    n = g.num_nodes
    torch.manual_seed(SEED)
    model = ga.GNNModel(ga.GNNConfig(1, 1, 64, 64, 64)).to(DEV)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
    plan = ga.StackForward(model.stack(), g)
    desc, nl = plan.desc, len(plan.desc)
    assert [(d.fin, d.fout) for d in desc] == [(64, 64), (64, 32), (32, 16), (16, 32), (32, 64), (64, 64)]
    x = _inputs(n, 1, 64)
    ev = ga.KernelEvents(12)
    got = plan.run(x, events=ev)
    assert sorted(k for k, *_ in ev.durations()) == ["chain"] * 3 + ["layer"] * 3
    assert torch.isfinite(got).all()
    W = [plan._keep[3 * i] for i in range(nl)]
    B = [plan._keep[3 * i + 1] for i in range(nl)]
    c = [_lib.dense_contract(d.contract) for d in desc]
    relu = [bool(d.relu) for d in desc]
    h, _ = _chain(g, x, W[0], W[1], B[0], relu[0], False, c[0], 1, 0)          # layer 0 + layer 1's projection
    h, _ = _chain(g, h, W[2], None, B[1], relu[1], True, c[2], 1, 0)           # layer 1's gather + layer 2's projection
    h, _ = _chain(g, h, None, None, B[2], relu[2], True, _lib.CONTRACT_BF16X3, 1, 0)
    for i in (3, 4, 5):
        h, _ = _layer(g, h, W[i], B[i], relu[i], c[i], 1, 0)
    assert torch.equal(got, h)
