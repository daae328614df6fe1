"""Index mode of K4 / K5 (gather_rows.h, IM): with index_mode = 2 the lanes that share a destination row load the row's
64-byte record [8 column indices | 8 weights] once between them and broadcast it inside the lane group, instead of
every lane loading all of it.  It is a way of fetching the same numbers -- every output element is still the fma chain
over the row's slots in slot order -- so mode 2 must equal mode 1 BIT FOR BIT (compared as int32 patterns: a -0.0 is not
a +0.0 here, and x holds a row of -0.0), at every width, contraction, depth, forced block size (1 to 8 passes per wave,
both peeled endings of the depth-2 loop), with 7 and with 8 gathered entries, on partial blocks and for several
members.  Outputs are pre-filled with NaN and followed by a NaN guard: every row < N must be written, nothing behind
the last row may be."""
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
GRAPHS = ["mesh3", "ring65", "mesh10-hilbert", "one", "circ70"]
FLAGS = [(True, True), (False, False), (True, False), (False, True)]       # (bias, relu)
# (fin, f1, f2, pre): every supported form of the widths 16 / 32 / 64 -- chained, activation-first, the plain gather
CHAIN_FORMS = ([(fi, f1, f2, False) for fi in WIDTHS for f1 in WIDTHS for f2 in WIDTHS if f2 < f1] +
               [(fi, f1, 0, True) for fi in WIDTHS for f1 in (0,) + WIDTHS])


@pytest.fixture(scope="module")
def ga(hip_lib):
    import gwen_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return gwen_amd


_graphs = {}


def _graph(ga, name):
    """The prepared graph, built once per module.  mesh3: N = 92 (below every block size, absent rows in the last pass);
    ring65: N = 64 + 1 (one full block and a one-row block); mesh10-hilbert: N = 1 002 (many blocks, the last one
    partial); one: a single node; circ70: the circulant on 70 nodes with sources i +-1, +-2, +-3, +4 and the self loop --
    a uniform layout with 8 stored entries per row, so the record form gathers whole groups; random: 300 rows of
    0 .. 40 entries (non-uniform layout: no record form)."""
    if name in _graphs:
        return _graphs[name]

    def prep(ei, n):
        return ga.prepare_graph(torch.from_numpy(np.ascontiguousarray(ei.astype(np.int64))).to(DEV), n)

    if name.startswith("mesh"):
        m = ga.geodesic_mesh(3 if name == "mesh3" else 10, reorder="hilbert" if name.endswith("hilbert") else None)
        g = prep(m.edge_index, m.num_nodes)
        assert g.num_nodes == (92 if name == "mesh3" else 1002)
        assert g.grouped()[0] is None and g.entries() == 7
    elif name == "ring65":
        i = np.arange(65)
        g = prep(np.stack([np.concatenate([i, i]), np.concatenate([(i + 1) % 65, (i - 1) % 65])]), 65)
        assert g.grouped()[0] is None and g.entries() == 7
    elif name == "one":
        g = prep(np.zeros((2, 0), dtype=np.int64), 1)
        assert g.num_nodes == 1 and g.grouped()[0] is None
    elif name == "circ70":
        i = np.arange(70)
        offs = (1, -1, 2, -2, 3, -3, 4)
        g = prep(np.stack([np.concatenate([(i + o) % 70 for o in offs]), np.concatenate([i] * len(offs))]), 70)
        assert (np.diff(g.rowptr.cpu().numpy()) == 8).all()
        assert g.grouped()[0] is None and g.entries() == 8
    elif name == "random":
        rng = np.random.default_rng(SEED)
        n = 300
        deg = rng.integers(0, 41, size=n)
        deg[[0, 17, 63, 64, 299]] = 0
        dst = np.repeat(np.arange(n), deg)
        src = np.concatenate([rng.choice(n, size=d, replace=False) for d in deg])
        w = torch.from_numpy(rng.standard_normal(dst.size).astype(np.float32)).to(DEV)
        g = ga.prepare_graph(torch.from_numpy(np.stack([src, dst]).astype(np.int64)).to(DEV), n, w,
                             add_self_loops=False, normalize=False)
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


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _layer(g, x, w, b, relu, contract, depth, rows, mode, expect=0):
    from gwen_amd import _lib
    gr, gc, gv = g.grouped()
    m = 1 if x.dim() == 2 else x.size(0)
    n, fin, fout = g.num_nodes, w.size(1), w.size(0)
    out, guard = _out((*x.shape[:-1], fout))
    rc = _lib.lib().gwen_gcn_layer_tuned2_f32(_p(gr), _p(gc), _p(gv), _p(x), _p(w), _p(b), _p(out), n, fin, fout, fin,
                                              fout, m, n * fin, n * fout, int(relu), contract, g.entries(), depth, rows,
                                              mode, _st())
    assert rc == expect, (rc, fin, fout, contract, depth, rows, mode)
    return out, guard


def _chain(g, x, w1, w2, b, relu, pre, contract, depth, rows, mode, expect=0):
    from gwen_amd import _lib
    gr, gc, gv = g.grouped()
    m = 1 if x.dim() == 2 else x.size(0)
    n, fin = g.num_nodes, x.size(-1)
    f1 = 0 if w1 is None else w1.size(0)
    f2 = 0 if w2 is None else w2.size(0)
    fw = f2 or f1 or fin
    out, guard = _out((*x.shape[:-1], fw))
    rc = _lib.lib().gwen_gcn_chain_tuned2_f32(_p(gr), _p(gc), _p(gv), _p(x), _p(w1), _p(w2), _p(b), _p(out), n, fin, f1,
                                              f2, int(pre), int(relu), m, n * fin, n * fw, contract, g.entries(), depth,
                                              rows, mode, _st())
    assert rc == expect, (rc, fin, f1, f2, pre, contract, depth, rows, mode)
    return out, guard


def _inputs(n, members, fin, seed=SEED):
    """Random rows; from three rows on, row 1 and the last row of every member are all -0.0."""
    g = torch.Generator().manual_seed(seed + 131 * fin + members)
    x = torch.randn(members, n, fin, generator=g)
    if n > 2:
        x[:, 1] = -0.0
        x[:, n - 1] = -0.0
        assert torch.signbit(x[:, 1]).all() and (x[:, 1] == 0).all()
    return (x[0] if members == 1 else x).contiguous().to(DEV)


def _params(fin, fout, seed=0):
    g = torch.Generator().manual_seed(SEED + 7 * fin + fout + seed)
    return (torch.randn(fout, fin, generator=g) / fin ** 0.5).to(DEV), (torch.randn(fout, generator=g) * 0.1).to(DEV)


@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("name", GRAPHS)
def test_k4_records_equal_group_loads(ga, name, members):
    """k_layer at all nine width pairs on bf16x3 / bf16x6 / fp32, both depths, every valid block size, bias and ReLU on
    and off."""
    from gwen_amd import _lib
    g = _graph(ga, name)
    n = g.num_nodes
    for fin in WIDTHS:
        x = _inputs(n, members, fin)
        for fout in WIDTHS:
            w, b = _params(fin, fout)
            for contract in (_lib.CONTRACT_BF16X3, _lib.CONTRACT_BF16X6, _lib.CONTRACT_F32):
                for rows in LAYER_ROWS[fin]:
                    for depth in (1, 2):
                        for bias, relu in (FLAGS if rows in (0, 112, 96) else FLAGS[:2]):
                            what = (name, members, fin, fout, contract, rows, depth, bias, relu)
                            one, g1 = _layer(g, x, w, b if bias else None, relu, contract, depth, rows, 1)
                            two, g2 = _layer(g, x, w, b if bias else None, relu, contract, depth, rows, 2)
                            _whole(one, g1, what)
                            _whole(two, g2, what)
                            assert _same_bits(one, two), what


@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("name", GRAPHS)
def test_k5_records_equal_group_loads(ga, name, members):
    """k_chain in every chained and activation-first form of the three widths and k_gather, on both splits, both
    depths, every valid block size."""
    from gwen_amd import _lib
    g = _graph(ga, name)
    n = g.num_nodes
    ran = 0
    for fin, f1, f2, pre in CHAIN_FORMS:
        x = _inputs(n, members, fin)
        w1 = _params(fin, f1)[0] if f1 else None
        w2 = _params(f1, f2, seed=1)[0] if f2 else None
        bvec = (torch.randn(fin if pre else f1, generator=torch.Generator().manual_seed(SEED + fin + f1)) * 0.1).to(DEV)
        for contract in (_lib.CONTRACT_BF16X3, _lib.CONTRACT_BF16X6):
            if not _lib.lib().gwen_gcn_chain_supported(fin, f1, f2, int(pre), contract):
                continue
            ran += 1
            for rows in (CHAIN_ROWS[fin] if f1 else (0, 1024 // fin)):
                for depth in (1, 2):
                    for bias, relu in (FLAGS if rows in (0, 112, 96) else FLAGS[:2]):
                        what = (name, members, fin, f1, f2, pre, contract, rows, depth, bias, relu)
                        one, g1 = _chain(g, x, w1, w2, bvec if bias else None, relu, pre, contract, depth, rows, 1)
                        two, g2 = _chain(g, x, w1, w2, bvec if bias else None, relu, pre, contract, depth, rows, 2)
                        _whole(one, g1, what)
                        _whole(two, g2, what)
                        assert _same_bits(one, two), what
    assert ran >= 2 * (9 + 9 + 3) - 6              # all forms on bf16x3; bf16x6 may lack a few for their LDS


def test_mode_is_checked(ga):
    """Mode 2 needs the uniform layout; a mode outside 0 .. 2 is refused; a refused call writes nothing."""
    from gwen_amd import _lib
    c = _lib.CONTRACT_BF16X3
    g = _graph(ga, "random")
    n = g.num_nodes
    x = _inputs(n, 1, 64)
    w, b = _params(64, 64)
    w2 = _params(64, 32, seed=1)[0]
    for out, guard in (_layer(g, x, w, b, True, c, 0, 0, 2, expect=EINVAL),
                       _chain(g, x, w, w2, b, True, False, c, 0, 0, 2, expect=EINVAL),
                       _chain(g, x, w, None, b, True, True, c, 0, 0, 2, expect=EINVAL),
                       _chain(g, x, None, None, None, True, True, c, 0, 0, 2, expect=EINVAL)):
        assert torch.isnan(out).all() and torch.isnan(guard).all()
    for mode in (0, 1):                            # the library's choice with a row pointer is mode 1
        a, _ = _layer(g, x, w, b, True, c, 0, 0, mode)
        assert torch.isfinite(a).all()
    g = _graph(ga, "mesh3")
    x = _inputs(g.num_nodes, 1, 64)
    for mode in (-1, 3, 9):
        for out, guard in (_layer(g, x, w, b, True, c, 0, 0, mode, expect=EINVAL),
                           _chain(g, x, w, w2, b, True, False, c, 0, 0, mode, expect=EINVAL),
                           _chain(g, x, None, None, None, True, True, c, 0, 0, mode, expect=EINVAL)):
            assert torch.isnan(out).all() and torch.isnan(guard).all()


def test_mode_zero_is_the_table(ga):
    """index_mode = 0 runs the mode the library names, and the older entry points are index_mode = 0."""
    from gwen_amd import _lib, ops
    L = _lib.lib()
    g = _graph(ga, "mesh10-hilbert")
    n = g.num_nodes
    for fin in WIDTHS:
        x = _inputs(n, 1, fin)
        for fout in WIDTHS:
            w, b = _params(fin, fout)
            for contract in (_lib.CONTRACT_BF16X3, _lib.CONTRACT_BF16X6, _lib.CONTRACT_F32):
                assert L.gwen_gcn_layer_index_mode(fin, fout, contract) in (1, 2)
                auto, ga_ = _layer(g, x, w, b, True, contract, 0, 0, 0)
                _whole(auto, ga_, (fin, fout, contract))
                assert _same_bits(auto, _layer(g, x, w, b, True, contract, 0, 0, 1)[0])
    x, (w, b) = _inputs(n, 1, 64), _params(64, 64)
    w2 = _params(64, 32, seed=1)[0]
    want = ops.layer_fused(g, x, w, b, relu=True, contract="bf16x6")
    for mode in (1, 2):
        assert _same_bits(want, ops.layer_fused(g, x, w, b, relu=True, contract="bf16x6", index_mode=mode))
        assert _same_bits(want, ops.layer_fused(g, x, w, b, relu=True, contract="bf16x6", depth=1, block_rows=96,
                                                index_mode=mode))
    want = ops.chain(g, x, w, w2, b, True, False, contract="bf16x6")
    for mode in (1, 2):
        assert _same_bits(want, ops.chain(g, x, w, w2, b, True, False, contract="bf16x6", index_mode=mode))
    want = ops.chain(g, x, None, None, b, True, True)
    assert _same_bits(want, ops.chain(g, x, None, None, b, True, True, index_mode=2))
    with pytest.raises(Exception):
        ops.layer_fused(g, x, w, b, index_mode=5)


def test_stack_equals_mode_one_layers(ga):
    """StackForward of GNNModel(64, 64) on the nu = 10 mesh, whatever modes the library ships, is bit for bit the chain
    of single-kernel calls with every layer forced to index_mode = 1."""
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
    got = plan.run(x)
    assert torch.isfinite(got).all()
    W = [plan._keep[3 * i] for i in range(nl)]
    B = [plan._keep[3 * i + 1] for i in range(nl)]
    c = [_lib.dense_contract(d.contract) for d in desc]
    relu = [bool(d.relu) for d in desc]
    h, _ = _chain(g, x, W[0], W[1], B[0], relu[0], False, c[0], 0, 0, 1)       # layer 0 + layer 1's projection
    h, _ = _chain(g, h, W[2], None, B[1], relu[1], True, c[2], 0, 0, 1)        # layer 1's gather + layer 2's projection
    h, _ = _chain(g, h, None, None, B[2], relu[2], True, _lib.CONTRACT_BF16X3, 0, 0, 1)
    for i in (3, 4, 5):
        h, _ = _layer(g, h, W[i], B[i], relu[i], c[i], 0, 0, 1)
    assert _same_bits(got, h)
