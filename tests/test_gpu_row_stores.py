"""Row stores of the narrow K4 forward (k_layer's RS; the trailing argument of gwen_gcn_layer_tuned5_f32): the written-through
result tile leaves as whole rows through an fp32 out tile in LDS instead of as the MFMA holds it.  The switch changes how the
output bytes travel, never a value: row_stores = 2 is compared with row_stores = 1 of the SAME call as int32 patterns over the
whole allocation, on outputs laid out by tests/strided.py -- two guard rows in front of the output and the arena's guard
behind it, row pitches Fout, Fout + 4 and 2 Fout, a member stride with slack -- whose checker proves every logical cell
written and every other cell (pitch gaps, guards, member gaps) unchanged.

Graphs: the geodesic meshes nu = 1, 2, 6 (12, 42, 362 nodes: less than one 16-row tile, less than one block, several blocks
with a ragged last one at every block size -- 362 = 4 * 80 + 42 = 5 * 64 + 42 = 3 * 96 + 74 = 3 * 112 + 26 = 2 * 128 + 106) and
a graph of one row.  Per width pair the full product contraction x graph x block rows x gathered entries x packed / unpacked
W x members (1 / 3) is run; the row pitch, the member slack, bias / NULL and ReLU cycle through it on counters of co-prime
periods (3, 5, 7, 11; the product's inner axes have periods 2 and 4), and the test asserts that every value of every axis
was met and that packed and unpacked W met both member counts at every pitch."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import strided
from helpers import SEED

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WIDTHS = (16, 32, 64)
GRAPHS = (0, 1, 2, 6)                          # 0: the graph of one row; else the geodesic mesh of that nu
# block_rows a width accepts (0 = the library's choice): whole gather passes of 1024 / Fin rows; 80: packed W at Fin = 64
LAYER_ROWS = {64: (0, 64, 80, 96, 112, 128), 32: (0, 64, 96, 128), 16: (0, 64, 128)}


@pytest.fixture(scope="module")
def ga(hip_lib):
    import gwen_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return gwen_amd


_graphs = {}


def _graph(ga, nu):
    if nu not in _graphs:
        if nu == 0:
            g = ga.prepare_graph(torch.zeros(2, 1, dtype=torch.int64, device=DEV), 1)      # one node, its self loop
            assert g.num_nodes == 1
        else:
            m = ga.geodesic_mesh(nu)
            g = ga.prepare_graph(torch.from_numpy(np.ascontiguousarray(m.edge_index.astype(np.int64))).to(DEV), m.num_nodes)
            assert g.num_nodes == 10 * nu * nu + 2
        assert g.grouped()[0] is None and g.entries() == 7
        _graphs[nu] = g
    return _graphs[nu]


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


_cache = {}


def _inputs(rows, members, fin):
    """[members, rows, fin], shared by every case of a shape."""
    key = ("x", rows, members, fin)
    if key not in _cache:
        x = torch.randn(members, rows, fin, generator=torch.Generator().manual_seed(SEED + 131 * fin + members + rows))
        _cache[key] = x.contiguous().to(DEV)
    return _cache[key]


def _params(fin, fout, contract, seed=0):
    """(W, bias, packed images of W) of a width pair."""
    from gwen_amd import _lib
    key = ("w", fin, fout, contract, seed)
    if key not in _cache:
        g = torch.Generator().manual_seed(SEED + 7 * fin + fout + seed)
        w = (torch.randn(fout, fin, generator=g) / fin ** 0.5).to(DEV)
        b = (torch.randn(fout, generator=g) * 0.1).to(DEV)
        nbytes = _lib.lib().gwen_gcn_packw_bytes(fin, fout, contract)
        wp = torch.zeros(nbytes // 4, device=DEV)
        assert _lib.lib().gwen_gcn_packw_f32(_p(w), fin, fout, contract, _p(wp), _st()) == 0
        _cache[key] = (w, b, wp)
    return _cache[key]


def _arena(members, n, width, pitch, slack):
    a = strided.Arena(DEV)
    out = a.output(members, n, width, strided.Layout("rows", pitch, n * pitch + slack, 2 * pitch))
    a.commit()
    return a, out


def _call(g, x, w, b, wp, packed, relu, contract, rows, entries, out, members, store_mode=3):
    """launch(row_stores) -> return code, store mode 3 forced (the library's own choice is 1 on most of these shapes)."""
    from gwen_amd import _lib
    _, gc, gv = g.grouped()
    fout, fin = w.shape
    n = g.num_nodes
    return lambda rs: _lib.lib().gwen_gcn_layer_tuned5_f32(
        None, _p(gc), _p(gv), _p(x), _p(w), _p(b), C.c_void_p(out.ptr), n, fin, fout, fin, out.ld, members,
        n * fin, out.mstride, int(relu), contract, entries, 0, rows, 0, _p(wp) if packed else None,
        2 if packed else 1, _st(), store_mode, rs)


def _rows_equal(arena, launch, what):
    """row_stores = 1, then 2, on the same allocation: each run passes the arena's checker, and 2 leaves the allocation bit
    for bit as 1 left it."""
    assert launch(1) == 0, what
    arena.verify(str(what))
    want = arena.buf.view(torch.int32).clone()
    arena.reset()
    assert launch(2) == 0, what
    arena.verify(str((what, "row stores")))
    assert torch.equal(arena.buf.view(torch.int32), want), what
    return want


def _contracts():
    from gwen_amd import _lib
    return (_lib.CONTRACT_BF16X3, _lib.CONTRACT_BF16X6)


@pytest.mark.parametrize("fin,fout", list(itertools.product(WIDTHS, repeat=2)))
def test_row_stores_equal_lane_stores(ga, fin, fout):
    k = 0
    seen = set()
    for contract in _contracts():
        w, b, wp = _params(fin, fout, contract)
        for nu in GRAPHS:
            g = _graph(ga, nu)
            n = g.num_nodes
            for rows, entries, packed in itertools.product(LAYER_ROWS[fin], (7, 8), (False, True)):
                if rows == 80 and not packed:                          # 80 rows: the packed kernels only
                    continue
                for members in (1, 3):                                 # both with every kernel: no counter to alias with
                    k += 1
                    pitch = (fout, fout + 4, 2 * fout)[k % 3]
                    slack = 4 * (1 + k % 5)
                    bias, relu = k % 7 < 4, k % 11 < 6
                    seen.add((packed, members, pitch, bias, relu))
                    x = _inputs(n, members, fin)
                    arena, out = _arena(members, n, fout, pitch, slack)
                    what = ("k4", fin, fout, contract, nu, rows, entries, packed, members, pitch, slack, bias, relu)
                    _rows_equal(arena, _call(g, x, w, b if bias else None, wp, packed, relu, contract, rows, entries, out,
                                             members), what)
    for axis, values in enumerate(((False, True), (1, 3), (fout, fout + 4, 2 * fout), (False, True), (False, True))):
        assert {s[axis] for s in seen} == set(values), (axis, seen)
    # packed / unpacked W meets both member counts and every pitch (the shipped form is unpacked W with one member)
    assert {s[:3] for s in seen} == set(itertools.product((False, True), (1, 3), (fout, fout + 4, 2 * fout))), seen


@pytest.mark.parametrize("fin,fout", [(64, 64), (32, 64), (16, 32)])
def test_library_choice_is_one_of_the_two(ga, fin, fout):
    """row_stores = 0 and store_mode = 0 with one member -- what the stack launcher runs -- against lane stores, mode 1."""
    from gwen_amd import _lib
    g = _graph(ga, 6)
    n = g.num_nodes
    w, b, wp = _params(fin, fout, _lib.CONTRACT_BF16X6)
    x = _inputs(n, 1, fin)
    for pitch in (fout, fout + 4):
        arena, out = _arena(1, n, fout, pitch, 0)
        assert _call(g, x, w, b, wp, False, True, _lib.CONTRACT_BF16X6, 0, 7, out, 1, store_mode=1)(1) == 0
        arena.verify("plain")
        want = arena.buf.view(torch.int32).clone()
        arena.reset()
        assert _call(g, x, w, b, wp, False, True, _lib.CONTRACT_BF16X6, 0, 7, out, 1, store_mode=0)(0) == 0
        arena.verify("library's choice")
        assert torch.equal(arena.buf.view(torch.int32), want)


@pytest.mark.parametrize("fin,fout", [(64, 64), (16, 32), (32, 16)])
def test_special_values_travel_unchanged(ga, fin, fout):
    """NaN, +-Inf and -0 in x: whatever the arithmetic makes of them, both layouts store the same patterns."""
    from gwen_amd import _lib
    g = _graph(ga, 6)
    n = g.num_nodes
    x = _inputs(n, 1, fin).clone()
    x[0, 3, :] = -0.0
    x[0, 100, 1] = float("nan")
    x[0, 200, 2] = float("inf")
    x[0, 300, 3] = float("-inf")
    x[0, n - 1, :] = -0.0
    for contract in _contracts():
        w, b, wp = _params(fin, fout, contract)
        for relu in (False, True):
            arena, out = _arena(1, n, fout, fout + 4, 8)
            _rows_equal(arena, _call(g, x, w, b, wp, False, relu, contract, 0, 7, out, 1), ("special", fin, fout, contract))
            vals = out.values()
            assert torch.isnan(vals).any() and not torch.isnan(vals).all()


def test_same_call_twice(ga):
    """The same row-store launch twice: bitwise the same allocation (nothing depends on what LDS or the output held)."""
    from gwen_amd import _lib
    g = _graph(ga, 6)
    n = g.num_nodes
    for fin, fout, rows, packed in ((64, 64, 80, True), (32, 64, 64, False), (16, 32, 64, False)):
        w, b, wp = _params(fin, fout, _lib.CONTRACT_BF16X6)
        x = _inputs(n, 3, fin)
        arena, out = _arena(3, n, fout, 2 * fout, 12)
        launch = _call(g, x, w, b, wp, packed, True, _lib.CONTRACT_BF16X6, rows, 7, out, 3)
        assert launch(2) == 0
        arena.verify("first")
        first = arena.buf.view(torch.int32).clone()
        assert launch(2) == 0                                          # over its own output, no reset
        arena.verify("second")
        assert torch.equal(arena.buf.view(torch.int32), first)
        arena.reset()
        assert launch(2) == 0
        arena.verify("third")
        assert torch.equal(arena.buf.view(torch.int32), first)


def test_c2_stack_equals_per_layer_calls_without_row_stores(ga):
    """The c2-shaped StackForward at nu = 6 -- the library's choices, row stores included -- bit for bit the chain of
    per-layer calls with row_stores = 1."""
    from gwen_amd import _lib
    L = _lib.lib()
    g = _graph(ga, 6)
    n = g.num_nodes
    _, gc, gv = g.grouped()
    torch.manual_seed(SEED)
    model = ga.GNNModel(ga.GNNConfig(1, 1, 64, 64, 64)).to(DEV)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
    plan = ga.StackForward(model.stack(), g)
    desc, nl = plan.desc, len(plan.desc)
    assert [(d.fin, d.fout) for d in desc] == [(64, 64), (64, 32), (32, 16), (16, 32), (32, 64), (64, 64)]
    W = [plan._keep[3 * i] for i in range(nl)]
    B = [plan._keep[3 * i + 1] for i in range(nl)]
    c = [_lib.dense_contract(d.contract) for d in desc]
    relu = [int(bool(d.relu)) for d in desc]
    x = _inputs(n, 1, 64)[0].contiguous()

    def chain(h, w1, w2, b, r, pre, contract):
        fin = h.size(-1)
        f1 = 0 if w1 is None else w1.size(0)
        f2 = 0 if w2 is None else w2.size(0)
        fw = f2 or f1 or fin
        out = torch.full((n, fw), float("nan"), device=DEV)
        assert L.gwen_gcn_chain_tuned3_f32(None, _p(gc), _p(gv), _p(h), _p(w1), _p(w2), _p(b), _p(out), n, fin, f1, f2, int(pre),
                                           r, 1, n * fin, n * fw, contract, 7, 0, 0, 0, None, None, 0, _st()) == 0
        return out

    def layer(h, w, b, r, contract):
        fout, fin = w.shape
        out = torch.full((n, fout), float("nan"), device=DEV)
        assert L.gwen_gcn_layer_tuned5_f32(None, _p(gc), _p(gv), _p(h), _p(w), _p(b), _p(out), n, fin, fout, fin, fout, 1,
                                           n * fin, n * fout, r, contract, 7, 0, 0, 0, None, 0, _st(), 0, 1) == 0
        return out

    h = chain(x, W[0], W[1], B[0], relu[0], False, c[0])
    h = chain(h, W[2], None, B[1], relu[1], True, c[2])
    h = chain(h, None, None, B[2], relu[2], True, _lib.CONTRACT_BF16X3)
    for i in (3, 4, 5):
        h = layer(h, W[i], B[i], relu[i], c[i])
    assert torch.isfinite(h).all()
    ev = ga.KernelEvents(12)
    got = plan.run(x, events=ev).clone()
    assert [k for k, *_ in ev.durations()] == ["chain"] * 3 + ["layer"] * 3
    assert torch.equal(got.view(torch.int32), h.view(torch.int32))
    assert torch.equal(plan.run(x).view(torch.int32), h.view(torch.int32))
