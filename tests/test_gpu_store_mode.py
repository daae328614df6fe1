"""The store mode of the narrow K4 / K5 forward and of k_gather (gather_rows.h, store_out; the trailing argument of
gwen_gcn_{layer,chain}_tuned4_f32): a forced mode changes how the output bytes travel, never a value.  Every forced mode
the build has is compared with mode 1 of the SAME call as int32 patterns over the whole allocation (x holds rows of -0.0;
the output allocation is pre-filled with a NaN payload), on outputs laid out by tests/strided.py -- guard rows in front of
and behind the output, row pitches Fout, Fout + 4 and 2 Fout for K4, a member stride with slack -- whose checker proves
every logical cell written and every other cell unchanged.

Shapes: N in {1, 15, 17, 79, 81, 162} are the first rows of the nu = 4 mesh (162 nodes: a grid of one block, a partial
last row tile, a partial last block) and 1 692 is the nu = 13 mesh (several blocks at every block size).  The full product
(width pair or form) x contraction x block rows x N is run; gathered entries (7 / 8), packed / unpacked W, members (1 / 3),
the row pitch and bias / ReLU cycle through it on counters of co-prime periods, so every value of every axis meets every
kernel."""
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
EINVAL = -1
MODES = (3,)                                   # the forced modes this build has beside 1 (2 and 4: reserved, refused)
NS = (1, 15, 17, 79, 81, 162, 1692)
# block_rows a width accepts (0 = the library's choice): whole gather passes of 1024 / Fin rows; 80: packed W at Fin = 64
LAYER_ROWS = {64: (0, 64, 80, 96, 112, 128), 32: (0, 64, 96, 128), 16: (0, 64, 128)}
CHAIN_ROWS = {64: (0, 64, 80, 96, 112), 32: (0, 64, 96), 16: (0, 64)}
CHAIN_FORMS = ((64, 64, 32, False), (32, 16, 0, True), (64, 32, 0, True))


@pytest.fixture(scope="module")
def ga(hip_lib):
    import gwen_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return gwen_amd


_graphs = {}


def _graph(ga, n):
    """The graph whose first n rows are launched: the nu = 4 mesh up to 162 rows, the nu = 13 mesh for 1 692."""
    nu = 4 if n <= 162 else 13
    if nu not in _graphs:
        m = ga.geodesic_mesh(nu)
        g = ga.prepare_graph(torch.from_numpy(np.ascontiguousarray(m.edge_index.astype(np.int64))).to(DEV), m.num_nodes)
        assert g.num_nodes == 10 * nu * nu + 2 and g.grouped()[0] is None and g.entries() == 7
        _graphs[nu] = g
    assert n <= _graphs[nu].num_nodes
    return _graphs[nu]


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


_cache = {}


def _inputs(rows, members, fin):
    """[members, rows, fin], shared by every case of a shape; rows 1 and rows - 1 of every member are all -0.0."""
    key = ("x", rows, members, fin)
    if key not in _cache:
        x = torch.randn(members, rows, fin, generator=torch.Generator().manual_seed(SEED + 131 * fin + members))
        x[:, 1] = -0.0
        x[:, rows - 1] = -0.0
        _cache[key] = x.contiguous().to(DEV)
    return _cache[key]


def _params(fin, fout, contract, seed=0):
    """(W, bias, packed images of W) of a width pair."""
    from gwen_amd import _lib
    key = ("w", fin, fout, contract, seed)
    if key not in _cache:
        g = torch.Generator().manual_seed(SEED + 7 * fin + fout + seed)
        w = (torch.randn(fout, fin, generator=g) / fin ** 0.5).to(DEV)
        b = (torch.randn(max(fin, fout), generator=g) * 0.1).to(DEV)
        nbytes = _lib.lib().gwen_gcn_packw_bytes(fin, fout, contract)
        wp = torch.zeros(nbytes // 4, device=DEV)
        assert _lib.lib().gwen_gcn_packw_f32(_p(w), fin, fout, contract, _p(wp), _st()) == 0
        _cache[key] = (w, b, wp)
    return _cache[key]


def _arena(members, n, width, pitch, slack):
    """One output [members, n, width] at row pitch `pitch` and member stride n * pitch + slack, two guard rows in front of
    the first logical cell (beside the arena's own lead-in) and the arena's guard (at least 64 pitches) behind."""
    a = strided.Arena(DEV)
    out = a.output(members, n, width, strided.Layout("store", pitch, n * pitch + slack, 2 * pitch))
    a.commit()
    return a, out


def _both_modes(arena, launch, what):
    """launch(mode) -> return code.  Mode 1, then every forced mode, on the same allocation: each run passes the arena's
    checker and leaves the allocation bit for bit as mode 1 left it."""
    assert launch(1) == 0, what
    arena.verify(str(what))
    want = arena.buf.view(torch.int32).clone()
    for mode in MODES:
        arena.reset()
        assert launch(mode) == 0, (what, mode)
        arena.verify(str((what, mode)))
        assert torch.equal(arena.buf.view(torch.int32), want), (what, mode)
    for mode in (2, 4):                                    # reserved: refused, nothing written
        arena.reset()
        assert launch(mode) == EINVAL, (what, mode)
        torch.cuda.synchronize()
        assert torch.equal(arena.buf.view(torch.int32), arena.before), (what, mode)


def _layer_call(g, x, n, w, b, wp, packed, relu, contract, rows, entries, out, members):
    from gwen_amd import _lib
    _, gc, gv = g.grouped()
    fout, fin = w.shape
    return lambda mode: _lib.lib().gwen_gcn_layer_tuned4_f32(
        None, _p(gc), _p(gv), _p(x), _p(w), _p(b), C.c_void_p(out.ptr), n, fin, fout, fin, out.ld, members,
        g.num_nodes * fin, out.mstride, int(relu), contract, entries, 0, rows, 0, _p(wp) if packed else None,
        2 if packed else 1, _st(), mode)


def _chain_call(g, x, n, fin, w1, w2, b, w1p, w2p, packed, relu, pre, contract, rows, entries, out, members):
    from gwen_amd import _lib
    _, gc, gv = g.grouped()
    f1 = 0 if w1 is None else w1.size(0)
    f2 = 0 if w2 is None else w2.size(0)
    return lambda mode: _lib.lib().gwen_gcn_chain_tuned4_f32(
        None, _p(gc), _p(gv), _p(x), _p(w1), _p(w2), _p(b), C.c_void_p(out.ptr), n, fin, f1, f2, int(pre), int(relu), members,
        g.num_nodes * fin, out.mstride, contract, entries, 0, rows, 0, _p(w1p) if packed else None,
        _p(w2p) if packed and f2 else None, 2 if packed else 1, _st(), mode)


def _contracts():
    from gwen_amd import _lib
    return (_lib.CONTRACT_BF16X3, _lib.CONTRACT_BF16X6)


@pytest.mark.parametrize("fin,fout", list(itertools.product(WIDTHS, repeat=2)))
def test_k4_forced_modes_equal_mode_1(ga, fin, fout):
    k = 0
    seen = set()
    for contract in _contracts():
        w, b, wp = _params(fin, fout, contract)
        for n in NS:
            g = _graph(ga, n)
            for rows in LAYER_ROWS[fin]:
                k += 1
                packed = rows == 80 or k % 2 == 0                      # 80 rows: the packed kernels only
                entries = 7 + (k // 2) % 2
                members = (1, 3)[(k // 4) % 2] if n <= 162 else 1 + 2 * (k % 2)
                pitch = (fout, fout + 4, 2 * fout)[k % 3]
                slack = 4 * (k % 5)
                bias, relu = k % 3 != 1, k % 7 < 4
                seen.add((packed, entries, members, pitch))
                x = _inputs(g.num_nodes, members, fin)
                arena, out = _arena(members, n, fout, pitch, slack)
                what = ("k4", fin, fout, contract, n, rows, packed, entries, members, pitch, slack, bias, relu)
                _both_modes(arena, _layer_call(g, x, n, w, b[:fout] if bias else None, wp, packed, relu, contract, rows,
                                               entries, out, members), what)
    for axis, values in enumerate(((False, True), (7, 8), (1, 3), (fout, fout + 4, 2 * fout))):
        assert {s[axis] for s in seen} == set(values), (axis, seen)


@pytest.mark.parametrize("fin,f1,f2,pre", CHAIN_FORMS)
def test_k5_forced_modes_equal_mode_1(ga, fin, f1, f2, pre):
    from gwen_amd import _lib
    k = 0
    seen = set()
    for contract in _contracts():
        assert _lib.lib().gwen_gcn_chain_supported(fin, f1, f2, int(pre), contract) == 1
        w1, b, w1p = _params(fin, f1, contract)
        w2, _, w2p = _params(f1, f2, contract, seed=1) if f2 else (None, None, None)
        for n in NS:
            g = _graph(ga, n)
            for rows in CHAIN_ROWS[fin]:
                k += 1
                packed = rows == 80 or k % 2 == 0
                entries = 7 + (k // 2) % 2
                members = (1, 3)[(k // 4) % 2] if n <= 162 else 1 + 2 * (k % 2)
                slack = 4 * (k % 5)
                bias, relu = k % 3 != 1, k % 7 < 4
                seen.add((packed, entries, members))
                x = _inputs(g.num_nodes, members, fin)
                fw = f2 or f1
                arena, out = _arena(members, n, fw, fw, slack)
                what = ("k5", fin, f1, f2, pre, contract, n, rows, packed, entries, members, slack, bias, relu)
                bvec = b[:fin if pre else f1] if bias else None
                _both_modes(arena, _chain_call(g, x, n, fin, w1, w2, bvec, w1p, w2p, packed, relu, pre, contract, rows,
                                               entries, out, members), what)
    for axis, values in enumerate(((False, True), (7, 8), (1, 3))):
        assert {s[axis] for s in seen} == set(values), (axis, seen)


@pytest.mark.parametrize("fin", WIDTHS)
def test_gather_forced_modes_equal_mode_1(ga, fin):
    k = 0
    for contract in _contracts():                          # k_gather contracts nothing: the argument only passes the checks
        _, b, _ = _params(fin, fin, contract)
        for n in NS:
            g = _graph(ga, n)
            for entries in (7, 8):
                for members in (1, 3):
                    k += 1
                    slack = 4 * (k % 5)
                    bias, relu = k % 3 != 1, k % 2 == 0
                    x = _inputs(g.num_nodes, members, fin)
                    arena, out = _arena(members, n, fin, fin, slack)
                    what = ("gather", fin, contract, n, entries, members, slack, bias, relu)
                    _both_modes(arena, _chain_call(g, x, n, fin, None, None, b[:fin] if bias else None, None, None, False,
                                                   relu, True, contract, 0, entries, out, members), what)


@pytest.mark.parametrize("mode", MODES)
def test_three_launches_on_one_stream(ga, mode):
    """K5 32 -> 16 activation-first in a forced mode, then k_gather<16>, then K4 16 -> 32 -- the middle of the 64-channel
    stack -- on one stream with nothing in between: each launch reads what the one before stored.  Bitwise the mode-1
    chain, and the second call bitwise the first."""
    from gwen_amd import ops
    n = 1692
    g = _graph(ga, n)
    x = _inputs(n, 1, 32)[0]
    c = "bf16x6"
    from gwen_amd import _lib
    w1, b1, _ = _params(32, 16, _lib.CONTRACT_BF16X6)
    w3, b3, _ = _params(16, 32, _lib.CONTRACT_BF16X6)

    def run(m):
        t = ops.chain(g, x, w1, None, b1[:32], True, True, contract=c, store_mode=m)
        t = ops.chain(g, t, None, None, b3[:16], True, True, contract=c, store_mode=1 if m == 1 else mode)
        return ops.layer_fused(g, t, w3, b3[:32], relu=True, contract=c, store_mode=1 if m == 1 else mode)

    want = run(1)
    first = run(mode)
    second = run(mode)
    torch.cuda.synchronize()
    assert torch.isfinite(want).all()
    assert torch.equal(want.view(torch.int32), first.view(torch.int32))
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))
