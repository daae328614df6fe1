"""The store mode of the narrow K4 / K5 forward through the C ABI (gwen_gcn_{layer,chain}_tuned4_f32 and the two mode
queries): which modes are admitted where, that the older entry points are tuned4 with mode 0, and what the queries answer.
CPU only: every call below returns before the first HIP call (N = 0, or a refusal); no pointer is dereferenced."""
import itertools

import pytest

EINVAL = -1
X3, F32, X6 = 0, 1, 2
WIDTHS = (16, 32, 64)
NULL7, NULL8 = (None,) * 7, (None,) * 8
ROWPTR = 0x1000                                # some non-null address: the non-uniform layout


def _layer(lib, fin=64, fout=64, exact=X6, mode=0, n=0, rowptr=None, entries=8, depth=0, rows=0, index_mode=0, members=1):
    return lib.gwen_gcn_layer_tuned4_f32(rowptr, *NULL7[1:], n, fin, fout, fin, fout, members, 0, 0, 0, exact, entries, depth,
                                         rows, index_mode, None, 0, None, mode)


def _layer3(lib, fin, fout, exact, n=0, entries=8, depth=0, rows=0, index_mode=0):
    return lib.gwen_gcn_layer_tuned3_f32(*NULL7, n, fin, fout, fin, fout, 1, 0, 0, 0, exact, entries, depth, rows, index_mode,
                                         None, 0, None)


def _chain(lib, fin=64, f1=64, f2=32, pre=0, contract=X6, mode=0, n=0, rowptr=None, entries=8, depth=0, rows=0,
           index_mode=0, members=1):
    return lib.gwen_gcn_chain_tuned4_f32(rowptr, *NULL8[1:], n, fin, f1, f2, pre, 1, members, 0, 0, contract, entries, depth,
                                         rows, index_mode, None, None, 0, None, mode)


def _chain3(lib, fin, f1, f2, pre, contract, n=0, entries=8, depth=0, rows=0, index_mode=0):
    return lib.gwen_gcn_chain_tuned3_f32(*NULL8, n, fin, f1, f2, pre, 1, 1, 0, 0, contract, entries, depth, rows, index_mode,
                                         None, None, 0, None)


@pytest.mark.parametrize("mode", [-1, 5, 9])
def test_store_mode_outside_0_4_is_refused(hip_lib, mode):
    assert _layer(hip_lib, mode=mode) == EINVAL
    assert _chain(hip_lib, mode=mode) == EINVAL
    assert _chain(hip_lib, 32, 16, 0, 1, mode=mode) == EINVAL
    assert _chain(hip_lib, 16, 0, 0, 1, mode=mode) == EINVAL
    # ... with rows to launch as well: the refusal comes before any HIP call
    assert _layer(hip_lib, mode=mode, n=100) == EINVAL and _chain(hip_lib, mode=mode, n=100) == EINVAL


def test_modes_0_and_1_exist_everywhere(hip_lib):
    for fin, fout in itertools.product((16, 32, 64, 128, 256), repeat=2):
        for exact in (X3, F32, X6):
            for mode in (0, 1):
                assert _layer(hip_lib, fin, fout, exact, mode) == 0
                assert _layer(hip_lib, fin, fout, exact, mode, rowptr=ROWPTR) == 0
    for mode in (0, 1):
        assert _chain(hip_lib, 128, 128, 0, 1, X3, mode) == 0
        assert _chain(hip_lib, 64, 64, 32, 0, X6, mode, rowptr=ROWPTR) == 0
        assert _chain(hip_lib, 128, 0, 0, 1, X6, mode) == 0


def test_written_through_stores_where_they_exist(hip_lib):
    """Mode 3: narrow widths, a bf16 split, the uniform layout, the library's depth and index mode for the shape."""
    for fin, fout in itertools.product(WIDTHS, repeat=2):
        for exact in (X3, X6):
            for entries in (7, 8):
                assert _layer(hip_lib, fin, fout, exact, 3, entries=entries) == 0
            d, im = hip_lib.gwen_gcn_layer_depth(fin, fout, exact), hip_lib.gwen_gcn_layer_index_mode(fin, fout, exact)
            assert _layer(hip_lib, fin, fout, exact, 3, depth=d, index_mode=im) == 0
            assert _layer(hip_lib, fin, fout, exact, 3, depth=3 - d) == EINVAL            # the other depth: not built
            assert _layer(hip_lib, fin, fout, exact, 3, index_mode=3 - im) == EINVAL      # the other index mode: not built
            assert _layer(hip_lib, fin, fout, exact, 3, members=3) == 0
    for fin, f1, f2, pre in ((64, 64, 32, 0), (32, 16, 0, 1), (64, 32, 0, 1), (64, 64, 16, 0), (16, 32, 0, 1)):
        for c in (X3, X6):
            assert hip_lib.gwen_gcn_chain_supported(fin, f1, f2, pre, c) == 1
            assert _chain(hip_lib, fin, f1, f2, pre, c, 3) == 0
            assert _chain(hip_lib, fin, f1, f2, pre, c, 3, entries=7) == 0
            d = hip_lib.gwen_gcn_chain_depth(fin, f1, f2, pre, c)
            im = hip_lib.gwen_gcn_chain_index_mode(fin, f1, f2, pre, c)
            assert _chain(hip_lib, fin, f1, f2, pre, c, 3, depth=d, index_mode=im) == 0
            assert _chain(hip_lib, fin, f1, f2, pre, c, 3, depth=3 - d) == EINVAL
            assert _chain(hip_lib, fin, f1, f2, pre, c, 3, index_mode=3 - im) == EINVAL
    for fin in WIDTHS:                                             # the plain gather: one code at both depths
        for depth in (0, 1, 2):
            assert _chain(hip_lib, fin, 0, 0, 1, X6, 3, depth=depth) == 0
        assert _chain(hip_lib, fin, 0, 0, 1, X6, 3, index_mode=2) == EINVAL


@pytest.mark.parametrize("mode", [2, 3, 4])
def test_modes_2_to_4_are_refused_where_they_do_not_exist(hip_lib, mode):
    """Wide widths, a row pointer, exact = 1 (the fp32-input MFMA): GWEN_EINVAL, with and without rows to launch -- the
    refusal comes before any HIP call (this test runs without a GPU)."""
    for n in (0, 100):
        for fin, fout in ((128, 64), (64, 128), (128, 128), (256, 256), (256, 16)):
            assert _layer(hip_lib, fin, fout, X6, mode, n=n) == EINVAL
            assert _layer(hip_lib, fin, fout, X3, mode, n=n) == EINVAL
        for fin, fout in itertools.product(WIDTHS, repeat=2):
            assert _layer(hip_lib, fin, fout, X6, mode, n=n, rowptr=ROWPTR) == EINVAL
            assert _layer(hip_lib, fin, fout, F32, mode, n=n) == EINVAL
        assert _chain(hip_lib, 128, 128, 0, 1, X3, mode, n=n) == EINVAL
        assert _chain(hip_lib, 128, 64, 0, 1, X3, mode, n=n) == EINVAL
        assert _chain(hip_lib, 128, 0, 0, 1, X6, mode, n=n) == EINVAL
        assert _chain(hip_lib, 64, 64, 32, 0, X6, mode, n=n, rowptr=ROWPTR) == EINVAL
        assert _chain(hip_lib, 32, 16, 0, 1, X6, mode, n=n, rowptr=ROWPTR) == EINVAL
        assert _chain(hip_lib, 16, 0, 0, 1, X6, mode, n=n, rowptr=ROWPTR) == EINVAL
        assert _chain(hip_lib, 64, 64, 32, 0, F32, mode, n=n) == EINVAL


@pytest.mark.parametrize("mode", [2, 4])
def test_row_stores_are_not_built(hip_lib, mode):
    """Modes 2 and 4 (whole rows through LDS) are reserved numbers of the ABI: refused on every shape."""
    for fin, fout in itertools.product(WIDTHS, repeat=2):
        assert _layer(hip_lib, fin, fout, X6, mode) == EINVAL
    assert _chain(hip_lib, 64, 64, 32, 0, X6, mode) == EINVAL
    assert _chain(hip_lib, 16, 0, 0, 1, X6, mode) == EINVAL


def test_tuned3_is_tuned4_with_mode_0(hip_lib):
    """Over the grid of the launcher table (tests/golden/make_launcher_table.py: widths, contraction, entries, depth,
    block rows), with the index modes on top."""
    import importlib.util
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("make_launcher_table", os.path.join(here, "golden", "make_launcher_table.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    bad = []
    for fi, fo, exact, entries, depth, rows in itertools.product(G.L_WIDTHS, G.L_WIDTHS, G.L_EXACT, G.L_ENTRIES, G.DEPTHS5,
                                                                 G.BLOCK_ROWS):
        for im in (0, 2):
            a = _layer3(hip_lib, fi, fo, exact, 0, entries, depth, rows, im)
            b = _layer(hip_lib, fi, fo, exact, 0, 0, None, entries, depth, rows, im)
            if a != b:
                bad.append(("layer", fi, fo, exact, entries, depth, rows, im, a, b))
    for fi, f1, f2, pre, c, entries, depth, rows in itertools.product(G.C_WIDTHS, G.C_WIDTHS, G.C_WIDTHS, G.C_PRE,
                                                                      G.C_CONTRACT, G.C_ENTRIES, G.C_DEPTHS, G.BLOCK_ROWS):
        a = _chain3(hip_lib, fi, f1, f2, pre, c, 0, entries, depth, rows, 0)
        b = _chain(hip_lib, fi, f1, f2, pre, c, 0, 0, None, entries, depth, rows, 0)
        if a != b:
            bad.append(("chain", fi, f1, f2, pre, c, entries, depth, rows, a, b))
    assert not bad, (len(bad), bad[:5])


def test_mode_queries(hip_lib):
    for fin, fout in itertools.product(WIDTHS, repeat=2):
        for exact in (X3, X6):
            assert hip_lib.gwen_gcn_layer_store_mode(fin, fout, exact) in (1, 2, 3, 4)
        assert hip_lib.gwen_gcn_layer_store_mode(fin, fout, X3) == 1              # only bf16x6 was measured
        assert hip_lib.gwen_gcn_layer_store_mode(fin, fout, F32) == 1             # no modes on the fp32-input MFMA
    for fin, fout in ((128, 64), (64, 256), (256, 256)):
        assert hip_lib.gwen_gcn_layer_store_mode(fin, fout, X6) == 1              # nor for wide layers
    assert hip_lib.gwen_gcn_layer_store_mode(64, 64, 3) == 0 and hip_lib.gwen_gcn_layer_store_mode(24, 64, X6) == 0
    for fin, f1 in itertools.product(WIDTHS, repeat=2):
        for c in (X3, X6):
            if hip_lib.gwen_gcn_chain_supported(fin, f1, 0, 1, c):
                assert hip_lib.gwen_gcn_chain_store_mode(fin, f1, 0, 1, c) in (1, 2, 3, 4)
            for f2 in WIDTHS:
                want = (1, 2, 3, 4) if hip_lib.gwen_gcn_chain_supported(fin, f1, f2, 0, c) else (0,)
                assert hip_lib.gwen_gcn_chain_store_mode(fin, f1, f2, 0, c) in want
        assert hip_lib.gwen_gcn_chain_store_mode(fin, f1, 0, 1, X3) in (0, 1)
    for fin in WIDTHS:
        assert hip_lib.gwen_gcn_chain_store_mode(fin, 0, 0, 1, X6) in (1, 3)       # k_gather stores whole rows already
        assert hip_lib.gwen_gcn_chain_store_mode(fin, 0, 0, 1, X3) == hip_lib.gwen_gcn_chain_store_mode(fin, 0, 0, 1, X6)
    assert hip_lib.gwen_gcn_chain_store_mode(128, 128, 0, 1, X3) == 1
    assert hip_lib.gwen_gcn_chain_store_mode(64, 64, 32, 0, F32) == 0
    # the c2 step's shapes: what was measured decides (profiles/store_kernel_ab.tsv), and what ships is written down here
    shipped = {"layer": {(64, 64): 3, (32, 64): 3, (16, 32): 3},
               "chain": {(64, 64, 32, 0): 3, (32, 16, 0, 1): 3, (16, 0, 0, 1): 3}}
    for (fin, fout), mode in shipped["layer"].items():
        assert hip_lib.gwen_gcn_layer_store_mode(fin, fout, X6) == mode
    for (fin, f1, f2, pre), mode in shipped["chain"].items():
        assert hip_lib.gwen_gcn_chain_store_mode(fin, f1, f2, pre, X6) == mode
    # a mode the query names is one the entry point admits
    for fin, fout in itertools.product(WIDTHS, repeat=2):
        assert _layer(hip_lib, fin, fout, X6, hip_lib.gwen_gcn_layer_store_mode(fin, fout, X6)) == 0
    for fin, f1, f2, pre in ((64, 64, 32, 0), (32, 16, 0, 1), (64, 32, 0, 1), (16, 0, 0, 1)):
        assert _chain(hip_lib, fin, f1, f2, pre, X6, hip_lib.gwen_gcn_chain_store_mode(fin, f1, f2, pre, X6)) == 0
