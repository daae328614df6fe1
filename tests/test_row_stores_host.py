"""Row stores of the narrow K4 forward through the C ABI (gwen_gcn_layer_tuned5_f32 = tuned4 + a trailing row_stores, and
gwen_gcn_layer_row_stores): where 2 is admitted, that tuned4 is tuned5 with 0, and what the query answers.
CPU only: every call below returns before the first HIP call (N = 0, or a refusal); no pointer is dereferenced."""
import itertools

import pytest

EINVAL = -1
X3, F32, X6 = 0, 1, 2
WIDTHS = (16, 32, 64)
ALL_WIDTHS = (16, 32, 64, 128, 256)
NULL7 = (None,) * 7
ROWPTR = 0x1000                                # some non-null address: the non-uniform layout

# The table as shipped (layer_row_stores in csrc/layer.hip; profiles/rowstore_kernel_ab.tsv): what row_stores = 0 runs on
# bf16x6 with one member.  A change that moves an entry has to change this line too.
SHIPPED = {(32, 64): 2, (16, 32): 2}                # 64 -> 64, the third written-through K4 launch, measured no gain: 1


def _layer5(lib, fin=64, fout=64, exact=X6, mode=0, rs=0, n=0, rowptr=None, entries=8, depth=0, rows=0, index_mode=0,
            members=1):
    return lib.gwen_gcn_layer_tuned5_f32(rowptr, *NULL7[1:], n, fin, fout, fin, fout, members, 0, 0, 0, exact, entries, depth,
                                         rows, index_mode, None, 0, None, mode, rs)


def _layer4(lib, fin, fout, exact, mode=0, n=0, entries=8, depth=0, rows=0, index_mode=0, members=1):
    return lib.gwen_gcn_layer_tuned4_f32(*NULL7, n, fin, fout, fin, fout, members, 0, 0, 0, exact, entries, depth, rows,
                                         index_mode, None, 0, None, mode)


@pytest.mark.parametrize("rs", [-1, 3, 4, 9])
def test_row_stores_outside_0_2_is_refused(hip_lib, rs):
    for n in (0, 100):                                             # with rows to launch as well: before any HIP call
        assert _layer5(hip_lib, rs=rs, n=n) == EINVAL
        assert _layer5(hip_lib, mode=3, rs=rs, n=n) == EINVAL
        assert _layer5(hip_lib, 256, 256, X3, rs=rs, n=n) == EINVAL


def test_0_and_1_exist_everywhere(hip_lib):
    for fin, fout in itertools.product(ALL_WIDTHS, repeat=2):
        for exact in (X3, F32, X6):
            for rs in (0, 1):
                for mode in (0, 1):
                    assert _layer5(hip_lib, fin, fout, exact, mode, rs) == 0
                    assert _layer5(hip_lib, fin, fout, exact, mode, rs, rowptr=ROWPTR) == 0
                    assert _layer5(hip_lib, fin, fout, exact, mode, rs, members=3) == 0


def test_row_stores_where_they_exist(hip_lib):
    """2: exactly where store mode 3 is admitted and the resolved store mode is 3."""
    for fin, fout in itertools.product(WIDTHS, repeat=2):
        for exact in (X3, X6):
            for entries in (7, 8):
                assert _layer5(hip_lib, fin, fout, exact, 3, 2, entries=entries) == 0
            d, im = hip_lib.gwen_gcn_layer_depth(fin, fout, exact), hip_lib.gwen_gcn_layer_index_mode(fin, fout, exact)
            assert _layer5(hip_lib, fin, fout, exact, 3, 2, depth=d, index_mode=im) == 0
            assert _layer5(hip_lib, fin, fout, exact, 3, 2, depth=3 - d) == EINVAL            # the other depth: not built
            assert _layer5(hip_lib, fin, fout, exact, 3, 2, index_mode=3 - im) == EINVAL      # the other index mode
            assert _layer5(hip_lib, fin, fout, exact, 3, 2, members=3) == 0                   # forced, several members
            assert _layer5(hip_lib, fin, fout, exact, 1, 2) == EINVAL                         # store mode 1 forced
            assert _layer5(hip_lib, fin, fout, exact, 1, 2, n=100) == EINVAL
            # store mode 0: 2 goes where the library's own store mode is 3, i.e. with one member on a switched shape
            lib_mode = hip_lib.gwen_gcn_layer_store_mode(fin, fout, exact)
            assert _layer5(hip_lib, fin, fout, exact, 0, 2) == (0 if lib_mode == 3 else EINVAL)
            assert _layer5(hip_lib, fin, fout, exact, 0, 2, members=3) == EINVAL
            for mode in (2, 4):                                                               # the reserved numbers stay refused
                for rs in (0, 1, 2):
                    assert _layer5(hip_lib, fin, fout, exact, mode, rs) == EINVAL
            for rows in (64, 80, 96, 112, 128):                    # block rows: what the width admits without images
                want = 0 if rows != 80 and rows % (1024 // fin) == 0 else EINVAL
                assert _layer5(hip_lib, fin, fout, exact, 3, 2, rows=rows) == want
                assert _layer5(hip_lib, fin, fout, exact, 3, 1, rows=rows) == want


def test_row_stores_are_refused_where_they_do_not_exist(hip_lib):
    """Wide widths, a row pointer, exact = 1 (the fp32-input MFMA): GWEN_EINVAL whatever the store mode, with and without
    rows to launch -- the refusal comes before any HIP call (this test runs without a GPU)."""
    for n in (0, 100):
        for mode in (0, 1, 3):
            for fin, fout in ((128, 64), (64, 128), (128, 128), (256, 256), (256, 16)):
                assert _layer5(hip_lib, fin, fout, X6, mode, 2, n=n) == EINVAL
                assert _layer5(hip_lib, fin, fout, X3, mode, 2, n=n) == EINVAL
            for fin, fout in itertools.product(WIDTHS, repeat=2):
                assert _layer5(hip_lib, fin, fout, X6, mode, 2, n=n, rowptr=ROWPTR) == EINVAL
                assert _layer5(hip_lib, fin, fout, F32, mode, 2, n=n) == EINVAL


def test_tuned4_is_tuned5_with_0(hip_lib):
    """Over the grid of the launcher table (tests/golden/make_launcher_table.py: widths, contraction, entries, depth,
    block rows), with the index modes, the store modes and the members on top."""
    import importlib.util
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("make_launcher_table", os.path.join(here, "golden", "make_launcher_table.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    bad = []
    for fi, fo, exact, entries, depth, rows in itertools.product(G.L_WIDTHS, G.L_WIDTHS, G.L_EXACT, G.L_ENTRIES, G.DEPTHS5,
                                                                 G.BLOCK_ROWS):
        for im, mode, members in itertools.product((0, 2), (0, 1, 2, 3, 4, 5), (1, 3)):
            a = _layer4(hip_lib, fi, fo, exact, mode, 0, entries, depth, rows, im, members)
            b = _layer5(hip_lib, fi, fo, exact, mode, 0, 0, None, entries, depth, rows, im, members)
            if a != b:
                bad.append((fi, fo, exact, entries, depth, rows, im, mode, members, a, b))
    assert not bad, (len(bad), bad[:5])


def test_query(hip_lib):
    for fin, fout in itertools.product(WIDTHS, repeat=2):
        for exact in (X3, X6):
            assert hip_lib.gwen_gcn_layer_row_stores(fin, fout, exact) in (1, 2)
        assert hip_lib.gwen_gcn_layer_row_stores(fin, fout, X3) == 1               # only bf16x6 was measured
        assert hip_lib.gwen_gcn_layer_row_stores(fin, fout, F32) == 1              # no row stores on the fp32-input MFMA
    for fin, fout in ((128, 64), (64, 256), (256, 256)):
        for exact in (X3, F32, X6):
            assert hip_lib.gwen_gcn_layer_row_stores(fin, fout, exact) == 1        # nor for wide layers
    assert hip_lib.gwen_gcn_layer_row_stores(64, 64, 3) == 0 and hip_lib.gwen_gcn_layer_row_stores(24, 64, X6) == 0
    assert hip_lib.gwen_gcn_layer_row_stores(64, 64, -1) == 0
    # row stores only ride on the written-through kernels: the query never says 2 where the store mode query does not say 3
    for fin, fout in itertools.product(WIDTHS, repeat=2):
        for exact in (X3, X6):
            if hip_lib.gwen_gcn_layer_row_stores(fin, fout, exact) == 2:
                assert hip_lib.gwen_gcn_layer_store_mode(fin, fout, exact) == 3
    # what ships is written down here
    for fin, fout in itertools.product(WIDTHS, repeat=2):
        assert hip_lib.gwen_gcn_layer_row_stores(fin, fout, X6) == SHIPPED.get((fin, fout), 1), (fin, fout)
    # a value the query names is one the entry point admits, with the library's own store mode
    for fin, fout in itertools.product(ALL_WIDTHS, repeat=2):
        for exact in (X3, F32, X6):
            assert _layer5(hip_lib, fin, fout, exact, 0, hip_lib.gwen_gcn_layer_row_stores(fin, fout, exact)) == 0
