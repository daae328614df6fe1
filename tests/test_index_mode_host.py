"""The host-side answers of the index mode of K4 / K5 (csrc/layer.hip, csrc/chain.hip; gather_rows.h, IM):
gwen_gcn_layer_index_mode / gwen_gcn_chain_index_mode and the argument checks of the *_tuned2_f32 entry points.
index_mode 0 is the library's choice, 1 the per-lane group loads, 2 the record form -- narrow kernels on the uniform
layout only.  The *_tuned_f32 entry points are *_tuned2_f32 with 0.  CPU only: N = 0, so every call returns before the
first HIP call; the row pointer of the "non-uniform" calls is a host address that is never read."""
import ctypes as C
import itertools

import pytest

OK, EINVAL = 0, -1
WIDTHS = (8, 16, 32, 64, 128, 256)
NARROW = (16, 32, 64)
N7 = [None] * 7
N8 = [None] * 8


@pytest.fixture(scope="module")
def L(hip_lib):
    return hip_lib


@pytest.fixture(scope="module")
def rowptr():
    buf = (C.c_int32 * 4)()
    return C.cast(buf, C.c_void_p), buf                    # the buffer lives as long as the pointer


def _layer(L, fi, fo, exact, mode, rp=None, entries=7, depth=0, rows=0):
    return L.gwen_gcn_layer_tuned2_f32(rp, *N7[1:], 0, fi, fo, fi, fo, 1, 0, 0, 0, exact, entries, depth, rows, mode, None)


def _chain(L, fi, f1, f2, pre, contract, mode, rp=None, entries=7, depth=0, rows=0):
    return L.gwen_gcn_chain_tuned2_f32(rp, *N8[1:], 0, fi, f1, f2, pre, 0, 1, 0, 0, contract, entries, depth, rows, mode,
                                       None)


def test_layer_index_mode_names_a_mode(L):
    for fi, fo, exact in itertools.product(WIDTHS, WIDTHS, (-1, 0, 1, 2, 3)):
        got = L.gwen_gcn_layer_index_mode(fi, fo, exact)
        if not L.gwen_gcn_layer_supported(fi, fo) or exact not in (0, 1, 2):
            assert got == 0, (fi, fo, exact)
        elif fi > 64 or fo > 64:
            assert got == 1, (fi, fo, exact)                # the record form exists on narrow layers only
        else:
            assert got in (1, 2), (fi, fo, exact)
        assert (got == 0) == (L.gwen_gcn_layer_depth(fi, fo, exact) == 0)


def test_chain_index_mode_names_a_mode(L):
    W0 = (0,) + WIDTHS
    for fi, f1, f2, pre, contract in itertools.product(W0, W0, W0, (0, 1), (0, 1, 2, 3)):
        got = L.gwen_gcn_chain_index_mode(fi, f1, f2, pre, contract)
        if not L.gwen_gcn_chain_supported(fi, f1, f2, pre, contract):
            assert got == 0, (fi, f1, f2, pre, contract)
        elif fi > 64 or f1 > 64:
            assert got == 1, (fi, f1, f2, pre, contract)
        else:
            assert got in (1, 2), (fi, f1, f2, pre, contract)


def test_layer_mode_is_checked(L, rowptr):
    rp = rowptr[0]
    for fi, fo, exact in itertools.product(WIDTHS, WIDTHS, (0, 1, 2)):
        ok = bool(L.gwen_gcn_layer_supported(fi, fo))
        narrow = fi in NARROW and fo in NARROW
        for mode in (-1, 3, 7):
            assert _layer(L, fi, fo, exact, mode) == EINVAL
        for mode in (0, 1):
            assert _layer(L, fi, fo, exact, mode) == (OK if ok else EINVAL), (fi, fo, exact, mode)
            assert _layer(L, fi, fo, exact, mode, rp=rp) == (OK if ok else EINVAL), (fi, fo, exact, mode)
        assert _layer(L, fi, fo, exact, 2) == (OK if narrow else EINVAL), (fi, fo, exact)
        assert _layer(L, fi, fo, exact, 2, rp=rp) == EINVAL, (fi, fo, exact)       # records: uniform layout only
    # the other checks stand beside it
    assert _layer(L, 64, 64, 2, 2, entries=6) == EINVAL
    assert _layer(L, 64, 64, 2, 2, depth=3) == EINVAL
    assert _layer(L, 32, 64, 2, 2, rows=112) == EINVAL
    for depth, rows, entries in itertools.product((0, 1, 2), (0, 64, 96, 112, 128), (7, 8)):
        assert _layer(L, 64, 64, 2, 2, entries=entries, depth=depth, rows=rows) == OK


def test_chain_mode_is_checked(L, rowptr):
    rp = rowptr[0]
    W0 = (0, 16, 32, 64, 128)
    for fi, f1, f2, pre, contract in itertools.product(W0, W0, (0, 16, 32, 64), (0, 1), (0, 2)):
        ok = bool(L.gwen_gcn_chain_supported(fi, f1, f2, pre, contract))
        narrow = fi <= 64 and f1 <= 64
        for mode in (-1, 3):
            assert _chain(L, fi, f1, f2, pre, contract, mode) == EINVAL
        for mode in (0, 1):
            assert _chain(L, fi, f1, f2, pre, contract, mode) == (OK if ok else EINVAL), (fi, f1, f2, pre, contract)
            assert _chain(L, fi, f1, f2, pre, contract, mode, rp=rp) == (OK if ok else EINVAL)
        assert _chain(L, fi, f1, f2, pre, contract, 2) == (OK if ok and narrow else EINVAL), (fi, f1, f2, pre, contract)
        assert _chain(L, fi, f1, f2, pre, contract, 2, rp=rp) == EINVAL
    assert _chain(L, 64, 64, 32, 0, 2, 2, rows=128) == EINVAL
    assert _chain(L, 16, 0, 0, 1, 0, 2, rows=64) == OK and _chain(L, 16, 0, 0, 1, 0, 2, rows=32) == EINVAL


def test_tuned_is_tuned2_with_zero(L, rowptr):
    """The old entry points answer what the new ones answer with index_mode = 0, over widths, depth and block rows."""
    for rp in (None, rowptr[0]):
        for fi, fo, exact, depth, rows in itertools.product(WIDTHS, WIDTHS, (0, 1, 2, 3), (-1, 0, 1, 2, 3),
                                                            (0, 32, 64, 96, 112, 128)):
            old = L.gwen_gcn_layer_tuned_f32(rp, *N7[1:], 0, fi, fo, fi, fo, 1, 0, 0, 0, exact, 7, depth, rows, None)
            assert old == _layer(L, fi, fo, exact, 0, rp=rp, depth=depth, rows=rows), (fi, fo, exact, depth, rows)
        for fi, f1, f2, pre, depth, rows in itertools.product((16, 32, 64, 128), (0, 16, 32, 64, 128), (0, 16, 32),
                                                              (0, 1), (0, 1, 2, 3), (0, 64, 96, 112, 128)):
            old = L.gwen_gcn_chain_tuned_f32(rp, *N8[1:], 0, fi, f1, f2, pre, 0, 1, 0, 0, 2, 7, depth, rows, None)
            assert old == _chain(L, fi, f1, f2, pre, 2, 0, rp=rp, depth=depth, rows=rows), (fi, f1, f2, pre, depth, rows)
