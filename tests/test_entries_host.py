"""Argument checks of the entries-per-group entry points (gwen_gcn_layer_entries_f32, gwen_gcn_chain_entries_f32,
gwen_gnn_forward_entries_f32, gwen_gcn_max_entries) through the C ABI.  CPU only: every call below returns before the
first HIP call."""
import ctypes as C

import pytest

EINVAL, ENOSPACE = -1, -3


def _layer(lib, entries, n=0):
    return lib.gwen_gcn_layer_entries_f32(None, None, None, None, None, None, None, n, 16, 16, 16, 16, 1, 0, 0, 0, 0,
                                          entries, None)


def _chain(lib, entries, n=0):
    return lib.gwen_gcn_chain_entries_f32(None, None, None, None, None, None, None, None, n, 64, 64, 32, 0, 1, 1, 0, 0, 0,
                                          entries, None)


@pytest.mark.parametrize("entries", [-1, 0, 1, 6, 9, 16])
def test_entries_outside_7_and_8_are_refused(hip_lib, entries):
    assert _layer(hip_lib, entries) == EINVAL
    assert _chain(hip_lib, entries) == EINVAL


@pytest.mark.parametrize("entries", [7, 8])
def test_entries_7_and_8_pass_the_check(hip_lib, entries):
    assert _layer(hip_lib, entries) == 0                   # N = 0: nothing to do
    assert _chain(hip_lib, entries) == 0
    assert _layer(hip_lib, entries, n=5) == EINVAL         # ... and the pointer checks still follow
    assert _chain(hip_lib, entries, n=5) == EINVAL


def test_stack_launcher_checks_entries(hip_lib):
    from gwen_amd import _lib
    gd = _lib.GraphDesc()
    gd.N = 0
    desc = (_lib.LayerDesc * 1)()
    desc[0].fin, desc[0].fout, desc[0].order, desc[0].contract = 16, 16, _lib.ORDER_AUTO, _lib.CONTRACT_BF16X3

    def run(entries):
        return hip_lib.gwen_gnn_forward_entries_f32(C.byref(gd), desc, 1, None, None, None, 0, 1, None, None, None, 0,
                                                    None, None, entries)
    for bad in (0, 6, 9):
        assert run(bad) == EINVAL
    for ok in (7, 8):
        assert run(ok) == ENOSPACE                         # past the entries check: no scratch was given
    assert hip_lib.gwen_gnn_forward_f32(C.byref(gd), desc, 1, None, None, None, 0, 1, None, None, None, 0,
                                        None, None) == ENOSPACE


def test_max_entries_argument_checks(hip_lib):
    assert hip_lib.gwen_gcn_max_entries(None, -1, None, None) == EINVAL
    assert hip_lib.gwen_gcn_max_entries(None, 0, None, None) == EINVAL       # nowhere to write the bound
    assert hip_lib.gwen_gcn_max_entries(None, 5, 16, None) == EINVAL         # rows without a row pointer
