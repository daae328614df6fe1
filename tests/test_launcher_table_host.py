"""Every host-side rule of the K4 / K5 launchers (csrc/layer.hip, csrc/chain.hip) answers what it answered before the
block geometry became one set of constexpr functions and the dispatch macros one helper: supported widths, the library's
gather depth and the return codes of the argument checks over the grid of tests/golden/make_launcher_table.py, against
tests/golden/launcher_table.npz (generated on the commit before that change).  CPU only: null pointers and N = 0, so
every call returns before the first HIP call."""
import importlib.util
import os

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_launcher_table", os.path.join(_HERE, "golden", "make_launcher_table.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@pytest.fixture(scope="module")
def table(hip_lib):
    return G.table(hip_lib)                                # computed once: about 2e5 calls through ctypes


def test_launcher_rules_answer_as_before(table):
    want, got = np.load(G.FIXTURE), table
    assert sorted(got) == sorted(want.files)
    for name in want.files:
        assert got[name].shape == want[name].shape, name
        diff = np.argwhere(got[name] != want[name])
        assert diff.size == 0, (name, len(diff), "first differing grid index", diff[0].tolist(),
                                int(got[name][tuple(diff[0])]), int(want[name][tuple(diff[0])]))


def test_the_three_entry_points_agree(table):
    t = table
    e8, d0, r0 = G.L_ENTRIES.index(8), G.DEPTHS5.index(0), G.BLOCK_ROWS.index(0)
    assert np.array_equal(t["layer_plain"], t["layer_entries"][..., e8])                 # _f32 = _entries_f32(..., 8)
    assert np.array_equal(t["layer_entries"], t["layer_tuned"][..., d0, r0])             # _entries_f32 = _tuned_f32(..., 0, 0)
    e8, d0 = G.C_ENTRIES.index(8), G.C_DEPTHS.index(0)
    assert np.array_equal(t["chain_plain"], t["chain_entries"][..., e8])
    assert np.array_equal(t["chain_entries"], t["chain_tuned"][..., d0, r0])
