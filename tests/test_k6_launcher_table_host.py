"""Every host-side rule of the K6 launchers (csrc/interact.hip, csrc/interact_rows.hip) answers what it answered before
their arguments became structs (csrc/interact.h) and their dispatch macros gwen::dispatch: supported widths, tiers and
LayerNorm shapes, rows per pass, workspace sizes, tile counts and the return codes of the argument checks over the cases
of tests/golden/make_k6_launcher_table.py, against tests/golden/k6_launcher_table.npz (generated on the commit before
that change).  CPU only: fake pointers, and every case is refused -- or answered, at R == 0 -- before the first HIP
call; the generator asserts that from each case's own description."""
import importlib.util
import os

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_k6_launcher_table",
                                               os.path.join(_HERE, "golden", "make_k6_launcher_table.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@pytest.fixture(scope="module")
def table(hip_lib):
    return G.table(hip_lib)                                # computed once: about 7e3 calls through ctypes


def test_k6_rules_answer_as_before(table):
    want, got = np.load(G.FIXTURE), table
    assert sorted(got) == sorted(want.files)
    for name in want.files:
        assert got[name].shape == want[name].shape, name
        diff = np.argwhere(got[name] != want[name])
        assert diff.size == 0, (name, len(diff), "first differing index", diff[0].tolist(),
                                int(got[name][tuple(diff[0])]), int(want[name][tuple(diff[0])]))


def test_only_a_case_without_defect_is_answered_ok(table):
    fwd = [G.fwd_case(**kw) for _, kw in G.fwd_cases()]
    bwd = [G.bwd_case(**kw) for _, kw in G.bwd_cases()]
    assert [rc == 0 for rc in table["ln_f32"]] == [not d for _, d in fwd]
    assert [rc == 0 for rc in table["bwd_contract_f32"]] == [not d for _, d in bwd]
    assert (table["edge_tiles"] != 0).all()
    # the last check before a launch, as a case's only defect
    alone = [rc for (_, d), rc in zip(fwd, table["ln_f32"]) if len(d) == 1 and d[0].startswith("misaligned")]
    assert len(alone) >= 8 * 11 and set(alone) == {-1}


def test_the_entry_points_forward_as_the_header_says(table):
    t = table
    fwd = [a for a, _ in (G.fwd_case(**kw) for _, kw in G.fwd_cases())]
    no_ln = np.array([a[25] is None and a[26] is None for a in fwd])
    assert np.array_equal(t["contract_f32"], t["ln_f32"][no_ln])                    # _contract_f32 = _ln_f32(NULL, NULL)
    bf16x3 = np.array([a[24] == 0 for a in fwd])[no_ln]
    assert np.array_equal(t["f32"], t["contract_f32"][bf16x3])                       # _f32 = _contract_f32(BF16X3)
    bwd = [a for a, _ in (G.bwd_case(**kw) for _, kw in G.bwd_cases())]
    assert np.array_equal(t["bwd_f32"], t["bwd_contract_f32"][np.array([a[12] == 0 for a in bwd])])
    assert np.array_equal(t["workspace_bytes"], t["contract_workspace_bytes"][:, G.CONTRACTS.index(0)])
