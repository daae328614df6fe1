"""The prologues of K4 (k_layer), K5 (k_chain) and the plain gather (k_gather) -- bias loaded unconditionally, the W
split in the shadow of the first row loads, the narrow K4 without its chunk loop -- are a change of ORDER only: every
output must be bit for bit (``array_equal`` on the bit patterns, so signed zeros count) what the commit before that
change computed on the MI355X, which tests/golden/prologue_parent.npz records (tests/golden/make_prologue_golden.py:
the cases, the inputs and what is stored).

Graphs: geodesic nu = 3 (N = 92) and nu = 6 (N = 362), N = 1, N = 5, and a random non-uniform graph of 150 nodes with
a row of 20 entries and an empty row.  Kernels: the six of the c2 step and K4 64 -> 64 on bf16x3 and fp32.  Each with
and without bias, ReLU off and on, 1 and 3 members, 7 and 8 gathered entries (uniform layouts), and through the
``*_tuned_f32`` entry points at depth 1 and 2 and at every block size of ROWS (1 .. 7 gather passes).  The inputs hold
a row that aggregates to -0.0, which the bias-free plain gather has to hand on as -0.0."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_prologue_golden", os.path.join(_HERE, "golden", "make_prologue_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@pytest.fixture(scope="module")
def golden(hip_lib):
    assert torch.cuda.is_available(), "these tests need the MI355X"
    z = np.load(G.FIXTURE)
    sha = {k.decode(): z["sha256"][i] for i, k in enumerate(z["keys"])}
    data, off = {}, 0
    for k, shape in zip(z["data_keys"], z["data_shapes"]):
        n = int(np.prod(shape))
        data[k.decode()] = z["data"][off:off + n].reshape(shape)          # uint32: the bit patterns
        off += n
    assert off == z["data"].size
    return sha, data


@pytest.mark.parametrize("name", G.GRAPHS)
def test_outputs_are_the_parents_bit_for_bit(golden, name):
    sha, data = golden
    gr = G.make_graph(name)
    xs, seen = {}, 0
    for key, form, members, entries, bias, relu in G.cases(gr):
        fin = form[1]
        if (members, fin) not in xs:
            xs[(members, fin)] = G.inputs(gr, members, fin)
        x = xs[(members, fin)]
        first = None
        for depth, rows in G.variants(form):
            what = (key, depth, rows)
            out, guard = G.run(gr, form, x, bias, relu, entries, depth, rows)
            assert torch.isnan(guard).all(), ("written behind the last row", what)
            if first is not None:
                assert torch.equal(G.bits(first), G.bits(out)), ("differs from the first variant", what)
                continue
            first = out
            a = out.cpu().numpy()
            assert np.isfinite(a).all(), ("a row < N was not written", what)
            if key in data:
                part = a if G.stores_full(gr, members) else a[:64]
                assert np.array_equal(part.view(np.uint32), data[key]), what
            assert np.array_equal(G.sha(a), sha[key]), what
        seen += 1
    assert seen == sum(k.startswith(name + "/") for k in sha)


def test_fixture_holds_a_negative_zero_row(golden):
    """The bias-free plain gather (form 2) on the ring of five hands on the -0.0 of its last row: the case
    ``acc + 0`` would break."""
    _, data = golden
    for relu in (0, 1):
        for entries in (7, 8):
            a = data[f"five/2/m1/e{entries}/b0/r{relu}"]
            assert (a[4] == 0x80000000).all() and not (a[:4] == 0x80000000).any()
