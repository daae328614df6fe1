"""The launchers' own block-rows choice BEYOND one resident round of 64-row blocks (K4: csrc/layer.hip, launch(); K5:
csrc/chain.hip, launch_ns): the branch that the other GPU tests do not reach at their sizes.  It needs
ceil(N / 64) > 256 x blocks-per-CU; at up to 8 blocks per CU that is N > 131 072, so the graph is a ring lattice
(i -> i +- 1, +- 2, +- 3) of N = 140 000 nodes, one member: uniform layout, 7 entries a row with the self loop.
Block rows and depth change no value, so the library's choice (block_rows = 0, depth = 0) must equal 64-row blocks at
depth 1 bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import SEED

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = 140_000


@pytest.fixture(scope="module")
def ring(hip_lib):
    import gwen_amd as ga
    assert torch.cuda.is_available(), "these tests need the MI355X"
    i = np.arange(N)
    ei = np.stack([np.concatenate([i] * 6), np.concatenate([(i + d) % N for d in (1, -1, 2, -2, 3, -3)])]).astype(np.int64)
    g = ga.prepare_graph(torch.from_numpy(ei).to(DEV), N)
    assert g.num_nodes == N and g.grouped()[0] is None and g.entries() == 7
    return g


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _run(g, x, w1, w2, b, contract, entries, depth, rows):
    """K4 (w2 None) or K5 through the *_tuned_f32 entry points; the output behind a NaN fill."""
    from gwen_amd import _lib
    _, gc, gv = g.grouped()
    fin, f1, f2 = x.size(1), w1.size(0), 0 if w2 is None else w2.size(0)
    out = torch.full((N, f2 or f1), float("nan"), device=DEV)
    st = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    if w2 is None:
        rc = _lib.lib().gwen_gcn_layer_tuned_f32(None, _p(gc), _p(gv), _p(x), _p(w1), _p(b), _p(out), N, fin, f1, fin, f1, 1,
                                                 N * fin, N * f1, 1, contract, entries, depth, rows, st)
    else:
        rc = _lib.lib().gwen_gcn_chain_tuned_f32(None, _p(gc), _p(gv), _p(x), _p(w1), _p(w2), _p(b), _p(out), N, fin, f1, f2,
                                                 0, 1, 1, N * fin, N * f2, contract, entries, depth, rows, st)
    assert rc == 0, (rc, fin, f1, f2, contract, entries, depth, rows)
    return out


@pytest.mark.parametrize("fin,f1,f2", [(16, 16, 0), (32, 64, 0), (64, 64, 0), (64, 64, 32)])
def test_own_choice_equals_64_row_blocks(ring, fin, f1, f2):
    from gwen_amd import _lib
    gen = torch.Generator().manual_seed(SEED + 131 * fin + f1)
    x = torch.randn(N, fin, generator=gen).to(DEV)
    w1 = (torch.randn(f1, fin, generator=gen) / fin ** 0.5).to(DEV)
    w2 = (torch.randn(f2, f1, generator=gen) / f1 ** 0.5).to(DEV) if f2 else None
    b = (torch.randn(f1, generator=gen) * 0.1).to(DEV)
    for contract in (_lib.CONTRACT_BF16X6, _lib.CONTRACT_BF16X3):
        for entries in (7, 8):
            own = _run(ring, x, w1, w2, b, contract, entries, 0, 0)
            want = _run(ring, x, w1, w2, b, contract, entries, 1, 64)
            assert torch.isfinite(want).all()
            assert torch.equal(own.view(torch.int32), want.view(torch.int32)), (fin, f1, f2, contract, entries)
