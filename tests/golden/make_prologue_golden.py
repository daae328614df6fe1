#!/usr/bin/env python3
"""Generates tests/golden/prologue_parent.npz -- the outputs of K4 (k_layer), K5 (k_chain) and the plain gather
(k_gather) as computed on the MI355X by the commit BEFORE their prologues were reordered (bias loaded unconditionally,
the W split moved behind the first row loads, the narrow K4 without its chunk loop).  The reordering changes no
arithmetic, so tests/test_gpu_prologue.py asserts every output bit for bit -- signed zeros included -- against this file.

Run it ON THAT PARENT COMMIT, on the GPU:

    python tests/golden/make_prologue_golden.py [--out FILE]      # default: the .npz next to this file

It also defines the cases (graphs, inputs, kernel forms), which the test imports, so both always agree.

Per (graph, kernel form, members, entries, bias, relu) ONE output is stored: block_rows and depth change no value
(tests/test_gpu_gather_depth.py), which the generator checks again on the parent (bitwise) before it stores anything.
Stored: the SHA-256 of the output's bytes for every case; the whole output for N = 1 and N = 5 at one member; the first
64 rows for the nu = 6 mesh at one member and 7 entries with bias and ReLU.  Inputs come from fixed CPU seeds.
"""
import ctypes as C
import functools
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 23
DEV = "cuda:0"
GUARD = 1024                                   # NaN floats behind the last row: nothing may be written there
FIXTURE = os.path.join(HERE, "prologue_parent.npz")
GRAPHS = ("mesh3", "mesh6", "one", "five", "random")
X3, F32, X6 = 0, 1, 2                          # GWEN_CONTRACT_*
# (kind, Fin, F1, F2, pre, contract): the six kernels of the c2 step, then K4 64 -> 64 on the two other contractions
FORMS = (("chain", 64, 64, 32, 0, X6), ("chain", 32, 16, 0, 1, X6), ("gather", 16, 0, 0, 1, X3),
         ("layer", 16, 32, 0, 0, X6), ("layer", 32, 64, 0, 0, X6), ("layer", 64, 64, 0, 0, X6),
         ("layer", 64, 64, 0, 0, X3), ("layer", 64, 64, 0, 0, F32))
# block_rows per gathered width (0: the library's choice): 64 rows are 1 / 2 / 4 gather passes at 16 / 32 / 64 channels,
# 96 are 3 at 32 (the c2 choice of K4 32 -> 64), 112 are 7 at 64
ROWS = {64: (0, 64, 112), 32: (0, 64, 96), 16: (0, 64)}
NEG_DENORMAL = -1.4e-45                        # times a weight below 1/2 it rounds to -0.0


class Graph:
    """A prepared graph, its edge list (src, dst, weight or None) and the row whose inputs aggregate to -0.0."""

    def __init__(self, name, g, src, dst, w, target):
        self.name, self.g, self.src, self.dst, self.w, self.target = name, g, src, dst, w, target
        self.n = g.num_nodes
        self.entries = (7, 8) if g.grouped()[0] is None and g.entries() == 7 else (8,)


def make_graph(name):
    import gwen_amd as ga

    def prep(ei, n, w=None, **kw):
        t = torch.from_numpy(np.ascontiguousarray(ei.astype(np.int64))).to(DEV)
        return ga.prepare_graph(t, n, None if w is None else torch.from_numpy(w).to(DEV), **kw)

    if name in ("mesh3", "mesh6"):             # N = 92: one partial block at 112 rows; N = 362: a partial last block
        m = ga.geodesic_mesh(3 if name == "mesh3" else 6)
        ei = m.edge_index
        g = prep(ei, m.num_nodes)
        assert g.num_nodes == (92 if name == "mesh3" else 362) and g.grouped()[0] is None and g.entries() == 7
        return Graph(name, g, ei[0], ei[1], None, g.num_nodes - 1)
    if name == "one":                          # a single node: its self loop only
        ei = np.zeros((2, 0), np.int64)
        return Graph(name, prep(ei, 1), ei[0], ei[1], None, None)
    if name == "five":                         # a ring of five
        i = np.arange(5)
        ei = np.stack([np.concatenate([i, i]), np.concatenate([(i + 1) % 5, (i - 1) % 5])])
        return Graph(name, prep(ei, 5), ei[0], ei[1], None, 4)
    if name == "random":                       # non-uniform layout: a row of 20 entries (the long-row loop), an empty row
        rng = np.random.default_rng(SEED)
        n = 150
        deg = rng.integers(1, 9, size=n)
        deg[3], deg[70], deg[n - 1] = 20, 0, 8       # the -0.0 row: a whole group, no zero-weight padding (0 * x = +0)
        dst = np.repeat(np.arange(n), deg)
        src = np.concatenate([rng.choice(n, size=d, replace=False) for d in deg])
        w = rng.standard_normal(dst.size).astype(np.float32)
        w = np.where(np.abs(w) > 0.45, 0.1 * w, w).astype(np.float32)   # every |weight| below 1/2: the -0.0 row needs it
        g = prep(np.stack([src, dst]), n, w, add_self_loops=False, normalize=False)
        lens = np.diff(g.rowptr.cpu().numpy())
        assert lens.min() == 0 and lens.max() == 20 and g.grouped()[0] is not None and g.entries() == 8
        return Graph(name, g, src, dst, w, n - 1)
    raise KeyError(name)


def inputs(gr, members, fin):
    """x [members, N, fin] (or [N, fin]) from a CPU seed.  The sources of the target row hold denormals whose products
    with the row's weights are negative and round to -0.0, so the row aggregates to -0.0 in every channel."""
    gen = torch.Generator().manual_seed(SEED + 131 * fin + members + 977 * GRAPHS.index(gr.name))
    x = torch.randn(members, gr.n, fin, generator=gen)
    if gr.target is not None:
        sel = gr.dst == gr.target
        srcs = gr.src[sel]
        sign = np.ones(srcs.size, np.float32) if gr.w is None else np.sign(gr.w[sel])
        for s, sg in zip(srcs, sign):
            x[:, int(s), :] = float(NEG_DENORMAL * sg)
        if gr.w is None:                       # normalised mesh: the self loop is a source too
            x[:, gr.target, :] = NEG_DENORMAL
    return (x[0] if members == 1 else x).contiguous().to(DEV)


@functools.lru_cache(maxsize=None)
def params(fin, fout, seed=0):
    gen = torch.Generator().manual_seed(SEED + 7 * fin + fout + seed)
    return ((torch.randn(fout, fin, generator=gen) / fin ** 0.5).to(DEV), (torch.randn(fout, generator=gen) * 0.1).to(DEV))


@functools.lru_cache(maxsize=None)
def chain_bias(width, seed):
    return (torch.randn(width, generator=torch.Generator().manual_seed(SEED + seed)) * 0.1).to(DEV)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def run(gr, form, x, bias, relu, entries, depth, rows):
    """One launch through the *_tuned_f32 entry points.  Returns (out, guard): NaN-filled before the launch."""
    from gwen_amd import _lib
    kind, fin, f1, f2, pre, contract = form
    g = gr.g
    grp, gc, gv = g.grouped()
    m = 1 if x.dim() == 2 else x.size(0)
    n = gr.n
    fw = f2 or f1 or fin
    buf = torch.full((m * n * fw + GUARD,), float("nan"), device=DEV)
    out, guard = buf[:m * n * fw].view(*x.shape[:-1], fw), buf[m * n * fw:]
    st = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    if kind == "layer":
        w, b = params(fin, f1)
        rc = _lib.lib().gwen_gcn_layer_tuned_f32(_p(grp), _p(gc), _p(gv), _p(x), _p(w), _p(b if bias else None), _p(out),
                                                 n, fin, f1, fin, f1, m, n * fin, n * f1, int(relu), contract, entries,
                                                 depth, rows, st)
    else:
        w1 = params(fin, f1)[0] if f1 else None
        w2 = params(f1, f2, seed=1)[0] if f2 else None
        nb = fin if pre else f1
        b = chain_bias(nb, fin + f1)
        rc = _lib.lib().gwen_gcn_chain_tuned_f32(_p(grp), _p(gc), _p(gv), _p(x), _p(w1), _p(w2), _p(b if bias else None),
                                                 _p(out), n, fin, f1, f2, pre, int(relu), m, n * fin, n * fw, contract,
                                                 entries, depth, rows, st)
    assert rc == 0, (rc, gr.name, form, entries, depth, rows)
    return out, guard


def variants(form):
    """(depth, block_rows) of a form; the first one is the library's own choice of block size at depth 1."""
    kind, fin = form[0], form[1]
    if kind == "gather":
        return [(1, 0), (2, 0), (1, 1024 // fin), (2, 1024 // fin)]
    return [(d, r) for r in ROWS[fin] for d in (1, 2)]


def cases(gr):
    """(key, form, members, entries, bias, relu) in the fixture's order."""
    for fi, form in enumerate(FORMS):
        for members in (1, 3):
            for entries in gr.entries:
                for bias in (True, False):
                    for relu in (0, 1):
                        yield f"{gr.name}/{fi}/m{members}/e{entries}/b{int(bias)}/r{relu}", form, members, entries, bias, relu


def stores_full(gr, members):
    return gr.name in ("one", "five") and members == 1


def stores_head(gr, members, entries, bias, relu):
    return gr.name == "mesh6" and members == 1 and entries == 7 and bias and relu == 1


def bits(t):
    return t.contiguous().view(torch.int32)


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def main():
    import gwen_amd  # noqa: F401
    from gwen_amd import build as _b
    _b.build()
    keys, shas, data_keys, data_shapes, data = [], [], [], [], []
    for name in GRAPHS:
        gr = make_graph(name)
        xs = {}
        for key, form, members, entries, bias, relu in cases(gr):
            fin = form[1]
            if (members, fin) not in xs:
                xs[(members, fin)] = inputs(gr, members, fin)
            x = xs[(members, fin)]
            first = None
            for depth, rows in variants(form):
                out, guard = run(gr, form, x, bias, relu, entries, depth, rows)
                assert torch.isfinite(out).all() and torch.isnan(guard).all(), (key, depth, rows)
                if first is None:
                    first = out
                else:
                    assert torch.equal(bits(first), bits(out)), ("the parent's variants differ", key, depth, rows)
            a = first.cpu().numpy()
            keys.append(key)
            shas.append(sha(a))
            if stores_full(gr, members) or stores_head(gr, members, entries, bias, relu):
                part = a if stores_full(gr, members) else a[:64]
                data_keys.append(key)
                data_shapes.append(part.shape)
                data.append(part.reshape(-1).copy())
            if form[0] == "gather" and not bias and gr.target is not None:
                row = a.reshape(members, gr.n, -1)[:, gr.target]
                assert (np.signbit(row) & (row == 0)).all(), ("the target row did not aggregate to -0.0", key, row.ravel()[:4])
        print(name, "done:", len(keys), "cases", flush=True)
    fixture = {"keys": np.array(keys, dtype="S"), "sha256": np.stack(shas),
               "data_keys": np.array(data_keys, dtype="S"), "data_shapes": np.array(data_shapes, np.int64),
               "data": np.concatenate(data).view(np.uint32)}
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE
    np.savez_compressed(path, **fixture)
    print(path, os.path.getsize(path), "bytes", len(keys), "cases", len(data_keys), "stored arrays")


if __name__ == "__main__":
    main()
