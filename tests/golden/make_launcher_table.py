#!/usr/bin/env python3
"""Generates tests/golden/launcher_table.npz -- what every host-side rule of the K4 / K5 launchers (csrc/layer.hip,
csrc/chain.hip) answers, as answered by the commit BEFORE their block geometry became one set of constexpr functions and
their dispatch macros one helper: which widths are supported, the library's gather depth, and the return code of the
*_tuned_f32 argument checks (widths, contraction, entries, depth, block_rows) over the whole grid below.  The refactor
changes no rule, so tests/test_launcher_table_host.py recomputes the table on the built library and requires equality.

Run it ON THAT PARENT COMMIT (CPU only: null pointers and N = 0, so every call returns before the first HIP call):

    python tests/golden/make_launcher_table.py [--out FILE]      # default: the .npz next to this file

It also defines the grid, which the test imports, so both always agree.
"""
import ctypes as C
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(HERE, "launcher_table.npz")
BLOCK_ROWS = (0, 16, 32, 48, 64, 80, 96, 112, 128, 144, 192, 256, 512)
DEPTHS5 = (-1, 0, 1, 2, 3)
L_WIDTHS = (8, 16, 32, 64, 128, 256, 512)          # K4: Fin, Fout (and the backward's Fg, Fx)
L_EXACT = (-1, 0, 1, 2, 3)
L_ENTRIES = (6, 7, 8, 9)
C_WIDTHS = (0, 16, 32, 64, 128, 256)               # K5: Fin, F1, F2
C_PRE = (0, 1)
C_CONTRACT = (0, 1, 2, 3)
C_ENTRIES = (7, 8)
C_DEPTHS = (0, 1, 2)


def _grid(fn, *axes):
    """fn over the product of the axes as an int8 array of their shape (every code and answer here fits)."""
    out = np.array([fn(*p) for p in itertools.product(*axes)], dtype=np.int64)
    assert np.abs(out).max() < 128
    return out.astype(np.int8).reshape([len(a) for a in axes])


def table(lib):
    """{name: int8 array} -- every answer of the launchers' host-side rules over the grid above."""
    N = [None]

    def layer_tuned(fi, fo, exact, entries, depth, rows):
        return lib.gwen_gcn_layer_tuned_f32(*N * 7, 0, fi, fo, fi, fo, 1, 0, 0, 0, exact, entries, depth, rows, None)

    def layer_entries(fi, fo, exact, entries):
        return lib.gwen_gcn_layer_entries_f32(*N * 7, 0, fi, fo, fi, fo, 1, 0, 0, 0, exact, entries, None)

    def layer_plain(fi, fo, exact):
        return lib.gwen_gcn_layer_f32(*N * 7, 0, fi, fo, fi, fo, 1, 0, 0, 0, exact, None)

    def chain_tuned(fi, f1, f2, pre, contract, entries, depth, rows):
        return lib.gwen_gcn_chain_tuned_f32(*N * 8, 0, fi, f1, f2, pre, 0, 1, 0, 0, contract, entries, depth, rows, None)

    def chain_entries(fi, f1, f2, pre, contract, entries):
        return lib.gwen_gcn_chain_entries_f32(*N * 8, 0, fi, f1, f2, pre, 0, 1, 0, 0, contract, entries, None)

    def chain_plain(fi, f1, f2, pre, contract):
        return lib.gwen_gcn_chain_f32(*N * 8, 0, fi, f1, f2, pre, 0, 1, 0, 0, contract, None)

    def bwd(fg, fx, contract, with_bias):
        # both NULL or both non-NULL; *bias_chunks is written (0) before the first argument check: a host int64
        chunks = C.c_int64(-1)
        rc = lib.gwen_gcn_layer_bwd_bias_f32(*N * 8, 0, fg, fx, 1, contract, C.byref(chunks) if with_bias else None,
                                             C.byref(chunks) if with_bias else None, None)
        assert chunks.value == (0 if with_bias else -1)
        return rc

    W = L_WIDTHS
    return {
        "layer_supported": _grid(lib.gwen_gcn_layer_supported, W, W),
        "layer_depth": _grid(lib.gwen_gcn_layer_depth, W, W, L_EXACT),
        "layer_tuned": _grid(layer_tuned, W, W, L_EXACT, L_ENTRIES, DEPTHS5, BLOCK_ROWS),
        "layer_entries": _grid(layer_entries, W, W, L_EXACT, L_ENTRIES),
        "layer_plain": _grid(layer_plain, W, W, L_EXACT),
        "layer_bwd": _grid(bwd, W, W, C_CONTRACT, (0, 1)),
        "chain_supported": _grid(lib.gwen_gcn_chain_supported, C_WIDTHS, C_WIDTHS, C_WIDTHS, C_PRE, C_CONTRACT),
        "chain_depth": _grid(lib.gwen_gcn_chain_depth, C_WIDTHS, C_WIDTHS, C_WIDTHS, C_PRE, C_CONTRACT),
        "chain_tuned": _grid(chain_tuned, C_WIDTHS, C_WIDTHS, C_WIDTHS, C_PRE, C_CONTRACT, C_ENTRIES, C_DEPTHS, BLOCK_ROWS),
        "chain_entries": _grid(chain_entries, C_WIDTHS, C_WIDTHS, C_WIDTHS, C_PRE, C_CONTRACT, C_ENTRIES),
        "chain_plain": _grid(chain_plain, C_WIDTHS, C_WIDTHS, C_WIDTHS, C_PRE, C_CONTRACT),
    }


def main():
    from gwen_amd import build as _b
    _b.build()
    from gwen_amd import _lib
    t = table(_lib.lib())
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE
    np.savez_compressed(path, **t)
    print(path, os.path.getsize(path), "bytes;", {k: (v.shape, int((v == 0).sum())) for k, v in t.items()})


if __name__ == "__main__":
    main()
