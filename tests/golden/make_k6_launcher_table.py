#!/usr/bin/env python3
"""Generates tests/golden/k6_launcher_table.npz -- what every host-side rule of the K6 launchers (csrc/interact.hip,
csrc/interact_rows.hip) answers, as answered by the commit BEFORE their arguments became structs (csrc/interact.h) and
their dispatch macros gwen::dispatch: the supported widths / tiers / LayerNorm shapes, rows per pass, workspace sizes,
tile counts, and the return code of the argument checks of gwen_mlp2_ln_f32 / _contract_f32 / _f32,
gwen_mlp2_bwd_contract_f32 / _bwd_f32 and gwen_edge_tiles over the cases below.  The refactor changes no rule, so
tests/test_k6_launcher_table_host.py recomputes the table on the built library and requires equality.

Run it ON THAT PARENT COMMIT:

    python tests/golden/make_k6_launcher_table.py [--out FILE]      # default: the .npz next to this file

Pointers are fake addresses that are never dereferenced.  No case may get as far as a HIP call (the suite also runs
where a GPU would take a launch on fake addresses): every case of a launching entry point either carries at least one
DEFECT -- something the header says is refused -- or has R == 0 without `agg` (answered GWEN_OK before any HIP call).
That is asserted from the case's own description (`defects`, planted by the builders below), not from what the
library returns.  Most cases end in a TAIL defect, chosen so that its code tells how far the checks got: a misaligned A
(the alignment check is the last one before a launch: GWEN_EINVAL), R = 2^31 (GWEN_ERANGE, in the middle of the order) or
a workspace one byte short at 256 channels (GWEN_ENOSPACE, last but one).

It also defines the cases, which the test imports, so both always agree.
"""
import itertools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(HERE, "k6_launcher_table.npz")
WIDTHS = (0, 16, 32, 48, 64, 128, 256, 512)
BUILT = (32, 64, 128, 256)
CONTRACTS = (-1, 0, 1, 2, 3, 7)
TIERS = (0, 3)                                     # GWEN_CONTRACT_BF16X3, GWEN_CONTRACT_F16X3
ACTS = (-1, 0, 1, 2, 3)
ROWS = (-1, 0, 10, 2 ** 31 - 128, 2 ** 31)
TABLES = ("none", "g1_self", "g1_idx", "both_idx", "g2_only", "idx_no_table", "g1_self_short",
          "both_self", "g1_self_g2_idx", "g1_idx_g2_self")       # the last three: addressed in a pair that is not built
PITCHES = (-4, 0, 2, 4)                            # ld = F + this
SHAPES = (-1, 0, 1, 2)                             # GWEN_MLP2_LN_EDGE = 0, _NODE = 1
EPS = (-1.0, float("nan"), 1e-5)

# fake, 16-byte aligned, pairwise different addresses
P = {n: 0x100000 * (i + 1) for i, n in enumerate(
    ("A", "W1", "G1", "idx1", "G2", "idx2", "b1", "W2", "b2", "res", "out", "rowptr", "tile_row", "agg", "ln_g", "ln_b",
     "workspace", "ge", "W2t", "d1", "T", "dst", "Wet", "g_pre1", "g_e"))}
FWD_ALIGNED = ("A", "W1", "G1", "G2", "b1", "W2", "b2", "res", "out", "agg", "workspace", "ln_g", "ln_b")
BWD_ALIGNED = ("ge", "W2t", "d1", "T", "Wet", "g_pre1", "g_e", "workspace")


def _need(F, contract):                            # gwen_mlp2_contract_workspace_bytes, as the header states it
    return 2 * 2 * F * F * 2 + (2 * F * 4 if contract == 3 else 0) if F == 256 else 0


def fwd_case(F=64, contract=0, act=0, tables="none", pitch=0, big_table=False, R=10, agg="none", out="set", res="none",
             ln="none", eps=1e-5, ws="enough", misalign=None, tail=None):
    """-> (arguments of gwen_mlp2_ln_f32, the defects planted).  agg: none / full / no_rowptr / no_tile_row / no_tiles;
    out: set / unset / alias; res: none / a / other; ln: none / gamma / beta / both; ws: null / short / enough;
    misalign: a name of FWD_ALIGNED; tail: None / align / range / ws_short."""
    defects = []
    if tail == "range":
        R = 2 ** 31
    if tail == "ws_short":
        ws = "short"
    if tail == "align":
        misalign = "A"
    ok_f, ok_c = F in BUILT, contract in TIERS
    if not ok_f:
        defects.append("width")
    if not ok_c:
        defects.append("contract")
    if act not in (0, 1, 2):
        defects.append("act")
    if R < 0 or R >= 2 ** 31 - 128:
        defects.append("rows")
    p = dict(P)
    if misalign is not None:
        p[misalign] += 4
    g1 = tables not in ("none", "g2_only", "idx_no_table")
    g2 = tables in ("both_idx", "g2_only", "both_self", "g1_self_g2_idx", "g1_idx_g2_self")
    i1 = tables in ("g1_idx", "both_idx", "idx_no_table", "g1_idx_g2_self")
    i2 = tables in ("both_idx", "g2_only", "g1_self_g2_idx")
    ld = F + pitch
    rows1 = (max(R, 0) if not i1 else 17) - (1 if tables == "g1_self_short" else 0)
    rows2 = max(R, 0) if not i2 else 29
    if big_table:
        rows1 = (2 ** 32 + 4 * ld - 1) // (4 * ld) if ld > 0 else rows1
    if tables in ("g2_only", "idx_no_table"):
        defects.append("table without its partner")
    if tables == "g1_self_short" and R > 0:
        defects.append("row-for-row table shorter than R")
    if tables in ("both_self", "g1_self_g2_idx", "g1_idx_g2_self"):
        defects.append("table pair that is not built")
    if (g1 or g2) and pitch in (-4, 2):
        defects.append("pitch")
    if g1 and big_table and ld > 0:
        defects.append("table of 2^32 bytes")
    n_agg = 5 if agg != "none" else 0
    if agg not in ("none", "full"):
        defects.append("agg without its tiling")
    if out == "unset" and agg == "none" and R != 0:
        defects.append("nothing to write")
    if out == "alias" and g1:
        defects.append("out aliases a table")
    resp = {"none": None, "a": p["A"], "other": p["res"]}[res]
    if ln in ("gamma", "beta"):
        defects.append("one norm pointer")
    if ln == "both":
        edge = tables == "both_idx" and agg != "none" and res == "a"
        node = tables == "g1_self" and agg == "none" and res == "other"
        if not (edge or node) or F != 64 or not ok_c or not eps >= 0:
            defects.append("norm without a fused instantiation, or a bad eps")
    need = _need(F, contract) if ok_f and ok_c else 0
    if need > 0 and ws != "enough":
        defects.append("workspace")
    present = {"A": True, "W1": True, "W2": True, "b1": True, "b2": True, "G1": g1, "G2": g2, "res": res == "other",
               "out": out != "unset", "agg": agg != "none", "workspace": need > 0 and ws != "null",
               "ln_g": ln in ("gamma", "both"), "ln_b": ln in ("beta", "both")}
    if misalign is not None and present[misalign]:
        defects.append("misaligned " + misalign)
    if agg != "none":
        assert R != 0, "R == 0 with agg would reach hipMemsetAsync"
    assert defects or (R == 0 and agg == "none"), "a case without a defect would launch"
    args = (p["A"], p["W1"], p["G1"] if g1 else None, p["idx1"] if i1 else None, rows1, ld,
            p["G2"] if g2 else None, p["idx2"] if i2 else None, rows2, ld, p["b1"], p["W2"], p["b2"], resp,
            {"set": p["out"], "unset": None, "alias": p["G1"]}[out], R, F, act,
            p["rowptr"] if agg not in ("none", "no_rowptr") else None,
            p["tile_row"] if agg not in ("none", "no_tile_row") else None,
            0 if agg in ("none", "no_tiles") else 3, p["agg"] if agg != "none" else None, n_agg, int(agg != "none"),
            contract, p["ln_g"] if ln in ("gamma", "both") else None, p["ln_b"] if ln in ("beta", "both") else None, eps,
            None if ws == "null" else p["workspace"], max(need - (ws == "short"), 0), None)
    return args, defects


def _tails(F):
    return ("align", "range") + (("ws_short",) if F == 256 else ())


def fwd_cases():
    """[(label, keyword arguments of fwd_case)] -- one axis of the header at a time on top of every built width and tier,
    each under every tail; the width x contract x act product whole."""
    out = []

    def add(label, **kw):
        out.append((label, kw))

    for F, c, a in itertools.product(WIDTHS, CONTRACTS, ACTS):
        for t in _tails(F):
            add("basic", F=F, contract=c, act=a, tail=t)
    for F, c in itertools.product(BUILT, TIERS):
        for t in _tails(F):
            for tb, pi in itertools.product(TABLES, PITCHES):
                add("tables", F=F, contract=c, tables=tb, pitch=pi, tail=t)
            for tb in ("g1_self", "g1_idx", "both_idx"):
                add("big", F=F, contract=c, tables=tb, big_table=True, tail=t)
                add("alias", F=F, contract=c, tables=tb, out="alias", tail=t)
            for ag, o in itertools.product(("none", "full", "no_rowptr", "no_tile_row", "no_tiles"), ("set", "unset")):
                add("agg", F=F, contract=c, tables="both_idx", agg=ag, out=o, tail=t)
            for r in ("none", "a", "other"):
                add("res", F=F, contract=c, res=r, tail=t)
            for w in ("null", "short", "enough"):
                add("ws", F=F, contract=c, ws=w, tail=t)
            for ln, e in itertools.product(("none", "gamma", "beta", "both"), EPS):
                add("ln_edge", F=F, contract=c, tables="both_idx", agg="full", res="a", ln=ln, eps=e, tail=t)
                add("ln_node", F=F, contract=c, tables="g1_self", res="other", ln=ln, eps=e, tail=t)
                add("ln_other", F=F, contract=c, tables="g1_idx", res="other", ln=ln, eps=e, tail=t)
        for r in ROWS:                                 # R itself; R == 0 only without agg (see fwd_case)
            for o in ("set", "unset"):
                add("rows", F=F, contract=c, R=r, out=o, tail=None if r != 10 else "align")
            if r != 0:
                add("rows_agg", F=F, contract=c, R=r, tables="both_idx", agg="full", tail=None if r != 10 else "align")
        # the last check before a launch, alone: each aligned pointer in turn, on the call that has them all
        for m in FWD_ALIGNED[:-2]:
            add("align_edge", F=F, contract=c, tables="both_idx", agg="full", res="other", misalign=m,
                tail=None if m != "workspace" or F == 256 else "align")
        for m in ("ln_g", "ln_b", "A", "out"):
            add("align_ln", F=F, contract=c, tables="both_idx", agg="full", res="a", ln="both", misalign=m)
        for tb in ("both_self", "g1_self_g2_idx", "g1_idx_g2_self"):      # refused by the dispatch itself
            add("pair", F=F, contract=c, tables=tb)
    return out


def bwd_case(F=64, contract=0, R=10, pitch=0, big_table=False, null=None, alias=None, ws="enough", misalign=None,
             tail=None):
    """-> (arguments of gwen_mlp2_bwd_contract_f32, defects).  null: a pointer name; alias: (a, b) -- b is passed as a."""
    defects = []
    if tail == "range":
        R = 2 ** 31
    if tail == "ws_short":
        ws = "short"
    if tail == "align":
        misalign = "ge"
    ok_f, ok_c = F in (64, 256), contract in TIERS
    if not ok_f:
        defects.append("width")
    if not ok_c:
        defects.append("contract")
    if R < 0 or R >= 2 ** 31 - 128 or R * F * 4 >= 2 ** 32:
        defects.append("rows")
    p = dict(P)
    if misalign is not None:
        p[misalign] += 4
    if null is not None:
        p[null] = None
        defects.append("missing " + null)
    if alias is not None:
        p[alias[1]] = p[alias[0]]
        if alias != ("ge", "g_e"):
            defects.append("aliasing")
    ld = F + pitch
    t_rows = (2 ** 32 + 4 * ld - 1) // (4 * ld) if big_table and ld > 0 else 7
    if pitch in (-4, 2):
        defects.append("pitch")
    if big_table and ld > 0:
        defects.append("table of 2^32 bytes")
    need = _need(F, contract) if ok_f and ok_c else 0
    if need > 0 and ws != "enough":
        defects.append("workspace")
    if misalign is not None and (misalign != "workspace" or (need > 0 and ws != "null")):
        defects.append("misaligned " + misalign)
    assert defects or R == 0, "a case without a defect would launch"
    args = (p["ge"], p["W2t"], p["d1"], p["T"], p["dst"], t_rows, ld, p["Wet"], p["g_pre1"], p["g_e"], R, F, contract,
            None if ws == "null" else p["workspace"], max(need - (ws == "short"), 0), None)
    return args, defects


def bwd_cases():
    out = []

    def add(label, **kw):
        out.append((label, kw))

    for F, c, r in itertools.product(WIDTHS, CONTRACTS, ROWS + (2 ** 24,)):
        add("basic", F=F, contract=c, R=r, tail=None if r != 10 else "align")
    for F, c in itertools.product((64, 256), TIERS):
        for t in _tails(F):
            for pi in PITCHES:
                add("pitch", F=F, contract=c, pitch=pi, tail=t)
            add("big", F=F, contract=c, big_table=True, tail=t)
            for n in ("ge", "W2t", "d1", "T", "dst", "Wet", "g_pre1", "g_e"):
                add("null", F=F, contract=c, null=n, tail=t if n != "ge" or t != "align" else "range")
            for al in (("ge", "g_pre1"), ("d1", "g_pre1"), ("g_e", "g_pre1"), ("d1", "g_e"), ("ge", "g_e")):
                add("alias", F=F, contract=c, alias=al, tail=t)
            for w in ("null", "short", "enough"):
                add("ws", F=F, contract=c, ws=w, tail=t)
        for m in BWD_ALIGNED:
            add("align", F=F, contract=c, misalign=m, tail=None if m != "workspace" or F == 256 else "align")
    return out


def tiles_cases():
    """[(arguments of gwen_edge_tiles, defects)]: every combination that is refused (a valid one launches, also at N = 0)."""
    out = []
    for N, E, T, missing in itertools.product((-1, 0, 10, 2 ** 31 - 2, 2 ** 31 - 1), (-1, 0, 10, 2 ** 31 - 129, 2 ** 31 - 128),
                                              (0, 1, 64, 128, 129), (None, "rowptr", "tile_row", "dst")):
        defects = [n for n, bad in (("N", N < 0 or N >= 2 ** 31 - 1), ("E", E < 0 or E >= 2 ** 31 - 128),
                                    ("T", T < 1 or T > 128), ("pointer", missing in ("rowptr", "tile_row")),
                                    ("dst", missing == "dst" and E > 0)) if bad]
        if defects:
            out.append(((None if missing == "rowptr" else P["rowptr"], N, E, T,
                         None if missing == "tile_row" else P["tile_row"], None if missing == "dst" else P["dst"], None),
                        defects))
    assert all(d for _, d in out)
    return out


def _codes(values):
    out = np.array(list(values), dtype=np.int64)
    assert set(np.unique(out).tolist()) <= {0, -1, -2, -3}, "a code that is no GWEN_* answer: some case reached HIP"
    return out.astype(np.int8)


def table(lib):
    """{name: array} -- every answer of K6's host-side rules over the cases above."""
    fwd = [fwd_case(**kw) for _, kw in fwd_cases()]
    bwd = [bwd_case(**kw) for _, kw in bwd_cases()]
    plain_ln = [a for a, _ in fwd if a[25] is None and a[26] is None]                # no norm pointers
    plain_bwd = [a for a, _ in bwd if a[12] == 0]
    grid = lambda fn, *axes: np.array([fn(*q) for q in itertools.product(*axes)], dtype=np.int64).reshape(
        [len(a) for a in axes])
    return {
        "supported": grid(lib.gwen_mlp2_supported, WIDTHS),
        "rows": grid(lib.gwen_mlp2_rows, WIDTHS),
        "contract_supported": grid(lib.gwen_mlp2_contract_supported, WIDTHS, CONTRACTS),
        "contract_workspace_bytes": grid(lib.gwen_mlp2_contract_workspace_bytes, WIDTHS, CONTRACTS),
        "workspace_bytes": grid(lib.gwen_mlp2_workspace_bytes, WIDTHS),
        "bwd_supported": grid(lib.gwen_mlp2_bwd_supported, WIDTHS),
        "bwd_rows": grid(lib.gwen_mlp2_bwd_rows, ROWS + (1, 127, 128, 129)),
        "ln_supported": grid(lib.gwen_mlp2_ln_supported, WIDTHS, CONTRACTS, SHAPES),
        "edge_tiles_count": grid(lib.gwen_edge_tiles_count, (-1, 0, 1, 134, 2 ** 31), (-1, 0, 1, 61, 64, 128)),
        "ln_f32": _codes(lib.gwen_mlp2_ln_f32(*a) for a, _ in fwd),
        "contract_f32": _codes(lib.gwen_mlp2_contract_f32(*a[:25], *a[28:]) for a in plain_ln),
        "f32": _codes(lib.gwen_mlp2_f32(*a[:24], *a[28:]) for a in plain_ln if a[24] == 0),
        "bwd_contract_f32": _codes(lib.gwen_mlp2_bwd_contract_f32(*a) for a, _ in bwd),
        "bwd_f32": _codes(lib.gwen_mlp2_bwd_f32(*a[:12], *a[13:]) for a in plain_bwd),
        "edge_tiles": _codes(lib.gwen_edge_tiles(*a) for a, _ in tiles_cases()),
    }


def main():
    from gwen_amd import build as _b
    _b.build()
    from gwen_amd import _lib
    t = table(_lib.lib())
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else FIXTURE
    np.savez_compressed(path, **t)
    print(path, os.path.getsize(path), "bytes;", {k: (v.shape, np.unique(v).tolist()[:8]) for k, v in t.items()})


if __name__ == "__main__":
    main()
