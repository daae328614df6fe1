"""Every leaf of K6's forward dispatch (csrc/interact.hip launch_tiles, csrc/interact_rows.hip gwen_mlp2_rows_launch /
launch_rows) runs the kernel it should: gwen_amd.interaction.mlp2 over the full product of width x table pair x tier x
(per-target sums or not) x residual kind -- 192 cases -- against the fp64 expressions of test_gpu_interaction_precision.

The accuracy bounds are the project's forward bounds per tier (FWD_TOL of test_gpu_interaction_layernorm).  They alone
would let "3xbf16 served by f16x3" pass, so every case also requires that the two tiers' outputs are NOT bitwise equal,
and that a second call repeats the first bit for bit.  The LayerNorm and backward leaves are walked by
test_fused_and_unfused_routes_agree and test_block_backward_*.

The graph's targets have in-degrees (0, 1, 130, 3, 0): an empty target at both ends, a single-entry row, and one row
longer than a pass of either kernel (64 and 128 rows); sums on half the cases, means on the other half.  Without a
graph: 65 rows, one more than a pass of k_mlp2.
"""
import functools

import pytest
import torch

from helpers import SEED, rel_err
from test_gpu_interaction_layernorm import FWD_TOL, TIERS, WIDTHS
from test_gpu_interaction_precision import _want

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIRS = ["none", "g1_self", "g1_idx", "both_idx"]                  # the table pairs that are built (include/gwen_hip.h)
RES = ["none", "a", "other"]
DEGREES = (0, 1, 130, 3, 0)


@functools.lru_cache(maxsize=None)
def _graph():
    from gwen_amd.interaction import interaction_graph
    dst = torch.repeat_interleave(torch.arange(len(DEGREES)), torch.tensor(DEGREES))
    src = torch.randint(0, 17, (dst.numel(),), generator=torch.Generator().manual_seed(SEED))
    g = interaction_graph(torch.stack([src, dst]).to(DEV), 17, len(DEGREES))
    assert g.num_edges == 134 and g.rowptr.tolist() == [0, 0, 1, 131, 134, 134]
    return g


@functools.lru_cache(maxsize=None)
def _case(F, pair, with_graph, res):
    """{tier: (out, agg, the same of a second call)} and the fp64 (out, agg) -- computed once for both tiers' cases"""
    from gwen_amd.interaction import mlp2
    k = (WIDTHS.index(F), PAIRS.index(pair), RES.index(res))
    mean = sum(k) % 2 == 1
    rows = 134 if with_graph else 65
    g = torch.Generator().manual_seed(SEED + 1000 * k[0] + 100 * k[1] + 10 * k[2] + with_graph)
    a = torch.randn(rows, F, generator=g)
    w1 = torch.randn(F, F, generator=g) / F ** 0.5
    w2 = torch.randn(F, F, generator=g) / F ** 0.5
    b1, b2 = torch.randn(F, generator=g), torch.randn(F, generator=g)
    t1, t2, ts = torch.randn(17, F, generator=g), torch.randn(29, F, generator=g), torch.randn(rows, F, generator=g)
    i1 = torch.randint(0, 17, (rows,), generator=g, dtype=torch.int32)
    i2 = torch.randint(0, 29, (rows,), generator=g, dtype=torch.int32)
    other = torch.randn(rows, F, generator=g)
    kw = {"none": {}, "g1_self": dict(g1=ts), "g1_idx": dict(g1=t1, idx1=i1),
          "both_idx": dict(g1=t1, idx1=i1, g2=t2, idx2=i2)}[pair]
    y = _want(a, w1, w2, b1, b2, "silu", kw.get("g1"), kw.get("idx1"), kw.get("g2"), kw.get("idx2"))
    want_out = y if res == "none" else (a if res == "a" else other).double() + y
    want_agg = None
    if with_graph:
        want_agg = torch.zeros(len(DEGREES), F, dtype=torch.float64)
        rp = _graph().rowptr.tolist()
        for d, n in enumerate(DEGREES):
            if n:
                want_agg[d] = y[rp[d]:rp[d + 1]].sum(0) / (n if mean else 1)
    ad = a.to(DEV)
    dv = {k_: v.to(DEV) for k_, v in kw.items()}
    dv.update(b1=b1.to(DEV), res={"none": None, "a": ad, "other": other.to(DEV)}[res], act="silu",
              graph=_graph() if with_graph else None, mean=mean)
    args = (ad, w1.to(DEV), w2.to(DEV), b2.to(DEV))
    got = {}
    for tier in TIERS:
        first, again = mlp2(*args, contract=tier, **dv), mlp2(*args, contract=tier, **dv)
        got[tier] = tuple(None if t is None else t.cpu() for t in first + again)
    return got, want_out, want_agg


@pytest.mark.parametrize("res", RES)
@pytest.mark.parametrize("with_graph", [False, True], ids=["rows", "graph"])
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("F", WIDTHS)
def test_leaf_runs_its_own_kernel(hip_lib, F, pair, tier, with_graph, res):
    got, want_out, want_agg = _case(F, pair, with_graph, res)
    out, agg, out2, agg2 = got[tier]
    other = got[TIERS[1 - TIERS.index(tier)]]
    errs = (rel_err(out, want_out), rel_err(agg, want_agg) if with_graph else 0.0)
    print(f"K6 leaf F={F} {pair} {tier} graph={with_graph} res={res}: rel err out {errs[0]:.3e} agg {errs[1]:.3e}")
    assert (agg is not None) == with_graph
    assert max(errs) <= FWD_TOL[tier], errs
    assert not torch.equal(out, other[0])                     # the other tier's kernel gives other bits
    assert torch.equal(out, out2) and (not with_graph or torch.equal(agg, agg2))
