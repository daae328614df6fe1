"""Regridding, host side (no GPU): argument validation of gwen_amd/regrid.py and of the C entry points' early returns,
the point sets' coincidence gap, and the numpy restatement of tests/regrid_ref.py against what must hold by
construction."""
import ctypes as C

import numpy as np
import pytest

import regrid_ref as R
from gridgraph_ref import dist2


@pytest.fixture(scope="module")
def ga():
    import gwen_amd
    return gwen_amd


def test_exports(ga):
    from gwen_amd import regrid
    assert ga.Regridder is regrid.Regridder and ga.nearest_neighbours is regrid.nearest_neighbours
    assert {"Regridder", "nearest_neighbours"} <= set(ga.__all__)


def test_python_layer_validates_without_a_gpu(ga):
    ok = R.points("mesh2")
    for bad in (np.array([[0.0, 0.0, 0.0]]), np.array([[np.nan, 0.0, 1.0]]), np.array([[np.inf, 0.0, 1.0]]),
                np.zeros((3, 2)), np.zeros(3)):
        for args in ((bad, ok), (ok, bad)):
            with pytest.raises(ValueError):
                ga.nearest_neighbours(*args, 4, "cuda:0")
            with pytest.raises(ValueError):
                ga.Regridder(*args, "cuda:0")
    for k in (0, 9, -1, 2.5, True):
        with pytest.raises(ValueError, match="k must be"):
            ga.nearest_neighbours(ok, ok, k, "cuda:0")
    for k in (0, 9):
        with pytest.raises(ValueError, match="k must be"):
            ga.Regridder(ok, ok, "cuda:0", k=k)
    none = np.zeros(ok.shape[0], dtype=bool)
    with pytest.raises(ValueError, match="no unmasked source"):
        ga.nearest_neighbours(ok, ok, 1, "cuda:0", src_mask=none)
    with pytest.raises(ValueError, match="no unmasked source"):
        ga.Regridder(ok, ok, "cuda:0", src_mask=none)
    with pytest.raises(ValueError, match="no unmasked source"):
        ga.nearest_neighbours(ok[:0], ok, 1, "cuda:0")
    with pytest.raises(ValueError, match="src_mask"):
        ga.nearest_neighbours(ok, ok, 1, "cuda:0", src_mask=np.ones(3, dtype=bool))
    with pytest.raises(ValueError, match="src_mask"):
        ga.nearest_neighbours(ok, ok, 1, "cuda:0", src_mask=np.ones(ok.shape[0]))           # not bool
    for d in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_distance"):
            ga.nearest_neighbours(ok, ok, 1, "cuda:0", max_distance=d)
    for r in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="initial_radius"):
            ga.nearest_neighbours(ok, ok, 1, "cuda:0", initial_radius=r)
    with pytest.raises(ValueError, match="method"):
        ga.Regridder(ok, ok, "cuda:0", method="bilinear")
    with pytest.raises(ValueError, match="uncovered"):
        ga.Regridder(ok, ok, "cuda:0", uncovered="zero")
    for p in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="power"):
            ga.Regridder(ok, ok, "cuda:0", power=p)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ga.nearest_neighbours(ok, ok, 1, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ga.Regridder(ok, ok, "cpu")


def test_from_weights_validates_without_a_gpu(ga):
    import torch
    ei = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ga.Regridder.from_weights(ei, torch.ones(3), 4, 4)
    with pytest.raises(ValueError):
        ga.Regridder.from_weights(ei.int(), torch.ones(3), 4, 4)
    with pytest.raises(ValueError):
        ga.Regridder.from_weights(ei, torch.ones(2), 4, 4)
    with pytest.raises(ValueError):
        ga.Regridder.from_weights(ei, torch.ones(3), -1, 4)


def test_launchers_validate_before_any_hip_call(hip_lib):
    n = C.c_size_t(0)
    assert hip_lib.gwen_knn_workspace_bytes(-1, 4, C.byref(n)) == -1
    assert hip_lib.gwen_knn_workspace_bytes(4, -1, C.byref(n)) == -1
    assert hip_lib.gwen_knn_workspace_bytes(4, 4, None) == -1
    assert hip_lib.gwen_knn_workspace_bytes(2 ** 31, 4, C.byref(n)) == -2
    assert hip_lib.gwen_knn_workspace_bytes(4, 2 ** 31 - 1, C.byref(n)) == -2

    def query(ns=4, nd=4, rows=None, nrows=4, k=4, radius=0.5, dmax=-1.0, out=8):
        return hip_lib.gwen_knn_query(8, None, ns, 8, nd, rows, nrows, k, radius, dmax, out, out, out, out, out, None, 0,
                                      None)
    for k in (0, 9, -3):
        assert query(k=k) == -1
    assert query(ns=-1) == -1 and query(nd=-1) == -1 and query(nrows=-1) == -1
    assert query(nrows=5) == -1 and query(nrows=3) == -1                  # more rows than targets; all rows but not Nd
    for r in (0.0, -1.0, float("nan"), float("inf")):
        assert query(radius=r) == -1
    assert query(dmax=float("nan")) == -1 and query(dmax=float("inf")) == -1
    assert query(ns=2 ** 31) == -2 and query(nd=2 ** 31, nrows=2 ** 31) == -2
    assert query(nd=0, nrows=0) == 0 and query(rows=8, nrows=0) == 0       # zero sizes: nothing to do
    assert query(out=None) == -1

    def weights(nd=4, k=4, method=1, power=1.0, ptr=8):
        return hip_lib.gwen_knn_weights(ptr, ptr, nd, k, method, power, ptr, ptr, None)
    for k in (0, 9):
        assert weights(k=k) == -1
    assert weights(nd=-1) == -1 and weights(method=2) == -1 and weights(method=-1) == -1
    for p in (0.0, -2.0, float("nan"), float("inf")):
        assert weights(power=p) == -1
    assert weights(nd=2 ** 31) == -2
    assert weights(nd=0, ptr=None) == 0 and weights(ptr=None) == -1


def test_point_sets_and_their_coincidence_gap():
    """Nothing lies between 'coincident to rounding' and 'clearly apart', so d2 <= 1e-24 is never decided by rounding.
    The pairs through which weights are built keep d2 <= 3.4e-32 or d2 >= 3.9e-6; the two pairs that only the SEARCH
    tests use (cap -> random, random -> random; the coincidence rule plays no part there) come as close as 2.1e-6."""
    assert R.points("latlon").shape == (684, 3) and R.points("mesh2").shape == (42, 3) and R.points("mesh1").shape == (12, 3)
    assert R.points("random").shape == (2000, 3) and R.points("cap").shape == (196, 3)
    pole = R.points("latlon")
    assert (pole[:36] == pole[0]).all() and (pole[-36:] == pole[-1]).all()
    for src, dst in R.PAIRS + (("mesh1", "random"), ("random", "random")):
        d2 = dist2(R.points(dst), R.points(src))
        high = 2.1e-6 if (src, dst) in (("cap", "random"), ("random", "random")) else R.GAP_HIGH
        assert not ((d2 > R.GAP_LOW) & (d2 < high)).any(), (src, dst)
    d2 = dist2(R.points("mesh2"), R.points("latlon"))
    on = (d2 <= R.COINCIDENT2).any(axis=1)
    assert on.sum() == 6 and ((d2 > 0) & (d2 <= R.COINCIDENT2)).any(axis=1).sum() == 3      # three only to ~1e-32


@pytest.mark.parametrize("name", ["random", "mesh3", "centres"])
def test_restatement_on_a_set_against_itself(name):
    p = R.points(name)
    n = p.shape[0]
    idx, d2, count = R.knn(p, p, 4)
    assert np.array_equal(idx[:, 0], np.arange(n)) and (d2[:, 0] == 0.0).all() and (count == 4).all()
    assert (np.diff(d2, axis=1) >= 0).all()
    w, entries = R.weights(d2, count)
    assert (entries == 1).all() and (w[:, 0] == 1.0).all() and (w[:, 1:] == 0.0).all()     # every point sits on itself
    ei, w32 = R.operator(idx, w, entries)
    assert np.array_equal(ei, np.stack([np.arange(n), np.arange(n)])) and (w32 == 1.0).all()


@pytest.mark.parametrize("power", [1.0, 2.0, 1.5])
def test_restatement_rows_sum_to_one_and_order_by_distance_then_index(power):
    src, dst = R.points("mesh3"), R.points("latlon")
    idx, d2, count = R.knn(src, dst, 4)
    full = dist2(dst, src)
    for t in (0, 1, 35, 36, 300, 683):                                  # 80 rows tie at the first cut
        order = sorted(range(src.shape[0]), key=lambda s: (full[t, s], s))[:4]
        assert list(idx[t]) == order and np.array_equal(d2[t], full[t, order])
    w, entries = R.weights(d2, count, "idw", power)
    assert np.abs(w.sum(axis=1) - 1.0).max() <= 1e-15 and (w >= 0).all()
    apart = d2[:, 0] > R.COINCIDENT2
    assert apart.all() and (entries == 4).all()
    assert (np.diff(w, axis=1) <= 0).all()                              # nearer sources weigh more
    idx, d2, count = R.knn(R.points("latlon"), R.points("mesh2"), 4)    # six nodes sit on lat-lon points
    w, entries = R.weights(d2, count, "idw", power)
    on = d2[:, 0] <= R.COINCIDENT2
    assert on.sum() == 6 and (entries[on] == 1).all() and (entries[~on] == 4).all()
    assert (w[on, 0] == 1.0).all() and (w[on, 1:] == 0.0).all() and np.abs(w.sum(axis=1) - 1.0).max() <= 1e-15


def test_restatement_mask_distance_and_padding():
    src, dst = R.points("latlon"), R.points("mesh2")
    mask = np.arange(src.shape[0]) % 3 != 0
    idx, d2, count = R.knn(src, dst, 4, src_mask=mask)
    assert mask[idx].all() and (count == 4).all()
    keep = np.flatnonzero(mask)
    i2, d22, _ = R.knn(src[keep], dst, 4)
    assert np.array_equal(keep[i2], idx) and np.array_equal(d22, d2)    # original indices, same distances
    idx, d2, count = R.knn(src, dst, 4, max_distance=0.05)
    assert (count < 4).any() and (count == 0).any()
    pad = np.arange(4)[None, :] >= count[:, None]
    assert (idx[pad] == -1).all() and np.isinf(d2[pad]).all() and (d2[~pad] <= 0.05 * 0.05).all()
    idx, d2, count = R.knn(src[:3], dst, 4)
    assert (count == 3).all() and (idx[:, 3] == -1).all() and np.isinf(d2[:, 3]).all()
    x = np.arange(12, dtype=np.float32).reshape(3, 4)
    ei, w32 = R.operator(*[a[:2] for a in (idx, *R.weights(d2, count))])
    got = R.apply_f32(ei, w32, x, 2)
    assert np.abs(got - R.dense(ei, w32, 3, 2) @ x).max() <= 1e-5
