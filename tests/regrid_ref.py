"""numpy restatements of the regridding contracts (include/gwen_hip.h, "Regridding"): brute force over every pair in
fp64 with the library's expressions term by term -- numpy does not fuse a multiply into an add and the library is built
with -ffp-contract=off, so both compute the same d2 bits and order every row identically."""
from __future__ import annotations

import numpy as np

from gridgraph_ref import dist2, unit

COINCIDENT2 = 1e-24


def knn(src_pos, dst_pos, k: int, max_distance=None, src_mask=None):
    """(idx int64 [Nd, k] padded with -1, d2 float64 [Nd, k] padded with +inf, count int64 [Nd]): row t = its
    min(k, candidates) candidates in ascending (d2, source index) order.  Candidates: the sources the mask keeps, and with
    max_distance D those with d2 <= D D."""
    s, d = unit(src_pos), unit(dst_pos)
    ns, nd = s.shape[0], d.shape[0]
    d2 = dist2(d, s) if ns and nd else np.zeros((nd, ns))
    ok = np.ones((nd, ns), dtype=bool)
    if src_mask is not None:
        ok &= np.asarray(src_mask, dtype=bool)[None, :]
    if max_distance is not None:
        dm = np.float64(max_distance)
        ok &= d2 <= dm * dm
    key = np.where(ok, d2, np.inf)
    order = np.argsort(key, axis=1, kind="stable")[:, :k]          # stable: the lowest index first among equal d2
    count = np.minimum(ok.sum(axis=1), k).astype(np.int64)
    idx = np.full((nd, k), -1, dtype=np.int64)
    out = np.full((nd, k), np.inf, dtype=np.float64)
    kk = order.shape[1]
    live = np.arange(kk)[None, :] < count[:, None]
    idx[:, :kk] = np.where(live, order, -1)
    out[:, :kk] = np.where(live, np.take_along_axis(d2, order, axis=1) if ns else np.inf, np.inf)
    return idx, out, count


def idw_term(d2, power: float):
    if power == 1.0:
        return 1.0 / np.sqrt(d2)
    if power == 2.0:
        return 1.0 / d2
    return np.power(np.sqrt(d2), -np.float64(power))


def weights(d2: np.ndarray, count: np.ndarray, method: str = "idw", power: float = 1.0):
    """(weights float64 [Nd, k] -- NOT yet rounded to fp32 --, entries int64 [Nd]).  idw: u_j / ((u_0 + u_1) + ...) with
    u = d^-power; a row whose nearest d2 <= 1e-24, and every row of "nearest", is ONE entry of weight 1."""
    nd, k = d2.shape
    w = np.zeros((nd, k), dtype=np.float64)
    entries = np.asarray(count, dtype=np.int64).copy()
    for t in range(nd):
        c = int(entries[t])
        if c == 0:
            continue
        if method == "nearest" or d2[t, 0] <= COINCIDENT2:
            w[t, 0], entries[t] = 1.0, 1
            continue
        u = idw_term(d2[t, :c], power)
        total = np.float64(0.0)
        for v in u:
            total = total + v
        w[t, :c] = u / total
    return w, entries


def operator(idx: np.ndarray, w: np.ndarray, entries: np.ndarray):
    """(edge_index int64 [2, E] sorted by (target, rank), weights float32 [E])."""
    nd, k = idx.shape
    keep = np.arange(k)[None, :] < entries[:, None]
    target = np.broadcast_to(np.arange(nd)[:, None], (nd, k))
    return np.stack([idx[keep], target[keep]]).astype(np.int64), w[keep].astype(np.float32)


def apply_f32(edge_index: np.ndarray, w32: np.ndarray, x: np.ndarray, num_dst: int) -> np.ndarray:
    """K2 restated in fp32: out[t] = ((w0 x0) + w1 x1) + ..., every product rounded, in stored order; x [..., Ns, C]."""
    x = np.asarray(x, dtype=np.float32)
    out = np.zeros(x.shape[:-2] + (num_dst, x.shape[-1]), dtype=np.float32)
    first = np.ones(num_dst, dtype=bool)
    for e in range(edge_index.shape[1]):
        s, t = int(edge_index[0, e]), int(edge_index[1, e])
        term = (w32[e] * x[..., s, :]).astype(np.float32)
        out[..., t, :] = term if first[t] else (out[..., t, :] + term).astype(np.float32)
        first[t] = False
    return out


def dense(edge_index: np.ndarray, w, num_src: int, num_dst: int) -> np.ndarray:
    """The operator as a dense float64 [Nd, Ns] matrix (duplicate entries add)."""
    a = np.zeros((num_dst, num_src), dtype=np.float64)
    np.add.at(a, (edge_index[1], edge_index[0]), np.asarray(w, dtype=np.float64))
    return a


# ---- the point sets of the regridding tests.  Every pair of points in them has d2 <= 3.4e-32 or d2 >= 3.9e-6
# (asserted in tests/test_regrid_host.py), so the 1e-24 coincidence rule is never decided by rounding.
GAP_LOW, GAP_HIGH = 3.4e-32, 3.9e-6
SETS = ("latlon", "mesh1", "mesh2", "mesh3", "centres", "random", "cap")
PAIRS = (("latlon", "mesh2"), ("latlon", "centres"), ("latlon", "random"), ("random", "latlon"), ("mesh3", "latlon"),
         ("cap", "random"))
_cache: dict = {}


def points(name: str) -> np.ndarray:
    """Unit vectors float64 [N, 3] of a named set (cached; callers must not write into them)."""
    if name not in _cache:
        import gwen_amd
        from helpers import SEED
        if name == "latlon":
            p = gwen_amd.latlon_grid(19, 36)[0]                       # 684 points, 36 coincident at each pole
        elif name in ("mesh1", "mesh2", "mesh3"):
            p = gwen_amd.geodesic_mesh(int(name[-1])).pos
        elif name == "centres":
            m = gwen_amd.geodesic_mesh(5)
            p = m.pos[m.faces].mean(axis=1)
        elif name == "random":
            p = np.random.default_rng(SEED).normal(size=(2000, 3))
        elif name == "cap":
            q = unit(np.random.default_rng(SEED + 1).normal(size=(4000, 3)))
            p = q[q[:, 2] > 0.9]
        else:
            raise KeyError(name)
        p = unit(p)
        p.setflags(write=False)
        _cache[name] = p
    return _cache[name]


def knn_cached(src: str, dst: str, k: int):
    key = ("knn", src, dst, k)
    if key not in _cache:
        _cache[key] = knn(points(src), points(dst), k)
    return _cache[key]
