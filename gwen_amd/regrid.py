"""Regridding: move a field from one point set on the unit sphere to another (lat-lon or Gaussian grid <-> model grid,
model grid -> stations), as ONE sparse operator applied by K2.

BUILD-DEFINED, PARITY UNPINNED -- the reference moves no field between point sets, so the contracts are this build's own
("Regridding"; include/gwen_hip.h; restated in numpy in tests/regrid_ref.py).

    search    the exact k nearest source points of every target (csrc/regrid.hip): one thread per target keeps its k best
              while the cell list of the grid graphs is walked for a radius R; rows that found fewer than k go round again
              at 2 R.  Host work per round: ONE read-back (the number of rows still short).
    weights   inverse distance (fp64, stored as fp32), or nearest; a target that sits on a source takes that source alone.
    apply     ``ops.propagate`` (K2) over the rectangular CSR: one launch for all members, terms added in stored order, so
              the result is restatable bit for bit; the backward is K2 over the transpose.

CELL data (one value per mesh face, per lat-lon box) is moved by the first-order CONSERVATIVE remap instead: a target cell
receives the area-weighted mean of the source cells it overlaps (``Regridder.conservative``; csrc/conserve.hip clips every
candidate pair of spherical polygons on the device; DESIGN.md, "Conservative regridding"; tests/conserve_ref.py).
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib, ops
from .graph import GraphCSR, _ptr, _stream, prepare_bipartite
from .gridgraph import (_INDEX_LIMIT, _check_orientation, _device, _workspace, containing_faces, radius_edges_device,
                        sphere_points, unit_vectors)
from .mesh import Mesh

MAX_K = 8
METHODS = {"nearest": _lib.REGRID_NEAREST, "idw": _lib.REGRID_IDW}
MIN_V, MAX_V = 3, 8                       # corners of a cell
KEEP_FRACTION = 1e-12                     # a pair is an entry when its overlap exceeds this fraction of the smaller cell
NORMALIZE = {"covered": _lib.CONSERVE_COVERED, "cell": _lib.CONSERVE_CELL}
_SIDE_TOL = 1e-12                         # a vertex this far on the wrong side of an edge's great circle: not convex


def _check_k(k) -> int:
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= MAX_K:
        raise ValueError(f"k must be an integer in 1 .. {MAX_K} (got {k!r})")
    return int(k)


def _sources(src_pos, src_mask) -> Tuple[np.ndarray, Optional[np.ndarray], int]:
    """(listed unit vectors, their original indices int32 or None, number of sources before the mask)."""
    s = unit_vectors(src_pos, "src_pos")
    ns = s.shape[0]
    if ns >= _INDEX_LIMIT:
        raise ValueError("regrid: point counts out of int32 range")
    ids = None
    if src_mask is not None:
        m = src_mask.detach().cpu().numpy() if isinstance(src_mask, Tensor) else np.asarray(src_mask)
        if m.dtype != np.bool_ or m.shape != (ns,):
            raise ValueError(f"src_mask must be bool [{ns}] (got {m.dtype} {m.shape})")
        ids = np.flatnonzero(m).astype(np.int32)
        s = np.ascontiguousarray(s[ids])
    if s.shape[0] == 0:
        raise ValueError("regrid: there is no unmasked source point")
    return s, ids, ns


def _max_distance(max_distance) -> float:
    if max_distance is None:
        return -1.0
    d = float(max_distance)
    if not (d >= 0.0 and math.isfinite(d)):
        raise ValueError(f"max_distance must be finite and >= 0 (got {max_distance})")
    return d


def knn_device(sp: Tensor, ids: Optional[Tensor], dp: Tensor, k: int, max_distance: float = -1.0,
               initial_radius: Optional[float] = None, stats: Optional[dict] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """The device part of ``nearest_neighbours``: listed source unit vectors float64 ``[Ns, 3]``, their reported indices
    int32 ``[Ns]`` (or None), target unit vectors ``[Nd, 3]``, nothing validated.  ``(idx int32 [Nd, k], d2 float64 [Nd, k],
    count int32 [Nd])``.  The doubling loop lives here: one read-back a round.  ``stats`` (a dict) receives ``rounds`` and
    ``initial_radius``."""
    dev, ns, nd = dp.device, sp.size(0), dp.size(0)
    L = _lib.lib()
    idx = torch.empty((nd, k), dtype=torch.int32, device=dev)
    d2 = torch.empty((nd, k), dtype=torch.float64, device=dev)
    count = torch.empty(nd, dtype=torch.int32, device=dev)
    if nd == 0:
        return idx, d2, count
    radius = min(math.sqrt(16.0 * k / max(ns, 1)), 2.0) if initial_radius is None else float(initial_radius)
    if not (radius > 0.0 and math.isfinite(radius)):
        raise ValueError(f"initial_radius must be finite and > 0 (got {initial_radius})")
    ws = _workspace(L.gwen_knn_workspace_bytes, "gwen_knn_workspace_bytes", dev, ns, nd)
    rows, lists, cur = None, [torch.empty(nd, dtype=torch.int32, device=dev), None], 0     # two row lists, in turn
    left = torch.zeros(1, dtype=torch.int32, device=dev)
    n, rounds, first = nd, 0, radius
    while n > 0:
        rounds += 1
        with torch.cuda.device(dev):
            rc = L.gwen_knn_query(_ptr(sp), _ptr(ids), ns, _ptr(dp), nd, _ptr(rows), n, k, radius, max_distance,
                                  _ptr(idx), _ptr(d2), _ptr(count), _ptr(lists[cur]), _ptr(left), _ptr(ws), ws.numel(),
                                  _stream(dev))
        _lib.check(rc, "gwen_knn_query")
        n = int(left.item())                       # the one read-back of the round: rows that found fewer than k
        if n > 0:
            rows, cur = lists[cur], cur ^ 1
            if lists[cur] is None:
                lists[cur] = torch.empty(n, dtype=torch.int32, device=dev)    # later rounds never list more rows
            radius *= 2.0
    if stats is not None:
        stats.update(rounds=rounds, initial_radius=first)
    return idx, d2, count


def nearest_neighbours(src_pos, dst_pos, k: int, device, max_distance: Optional[float] = None, src_mask=None,
                       initial_radius: Optional[float] = None) -> Tuple[Tensor, Tensor]:
    """The exact ``k`` nearest source points of every target point: ``(idx int64 [Nd, k], d2 float64 [Nd, k])`` on
    ``device``.  Row ``t`` holds its ``min(k, candidates)`` candidates in ascending ``(d2, source index)`` order -- the
    lowest index wins every tie -- padded with -1 / +inf.  Candidates are the sources ``src_mask`` keeps (bool ``[Ns]``;
    indices reported are the original ones) and, with ``max_distance`` (a chord length), those with ``d2 <= D D``;
    ``d2 = (dx dx + dy dy) + dz dz`` on ``dst - src`` in fp64 without fused multiply-add, so a numpy restatement computes
    the same bits.  Positions are normalised and validated on the host.  ``initial_radius`` only changes how many rounds
    the search takes, never the result.  ``ValueError``: non-finite or zero vectors, ``k`` outside 1 .. 8, no unmasked
    source."""
    k = _check_k(k)
    dmax = _max_distance(max_distance)
    s, ids, _ = _sources(src_pos, src_mask)
    d = unit_vectors(dst_pos, "dst_pos")
    if d.shape[0] >= _INDEX_LIMIT or d.shape[0] * k >= _INDEX_LIMIT:
        raise ValueError("regrid: point counts out of int32 range")
    if initial_radius is not None and not (float(initial_radius) > 0.0 and math.isfinite(float(initial_radius))):
        raise ValueError(f"initial_radius must be finite and > 0 (got {initial_radius})")
    dev = _device(device)
    idx, d2, _ = knn_device(torch.from_numpy(s).to(dev), None if ids is None else torch.from_numpy(ids).to(dev),
                            torch.from_numpy(d).to(dev), k, dmax, initial_radius)
    return idx.long(), d2


def knn_weights(d2: Tensor, count: Tensor, method: str = "idw", power: float = 1.0) -> Tuple[Tensor, Tensor]:
    """``(weights float32 [Nd, k], entries int32 [Nd])`` of ``gwen_knn_weights`` from the search's ``d2`` / ``count``."""
    nd, k = d2.shape
    dev = d2.device
    w = torch.empty((nd, k), dtype=torch.float32, device=dev)
    entries = torch.empty(nd, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().gwen_knn_weights(_ptr(d2), _ptr(count), nd, k, METHODS[method], float(power), _ptr(w),
                                         _ptr(entries), _stream(dev))
    _lib.check(rc, "gwen_knn_weights")
    return w, entries


class _Apply(torch.autograd.Function):
    """y = A x on K2; grad_x = A^T g on K2 over the transpose (hub sources take its long-row segment path)."""

    @staticmethod
    def forward(ctx, x: Tensor, graph: GraphCSR, fill: Optional[Tensor]) -> Tensor:
        ctx.graph = graph
        y = ops.propagate(graph, x)
        if fill is not None:                                    # uncovered targets: NaN rows (they have no entry)
            y = y.masked_fill(fill, float("nan"))
        return y

    @staticmethod
    def backward(ctx, g: Tensor):
        return ops.propagate(ctx.graph, g.contiguous(), transposed=True), None, None


class Regridder:
    """A field on ``src_pos`` -> the same field on ``dst_pos``, as one sparse operator built once.

    ``method="idw"``: inverse-distance weights ``d^-power`` over the ``k`` nearest sources, normalised in stored order
    (fp64, stored as fp32); a target within 1e-12 of a source takes that source alone with weight exactly 1.
    ``method="nearest"``: the nearest source, weight 1.  ``max_distance`` (a chord length) and ``src_mask`` (bool ``[Ns]``,
    True = use) restrict the candidates; a target left with none is ``uncovered``: ``"raise"`` -> ``ValueError``,
    ``"nan"`` -> its output rows are NaN (zero gradient) and ``.uncovered`` (bool ``[Nd]``) marks it.

    ``regridder(x)``: ``x`` fp32 ``[Ns, C]`` or ``[members, Ns, C]`` on the device -> ``[..., Nd, C]``; one K2 launch
    for all members, terms added in stored ``(target, rank)`` order; differentiable in ``x`` (the weights carry no
    gradient).  After one eager call (which builds the lazy layouts) the call is capturable in a ``torch.cuda.graph``.

    Attributes: ``num_src``, ``num_dst``, ``edge_index`` int64 ``[2, E]`` sorted by (target, rank), ``weights`` fp32
    ``[E]``, ``graph`` (the ``GraphCSR``), ``uncovered``."""

    def __init__(self, src_pos, dst_pos, device, method: str = "idw", k: int = 4, power: float = 1.0,
                 max_distance: Optional[float] = None, src_mask=None, uncovered: str = "raise"):
        if method not in METHODS:
            raise ValueError(f"method must be one of {sorted(METHODS)} (got {method!r})")
        if uncovered not in ("raise", "nan"):
            raise ValueError(f'uncovered must be "raise" or "nan" (got {uncovered!r})')
        k = 1 if method == "nearest" else _check_k(k)
        power = float(power)
        if not (power > 0.0 and math.isfinite(power)):
            raise ValueError(f"power must be finite and > 0 (got {power})")
        dmax = _max_distance(max_distance)
        s, ids, ns = _sources(src_pos, src_mask)
        d = unit_vectors(dst_pos, "dst_pos")
        nd = d.shape[0]
        if nd >= _INDEX_LIMIT or nd * k >= _INDEX_LIMIT:
            raise ValueError("regrid: point counts out of int32 range")
        dev = _device(device)
        idx, d2, count = knn_device(torch.from_numpy(s).to(dev), None if ids is None else torch.from_numpy(ids).to(dev),
                                    torch.from_numpy(d).to(dev), k, dmax)
        w, entries = knn_weights(d2, count, method, power)
        keep = torch.arange(k, device=dev)[None, :] < entries[:, None]                # [Nd, k], (target, rank) order
        target = torch.arange(nd, device=dev)[:, None].expand(nd, k)
        edge_index = torch.stack([idx.long()[keep], target[keep]])
        self._init(edge_index, w[keep], ns, nd, entries == 0, uncovered)

    def _init(self, edge_index: Tensor, weights: Tensor, num_src: int, num_dst: int, uncovered: Optional[Tensor],
              policy: str = "raise", what: str = "target points have no source candidate (max_distance / src_mask)") -> None:
        self.num_src, self.num_dst = int(num_src), int(num_dst)
        self.edge_index, self.weights = edge_index.contiguous(), weights.contiguous()
        missing = int(uncovered.sum().item()) if uncovered is not None and uncovered.numel() else 0
        if missing and policy == "raise":
            raise ValueError(f'Regridder: {missing} of {num_dst} {what}; pass uncovered="nan" to fill them with NaN')
        self.uncovered = uncovered if uncovered is not None else \
            torch.zeros(num_dst, dtype=torch.bool, device=edge_index.device)
        self._fill = self.uncovered[:, None] if missing else None
        self.graph = prepare_bipartite(self.edge_index, self.num_src, self.num_dst, self.weights, mean=False)

    @classmethod
    def from_weights(cls, edge_index: Tensor, weight: Tensor, num_src: int, num_dst: int) -> "Regridder":
        """Wrap an operator the caller already has: ``edge_index`` int64 ``[2, E]`` on the device (row 0 = source, row
        1 = target), ``weight`` ``[E]``.  A target's terms are added in the order its edges are given."""
        if not isinstance(edge_index, Tensor) or edge_index.dtype != torch.int64 or edge_index.dim() != 2 \
                or edge_index.size(0) != 2:
            raise ValueError("edge_index must be an int64 tensor [2, E]")
        if not isinstance(weight, Tensor) or weight.dim() != 1 or weight.numel() != edge_index.size(1):
            raise ValueError("weight must have shape [E]")
        if num_src < 0 or num_dst < 0:
            raise ValueError("num_src and num_dst must be >= 0")
        if not edge_index.is_cuda or weight.device != edge_index.device:
            raise RuntimeError("gwen_amd needs edge_index and weight on one HIP device; there is no CPU fallback")
        self = cls.__new__(cls)
        self._init(edge_index, weight.detach().to(torch.float32), num_src, num_dst, None)
        return self

    @classmethod
    def from_mesh(cls, mesh: Mesh, dst_pos, device) -> "Regridder":
        """Barycentric interpolation of a field on the mesh NODES: every target receives from the three corners of the
        face that contains it (``containing_faces``), in corner order, with the fp64 weights rounded to fp32."""
        face, w = containing_faces(dst_pos, mesh, device)
        nd = face.numel()
        corners = torch.from_numpy(np.ascontiguousarray(mesh.faces, dtype=np.int64)).to(face.device)[face]     # [Nd, 3]
        edge_index = torch.stack([corners.reshape(-1),
                                  torch.arange(nd, dtype=torch.int64, device=face.device).repeat_interleave(3)])
        self = cls.__new__(cls)
        self._init(edge_index, w.reshape(-1).to(torch.float32), mesh.num_nodes, nd, None)
        return self

    def __call__(self, x: Tensor) -> Tensor:
        ops._require(x, "x")
        if x.dim() not in (2, 3) or x.size(-2) != self.num_src:
            raise ValueError(f"expected [{self.num_src}, C] or [members, {self.num_src}, C], got {tuple(x.shape)}")
        if x.device != self.graph.device:
            raise RuntimeError("x and the regridder are on different devices")
        return _Apply.apply(x, self.graph, self._fill)

    @classmethod
    def conservative(cls, src_cells, dst_cells, device, normalize: str = "covered", min_coverage: float = 1e-9,
                     uncovered: str = "raise") -> "Regridder":
        """First-order conservative remap of CELL data: target cell ``t`` receives ``sum_s w_ts x_s`` over the source
        cells it overlaps, ``A_ts`` being the area of the intersection of the two spherical polygons (``cell_overlaps``).

        ``normalize="covered"``: ``w_ts = A_ts / sum_s A_ts`` -- the mean over the covered part, so a constant field stays
        constant on a partially covered target.  ``"cell"``: ``w_ts = A_ts / A_t`` -- the global integral
        ``sum_t A_t y_t = sum_s A_s x_s`` is preserved (what the source does not cover counts as zero).  On two full
        tessellations the two agree to rounding.  ``coverage = sum_s A_ts / A_t``; a target with ``coverage <
        min_coverage`` is uncovered and carries no entry: ``uncovered="raise"`` -> ``ValueError``, ``"nan"`` -> NaN rows
        with zero gradient.  Cell sets are ``[N, V, 3]`` as ``mesh_cells`` / ``mesh_dual_cells`` / ``latlon_cells`` give
        them (see ``check_cells``).  The operator is applied by K2 like every other ``Regridder``: entries of a target in
        ascending source order, bitwise restatable, differentiable in ``x``, capturable after one eager call.

        Extra attributes: ``src_area`` / ``dst_area`` float64 ``[Ns]`` / ``[Nd]``, ``coverage`` float64 ``[Nd]``."""
        if normalize not in NORMALIZE:
            raise ValueError(f"normalize must be one of {sorted(NORMALIZE)} (got {normalize!r})")
        if uncovered not in ("raise", "nan"):
            raise ValueError(f'uncovered must be "raise" or "nan" (got {uncovered!r})')
        min_coverage = float(min_coverage)
        if not (0.0 <= min_coverage <= 1.0):
            raise ValueError(f"min_coverage must be in [0, 1] (got {min_coverage})")
        edge_index, area, src_area, dst_area = cell_overlaps(src_cells, dst_cells, device)
        nd = dst_area.numel()
        w, coverage = overlap_weights(edge_index, area, dst_area, normalize)
        missing = (coverage < min_coverage) | (coverage <= 0.0)
        keep = ~missing[edge_index[1]]                      # an uncovered target carries no entry: nothing reaches it
        self = cls.__new__(cls)
        self.src_area, self.dst_area, self.coverage = src_area, dst_area, coverage
        self._init(edge_index[:, keep], w[keep], src_area.numel(), nd, missing, uncovered,
                   what="target cells overlap no source cell (coverage < min_coverage)")
        return self


# ---- cells: convex spherical polygons [N, V, 3], counter-clockwise seen from outside, great-circle edges

def mesh_cells(mesh: Mesh) -> np.ndarray:
    """The faces of ``mesh`` as cells, float64 ``[F, 3, 3]`` (face order, corner order), after the orientation check."""
    _check_orientation(mesh)
    return np.ascontiguousarray(np.asarray(mesh.pos, dtype=np.float64)[np.asarray(mesh.faces)])


def mesh_dual_cells(mesh: Mesh) -> np.ndarray:
    """The cell of every mesh NODE, float64 ``[N, 6, 3]``: the polygon through the normalised centres of the node's
    incident faces, counter-clockwise seen from outside (ascending angle about the node in the tangent frame ``(e1, n x
    e1)``, ``e1`` = the coordinate axis of the node's smallest component made tangent).  The twelve pentagons repeat
    their last vertex.  The dual cells tile the sphere, so a field on mesh nodes can take part in a conservative remap."""
    _check_orientation(mesh)
    pos, faces = np.asarray(mesh.pos, dtype=np.float64), np.asarray(mesh.faces)
    n = pos.shape[0]
    c = pos[faces].sum(axis=1)
    c /= np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])[:, None]
    node, face = faces.reshape(-1), np.repeat(np.arange(faces.shape[0]), 3)
    deg = np.bincount(node, minlength=n)
    if n and (deg.min() < 3 or deg.max() > 6):
        raise ValueError("mesh_dual_cells: every node needs 3 .. 6 incident faces")
    axis = np.zeros_like(pos)
    axis[np.arange(n), np.argmin(np.abs(pos), axis=1)] = 1.0
    e1 = axis - (axis * pos).sum(axis=1)[:, None] * pos
    e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    e2 = np.cross(pos, e1)
    v = c[face]
    ang = np.arctan2((v * e2[node]).sum(axis=1), (v * e1[node]).sum(axis=1))
    order = np.lexsort((ang, node))
    node, face = node[order], face[order]
    start = np.concatenate([[0], np.cumsum(deg)])
    rank = np.arange(node.size) - start[node]
    out = np.empty((n, 6, 3), dtype=np.float64)
    last = face[start[1:] - 1]
    out[:] = c[last][:, None, :]                          # fewer than 6: the last vertex repeated
    out[node, rank] = c[face]
    return out


def latlon_cells(nlat: int, nlon: int, poles: bool = True) -> np.ndarray:
    """The cells of ``latlon_grid(nlat, nlon, poles)``, float64 ``[nlat * nlon, 4, 3]``, in its order and with its
    latitudes: corners ``(lo, lon - d/2), (lo, lon + d/2), (hi, lon + d/2), (hi, lon - d/2)``, ``lo`` / ``hi`` midway
    between rows and clipped at +-90, ``d = 360 / nlon``.  A cell that touches a pole is a wedge: its two polar corners
    coincide.  EDGES ARE GREAT-CIRCLE ARCS, also where the true box has a parallel (as in ESMF-style remaps); neighbours
    share the same arc, so the cells still tile the sphere exactly, but a cell is not exactly its lat-lon box (its area
    differs from the band weight of ``latlon_grid`` at second order in the cell size)."""
    if nlat < (2 if poles else 1) or nlon < 3:
        raise ValueError("latlon_cells needs nlon >= 3 and nlat >= 1 (>= 2 with poles)")
    k = np.arange(nlat, dtype=np.float64)
    if poles:
        step = 180.0 / (nlat - 1)
        lat = -90.0 + step * k
        lat[-1] = 90.0
    else:
        step = 180.0 / nlat
        lat = -90.0 + step * (k + 0.5)
    lat = 0.5 * (lat - lat[::-1])
    lo, hi = np.clip(lat - 0.5 * step, -90.0, 90.0), np.clip(lat + 0.5 * step, -90.0, 90.0)
    west = (360.0 / nlon) * (np.arange(nlon, dtype=np.float64) - 0.5)
    # a meridian must give the same bits to the cells on both sides of it: every corner comes from the list of WEST edges
    w_lo = sphere_points(lo[:, None], west[None, :]).reshape(nlat, nlon, 3)
    w_hi = sphere_points(hi[:, None], west[None, :]).reshape(nlat, nlon, 3)
    e_lo, e_hi = np.roll(w_lo, -1, axis=1), np.roll(w_hi, -1, axis=1)
    return np.ascontiguousarray(np.stack([w_lo, e_lo, e_hi, w_hi], axis=2).reshape(nlat * nlon, 4, 3))


def _cell_geometry(c: np.ndarray):
    """(centre [N, 3], squared chord radius [N]) by the library's expressions."""
    s = c[:, 0].copy()
    for k in range(1, c.shape[1]):
        s = s + c[:, k]
    m = s / np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])[:, None]
    d = c - m[:, None, :]
    return m, ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).max(axis=1)


def check_cells(cells, name: str = "cells") -> np.ndarray:
    """``cells`` as contiguous float64 ``[N, V, 3]`` with every vertex normalised, or ``ValueError``: a shape other than
    ``[N, V, 3]`` with 3 <= V <= 8, non-finite or zero vectors, N beyond int32, and -- with the number of cells that fail
    -- a cell with fewer than 3 distinct vertices (only consecutive vertices may coincide: any other repeat fails the
    next test), a vertex more than 1e-12 on the
    wrong side of another edge's great circle (the cell is not convex, or is clockwise), or a cell that does not fit a cap
    of chord radius 1 about its normalised vertex mean."""
    c = cells.detach().cpu().numpy() if isinstance(cells, Tensor) else np.asarray(cells)
    if c.ndim != 3 or c.shape[2] != 3 or not MIN_V <= c.shape[1] <= MAX_V:
        raise ValueError(f"{name} must have shape [N, V, 3] with {MIN_V} <= V <= {MAX_V} (got {c.shape})")
    n, v = c.shape[0], c.shape[1]
    if n >= _INDEX_LIMIT:
        raise ValueError(f"{name}: cell count out of int32 range")
    c = unit_vectors(np.asarray(c, dtype=np.float64).reshape(n * v, 3), name).reshape(n, v, 3)
    if n == 0:
        return c
    nxt = np.roll(c, -1, axis=1)
    live = (c != nxt).any(axis=2)                                              # [N, V]: edge k -> k + 1 has length
    bad = live.sum(axis=1) < 3
    if bad.any():
        raise ValueError(f"{name}: {int(bad.sum())} of {n} cells have fewer than 3 distinct vertices")
    nrm = np.stack([c[..., 1] * nxt[..., 2] - c[..., 2] * nxt[..., 1], c[..., 2] * nxt[..., 0] - c[..., 0] * nxt[..., 2],
                    c[..., 0] * nxt[..., 1] - c[..., 1] * nxt[..., 0]], axis=2)                          # [N, V(edge), 3]
    side = np.einsum("nek,npk->nep", nrm, c)                                   # vertex p against edge e
    side = np.where(live[:, :, None], side, 0.0)
    bad = (side < -_SIDE_TOL).any(axis=(1, 2)) | ~(side > _SIDE_TOL).any(axis=(1, 2))
    if bad.any():
        raise ValueError(f"{name}: {int(bad.sum())} of {n} cells are not convex and counter-clockwise seen from outside "
                         "(a vertex lies on the wrong side of another edge's great circle, or the cell has no area)")
    _, r2 = _cell_geometry(c)
    bad = ~(r2 <= 1.0)
    if bad.any():
        raise ValueError(f"{name}: {int(bad.sum())} of {n} cells do not fit a cap of chord radius 1 about their centre")
    return np.ascontiguousarray(c)


def cell_geometry_device(cells: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """``gwen_cell_areas`` on validated cells already on the device: ``(centre [N, 3], radius [N], area [N])`` float64."""
    dev, n, v = cells.device, cells.size(0), cells.size(1)
    centre = torch.empty((n, 3), dtype=torch.float64, device=dev)
    radius = torch.empty(n, dtype=torch.float64, device=dev)
    area = torch.empty(n, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().gwen_cell_areas(_ptr(cells), n, v, _ptr(centre), _ptr(radius), _ptr(area), _stream(dev))
    _lib.check(rc, "gwen_cell_areas")
    return centre, radius, area


def cell_areas(cells, device) -> Tensor:
    """The area (solid angle) of every cell, float64 ``[N]`` on ``device``: the fan sum of signed triangle solid angles
    ``2 atan2(a . (b x c), 1 + a . b + b . c + c . a)`` in fp64.  ``ValueError`` as ``check_cells``."""
    c = check_cells(cells)
    dev = _device(device)
    return cell_geometry_device(torch.from_numpy(c).to(dev))[2]


def overlap_areas_device(sc: Tensor, dc: Tensor, pairs: Tensor, s_geo, d_geo) -> Tensor:
    """``gwen_cell_overlap_areas``: float64 ``[E]`` for candidate ``pairs`` int64 ``[2, E]``; nothing validated."""
    dev, e = sc.device, pairs.size(1)
    area = torch.empty(e, dtype=torch.float64, device=dev)
    pairs = pairs.contiguous()
    with torch.cuda.device(dev):
        rc = _lib.lib().gwen_cell_overlap_areas(_ptr(sc), sc.size(0), sc.size(1), _ptr(dc), dc.size(0), dc.size(1),
                                                _ptr(pairs), e, _ptr(s_geo[0]), _ptr(s_geo[1]), _ptr(d_geo[0]),
                                                _ptr(d_geo[1]), _ptr(area), _stream(dev))
    _lib.check(rc, "gwen_cell_overlap_areas")
    return area


def cell_overlaps(src_cells, dst_cells, device, stats: Optional[dict] = None) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Every overlapping pair of a source and a target cell: ``(edge_index int64 [2, E] sorted by (target, source), area
    float64 [E], src_area float64 [Ns], dst_area float64 [Nd])`` on ``device``.

    Candidates are the pairs whose centres (normalised vertex means) are within ``max r_S + max r_T`` (``r`` = the largest
    chord from a cell's centre to its vertices; the fixed-radius search of the grid graphs); each candidate is one work
    item on the device: rejected when its own two caps are disjoint, else S is clipped against the great-circle
    half-spaces of T's edges and the polygon measured, all in fp64.  A pair is kept when ``area > 1e-12 min(A_S, A_T)``:
    cells that only share an edge or a corner give slivers of relative size ~1e-15.  ``stats`` (a dict) receives
    ``candidates``, ``kept`` and ``search_radius``.  ``ValueError`` as ``check_cells``, or too many candidates for int32."""
    s, d = check_cells(src_cells, "src_cells"), check_cells(dst_cells, "dst_cells")
    dev = _device(device)
    return cell_overlaps_device(torch.from_numpy(s).to(dev), torch.from_numpy(d).to(dev), stats)


def cell_overlaps_device(sc: Tensor, dc: Tensor, stats: Optional[dict] = None):
    """The device part of ``cell_overlaps``: validated cells float64 ``[N, V, 3]`` already on the device.  Two read-backs:
    the search radius and (inside the search) the number of candidates."""
    dev, ns, nd = sc.device, sc.size(0), dc.size(0)
    s_geo, d_geo = cell_geometry_device(sc), cell_geometry_device(dc)
    if ns == 0 or nd == 0:
        empty = torch.empty((2, 0), dtype=torch.int64, device=dev)
        return empty, torch.empty(0, dtype=torch.float64, device=dev), s_geo[2], d_geo[2]
    reach = float((s_geo[1].max() + d_geo[1].max()).item()) * (1.0 + 1e-12)     # read-back: no pair the kernel accepts
    pairs = radius_edges_device(s_geo[0], d_geo[0], reach)                      # is farther; sorted by (target, source)
    area = overlap_areas_device(sc, dc, pairs, s_geo, d_geo)
    keep = area > KEEP_FRACTION * torch.minimum(s_geo[2][pairs[0]], d_geo[2][pairs[1]])
    if stats is not None:
        stats.update(candidates=int(pairs.size(1)), kept=int(keep.sum().item()), search_radius=reach)
    return pairs[:, keep].contiguous(), area[keep], s_geo[2], d_geo[2]


def overlap_weights(edge_index: Tensor, area: Tensor, dst_area: Tensor, normalize: str = "covered"):
    """``(weights float32 [E], coverage float64 [Nd])`` of ``gwen_cell_overlap_weights`` for pairs sorted by target: the
    row pointer comes from integer counts, every row is summed in stored order."""
    dev, nd, e = area.device, dst_area.numel(), area.numel()
    rowptr = torch.zeros(nd + 1, dtype=torch.int64, device=dev)
    if e:
        torch.cumsum(torch.bincount(edge_index[1], minlength=nd), 0, out=rowptr[1:])
    w = torch.empty(e, dtype=torch.float32, device=dev)
    coverage = torch.empty(nd, dtype=torch.float64, device=dev)
    area = area.contiguous()
    with torch.cuda.device(dev):
        rc = _lib.lib().gwen_cell_overlap_weights(_ptr(rowptr), _ptr(area), _ptr(dst_area), nd, e, NORMALIZE[normalize],
                                                  _ptr(w), _ptr(coverage), _stream(dev))
    _lib.check(rc, "gwen_cell_overlap_weights")
    return w, coverage
