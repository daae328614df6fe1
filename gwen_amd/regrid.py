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
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib, ops
from .graph import GraphCSR, _ptr, _stream, prepare_bipartite
from .gridgraph import _INDEX_LIMIT, _device, _workspace, containing_faces, unit_vectors
from .mesh import Mesh

MAX_K = 8
METHODS = {"nearest": _lib.REGRID_NEAREST, "idw": _lib.REGRID_IDW}


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
              policy: str = "raise") -> None:
        self.num_src, self.num_dst = int(num_src), int(num_dst)
        self.edge_index, self.weights = edge_index.contiguous(), weights.contiguous()
        missing = int(uncovered.sum().item()) if uncovered is not None and uncovered.numel() else 0
        if missing and policy == "raise":
            raise ValueError(f"Regridder: {missing} of {num_dst} target points have no source candidate "
                             '(max_distance / src_mask); pass uncovered="nan" to fill them with NaN')
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
