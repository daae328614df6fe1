"""Grid <-> mesh graphs for ARBITRARY grid points (lat-lon, Gaussian, ICON cell centres, ...), built on the device.

BUILD-DEFINED, PARITY UNPINNED -- the reference has no grid <-> mesh graphs at all (its graph is the
complete graph over ensemble members), so nothing here can be compared with it; the contracts are this build's own
("Grid graphs"; include/gwen_hip.h; restated in numpy in tests/gridgraph_ref.py).  They follow the two
constructions of the published encode-process-decode weather models:

    grid -> mesh   every grid point is linked to the mesh nodes within a fixed radius, 0.6 x the longest mesh edge
    mesh -> grid   every grid point receives from the three corners of the mesh triangle that contains it

Both are one fixed-radius neighbour query on the unit sphere through a uniform cell list (csrc/gridgraph.hip), in fp64,
atomic-free and bitwise reproducible.  Host work is O(N): normalisation, validation and one read-back of the edge count.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib
from .graph import _ptr, _stream
from .mesh import Mesh

RADIUS_FACTOR = 0.6          # default g2m radius in units of the longest mesh edge
_INDEX_LIMIT = 2 ** 31 - 1


def sphere_points(lat_deg, lon_deg) -> np.ndarray:
    """Unit vectors ``[N, 3]`` float64 of latitude / longitude in degrees (broadcast against each other, flattened):
    ``(cos lat cos lon, cos lat sin lon, sin lat)``."""
    lat, lon = np.broadcast_arrays(np.asarray(lat_deg, dtype=np.float64), np.asarray(lon_deg, dtype=np.float64))
    lat, lon = np.deg2rad(lat.reshape(-1)), np.deg2rad(lon.reshape(-1))
    cl = np.where(np.abs(lat) == 0.5 * np.pi, 0.0, np.cos(lat))      # the points of a pole row coincide exactly
    return np.stack([cl * np.cos(lon), cl * np.sin(lon), np.sin(lat)], axis=1)


def latlon_grid(nlat: int, nlon: int, poles: bool = True) -> Tuple[np.ndarray, np.ndarray]:
    """A regular ``nlat x nlon`` latitude-longitude grid: ``(pos [nlat * nlon, 3], weights [nlat * nlon])``, row-major
    ``(lat, lon)``, south to north, longitudes ``0, 360 / nlon, ...``.  ``poles=True``: latitudes -90 ... 90 inclusive
    (the ``nlon`` points of a pole row coincide); ``poles=False``: cell-centred latitudes.  The weights are the area of
    each point's latitude band (sin of its upper edge minus sin of its lower edge: midway between rows, clipped at the
    poles) shared among the row's ``nlon`` points and normalised to sum 1 -- the ``node_weights`` of ``gwen_amd.losses``
    and ``gwen_amd.products``."""
    if nlat < (2 if poles else 1) or nlon < 1:
        raise ValueError("latlon_grid needs nlon >= 1 and nlat >= 1 (>= 2 with poles)")
    k = np.arange(nlat, dtype=np.float64)
    if poles:
        step = 180.0 / (nlat - 1)
        lat = -90.0 + step * k
        lat[-1] = 90.0
    else:
        step = 180.0 / nlat
        lat = -90.0 + step * (k + 0.5)
    lat = 0.5 * (lat - lat[::-1])                                   # symmetric about the equator to the last bit
    lon = (360.0 / nlon) * np.arange(nlon, dtype=np.float64)
    pos = sphere_points(lat[:, None], lon[None, :])
    lo, hi = np.clip(lat - 0.5 * step, -90.0, 90.0), np.clip(lat + 0.5 * step, -90.0, 90.0)
    band = np.sin(np.deg2rad(hi)) - np.sin(np.deg2rad(lo))
    band = 0.5 * (band + band[::-1])
    w = np.repeat(band / nlon, nlon)
    return pos, w / w.sum()


def unit_vectors(pos, name: str = "pos") -> np.ndarray:
    """``[N, 3]`` float64, every row divided by ``sqrt((x x + y y) + z z)``."""
    p = np.ascontiguousarray(np.asarray(pos, dtype=np.float64))
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"{name} must have shape [N, 3] (got {p.shape})")
    if not np.isfinite(p).all():
        raise ValueError(f"{name} holds non-finite coordinates")
    n = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
    if not np.isfinite(n).all() or (n == 0.0).any():
        raise ValueError(f"{name} holds zero (or overflowing) vectors: they have no direction")
    return p / n[:, None]


def _device(device) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("gwen_amd builds grid graphs on a HIP device; there is no CPU fallback")
    return dev


def _workspace(fn, what: str, dev, *args) -> Tensor:
    nbytes = C.c_size_t(0)
    rc = fn(*args, C.byref(nbytes))
    if rc == -2:
        raise ValueError(f"{what}: sizes out of int32 range")
    _lib.check(rc, what)
    return torch.empty(max(int(nbytes.value), 1), dtype=torch.uint8, device=dev)


def radius_edges(src_pos, dst_pos, radius: float, device) -> Tensor:
    """Every pair ``(s, d)`` whose unit vectors are at most ``radius`` apart (chord length): int64 ``[2, E]`` on
    ``device``, row 0 = source, row 1 = target, sorted by ``(d, s)``.  Positions are normalised on the host in fp64
    first; the decision is ``(dx dx + dy dy) + dz dz <= radius radius`` on ``dst - src`` in fp64 without fused
    multiply-add, so a numpy restatement decides every pair identically.  Runs on the current stream; the edge count is
    read back once.  ``ValueError``: non-finite or zero vectors, ``radius <= 0``, more than 2^31 - 2 edges."""
    radius = float(radius)
    if not (radius > 0.0 and np.isfinite(radius)):
        raise ValueError(f"radius must be finite and > 0 (got {radius})")
    s, d = unit_vectors(src_pos, "src_pos"), unit_vectors(dst_pos, "dst_pos")
    ns, nd = s.shape[0], d.shape[0]
    if ns >= _INDEX_LIMIT or nd >= _INDEX_LIMIT:
        raise ValueError("radius_edges: point counts out of int32 range")
    dev = _device(device)
    return radius_edges_device(torch.from_numpy(s).to(dev), torch.from_numpy(d).to(dev), radius)


def radius_edges_device(sp: Tensor, dp: Tensor, radius: float, with_rowptr: bool = False):
    """The device part of ``radius_edges``: unit vectors float64 ``[N, 3]`` already on the device, nothing validated.
    ``with_rowptr``: also the int32 ``[num_dst + 1]`` row pointer over the target-sorted list."""
    dev, ns, nd = dp.device, sp.size(0), dp.size(0)
    L = _lib.lib()
    rowptr = torch.empty(nd + 1, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    ws = _workspace(L.gwen_radius_edges_workspace_bytes, "gwen_radius_edges_workspace_bytes", dev, ns, nd)
    with torch.cuda.device(dev):
        rc = L.gwen_radius_edges_count(_ptr(sp), ns, _ptr(dp), nd, radius, _ptr(total), _ptr(ws), ws.numel(),
                                       _stream(dev))
    _lib.check(rc, "gwen_radius_edges_count")
    e = int(total.item())                          # the one read-back: the size of the result
    if e >= _INDEX_LIMIT:
        raise ValueError(f"radius_edges: {e} edges do not fit int32 indices (radius {radius})")
    out = torch.empty((2, e), dtype=torch.int64, device=dev)
    sw = _workspace(L.gwen_radius_edges_fill_workspace_bytes, "gwen_radius_edges_fill_workspace_bytes", dev, e)
    with torch.cuda.device(dev):
        rc = L.gwen_radius_edges_fill(_ptr(sp), ns, _ptr(dp), nd, radius, e, _ptr(rowptr), _ptr(out), _ptr(ws),
                                      ws.numel(), _ptr(sw), sw.numel(), _stream(dev))
    _lib.check(rc, "gwen_radius_edges_fill")
    return (out, rowptr) if with_rowptr else out


def face_centres(mesh: Mesh) -> np.ndarray:
    """Normalised centre of every face, float64 ``[F, 3]``: the forecaster's default grid."""
    c = mesh.pos[mesh.faces].mean(axis=1)
    return c / np.linalg.norm(c, axis=1, keepdims=True)


def _check_orientation(mesh: Mesh) -> None:
    f = np.asarray(mesh.faces)
    if f.ndim != 2 or f.shape[1] != 3 or (f.size and (f.min() < 0 or f.max() >= mesh.num_nodes)):
        raise ValueError("mesh.faces must be [F, 3] indices into mesh.pos")
    a, b, c = mesh.pos[f[:, 0]], mesh.pos[f[:, 1]], mesh.pos[f[:, 2]]
    vol = np.einsum("ij,ij->i", a, np.cross(b, c))
    if f.size and not (vol > 0.0).all():
        raise ValueError(f"{int((vol <= 0.0).sum())} mesh faces are not positively oriented (a . (b x c) <= 0): "
                         "the containing-face test needs counter-clockwise faces seen from outside")


def containing_faces(points, mesh: Mesh, device) -> Tuple[Tensor, Tensor]:
    """``(face int64 [N], weights float64 [N, 3])`` on ``device``: the mesh face that contains each (normalised) point
    and the point's barycentric weights over the face's corners, in the corners' order.  Face ``(a, b, c)`` contains ``p``
    when ``det(p,b,c)``, ``det(p,c,a)`` and ``det(p,a,b)`` are all >= -1e-12; candidates are the faces whose normalised
    centre is within the mesh's longest edge of ``p``; a point on an edge or a vertex lies in several faces and the
    lowest face id wins.  Weights are the three determinants over their sum, so ``sum_i w_i v_i`` is parallel to ``p``.
    ``ValueError``: bad points, a face that is not positively oriented, or a point no candidate contains."""
    p = unit_vectors(points, "points")
    _check_orientation(mesh)
    dev = _device(device)
    n, nf = p.shape[0], int(mesh.faces.shape[0])
    if n and not nf:
        raise ValueError("containing_faces: the mesh has no faces")
    if not n:
        return torch.empty(0, dtype=torch.int64, device=dev), torch.empty((0, 3), dtype=torch.float64, device=dev)
    face, w = containing_faces_device(torch.from_numpy(p).to(dev), *mesh_on_device(mesh, dev), mesh.max_edge_length())
    missing = int((face < 0).sum().item())
    if missing:
        raise ValueError(f"containing_faces: {missing} of {n} points lie in no mesh face")
    return face.long(), w


def mesh_on_device(mesh: Mesh, dev) -> Tuple[Tensor, Tensor, Tensor]:
    """(positions float64 [Nm, 3], faces int64 [F, 3], normalised face centres float64 [F, 3]) on ``dev``."""
    return (torch.from_numpy(np.ascontiguousarray(mesh.pos, dtype=np.float64)).to(dev),
            torch.from_numpy(np.ascontiguousarray(mesh.faces, dtype=np.int64)).to(dev),
            torch.from_numpy(np.ascontiguousarray(face_centres(mesh))).to(dev))


def containing_faces_device(pt: Tensor, mesh_pos: Tensor, faces: Tensor, centres: Tensor, max_edge: float):
    """The device part of ``containing_faces``: ``(face int32 [N], weights float64 [N, 3])``, -1 where no face contains
    the point; inputs as ``mesh_on_device`` gives them, nothing validated."""
    dev, n, nf = pt.device, pt.size(0), faces.size(0)
    L = _lib.lib()
    face = torch.empty(n, dtype=torch.int32, device=dev)
    w = torch.empty((n, 3), dtype=torch.float64, device=dev)
    ws = _workspace(L.gwen_containing_faces_workspace_bytes, "gwen_containing_faces_workspace_bytes", dev, nf)
    with torch.cuda.device(dev):
        rc = L.gwen_containing_faces(_ptr(pt), n, _ptr(mesh_pos), mesh_pos.size(0), _ptr(faces), _ptr(centres), nf,
                                     float(max_edge), _ptr(face), _ptr(w), _ptr(ws), ws.numel(), _stream(dev))
    _lib.check(rc, "gwen_containing_faces")
    return face, w


def grid_graphs(mesh: Mesh, grid_pos, device, radius: Optional[float] = None):
    """``(g2m_edge_index, m2g_edge_index, info)`` for grid points anywhere on the sphere, int64 ``[2, E]`` on ``device``.

    g2m: grid point -> every mesh node within ``radius`` (default ``0.6 * mesh.max_edge_length()``), sorted by (mesh node,
    grid point).  m2g: the three corners of the containing face -> the grid point, grid points ascending, corners in the
    face's order.  ``ValueError`` when a grid point reaches no mesh node (it would never be encoded).  ``info``: ``radius``,
    ``g2m_edges`` / ``m2g_edges``, the degree extremes of both sides of g2m (``g2m_grid_degree_min/max``: mesh nodes a grid
    point sends to; ``g2m_mesh_degree_min/max``: grid points a mesh node receives from), of the mesh side of m2g
    (``m2g_mesh_degree_min/max``; a grid point always receives 3) and ``mesh_nodes_without_in_edge`` -- legal (a coarse
    grid under a fine mesh leaves mesh nodes that only hear from their mesh neighbours), so only reported."""
    r = RADIUS_FACTOR * mesh.max_edge_length() if radius is None else float(radius)
    g = unit_vectors(grid_pos, "grid_pos")
    n_grid, n_mesh = g.shape[0], mesh.num_nodes
    g2m = radius_edges(g, mesh.pos, r, device)
    out_deg = torch.bincount(g2m[0], minlength=n_grid)
    in_deg = torch.bincount(g2m[1], minlength=n_mesh)
    lonely = int((out_deg == 0).sum().item()) if n_grid else 0
    if lonely:
        raise ValueError(f"grid_graphs: {lonely} of {n_grid} grid points have no mesh node within radius {r:.6g}; "
                         "raise the radius or refine the mesh")
    face, _ = containing_faces(g, mesh, device)
    corners = torch.from_numpy(np.ascontiguousarray(mesh.faces, dtype=np.int64)).to(face.device)[face]      # [N, 3]
    m2g = torch.stack([corners.reshape(-1),
                       torch.arange(n_grid, dtype=torch.int64, device=face.device).repeat_interleave(3)])
    m_out = torch.bincount(m2g[0], minlength=n_mesh)

    def ext(t):
        return (int(t.min().item()), int(t.max().item())) if t.numel() else (0, 0)
    info = {"radius": r, "grid_nodes": n_grid, "mesh_nodes": n_mesh,
            "g2m_edges": int(g2m.size(1)), "m2g_edges": int(m2g.size(1)),
            "mesh_nodes_without_in_edge": int((in_deg == 0).sum().item())}
    for key, t in (("g2m_grid_degree", out_deg), ("g2m_mesh_degree", in_deg), ("m2g_mesh_degree", m_out)):
        info[key + "_min"], info[key + "_max"] = ext(t)
    return g2m, m2g, info
