"""numpy restatements of the grid-graph contracts (include/gwen_hip.h, "Grid graphs"): brute force over every pair, in
fp64, with the library's decision expressions term by term -- numpy does not fuse a multiply into an add, and the
library is built with -ffp-contract=off, so both decide every pair identically."""
from __future__ import annotations

import numpy as np

FACE_TOL = -1e-12


def unit(pos) -> np.ndarray:
    """Rows divided by sqrt((x x + y y) + z z)."""
    p = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    n = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
    return p / n[:, None]


def dist2(dst: np.ndarray, src: np.ndarray) -> np.ndarray:
    """[Nd, Ns] of (dx dx + dy dy) + dz dz on dst - src."""
    d = dst[:, None, :] - src[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def radius_edges(src_pos, dst_pos, radius: float) -> np.ndarray:
    """int64 [2, E], row 0 = source, row 1 = target, sorted by (target, source)."""
    s, d = unit(src_pos), unit(dst_pos)
    r = np.float64(radius)
    hit = dist2(d, s) <= r * r
    di, si = np.nonzero(hit)                    # row-major: target ascending, then source ascending
    return np.stack([si, di]).astype(np.int64)


def near_radius(src_pos, dst_pos, radius: float) -> float:
    """Smallest | |d - s| - radius | over all pairs: how far the set is from a pair that rounding could decide."""
    s, d = unit(src_pos), unit(dst_pos)
    if not s.size or not d.size:
        return np.inf
    return float(np.abs(np.sqrt(dist2(d, s)) - radius).min())


def det3(u, v, w):
    """u . (v x w) as (u0 (v1 w2 - v2 w1) + u1 (v2 w0 - v0 w2)) + u2 (v0 w1 - v1 w0)."""
    return (u[..., 0] * (v[..., 1] * w[..., 2] - v[..., 2] * w[..., 1])
            + u[..., 1] * (v[..., 2] * w[..., 0] - v[..., 0] * w[..., 2])) \
        + u[..., 2] * (v[..., 0] * w[..., 1] - v[..., 1] * w[..., 0])


def face_centres(mesh) -> np.ndarray:
    c = mesh.pos[mesh.faces].mean(axis=1)
    return c / np.linalg.norm(c, axis=1, keepdims=True)


def max_edge_length(mesh) -> float:
    d = mesh.pos[mesh.edge_index[1]] - mesh.pos[mesh.edge_index[0]]
    return float(np.sqrt((d * d).sum(axis=1).max()))


def accepted_faces(points, mesh) -> tuple:
    """(accept bool [N, F], dets float64 [N, F, 3]): face f is a candidate for point p when its normalised centre is
    within the longest mesh edge of p, and accepted when its three determinants are all >= -1e-12."""
    p = unit(points)
    a, b, c = (mesh.pos[mesh.faces[:, k]][None, :, :] for k in range(3))
    q = p[:, None, :]
    dets = np.stack([det3(q, b, c), det3(q, c, a), det3(q, a, b)], axis=-1)
    r = np.float64(max_edge_length(mesh))
    cand = dist2(p, face_centres(mesh)) <= r * r
    return cand & (dets >= FACE_TOL).all(axis=-1), dets


def containing_faces(points, mesh) -> tuple:
    """(face int64 [N] -- the lowest accepted id, -1 without one --, weights float64 [N, 3])."""
    acc, dets = accepted_faces(points, mesh)
    face = np.where(acc.any(axis=1), acc.argmax(axis=1), -1).astype(np.int64)
    d = dets[np.arange(acc.shape[0]), np.maximum(face, 0)]
    w = d / ((d[:, 0] + d[:, 1]) + d[:, 2])[:, None]
    w[face < 0] = 0.0
    return face, w
