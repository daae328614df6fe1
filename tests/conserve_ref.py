"""numpy restatement of the conservative-regridding contract (include/gwen_hip.h, "Conservative regridding"): the cell
generators, centre / radius / area of a cell, the Sutherland-Hodgman clip of one spherical polygon against the great-circle
half-spaces of another, candidate selection by the cap test over ALL pairs, the keep rule and the weights -- in fp64 with
the library's expressions term by term (numpy does not fuse a multiply into an add and the library is built with
-ffp-contract=off; only atan2 may differ in the last place, which is why areas are compared by tolerance).  The clip is
vectorised over pairs, not over vertices: every pair goes through exactly the scalar sequence of the contract."""
from __future__ import annotations

import functools

import numpy as np

MAX_POLY = 16
KEEP_FRACTION = 1e-12


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def tri(a, b, c):
    """Signed solid angle of the spherical triangle (a, b, c)."""
    return 2.0 * np.arctan2(dot(a, cross(b, c)), ((1.0 + dot(a, b)) + dot(b, c)) + dot(c, a))


def unit_cells(cells) -> np.ndarray:
    """[N, V, 3] float64 with every vertex divided by sqrt((x x + y y) + z z): what the library does to its input."""
    c = np.asarray(cells, dtype=np.float64)
    return np.ascontiguousarray(c / np.sqrt(dot(c, c))[..., None])


def fan_area(poly: np.ndarray, count: np.ndarray) -> np.ndarray:
    """(tri(P0, P1, P2) + tri(P0, P2, P3)) + ... over the first count vertices of every row of poly [E, M, 3]."""
    area = np.zeros(poly.shape[0])
    for k in range(2, poly.shape[1]):
        area = np.where(k < count, area + tri(poly[:, 0], poly[:, k - 1], poly[:, k]), area)
    return area


def geometry(cells: np.ndarray):
    """(centre [N, 3], radius [N], area [N]) of gwen_cell_areas."""
    s = cells[:, 0].copy()
    for k in range(1, cells.shape[1]):
        s = s + cells[:, k]
    centre = s / np.sqrt(dot(s, s))[:, None]
    d = cells - centre[:, None, :]
    radius = np.sqrt(dot(d, d).max(axis=1))
    return centre, radius, fan_area(cells, np.full(cells.shape[0], cells.shape[1]))


def clip(S: np.ndarray, T: np.ndarray):
    """S [E, VS, 3] clipped against every non-degenerate edge of T [E, VT, 3]: (polygon [E, 16, 3], count [E], the
    largest vertex count any pair reached -- the contract holds 16 and drops the rest)."""
    E, vs, vt = S.shape[0], S.shape[1], T.shape[1]
    rows = np.arange(E)
    cur = np.zeros((E, MAX_POLY, 3))
    cur[:, :vs] = S
    m = np.full(E, vs)
    peak = vs
    for j in range(vt):
        a, b = T[:, j], T[:, (j + 1) % vt]
        live = (a != b).any(axis=1) & (m > 0)
        if not live.any():
            continue
        n = cross(a, b)
        d = dot(n[:, None, :], cur)
        nxt, o = np.zeros_like(cur), np.zeros(E, dtype=np.int64)
        for k in range(MAX_POLY):
            act = live & (k < m)
            if not act.any():
                break
            kq = np.minimum(np.where(k + 1 == m, 0, k + 1), MAX_POLY - 1)
            p, q, dp, dq = cur[:, k], cur[rows, kq], d[:, k], d[rows, kq]
            in_p, in_q = dp >= 0.0, dq >= 0.0
            keep = act & in_p
            w = keep & (o < MAX_POLY)
            nxt[rows[w], o[w]] = p[w]
            o = o + keep
            crossing = act & (in_p != in_q)
            x = np.abs(dp)[:, None] * q + np.abs(dq)[:, None] * p
            with np.errstate(invalid="ignore", divide="ignore"):
                x = x / np.sqrt(dot(x, x))[:, None]
            w = crossing & (o < MAX_POLY)
            nxt[rows[w], o[w]] = x[w]
            o = o + crossing
        peak = max(peak, int(o[live].max()))
        cur = np.where(live[:, None, None], nxt, cur)
        m = np.where(live, np.minimum(o, MAX_POLY), m)
    return cur, m, peak


def overlaps(src_cells: np.ndarray, dst_cells: np.ndarray) -> dict:
    """Everything about one (source set, target set): the candidates of the cap test over all pairs in (target, source)
    order with their areas, and the kept pairs.  Keys: candidates int64 [2, C], candidate_area [C], relative [C] (area over
    the smaller cell), peak, src_area, dst_area, edge_index int64 [2, E], area [E]."""
    sc, sr, sa = geometry(src_cells)
    dc, dr, da = geometry(dst_cells)
    d = dc[:, None, :] - sc[None, :, :]
    reach = sr[None, :] + dr[:, None]
    t, s = np.nonzero(~(dot(d, d) > reach * reach))                    # row-major: sorted by (target, source)
    poly, count, peak = clip(src_cells[s], dst_cells[t])
    area = np.where(count >= 3, fan_area(poly, count), 0.0)
    small = np.minimum(sa[s], da[t])
    keep = area > KEEP_FRACTION * small
    return {"candidates": np.stack([s, t]), "candidate_area": area, "relative": area / small, "peak": peak,
            "src_area": sa, "dst_area": da, "edge_index": np.stack([s[keep], t[keep]]).astype(np.int64),
            "area": area[keep]}


def weights(edge_index: np.ndarray, area: np.ndarray, dst_area: np.ndarray, normalize: str = "covered"):
    """(weights float32 [E], coverage float64 [Nd]): every row summed in stored order in fp64."""
    total = np.zeros(dst_area.shape[0])
    np.add.at(total, edge_index[1], area)                              # unbuffered: one entry after the other
    den = total if normalize == "covered" else dst_area
    return (area / den[edge_index[1]]).astype(np.float32), total / dst_area


# ---- the generators, restated

def latlon_cells(nlat: int, nlon: int, poles: bool = True) -> np.ndarray:
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
    west = np.deg2rad((360.0 / nlon) * (np.arange(nlon, dtype=np.float64) - 0.5))

    def corners(lat_deg):
        la = np.deg2rad(lat_deg)
        cl = np.where(np.abs(la) == 0.5 * np.pi, 0.0, np.cos(la))
        return np.stack([cl[:, None] * np.cos(west)[None, :], cl[:, None] * np.sin(west)[None, :],
                         np.broadcast_to(np.sin(la)[:, None], (nlat, nlon))], axis=2)
    w_lo, w_hi = corners(lo), corners(hi)
    cells = np.stack([w_lo, np.roll(w_lo, -1, axis=1), np.roll(w_hi, -1, axis=1), w_hi], axis=2)
    return np.ascontiguousarray(cells.reshape(nlat * nlon, 4, 3))


def mesh_cells(mesh) -> np.ndarray:
    return np.ascontiguousarray(mesh.pos[mesh.faces])


def mesh_dual_cells(mesh) -> np.ndarray:
    """Node by node: the normalised centres of the incident faces by ascending angle about the node."""
    pos, faces = mesh.pos, mesh.faces
    c = pos[faces].sum(axis=1)
    c = c / np.sqrt(dot(c, c))[:, None]
    out = np.empty((pos.shape[0], 6, 3))
    for i, p in enumerate(pos):
        axis = np.zeros(3)
        axis[np.argmin(np.abs(p))] = 1.0
        e1 = axis - (axis * p).sum() * p
        e1 = e1 / np.linalg.norm(e1)
        e2 = np.cross(p, e1)
        f = np.flatnonzero((faces == i).any(axis=1))
        f = f[np.argsort(np.arctan2(c[f] @ e2, c[f] @ e1), kind="stable")]
        out[i] = c[np.concatenate([f, np.repeat(f[-1:], 6 - f.size)])]
    return out


def rotation() -> np.ndarray:
    """Rz(0.3) Ry(0.5) Rx(0.7)."""
    def rot(axis, a):
        c, s = np.cos(a), np.sin(a)
        m = np.eye(3)
        i, j = [(1, 2), (2, 0), (0, 1)][axis]
        m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
        return m
    return rot(2, 0.3) @ rot(1, 0.5) @ rot(0, 0.7)


# ---- the inputs of the conservative tests, by name.  tests/test_conserve_host.py asserts the gap they rest on: no
# candidate pair of any PAIRS entry has a relative overlap in (1e-14, 1e-7), so the 1e-12 keep rule is never decided by
# rounding and the device must list exactly the restatement's pairs.
GAP_LOW, GAP_HIGH = 1e-14, 1e-7
PAIRS = (("faces3", "ll9x16"), ("ll9x16", "faces3"), ("faces5", "ll17x32"), ("ll17x32", "faces5"),
         ("faces3", "faces3"), ("faces5", "faces5"), ("faces4", "rot4"), ("rot4", "faces4"), ("faces6", "rot6"),
         ("dual3", "ll9x16"), ("ll9x16", "dual3"), ("north5", "ll17x32"))
TESSELLATIONS = ("faces3", "faces4", "faces5", "faces6", "rot4", "rot6", "ll9x16", "ll17x32", "dual3")


@functools.lru_cache(maxsize=None)
def cells(name: str) -> np.ndarray:
    """A named cell set, normalised as the library normalises its input (cached; callers must not write into it)."""
    import gwen_amd
    if name.startswith("faces"):
        c = mesh_cells(gwen_amd.geodesic_mesh(int(name[5:])))
    elif name.startswith("rot"):
        c = cells("faces" + name[3:]) @ rotation().T
    elif name.startswith("dual"):
        c = mesh_dual_cells(gwen_amd.geodesic_mesh(int(name[4:])))
    elif name.startswith("ll"):
        nlat, nlon = name[2:].split("x")
        c = latlon_cells(int(nlat), int(nlon))
    elif name == "north5":                                             # the faces whose centre has z > 0: half a sphere
        c = cells("faces5")
        c = c[geometry(c)[0][:, 2] > 0.0]
    else:
        raise KeyError(name)
    c = unit_cells(c)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def overlaps_cached(src: str, dst: str) -> dict:
    return overlaps(cells(src), cells(dst))
