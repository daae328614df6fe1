"""Conservative regridding, host side (no GPU): the cell generators, every validation error of gwen_amd/regrid.py that
needs no device, the early returns of the C entry points, the numpy restatement of tests/conserve_ref.py against what must
hold by construction, and the GAP the GPU tests rest on: on every input pair they use, no candidate has a relative overlap
in (1e-14, 1e-7), so the 1e-12 keep rule is never decided by rounding."""
import numpy as np
import pytest

import conserve_ref as CR


@pytest.fixture(scope="module")
def ga():
    import gwen_amd
    return gwen_amd


def test_exports(ga):
    from gwen_amd import regrid
    names = {"mesh_cells", "mesh_dual_cells", "latlon_cells", "cell_areas", "cell_overlaps"}
    assert names <= set(ga.__all__) and all(getattr(ga, n) is getattr(regrid, n) for n in names)
    assert callable(ga.Regridder.conservative)


# ---- generators

def test_generators_equal_their_restatements(ga):
    for nu in (1, 2, 3, 5):
        m = ga.geodesic_mesh(nu)
        assert np.array_equal(ga.mesh_cells(m), CR.mesh_cells(m))
        assert np.array_equal(ga.mesh_dual_cells(m), CR.mesh_dual_cells(m))
    for args in ((9, 16), (17, 32), (8, 16, False), (2, 3)):
        assert np.array_equal(ga.latlon_cells(*args), CR.latlon_cells(*args))


def test_mesh_cells_are_the_faces_in_order(ga):
    m = ga.geodesic_mesh(3)
    c = ga.mesh_cells(m)
    assert c.shape == (180, 3, 3) and c.dtype == np.float64 and np.array_equal(c[7, 2], m.pos[m.faces[7, 2]])
    flipped = ga.Mesh(m.pos, m.edge_index, m.faces[:, ::-1].copy(), m.nu)
    with pytest.raises(ValueError, match="positively oriented"):
        ga.mesh_cells(flipped)
    with pytest.raises(ValueError, match="positively oriented"):
        ga.mesh_dual_cells(flipped)


@pytest.mark.parametrize("nu", [1, 2, 3, 5, 10])
def test_dual_cells_are_convex_ordered_and_tile_the_sphere(ga, nu):
    m = ga.geodesic_mesh(nu)
    c = ga.mesh_dual_cells(m)
    assert c.shape == (m.num_nodes, 6, 3)
    from gwen_amd.regrid import check_cells
    u = check_cells(c)                                                   # convex, counter-clockwise, >= 3 corners
    penta = (c[:, 5] == c[:, 4]).all(axis=1)
    assert penta.sum() == 12 and (c[:, :4] != c[:, 1:5]).any(axis=2).all() and (c[:, 0] != c[:, 5]).any(axis=1).all()
    centre, _, area = CR.geometry(u)
    assert np.abs((centre * m.pos).sum(axis=1) - 1.0).max() < 1e-3 * 25 / nu ** 2       # the cell sits on its node
    assert abs(area.sum() - 4 * np.pi) <= 6e-14 and (area > 0).all()


def test_latlon_cells_shape_order_corners_and_orientation(ga):
    nlat, nlon = 9, 16
    c = ga.latlon_cells(nlat, nlon)
    pos = ga.latlon_grid(nlat, nlon)[0]
    assert c.shape == (nlat * nlon, 4, 3) and c.dtype == np.float64
    lat = np.rad2deg(np.arcsin(c[..., 2])).reshape(nlat, nlon, 4)
    lon = np.rad2deg(np.arctan2(c[..., 1], c[..., 0])).reshape(nlat, nlon, 4)
    step = 180.0 / (nlat - 1)
    rows = -90.0 + step * np.arange(nlat)
    lo, hi = np.clip(rows - step / 2, -90, 90), np.clip(rows + step / 2, -90, 90)
    assert np.abs(lat[:, :, 0] - lo[:, None]).max() < 1e-12 and np.abs(lat[:, :, 1] - lo[:, None]).max() < 1e-12
    assert np.abs(lat[:, :, 2] - hi[:, None]).max() < 1e-12 and np.abs(lat[:, :, 3] - hi[:, None]).max() < 1e-12
    centre_lon = 22.5 * np.arange(nlon)
    for corner, off in ((0, -11.25), (1, 11.25), (2, 11.25), (3, -11.25)):
        want = (centre_lon + off + 180.0) % 360.0 - 180.0
        got = lon[1:-1, :, corner]                                       # away from the poles, where lon means something
        assert np.abs((got - want[None, :] + 180.0) % 360.0 - 180.0).max() < 1e-12
    # the wedges: the two polar corners coincide exactly, at the pole
    assert (c[:nlon, 0] == c[:nlon, 1]).all() and (c[:nlon, 0] == [0, 0, -1]).all()
    assert (c[-nlon:, 2] == c[-nlon:, 3]).all() and (c[-nlon:, 2] == [0, 0, 1]).all()
    # neighbours share their corners bit for bit: east of cell j = west of cell j + 1, top of row i = bottom of row i + 1
    g = c.reshape(nlat, nlon, 4, 3)
    assert np.array_equal(g[:, :, 1], np.roll(g[:, :, 0], -1, axis=1)) and np.array_equal(g[:-1, :, 3], g[1:, :, 0])
    # every grid point lies in its own cell, and the cell is counter-clockwise
    u = CR.unit_cells(c)
    nrm = CR.cross(u, np.roll(u, -1, axis=1))
    assert ((nrm * pos[:, None, :]).sum(axis=2) >= -1e-15).all()
    from gwen_amd.regrid import check_cells
    check_cells(c)
    mid = ga.latlon_cells(8, 16, poles=False)
    assert mid.shape == (128, 4, 3) and abs(CR.geometry(CR.unit_cells(mid))[2].sum() - 4 * np.pi) < 1e-13
    for bad in ((1, 16), (9, 2), (0, 16, False)):
        with pytest.raises(ValueError, match="latlon_cells"):
            ga.latlon_cells(*bad)


# ---- validation that needs no device

def test_python_layer_validates_without_a_gpu(ga):
    ok = CR.cells("faces3")
    tri = ok[:4].copy()

    def with_cell(cell):
        c = np.concatenate([tri, np.asarray(cell, dtype=np.float64)[None]])
        return c
    clockwise = tri[0][::-1]
    nan = tri[0].copy(); nan[1, 2] = np.nan
    zero = tri[0].copy(); zero[2] = 0.0
    two = np.stack([tri[0][0], tri[0][1], tri[0][1]])
    hemi = np.array([[1.0, 0, 0.01], [-0.5, 0.8660254037844386, 0.01], [-0.5, -0.8660254037844386, 0.01]])     # convex, but nearly half the sphere
    quad = CR.cells("ll9x16")[40]
    dent = quad.copy()
    dent[2] = CR.unit_cells((0.8 * quad[0] + 0.1 * quad[1] + 0.1 * quad[3])[None])[0]       # pulled inside: not convex
    bowtie = quad[[0, 2, 1, 3]]
    cases = [(with_cell(clockwise), "1 of 5 cells are not convex"), (with_cell(nan), "non-finite"),
             (with_cell(zero), "zero"), (with_cell(two), "1 of 5 cells have fewer than 3 distinct"),
             (with_cell(hemi), "1 of 5 cells do not fit a cap"), (ok[:, ::-1], "180 of 180 cells are not convex"),
             (np.zeros((4, 9, 3)), "3 <= V <= 8"), (np.zeros((4, 2, 3)), "3 <= V <= 8"), (np.zeros((4, 3)), "shape"),
             (np.zeros((4, 3, 2)), "shape"), (np.stack([quad, dent]), "1 of 2 cells are not convex"),
             (np.stack([quad, bowtie]), "1 of 2 cells are not convex")]
    for bad, message in cases:
        with pytest.raises(ValueError, match=message):
            ga.cell_areas(bad, "cuda:0")
        for args in ((bad, ok), (ok, bad)):
            with pytest.raises(ValueError, match=message):
                ga.cell_overlaps(*args, "cuda:0")
            with pytest.raises(ValueError, match=message):
                ga.Regridder.conservative(*args, "cuda:0")
    from gwen_amd.regrid import check_cells

    with pytest.raises(ValueError, match="int32"):                       # counts beyond int32 (a view: no memory)
        check_cells(np.broadcast_to(ok[:1], (2 ** 31 - 1, 3, 3)))
    with pytest.raises(ValueError, match="normalize"):
        ga.Regridder.conservative(ok, ok, "cuda:0", normalize="area")
    with pytest.raises(ValueError, match="uncovered"):
        ga.Regridder.conservative(ok, ok, "cuda:0", uncovered="zero")
    for c in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="min_coverage"):
            ga.Regridder.conservative(ok, ok, "cuda:0", min_coverage=c)
    for call in (lambda: ga.cell_areas(ok, "cpu"), lambda: ga.cell_overlaps(ok, ok, "cpu"),
                 lambda: ga.Regridder.conservative(ok, ok, "cpu")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    # what is accepted comes back normalised, contiguous, float64; scaled input is the same cell
    got = check_cells(3.0 * ok.astype(np.float64))
    assert got.dtype == np.float64 and got.flags.c_contiguous and np.abs(got - ok).max() <= 2.3e-16


def test_launchers_validate_before_any_hip_call(hip_lib):
    def areas(n=4, v=3, ptr=8):
        return hip_lib.gwen_cell_areas(ptr, n, v, ptr, ptr, ptr, None)
    assert areas(v=2) == -1 and areas(v=9) == -1 and areas(n=-1) == -1 and areas(ptr=None) == -1
    assert areas(n=2 ** 31 - 1) == -2 and areas(n=0, ptr=None) == 0

    def overlap(ns=4, vs=3, nd=4, vt=4, e=5, ptr=8):
        return hip_lib.gwen_cell_overlap_areas(ptr, ns, vs, ptr, nd, vt, ptr, e, ptr, ptr, ptr, ptr, ptr, None)
    assert overlap(vs=2) == -1 and overlap(vt=9) == -1 and overlap(ns=-1) == -1 and overlap(nd=-1) == -1
    assert overlap(e=-1) == -1 and overlap(ptr=None) == -1
    assert overlap(ns=2 ** 31) == -2 and overlap(nd=2 ** 31 - 1) == -2 and overlap(e=2 ** 31 - 1) == -2
    assert overlap(e=0, ptr=None) == 0

    def weights(nd=4, e=5, mode=0, ptr=8):
        return hip_lib.gwen_cell_overlap_weights(ptr, ptr, ptr, nd, e, mode, ptr, ptr, None)
    assert weights(mode=2) == -1 and weights(mode=-1) == -1 and weights(nd=-1) == -1 and weights(e=-1) == -1
    assert weights(ptr=None) == -1 and weights(nd=2 ** 31) == -2 and weights(e=2 ** 31) == -2
    assert weights(nd=0, ptr=None) == 0


# ---- the restatement

@pytest.mark.parametrize("name", CR.TESSELLATIONS)
def test_restated_areas_tile_the_sphere(name):
    c = CR.cells(name)
    centre, radius, area = CR.geometry(c)
    assert (area > 0).all() and abs(area.sum() - 4 * np.pi) <= 6e-14
    assert np.abs(CR.dot(centre, centre) - 1.0).max() <= 4.5e-16 and (radius > 0).all() and radius.max() < 0.5
    if name.startswith("faces"):
        import gwen_amd
        assert np.abs(area - gwen_amd.geodesic_mesh(int(name[5:])).face_areas()).max() <= 1e-14


def test_restated_clip_on_cells_worked_by_hand():
    octant = np.array([[[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]])
    assert abs(CR.geometry(octant)[2][0] - np.pi / 2) < 1e-15
    poly, count, peak = CR.clip(octant, octant)
    assert count[0] == 3 and peak == 3 and abs(CR.fan_area(poly, count)[0] - np.pi / 2) < 1e-15
    # the octant x >= 0, y >= 0, z >= 0 against the lune 0 <= lon <= 45 degrees of the northern hemisphere: pi / 4
    r = np.sqrt(0.5)
    lune = np.array([[[1.0, 0, 0], [r, r, 0], [0, 0, 1.0], [0, 0, 1.0]]])              # a wedge: the corner repeated
    for s, t in ((octant, lune), (lune, octant)):
        poly, count, _ = CR.clip(s, t)
        assert abs(CR.fan_area(poly, count)[0] - np.pi / 4) < 1e-15
    away = np.array([[[-1.0, 0, 0], [0, 0, -1.0], [0, -1.0, 0]]])                      # the opposite octant
    poly, count, _ = CR.clip(octant, away)
    assert count[0] < 3 or abs(CR.fan_area(poly, count)[0]) < 1e-15


@pytest.mark.parametrize("src,dst", CR.PAIRS)
def test_the_gap_and_the_partition_on_every_test_input(src, dst):
    """No candidate is anywhere near the keep rule; the kept areas partition both sides; at most 16 vertices."""
    o = CR.overlaps_cached(src, dst)
    rel = o["relative"]
    assert not ((rel > CR.GAP_LOW) & (rel < CR.GAP_HIGH)).any() and o["peak"] <= CR.MAX_POLY
    ei, area = o["edge_index"], o["area"]
    assert np.array_equal(np.lexsort((ei[0], ei[1])), np.arange(ei.shape[1]))            # sorted by (target, source)
    assert (rel[rel <= CR.GAP_LOW] <= 3.4e-15).all() and rel[rel >= CR.GAP_HIGH].min() >= 3.6e-6
    cols = np.bincount(ei[0], weights=area, minlength=o["src_area"].size)
    rows = np.bincount(ei[1], weights=area, minlength=o["dst_area"].size)
    assert np.abs(cols / o["src_area"] - 1.0).max() <= 7.4e-15                          # the target tiles the sphere
    if src != "north5":
        assert np.abs(rows / o["dst_area"] - 1.0).max() <= 7.4e-15
    else:
        cover = rows / o["dst_area"]
        assert (cover == 0).sum() > 100 and ((cover > 1e-3) & (cover < 0.999)).sum() > 10 and (cover > 1 - 1e-14).sum() > 100
    if src == dst:                                                       # a tessellation onto itself: the diagonal
        n = o["src_area"].size
        assert np.array_equal(ei, np.stack([np.arange(n), np.arange(n)])) and np.abs(rel[rel > 0.5] - 1.0).max() <= 4e-15
        w, cover = CR.weights(ei, area, o["dst_area"])
        assert (w == 1.0).all() and np.abs(cover - 1.0).max() <= 4e-15
    if (src, dst) == ("ll17x32", "faces5"):
        assert np.bincount(ei[1]).max() == 34                            # a triangle at the pole: every wedge of the row


def test_restated_weights():
    o = CR.overlaps_cached("north5", "ll17x32")
    ei, area, da = o["edge_index"], o["area"], o["dst_area"]
    covered, cover = CR.weights(ei, area, da, "covered")
    cell, cover2 = CR.weights(ei, area, da, "cell")
    assert covered.dtype == np.float32 and np.array_equal(cover, cover2)
    rows = np.bincount(ei[1], weights=covered.astype(np.float64), minlength=da.size)
    has = np.bincount(ei[1], minlength=da.size) > 0
    assert np.abs(rows[has] - 1.0).max() <= 10 * 2.0 ** -24 and (rows[~has] == 0).all()
    rows = np.bincount(ei[1], weights=cell.astype(np.float64), minlength=da.size)
    assert np.abs(rows - cover).max() <= 10 * 2.0 ** -24
