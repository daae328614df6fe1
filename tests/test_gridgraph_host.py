"""Grid graphs, host side (no GPU): the point-set helpers, ``Mesh.max_edge_length``, argument validation, and the numpy
restatements of tests/gridgraph_ref.py against closed forms -- the mesh's own face centres must reproduce the
forecaster's default grid <-> mesh edges."""
import numpy as np
import pytest

import gridgraph_ref as R


@pytest.fixture(scope="module")
def ga():
    import gwen_amd
    return gwen_amd


def test_sphere_points_are_unit_vectors_in_lat_lon_convention(ga):
    p = ga.sphere_points([0.0, 0.0, 90.0, -90.0, 45.0], [0.0, 90.0, 17.0, 250.0, 180.0])
    assert p.shape == (5, 3) and p.dtype == np.float64
    assert np.abs(np.linalg.norm(p, axis=1) - 1.0).max() <= 4e-16
    assert np.allclose(p[0], [1, 0, 0], atol=1e-16) and np.allclose(p[1], [0, 1, 0], atol=1e-16)
    assert np.array_equal(p[2], [0.0, 0.0, 1.0]) and np.array_equal(p[3], [0.0, 0.0, -1.0])       # poles: exact
    assert np.allclose(p[4], [-np.sqrt(0.5), 0.0, np.sqrt(0.5)], atol=1e-15)
    assert ga.sphere_points(np.zeros((3, 1)), np.zeros((1, 4))).shape == (12, 3)                   # broadcast, flattened


@pytest.mark.parametrize("nlat,nlon,poles", [(19, 36, True), (18, 36, False), (2, 1, True), (7, 5, False)])
def test_latlon_grid_order_and_weights(ga, nlat, nlon, poles):
    pos, w = ga.latlon_grid(nlat, nlon, poles)
    assert pos.shape == (nlat * nlon, 3) and w.shape == (nlat * nlon,)
    assert np.abs(np.linalg.norm(pos, axis=1) - 1.0).max() <= 4e-16
    z = pos[:, 2].reshape(nlat, nlon)
    assert np.all(z == z[:, :1]) and np.all(np.diff(z[:, 0]) > 0)               # row-major (lat, lon), south to north
    if poles:
        assert np.all(pos[:nlon] == [0.0, 0.0, -1.0]) and np.all(pos[-nlon:] == [0.0, 0.0, 1.0])   # coincident pole rows
    else:
        assert abs(z[0, 0]) < 1.0
    lon = np.arctan2(pos[:, 1], pos[:, 0]).reshape(nlat, nlon)[nlat // 2 if not poles or nlat > 2 else 0]
    if nlon > 1 and nlat > 2:
        assert np.all(np.diff(np.mod(lon, 2 * np.pi)) > 0)                      # longitudes ascending from 0
    assert abs(w.sum() - 1.0) <= 1e-15 and np.all(w > 0)
    w2 = w.reshape(nlat, nlon)
    assert np.array_equal(w2, w2[::-1]) and np.all(w2 == w2[:, :1])             # symmetric about the equator
    # a band's weight is its share of the sphere: sin(upper edge) - sin(lower edge), over 2
    step = 180.0 / (nlat - 1 if poles else nlat)
    lat = np.rad2deg(np.arcsin(z[:, 0]))
    band = np.sin(np.deg2rad(np.clip(lat + step / 2, -90, 90))) - np.sin(np.deg2rad(np.clip(lat - step / 2, -90, 90)))
    assert np.allclose(w2.sum(axis=1), band / 2.0, atol=1e-12)


def test_latlon_grid_rejects_bad_sizes(ga):
    for args in ((1, 4, True), (0, 4, False), (4, 0, True)):
        with pytest.raises(ValueError):
            ga.latlon_grid(*args)


@pytest.mark.parametrize("nu", [1, 2, 5])
def test_max_edge_length_against_numpy(ga, nu):
    m = ga.geodesic_mesh(nu)
    want = max(np.linalg.norm(m.pos[j] - m.pos[i]) for i, j in m.edge_index.T)
    assert abs(m.max_edge_length() - want) <= 1e-15
    assert m.max_edge_length() == R.max_edge_length(m)
    empty = ga.Mesh(pos=m.pos, edge_index=np.zeros((2, 0), dtype=np.int64), faces=m.faces, nu=nu)
    assert empty.max_edge_length() == 0.0


def test_argument_validation_raises_without_a_gpu(ga):
    from gwen_amd.forecaster import InteractionForecaster
    m = ga.geodesic_mesh(2)
    ok = m.pos[:4]
    for bad in (np.array([[0.0, 0.0, 0.0]]), np.array([[np.nan, 0.0, 1.0]]), np.array([[np.inf, 0.0, 1.0]]),
                np.zeros((3, 2)), np.zeros(3)):
        with pytest.raises(ValueError):
            ga.radius_edges(bad, ok, 0.5, "cuda:0")
        with pytest.raises(ValueError):
            ga.radius_edges(ok, bad, 0.5, "cuda:0")
        with pytest.raises(ValueError):
            ga.containing_faces(bad, m, "cuda:0")
        with pytest.raises(ValueError):
            ga.grid_graphs(m, bad, "cuda:0")
        with pytest.raises(ValueError):
            InteractionForecaster.prepare(m, "cuda:0", grid_pos=bad)
    for r in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ga.radius_edges(ok, ok, r, "cuda:0")
    with pytest.raises(ValueError):
        InteractionForecaster.prepare(m, "cuda:0", radius=0.3)                   # a radius without grid points
    flipped = ga.Mesh(pos=m.pos, edge_index=m.edge_index, faces=m.faces[:, ::-1].copy(), nu=2)
    with pytest.raises(ValueError, match="oriented"):
        ga.containing_faces(ok, flipped, "cuda:0")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ga.radius_edges(ok, ok, 0.5, "cpu")


def test_launchers_validate_before_any_hip_call(hip_lib):
    import ctypes as C
    n = C.c_size_t(0)
    assert hip_lib.gwen_gridgraph_cells(2.5) == 1 and hip_lib.gwen_gridgraph_cells(0.5) == 4
    assert hip_lib.gwen_gridgraph_cells(0.7) == 2 and hip_lib.gwen_gridgraph_cells(1e-3) == 128        # the cap
    assert hip_lib.gwen_gridgraph_cells(0.0) == -1 and hip_lib.gwen_gridgraph_cells(float("nan")) == -1
    assert hip_lib.gwen_radius_edges_workspace_bytes(-1, 4, C.byref(n)) == -1
    assert hip_lib.gwen_radius_edges_workspace_bytes(2 ** 31, 4, C.byref(n)) == -2
    assert hip_lib.gwen_radius_edges_count(None, 4, None, 4, 0.5, None, None, 0, None) == -1
    assert hip_lib.gwen_radius_edges_count(8, 4, 8, 4, -0.5, 8, None, 0, None) == -1
    assert hip_lib.gwen_radius_edges_fill_workspace_bytes(2 ** 31 - 1, C.byref(n)) == -2
    assert hip_lib.gwen_radius_edges_fill(8, 4, 8, 4, 0.5, 2 ** 31 - 1, 8, 8, 8, 0, 8, 0, None) == -2  # total out of range
    assert hip_lib.gwen_radius_edges_fill(8, 4, 8, 4, 0.5, 5, None, 8, 8, 0, 8, 0, None) == -1
    assert hip_lib.gwen_containing_faces(None, 0, None, 0, None, None, 0, 0.5, None, None, None, 0, None) == 0
    assert hip_lib.gwen_containing_faces(None, 3, None, 0, None, None, 0, 0.5, None, None, None, 0, None) == -1


@pytest.mark.parametrize("nu", [2, 3, 4, 5])
def test_restatements_on_the_meshs_own_face_centres(ga, nu):
    """Closed form: at the default radius a face centre reaches exactly its three corners (E = 3 F), and face f contains
    centre f with weights 1/3."""
    from gwen_amd.g2m import grid_mesh_edges
    m = ga.geodesic_mesh(nu)
    c = R.face_centres(m)
    nf = m.faces.shape[0]
    assert (R.det3(m.pos[m.faces[:, 0]], m.pos[m.faces[:, 1]], m.pos[m.faces[:, 2]]) > 0).all()    # positively oriented
    ei = R.radius_edges(c, m.pos, 0.6 * m.max_edge_length())
    g2m, _ = grid_mesh_edges(m)
    assert ei.shape == (2, 3 * nf)
    assert {tuple(e) for e in ei.T} == {tuple(e) for e in g2m.T}
    assert np.array_equal(ei, ei[:, np.lexsort((ei[0], ei[1]))])                 # (target, source) order
    face, w = R.containing_faces(c, m)
    assert np.array_equal(face, np.arange(nf))
    assert np.abs(w - 1.0 / 3.0).max() <= 1e-14 and np.abs(w.sum(axis=1) - 1.0).max() <= 1e-15
    back = (w[:, :, None] * m.pos[m.faces]).sum(axis=1)
    assert np.abs(R.unit(back) - c).max() <= 1e-15
    # the furthest point of a face from its centre is a corner: it must be inside the default g2m radius (0.6 x the
    # longest edge), and then the candidate radius of the containing-face search (1.0 x) is safe with a wide margin
    far = np.linalg.norm(m.pos[m.faces] - c[:, None, :], axis=2).max()
    assert far < 0.6 * m.max_edge_length()


def test_restatement_ties_and_misses(ga):
    m = ga.geodesic_mesh(2)
    acc, _ = R.accepted_faces(m.pos, m)                                          # a vertex lies in 5 or 6 faces
    assert set(acc.sum(axis=1)) == {5, 6}
    face, w = R.containing_faces(m.pos, m)
    for v in range(m.num_nodes):
        assert face[v] == min(f for f in range(m.faces.shape[0]) if v in m.faces[f])
        assert np.abs(w[v] - (m.faces[face[v]] == v)).max() <= 1e-15            # all weight on the vertex itself
    assert R.radius_edges(m.pos[:0], m.pos, 0.5).shape == (2, 0) and R.radius_edges(m.pos, m.pos[:0], 0.5).shape == (2, 0)
