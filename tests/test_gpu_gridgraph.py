"""Grid graphs on the device (csrc/gridgraph.hip, gwen_amd/gridgraph.py; BUILD-DEFINED, parity unpinned) against the numpy
restatements of tests/gridgraph_ref.py: the radius edges EXACTLY (same [2, E] tensor, no tolerance), the containing
face by id and its weights to 1e-12, and the forecaster on a lat-lon grid against the fp64 oracle."""
import functools

import numpy as np
import pytest
import torch

import gridgraph_ref as R
from helpers import REL_TOL, SEED, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NUS = [2, 3, 5]
SETS = ["latlon", "random", "centres"]


@pytest.fixture(scope="module")
def ga(hip_lib):
    import gwen_amd
    return gwen_amd


@functools.lru_cache(maxsize=None)
def mesh(nu):
    import gwen_amd
    return gwen_amd.geodesic_mesh(nu)


@functools.lru_cache(maxsize=None)
def points(name, nu):
    import gwen_amd
    if name == "latlon":
        return gwen_amd.latlon_grid(19, 36)[0]                                  # 684 points, 36 coincident at each pole
    if name == "random":
        return np.random.default_rng(SEED).normal(size=(2000, 3))               # normalised by the library
    return R.face_centres(mesh(nu))


def cap_radius(hip_lib):
    """A radius whose 2 / R exceeds the cell cap: cells are larger than R there."""
    r = 0.01
    assert 2.0 / r > hip_lib.gwen_gridgraph_cells(r) == hip_lib.gwen_gridgraph_cells(1e-6)
    return r


@functools.lru_cache(maxsize=None)
def want_edges(name, nu, radius):
    return R.radius_edges(points(name, nu), mesh(nu).pos, radius)


def default_radius(nu):
    return 0.6 * mesh(nu).max_edge_length()


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("nu", NUS)
def test_radius_edges_equal_the_restatement_exactly(ga, hip_lib, nu, name):
    """Default radius (several cells an axis), 2.5 (everything links, one cell), 1e-3 (nothing links, except that the
    nu = 2 mesh has nodes at both poles and on the equator that coincide with 76 lat-lon points) and a radius past the
    cell cap: the same tensor, in (target, source) order.  No pair of these sets is within 1e-9 of the default radius, so
    equality of the decision is not a matter of luck."""
    m, p = mesh(nu), points(name, nu)
    assert R.near_radius(p, m.pos, default_radius(nu)) > 1e-9
    for radius in (default_radius(nu), 2.5, 1e-3, cap_radius(hip_lib)):
        got = ga.radius_edges(p, m.pos, radius, DEV)
        want = want_edges(name, nu, radius)
        assert got.dtype == torch.int64 and got.device.type == "cuda" and tuple(got.shape) == want.shape
        assert np.array_equal(got.cpu().numpy(), want), (name, nu, radius)
        if radius == 2.5:
            assert got.size(1) == p.shape[0] * m.num_nodes
        if radius == 1e-3:
            assert got.size(1) == (76 if (name, nu) == ("latlon", 2) else 0)
    assert want_edges(name, nu, default_radius(nu)).shape[1] > 0


def test_radius_edges_past_the_cell_cap_with_edges(ga, hip_lib):
    """Cells larger than the radius and pairs to find: the random points against themselves at R = 0.01 (every point
    finds itself, and some a neighbour)."""
    p = points("random", 2)
    r = cap_radius(hip_lib)
    want = R.radius_edges(p, p, r)
    assert want.shape[1] > p.shape[0]
    assert np.array_equal(ga.radius_edges(p, p, r, DEV).cpu().numpy(), want)


def test_radius_edges_without_sources_or_targets(ga):
    m = mesh(3)
    for src, dst in ((m.pos[:0], m.pos), (m.pos, m.pos[:0]), (m.pos[:0], m.pos[:0])):
        for radius in (default_radius(3), 2.5):
            got = ga.radius_edges(src, dst, radius, DEV)
            assert got.dtype == torch.int64 and tuple(got.shape) == (2, 0)


@pytest.mark.parametrize("nu", NUS)
def test_axis_points_and_coincident_points(ga, hip_lib, nu):
    """Coordinates of exactly +-1 map to a valid cell; 50 copies of one point are 50 sources of the same targets."""
    m = mesh(nu)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
    copies = np.repeat(m.pos[7:8] * 3.0, 50, axis=0)                            # (not unit length: normalised first)
    p = np.concatenate([axes, copies, axes])
    for radius in (default_radius(nu), 0.5, 2.0, 2.5, cap_radius(hip_lib)):
        for src, dst in ((p, m.pos), (m.pos, p), (p, p)):
            want = R.radius_edges(src, dst, radius)
            got = ga.radius_edges(src, dst, radius, DEV).cpu().numpy()
            assert np.array_equal(got, want), (nu, radius)
    want = R.radius_edges(p, m.pos, default_radius(nu))
    assert np.sum((want[0] >= 6) & (want[0] < 56)) % 50 == 0 and np.sum(want[1] == 7) >= 50


@pytest.mark.parametrize("nu", NUS)
def test_containing_faces_of_interior_points(ga, nu):
    m, p = mesh(nu), points("random", nu)
    acc, _ = R.accepted_faces(p, m)
    assert (acc.sum(axis=1) == 1).all()                                         # strictly inside one face each
    want_f, want_w = R.containing_faces(p, m)
    face, w = ga.containing_faces(p, m, DEV)
    assert face.dtype == torch.int64 and w.dtype == torch.float64 and tuple(w.shape) == (p.shape[0], 3)
    assert np.array_equal(face.cpu().numpy(), want_f)
    assert np.abs(w.cpu().numpy() - want_w).max() <= 1e-12


@pytest.mark.parametrize("name", ["latlon", "vertices", "centres"])
@pytest.mark.parametrize("nu", NUS)
def test_containing_faces_on_edges_vertices_and_poles(ga, nu, name):
    """Points on edges and vertices lie in up to 6 faces: the lowest accepted id wins, and the weights rebuild the
    point."""
    m = mesh(nu)
    p = m.pos if name == "vertices" else points(name, nu)
    acc, _ = R.accepted_faces(p, m)
    assert acc.any(axis=1).all()
    if name == "vertices":
        assert acc.sum(axis=1).min() >= 5
    face, w = ga.containing_faces(p, m, DEV)
    face, w = face.cpu().numpy(), w.cpu().numpy()
    assert np.array_equal(face, acc.argmax(axis=1))                             # the lowest id the restatement accepts
    back = R.unit((w[:, :, None] * m.pos[m.faces[face]]).sum(axis=1))
    assert np.abs(back - R.unit(p)).max(axis=1).max() <= 1e-12 and np.linalg.norm(back - R.unit(p), axis=1).max() <= 1e-12
    assert w.min() >= -1e-12 and np.abs(w.sum(axis=1) - 1.0).max() <= 1e-12
    if name == "centres":
        assert np.array_equal(face, np.arange(m.faces.shape[0])) and np.abs(w - 1.0 / 3.0).max() <= 1e-12


def test_two_runs_are_bitwise_equal_on_the_current_stream(ga):
    m, p = mesh(5), points("latlon", 5)
    side = torch.cuda.Stream(DEV)
    runs = []
    for stream in (None, side, None):
        with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream(DEV)):
            e = ga.radius_edges(p, m.pos, default_radius(5), DEV)
            f, w = ga.containing_faces(p, m, DEV)
            g2m, m2g, info = ga.grid_graphs(m, p, DEV)
        torch.cuda.synchronize()
        runs.append((e, f, w, g2m, m2g))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b) and a.dtype == b.dtype
    assert torch.equal(runs[0][0], runs[0][3])                                  # grid_graphs' g2m is radius_edges


@pytest.mark.parametrize("nu", NUS)
def test_grid_graphs_on_the_face_centres_are_the_default_graphs(ga, nu):
    from gwen_amd.g2m import grid_mesh_edges
    m = mesh(nu)
    g2m, m2g, info = ga.grid_graphs(m, points("centres", nu), DEV)
    a, b = grid_mesh_edges(m)
    as_set = lambda e: {tuple(x) for x in np.asarray(e).T}                      # noqa: E731
    assert as_set(g2m.cpu().numpy()) == as_set(a) and g2m.size(1) == a.shape[1]
    assert as_set(m2g.cpu().numpy()) == as_set(b) and m2g.size(1) == b.shape[1]
    nf = m.faces.shape[0]
    assert info["g2m_edges"] == info["m2g_edges"] == 3 * nf and info["grid_nodes"] == nf and info["mesh_nodes"] == m.num_nodes
    assert info["g2m_grid_degree_min"] == info["g2m_grid_degree_max"] == 3
    assert (info["g2m_mesh_degree_min"], info["g2m_mesh_degree_max"]) == (5, 6)
    assert (info["m2g_mesh_degree_min"], info["m2g_mesh_degree_max"]) == (5, 6)
    assert info["mesh_nodes_without_in_edge"] == 0 and info["radius"] == default_radius(nu)


def test_grid_graphs_info_on_the_latlon_grid(ga):
    """A coarse mesh under the lat-lon grid: the pole rows give long mesh rows (the K6 case of the forecaster test), and
    the degrees are those of the restatement."""
    m, p = mesh(2), points("latlon", 2)
    g2m, m2g, info = ga.grid_graphs(m, p, DEV)
    want = want_edges("latlon", 2, default_radius(2))
    in_deg = np.bincount(want[1], minlength=m.num_nodes)
    out_deg = np.bincount(want[0], minlength=p.shape[0])
    assert (info["g2m_mesh_degree_min"], info["g2m_mesh_degree_max"]) == (in_deg.min(), in_deg.max())
    assert (info["g2m_grid_degree_min"], info["g2m_grid_degree_max"]) == (out_deg.min(), out_deg.max())
    assert info["mesh_nodes_without_in_edge"] == int((in_deg == 0).sum()) and in_deg.max() > 64
    face, _ = R.containing_faces(p, m)
    want_m2g = np.stack([m.faces[face].reshape(-1), np.repeat(np.arange(p.shape[0]), 3)])
    assert np.array_equal(m2g.cpu().numpy(), want_m2g)


def test_grid_graphs_raise_when_a_grid_point_reaches_no_mesh_node(ga):
    m = mesh(2)
    with pytest.raises(ValueError, match=r"grid points have no mesh node within radius 0\.05"):
        ga.grid_graphs(m, points("latlon", 2), DEV, radius=0.05)
    from gwen_amd.forecaster import InteractionForecaster
    with pytest.raises(ValueError, match="no mesh node"):
        InteractionForecaster.prepare(m, DEV, grid_pos=points("latlon", 2), radius=0.05)


def _model(C, H, steps, seed=SEED):
    from gwen_amd.forecaster import InteractionForecaster
    torch.manual_seed(seed)
    model = InteractionForecaster(C, H, steps)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
    return model


def test_forecaster_on_the_face_centres_agrees_with_the_default_grid(ga):
    """The same edges in another order inside a row: one step agrees within REL_TOL, not bitwise."""
    from gwen_amd.forecaster import InteractionForecaster
    m = mesh(5)
    model = _model(8, 64, 1).to(DEV)
    x0 = torch.randn(m.faces.shape[0], 8, generator=torch.Generator().manual_seed(SEED)).to(DEV)
    default = InteractionForecaster.prepare(m, DEV)
    given = InteractionForecaster.prepare(m, DEV, grid_pos=points("centres", 5))
    assert given.grid_nodes == default.grid_nodes == m.faces.shape[0] and given.mesh_nodes == m.num_nodes
    assert given.g2m.num_edges == default.g2m.num_edges and given.m2g.num_edges == default.m2g.num_edges
    with torch.no_grad():
        a, b = model(x0, default), model(x0, given)
    assert rel_err(b, a) <= REL_TOL


@pytest.mark.parametrize("C,H,steps,nsteps", [(8, 32, 1, 2), (16, 64, 2, 2)])
def test_forecaster_on_the_latlon_grid_vs_oracle(ga, C, H, steps, nsteps):
    """grid -> mesh -> grid on a 19 x 36 lat-lon grid over the nu = 3 mesh: mesh rows of 62+ in-edges at the poles.  The
    oracle is fed the same edge lists and edge features."""
    from gwen_amd.forecaster import InteractionForecaster, edge_features
    from oracle import interaction_oracle as IO
    m, grid = mesh(3), points("latlon", 3)
    model = _model(C, H, steps)
    graphs = InteractionForecaster.prepare(m, DEV, grid_pos=grid)
    assert graphs.grid_nodes == 684 and graphs.g2m.max_degree >= 62
    g2m, m2g, _ = ga.grid_graphs(m, grid, DEV)
    a, b = g2m.cpu().numpy(), m2g.cpu().numpy()
    assert np.array_equal(a, want_edges("latlon", 3, default_radius(3)))
    upos = ga.gridgraph.unit_vectors(grid)
    f = [torch.from_numpy(x).double() for x in (edge_features(upos, m.pos, a), edge_features(m.pos, m.pos, m.edge_index),
                                                 edge_features(m.pos, upos, b))]
    sd = {k: v.double() for k, v in model.state_dict().items()}
    x0 = torch.randn(684, C, generator=torch.Generator().manual_seed(SEED))
    want, cur = [], x0.double()
    for _ in range(nsteps):
        cur = IO.forecaster_step(sd, cur, torch.from_numpy(m.pos.astype(np.float32)).double(), torch.from_numpy(a),
                                 torch.from_numpy(m.edge_index), torch.from_numpy(b), *f, steps)
        want.append(cur)
    model = model.to(DEV)
    got = model.rollout(x0.to(DEV), graphs, nsteps)
    with torch.no_grad():
        one = model(x0.to(DEV), graphs)
    assert torch.equal(one, got[0])
    for g_, w_ in zip(got, want):
        err = rel_err(g_, w_)
        print(f"latlon forecaster C={C} H={H}: rel err {err:.3e} (bound {REL_TOL:.0e})")
        assert err <= REL_TOL
    replayed = model.rollout(x0.to(DEV), graphs, nsteps, graphed=True)
    assert all(torch.equal(p, q) for p, q in zip(replayed, got))


def test_members_axis_on_the_latlon_grid(ga):
    from gwen_amd.forecaster import InteractionForecaster
    m = mesh(3)
    model = _model(8, 32, 2).to(DEV).eval()
    graphs = InteractionForecaster.prepare(m, DEV, grid_pos=points("latlon", 3))
    xm = torch.randn(3, 684, 8, generator=torch.Generator().manual_seed(SEED)).to(DEV)
    with torch.no_grad():
        together = model(xm, graphs)
        assert tuple(together.shape) == (3, 684, 8)
        assert torch.equal(together, torch.stack([model(xm[i], graphs) for i in range(3)]))
    assert graphs.batched(3).grid_nodes == 684 and graphs.batched(3).mesh_nodes == m.num_nodes


def test_grid_mesh_grid_model_takes_a_grid(ga):
    """GridMeshGridModel.prepare(grid_pos=...): on the face centres the mean-aggregating layers see the default graphs'
    edge sets, so one forward agrees within REL_TOL."""
    from gwen_amd.g2m import GridMeshGridModel
    m = mesh(3)
    torch.manual_seed(SEED)
    model = GridMeshGridModel(8, 32, 1).to(DEV)
    x = torch.randn(m.faces.shape[0], 8, generator=torch.Generator().manual_seed(SEED)).to(DEV)
    with torch.no_grad():
        a = model(x, model.prepare(m, DEV))
        b = model(x, model.prepare(m, DEV, grid_pos=points("centres", 3)))
        c = model(torch.randn(684, 8, device=DEV), model.prepare(m, DEV, grid_pos=points("latlon", 3)))
    assert rel_err(b, a) <= REL_TOL and tuple(c.shape) == (684, 8) and bool(torch.isfinite(c).all())


@pytest.mark.parametrize("swap", [False, True])
def test_row_pointer_and_either_query_side(ga, swap):
    """The larger set queries the cell list of the smaller: both orientations give the restatement's list, and the row
    pointer the fill returns is the target histogram of that list."""
    from gwen_amd import gridgraph as G
    m, p = mesh(3), points("random", 3)
    src, dst = (m.pos, p) if swap else (p, m.pos)                               # 2000 sources > 92 targets, and back
    for radius in (default_radius(3), 2.5, 1e-3):
        want = R.radius_edges(src, dst, radius)
        sp, dp = (torch.from_numpy(G.unit_vectors(x)).to(DEV) for x in (src, dst))
        got, rowptr = G.radius_edges_device(sp, dp, radius, with_rowptr=True)
        assert np.array_equal(got.cpu().numpy(), want)
        want_rp = np.concatenate([[0], np.cumsum(np.bincount(want[1], minlength=dst.shape[0]))])
        assert rowptr.dtype == torch.int32 and np.array_equal(rowptr.cpu().numpy(), want_rp)
