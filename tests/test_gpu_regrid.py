"""Regridding on the device (csrc/regrid.hip, gwen_amd/regrid.py; BUILD-DEFINED, parity unpinned) against the numpy
restatements of tests/regrid_ref.py: the k-nearest search EXACTLY (same indices, d2 bitwise), the weights to fp32
rounding, the apply bitwise against a sequential fp32 restatement, and the backward against the fp64 transpose."""
import functools

import numpy as np
import pytest
import torch

import gridgraph_ref as GR
import regrid_ref as R
from helpers import SEED

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def ga(hip_lib):
    import gwen_amd
    return gwen_amd


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def check_search(got, want):
    idx, d2 = got
    assert idx.dtype == torch.int64 and d2.dtype == torch.float64 and idx.device.type == "cuda"
    assert tuple(idx.shape) == want[0].shape and tuple(d2.shape) == want[1].shape
    assert np.array_equal(idx.cpu().numpy(), want[0])
    assert np.array_equal(bits(d2.cpu().numpy()), bits(want[1]))          # bitwise, +inf padding included


def field(n, c, members=None, seed=SEED):
    shape = (n, c) if members is None else (members, n, c)
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed + 7 * c + n))


@functools.lru_cache(maxsize=None)
def regridder(src, dst, method="idw", k=4, power=1.0):
    import gwen_amd
    return gwen_amd.Regridder(R.points(src), R.points(dst), DEV, method=method, k=k, power=power)


@functools.lru_cache(maxsize=None)
def want_operator(src, dst, method="idw", k=4, power=1.0):
    """(edge_index, weights fp64 [E], weights fp32 [E]) of the restatement."""
    idx, d2, count = R.knn_cached(src, dst, 1 if method == "nearest" else k)
    w, entries = R.weights(d2, count, method, power)
    ei, w32 = R.operator(idx, w, entries)
    keep = np.arange(idx.shape[1])[None, :] < entries[:, None]
    return ei, w[keep], w32


# ---- 1. the search equals the restatement exactly

@pytest.mark.parametrize("k", [1, 4, 8])
@pytest.mark.parametrize("src,dst", R.PAIRS)
def test_search_equals_the_restatement_exactly(ga, src, dst, k):
    want = R.knn_cached(src, dst, k)
    check_search(ga.nearest_neighbours(R.points(src), R.points(dst), k, DEV), want)
    if (src, dst, k) == ("mesh3", "latlon", 1):          # 80 rows tie exactly at the cut: the index rule decides
        i2, d2, _ = R.knn_cached(src, dst, 4)
        assert int((d2[:, 0] == d2[:, 1]).sum()) == 80 and (i2[:, 0] < i2[:, 1])[d2[:, 0] == d2[:, 1]].all()
    if (src, dst) == ("cap", "random"):                  # targets far from every source: several doublings
        assert np.sqrt(want[1][:, 0].max()) > 1.9


def test_fewer_sources_than_k_pads_the_rows(ga):
    src, dst = R.points("latlon")[100:103], R.points("mesh2")
    want = R.knn(src, dst, 4)
    idx, d2 = ga.nearest_neighbours(src, dst, 4, DEV)
    check_search((idx, d2), want)
    assert (idx[:, 3] == -1).all() and torch.isinf(d2[:, 3]).all() and (idx[:, :3] >= 0).all()


# ---- 2. the starting radius does not matter

def test_the_starting_radius_does_not_change_the_result(ga, hip_lib):
    want = R.knn_cached("cap", "random", 4)
    for r0 in (1e-3, None, 2.5):
        check_search(ga.nearest_neighbours(R.points("cap"), R.points("random"), 4, DEV, initial_radius=r0), want)
    r0 = 0.01                                            # past the cell cap: cells larger than the radius
    assert 2.0 / r0 > hip_lib.gwen_gridgraph_cells(r0) == hip_lib.gwen_gridgraph_cells(1e-6)
    p = R.points("random")
    want = R.knn_cached("random", "random", 4)
    check_search(ga.nearest_neighbours(p, p, 4, DEV, initial_radius=r0), want)
    check_search(ga.nearest_neighbours(p, p, 4, DEV), want)
    assert np.array_equal(want[0][:, 0], np.arange(p.shape[0]))


def test_two_builds_are_bitwise_equal(ga):
    a = ga.nearest_neighbours(R.points("latlon"), R.points("random"), 8, DEV)
    b = ga.nearest_neighbours(R.points("latlon"), R.points("random"), 8, DEV)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int64), b[1].view(torch.int64))
    r1, r2 = (ga.Regridder(R.points("latlon"), R.points("random"), DEV, power=1.5) for _ in range(2))
    assert torch.equal(r1.edge_index, r2.edge_index) and torch.equal(r1.weights, r2.weights)


# ---- 3. max_distance

D_MAX = 0.1        # the 10-degree lat-lon grid has points 0.17 apart at the equator: some targets reach none


def test_max_distance_truncates_rows_and_finds_uncovered_targets(ga):
    src, dst = R.points("latlon"), R.points("random")
    want = R.knn(src, dst, 4, max_distance=D_MAX)
    count = want[2]
    assert (count == 0).any() and ((count > 0) & (count < 4)).any() and (count == 4).any()
    for r0 in (None, 1e-3, 2.5):
        check_search(ga.nearest_neighbours(src, dst, 4, DEV, max_distance=D_MAX, initial_radius=r0), want)
    missing = int((count == 0).sum())
    with pytest.raises(ValueError, match=rf"{missing} of 2000 target points"):
        ga.Regridder(src, dst, DEV, max_distance=D_MAX)
    rg = ga.Regridder(src, dst, DEV, max_distance=D_MAX, uncovered="nan")
    assert rg.uncovered.dtype == torch.bool and np.array_equal(rg.uncovered.cpu().numpy(), count == 0)
    w, entries = R.weights(want[1], count)
    ei, w32 = R.operator(want[0], w, entries)
    assert np.array_equal(rg.edge_index.cpu().numpy(), ei) and np.abs(rg.weights.cpu().numpy() - w32).max() <= 2.4e-7
    x = field(684, 5, 3).to(DEV).requires_grad_()
    y = rg(x)
    nan_rows = torch.isnan(y).any(dim=-1)
    assert torch.equal(nan_rows, rg.uncovered[None, :].expand(3, -1)) and torch.isnan(y[:, rg.uncovered]).all()
    g = torch.ones_like(y)
    g[:, rg.uncovered] = float("nan")                    # whatever arrives at an uncovered row is dropped
    y.backward(g)
    assert torch.isfinite(x.grad).all()
    full = ga.Regridder(src, dst, DEV, max_distance=2.0)                     # covers everything: same as no limit
    assert not full.uncovered.any() and torch.equal(full.edge_index, regridder("latlon", "random").edge_index)


# ---- 4. src_mask

def test_src_mask_keeps_original_indices_and_stops_masked_values(ga):
    src, dst = R.points("latlon"), R.points("random")
    mask = np.arange(src.shape[0]) % 3 != 0
    want = R.knn(src, dst, 4, src_mask=mask)
    check_search(ga.nearest_neighbours(src, dst, 4, DEV, src_mask=mask), want)
    check_search(ga.nearest_neighbours(src, dst, 4, DEV, src_mask=torch.from_numpy(mask)), want)
    assert mask[want[0]].all()
    rg = ga.Regridder(src, dst, DEV, src_mask=mask)
    assert rg.num_src == 684 and mask[rg.edge_index[0].cpu().numpy()].all()
    x = field(684, 5)
    x[torch.from_numpy(~mask)] = float("nan")
    y = rg(x.to(DEV))
    assert torch.isfinite(y).all()
    both = R.knn(src, dst, 4, src_mask=mask, max_distance=0.2)
    check_search(ga.nearest_neighbours(src, dst, 4, DEV, src_mask=mask, max_distance=0.2), both)


# ---- 5. weights

@pytest.mark.parametrize("power", [1.0, 2.0, 1.5])
@pytest.mark.parametrize("src,dst", [("latlon", "mesh2"), ("latlon", "random"), ("mesh3", "latlon")])
def test_weights_against_the_fp64_restatement(ga, src, dst, power):
    rg = regridder(src, dst, power=power)
    ei, w64, _ = want_operator(src, dst, power=power)
    nd = R.points(dst).shape[0]
    assert rg.num_src == R.points(src).shape[0] and rg.num_dst == nd
    assert rg.edge_index.dtype == torch.int64 and np.array_equal(rg.edge_index.cpu().numpy(), ei)     # (target, rank)
    w = rg.weights.cpu().numpy()
    assert w.dtype == np.float32
    err = float(np.abs(w.astype(np.float64) - w64).max())
    print(f"weights {src} -> {dst} power {power}: max abs err {err:.3e} (bound 2.4e-7)")
    assert err <= 2.4e-7
    rows = np.zeros(nd)
    np.add.at(rows, ei[1], w.astype(np.float64))
    assert np.abs(rows - 1.0).max() <= 3e-7


def test_coincident_targets_take_their_source_alone(ga):
    rg = regridder("latlon", "mesh2")
    idx, d2, _ = R.knn_cached("latlon", "mesh2", 4)
    on = d2[:, 0] <= R.COINCIDENT2
    assert on.sum() == 6 and (d2[on, 0] > 0).sum() == 3
    ei, w = rg.edge_index.cpu().numpy(), rg.weights.cpu().numpy()
    per_row = np.bincount(ei[1], minlength=42)
    assert (per_row[on] == 1).all() and (per_row[~on] == 4).all()
    single = np.isin(ei[1], np.flatnonzero(on))
    assert (w[single] == np.float32(1.0)).all() and np.array_equal(ei[0][single], idx[on, 0])
    # NaN everywhere but at the six sources the targets sit on: their neighbours' NaN must not reach them
    x = field(684, 5)
    clean = torch.full_like(x, float("nan"))
    sel = torch.from_numpy(idx[on, 0])
    clean[sel] = x[sel]
    y = rg(clean.to(DEV)).cpu()
    assert torch.equal(y[torch.from_numpy(on)], x[sel])
    assert torch.isnan(y[torch.from_numpy(~on)]).any(dim=-1).all()


# ---- 6. apply

@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("C", [1, 5, 64])
def test_apply_is_bitwise_the_sequential_fp32_restatement(ga, C, members):
    rg = regridder("mesh3", "latlon")
    ei, w32 = rg.edge_index.cpu().numpy(), rg.weights.cpu().numpy()
    x = field(92, C, members)
    y = rg(x.to(DEV))
    assert tuple(y.shape) == (members, 684, C) and y.dtype == torch.float32
    want = R.apply_f32(ei, w32, x.numpy(), 684)
    assert np.array_equal(y.cpu().numpy().view(np.int32), want.view(np.int32))
    for m in range(members):                                                  # every member is the one-member call
        assert torch.equal(rg(x[m].to(DEV)), y[m])
    assert tuple(rg(x[0].to(DEV)).shape) == (684, C)


def test_apply_nearest_constant_and_errors(ga):
    near = regridder("latlon", "random", method="nearest")
    idx, _, _ = R.knn_cached("latlon", "random", 1)
    assert np.array_equal(near.edge_index.cpu().numpy(), np.stack([idx[:, 0], np.arange(2000)]))
    assert (near.weights == 1.0).all()
    x = field(684, 5, 3)
    assert torch.equal(near(x.to(DEV)).cpu(), x[:, torch.from_numpy(idx[:, 0])])                 # source rows, bitwise
    rg = regridder("latlon", "random")
    const = torch.full((684, 3), 2.5, device=DEV)
    assert float((rg(const) - 2.5).abs().max()) <= 1e-6
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rg(x)
    with pytest.raises(ValueError):
        rg(x[:, :100].to(DEV))
    with pytest.raises(TypeError):
        rg(x.double().to(DEV))
    assert rg.graph.num_nodes == 2000 and rg.graph.source_nodes == 684


def test_from_weights_wraps_a_given_operator(ga):
    rg = regridder("mesh3", "latlon")
    own = ga.Regridder.from_weights(rg.edge_index, rg.weights, 92, 684)
    x = field(92, 5, 3).to(DEV)
    assert torch.equal(own(x), rg(x)) and own.num_src == 92 and own.num_dst == 684 and not own.uncovered.any()


# ---- 7. backward

def transpose_bound(ei, w32, g, num_src):
    """(A^T g in fp64, (T + 2) 2^-24 |A|^T |g| element by element); T = the longest row of the transpose."""
    a = R.dense(ei, w32, num_src, g.shape[-2])
    t = int(np.bincount(ei[0], minlength=num_src).max())
    g = g.astype(np.float64)
    return np.swapaxes(a, 0, 1) @ g, (t + 2) * U24 * (np.swapaxes(np.abs(a), 0, 1) @ np.abs(g)), t


@pytest.mark.parametrize("src,dst,long_rows", [("mesh3", "latlon", False), ("mesh1", "random", True)])
def test_backward_against_the_fp64_transpose(ga, src, dst, long_rows):
    rg = regridder(src, dst)
    ns, nd = R.points(src).shape[0], R.points(dst).shape[0]
    ei, w32 = rg.edge_index.cpu().numpy(), rg.weights.cpu().numpy()
    grads = []
    for shape in ((nd, 5), (3, nd, 5)):
        x = torch.zeros(*shape[:-2], ns, 5, device=DEV, requires_grad=True)
        g = torch.randn(*shape, generator=torch.Generator().manual_seed(SEED + len(shape)))
        for _ in range(2):
            x.grad = None
            rg(x).backward(g.to(DEV))
            grads.append(x.grad.clone())
        assert torch.equal(grads[-1], grads[-2])                              # two runs are bitwise equal
        want, bound, t = transpose_bound(ei, w32, g.numpy(), ns)
        assert (t > 256) == long_rows
        err = np.abs(grads[-1].cpu().numpy().astype(np.float64) - want)
        print(f"backward {src} -> {dst} {shape}: longest transposed row {t}, worst err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert (err <= bound).all()
    assert rg.weights.grad is None and not rg.weights.requires_grad


# ---- 8. from_mesh

def test_from_mesh_is_barycentric_interpolation_from_the_nodes(ga):
    m = ga.geodesic_mesh(3)
    for name in ("random", "latlon"):
        p = R.points(name)
        face, w64 = GR.containing_faces(p, m)
        assert (face >= 0).all()
        rg = ga.Regridder.from_mesh(m, p, DEV)
        n = p.shape[0]
        want_ei = np.stack([m.faces[face].reshape(-1), np.repeat(np.arange(n), 3)])
        assert rg.num_src == m.num_nodes and rg.num_dst == n and np.array_equal(rg.edge_index.cpu().numpy(), want_ei)
        w = rg.weights.cpu().numpy()
        # the device's fp64 weights agree with numpy's to 1e-12 (tests/test_gpu_gridgraph.py); then one fp32 rounding
        assert w.dtype == np.float32 and np.abs(w.astype(np.float64) - w64.reshape(-1)).max() <= U24 + 1e-12
        lin = (m.pos @ np.array([0.3, -0.2, 0.4]) + 0.1)[:, None].astype(np.float32)      # linear in position, |.| < 1
        got = rg(torch.from_numpy(lin).to(DEV)).cpu().numpy().astype(np.float64)
        want = R.dense(want_ei, w64.reshape(-1), m.num_nodes, n) @ lin.astype(np.float64)
        assert np.abs(got - want).max() <= 1e-6


# ---- 9. end to end: forecaster -> stations -> CRPS -> backward

def test_crps_at_stations_reaches_the_forecasters_parameters(ga):
    from gwen_amd.forecaster import InteractionForecaster
    m = ga.geodesic_mesh(2)
    torch.manual_seed(SEED)
    model = InteractionForecaster(3, 32, steps=1).to(DEV)
    graphs = InteractionForecaster.prepare(m, DEV)
    grid = ga.gridgraph.face_centres(m)
    stations = np.random.default_rng(SEED + 2).normal(size=(50, 3))
    rg = ga.Regridder(grid, stations, DEV)
    x0 = field(grid.shape[0], 3, 2).to(DEV)
    obs = field(50, 3, seed=SEED + 3).to(DEV)
    y = model(x0, graphs)
    y.retain_grad()
    z = rg(y)
    z.retain_grad()
    loss = ga.ensemble_crps(z, obs)
    loss.backward()
    assert tuple(z.shape) == (2, 50, 3) and bool(torch.isfinite(loss))
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert any(float(p.grad.abs().max()) > 0 for p in model.parameters())
    # dL/dy = A^T dL/dz, with the dense operator formed in torch
    a = torch.zeros(50, grid.shape[0], dtype=torch.float64, device=DEV)
    a.index_put_((rg.edge_index[1], rg.edge_index[0]), rg.weights.double(), accumulate=True)
    gz = z.grad.double()
    want = a.t() @ gz
    t = int(torch.bincount(rg.edge_index[0], minlength=grid.shape[0]).max())
    bound = (t + 2) * U24 * (a.abs().t() @ gz.abs())
    assert bool(((y.grad.double() - want).abs() <= bound).all()) and float(y.grad.abs().max()) > 0


# ---- 10. capture

def test_call_is_capturable_after_one_eager_call(ga):
    rg = ga.Regridder(R.points("mesh3"), R.points("latlon"), DEV)
    x = field(92, 5, 3).to(DEV)
    eager = rg(x)                                        # builds the lazy layouts
    static_x = x.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        rg(static_x)                                     # warm-up on the capture stream
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = rg(static_x)
    for seed in (1, 2):
        fresh = field(92, 5, 3, seed=SEED + seed).to(DEV)
        static_x.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, rg(fresh))
    static_x.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
