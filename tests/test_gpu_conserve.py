"""Conservative regridding on the device (csrc/conserve.hip, gwen_amd/regrid.py; BUILD-DEFINED, parity unpinned) against
the numpy restatement of tests/conserve_ref.py: cell areas to 1e-13, the pair list EXACTLY (tests/test_conserve_host.py
asserts the gap that makes that fair), every overlap area within 1e-12 of the smaller cell, the partition of both sides on
the device's own numbers, identity, constants, conservation within a derived fp32 bound, the apply bitwise against the
sequential fp32 restatement, the backward against the fp64 transpose, partial coverage, reproducibility and capture."""
import functools

import numpy as np
import pytest
import torch

import conserve_ref as CR
import regrid_ref as R
from helpers import SEED
from test_gpu_regrid import field, transpose_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U24 = 2.0 ** -24
FULL = tuple(p for p in CR.PAIRS if p[0] != "north5")              # both sides tile the sphere


@pytest.fixture(scope="module")
def ga(hip_lib):
    import gwen_amd
    return gwen_amd


@functools.lru_cache(maxsize=None)
def device_overlaps(src, dst):
    import gwen_amd
    return tuple(t.cpu().numpy() for t in gwen_amd.cell_overlaps(CR.cells(src), CR.cells(dst), DEV))


@functools.lru_cache(maxsize=None)
def regridder(src, dst, normalize="covered", uncovered="raise"):
    import gwen_amd
    return gwen_amd.Regridder.conservative(CR.cells(src), CR.cells(dst), DEV, normalize=normalize, uncovered=uncovered)


def longest_row(ei, nd):
    return int(np.bincount(ei[1], minlength=nd).max())


# ---- 1. cell areas

@pytest.mark.parametrize("name", CR.TESSELLATIONS)
def test_cell_areas_equal_the_restatement_and_tile_the_sphere(ga, name):
    c = CR.cells(name)
    got = ga.cell_areas(c, DEV)
    assert got.dtype == torch.float64 and got.device.type == "cuda" and tuple(got.shape) == (c.shape[0],)
    got, want = got.cpu().numpy(), CR.geometry(c)[2]
    err = float(np.abs(got / want - 1.0).max())
    print(f"cell_areas {name}: max relative err {err:.3e} (bound 1e-13), sum - 4 pi {got.sum() - 4 * np.pi:.3e}")
    assert err <= 1e-13 and abs(got.sum() - 4 * np.pi) <= 1e-12


def test_cell_geometry_centre_and_radius(ga):
    from gwen_amd import regrid
    for name in ("dual3", "ll9x16"):
        c = CR.cells(name)
        centre, radius, _ = (t.cpu().numpy() for t in regrid.cell_geometry_device(torch.from_numpy(c.copy()).to(DEV)))
        wc, wr, _ = CR.geometry(c)
        assert np.abs(centre - wc).max() <= 4.5e-16 and np.abs(radius / wr - 1.0).max() <= 1e-15


# ---- 2. overlaps: the pair list exactly, the areas to 1e-12 of the smaller cell

@pytest.mark.parametrize("src,dst", CR.PAIRS)
def test_overlaps_list_the_restatements_pairs_with_its_areas(ga, src, dst):
    want = CR.overlaps_cached(src, dst)
    ei, area, sa, da = device_overlaps(src, dst)
    assert ei.dtype == np.int64 and area.dtype == np.float64
    assert np.array_equal(ei, want["edge_index"])                    # same pairs, same (target, source) order
    bound = 1e-12 * np.minimum(want["src_area"][ei[0]], want["dst_area"][ei[1]])
    err = np.abs(area - want["area"])
    print(f"overlaps {src} -> {dst}: {ei.shape[1]} pairs, longest row {longest_row(ei, da.size)}, "
          f"worst err / bound {float((err / bound).max()):.3e}")
    assert (err <= bound).all()
    assert np.abs(sa / want["src_area"] - 1.0).max() <= 1e-13 and np.abs(da / want["dst_area"] - 1.0).max() <= 1e-13
    if (src, dst) == ("ll17x32", "faces5"):
        assert longest_row(ei, da.size) == 34


# ---- 3. partition, on the device's own numbers

@pytest.mark.parametrize("src,dst", FULL)
def test_overlap_areas_partition_both_cells(ga, src, dst):
    ei, area, sa, da = device_overlaps(src, dst)
    rows = np.bincount(ei[1], weights=area, minlength=da.size)
    cols = np.bincount(ei[0], weights=area, minlength=sa.size)
    print(f"partition {src} -> {dst}: rows {float(np.abs(rows / da - 1).max()):.3e}, "
          f"columns {float(np.abs(cols / sa - 1).max()):.3e} (bound 1e-12)")
    assert np.abs(rows / da - 1.0).max() <= 1e-12 and np.abs(cols / sa - 1.0).max() <= 1e-12


# ---- 4. identity

@pytest.mark.parametrize("name", ["faces3", "faces5"])
@pytest.mark.parametrize("normalize", ["covered", "cell"])
def test_a_tessellation_onto_itself_is_the_identity(ga, name, normalize):
    n = CR.cells(name).shape[0]
    rg = regridder(name, name, "covered")
    assert rg.num_src == n and rg.num_dst == n
    assert torch.equal(rg.edge_index.cpu(), torch.arange(n).expand(2, n)) and bool((rg.weights == 1.0).all())
    x = field(n, 5, 3).to(DEV)
    assert torch.equal(rg(x), x)
    if normalize == "cell":                                          # A_tt / A_t: one rounding away from 1 at the most
        w = regridder(name, name, "cell").weights
        assert float((w - 1.0).abs().max()) <= U24


# ---- 5. constants

@pytest.mark.parametrize("src,dst", FULL)
def test_covered_weights_keep_a_constant(ga, src, dst):
    rg = regridder(src, dst)
    ns, nd = rg.num_src, rg.num_dst
    rows = torch.bincount(rg.edge_index[1], minlength=nd).double()
    y = rg(torch.ones(ns, 2, device=DEV))
    err = (y.double() - 1.0).abs().max(dim=1).values
    print(f"constants {src} -> {dst}: worst err / bound {float((err / ((rows + 2) * U24)).max()):.3f}")
    assert bool((err <= (rows + 2) * U24).all())


# ---- 6. conservation

@pytest.mark.parametrize("src,dst", FULL)
def test_cell_weights_conserve_the_integral(ga, src, dst):
    rg = regridder(src, dst, "cell")
    ns, nd = rg.num_src, rg.num_dst
    x = field(ns, 3)
    y = rg(x.to(DEV)).cpu().numpy().astype(np.float64)
    sa, da = rg.src_area.cpu().numpy(), rg.dst_area.cpu().numpy()
    x = x.numpy().astype(np.float64)
    got, want = (da[:, None] * y).sum(axis=0), (sa[:, None] * x).sum(axis=0)
    bound = (longest_row(rg.edge_index.cpu().numpy(), nd) + 2) * U24 * (sa[:, None] * np.abs(x)).sum(axis=0)
    print(f"conservation {src} -> {dst}: worst err / bound {float((np.abs(got - want) / bound).max()):.3e}")
    assert (np.abs(got - want) <= bound).all()


# ---- 7. apply and backward, as tests/test_gpu_regrid.py checks them

@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("src,dst", [("faces3", "ll9x16"), ("ll17x32", "faces5"), ("dual3", "ll9x16")])
def test_apply_is_bitwise_the_sequential_fp32_restatement(ga, src, dst, members):
    rg = regridder(src, dst)
    ns, nd = rg.num_src, rg.num_dst
    ei, w32 = rg.edge_index.cpu().numpy(), rg.weights.cpu().numpy()
    assert np.array_equal(ei, CR.overlaps_cached(src, dst)["edge_index"]) and w32.dtype == np.float32
    want_w, _ = CR.weights(ei, CR.overlaps_cached(src, dst)["area"], CR.overlaps_cached(src, dst)["dst_area"])
    assert np.abs(w32.astype(np.float64) - want_w).max() <= U24 + 1e-12          # one fp32 rounding of a weight <= 1
    x = field(ns, 5) if members == 1 else field(ns, 5, members)
    y = rg(x.to(DEV))
    assert tuple(y.shape) == tuple(x.shape[:-2]) + (nd, 5) and y.dtype == torch.float32
    want = R.apply_f32(ei, w32, x.numpy(), nd)
    assert np.array_equal(y.cpu().numpy().view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("src,dst", [("faces3", "ll9x16"), ("ll17x32", "faces5")])
def test_backward_against_the_fp64_transpose(ga, src, dst):
    rg = regridder(src, dst)
    ns, nd = rg.num_src, rg.num_dst
    ei, w32 = rg.edge_index.cpu().numpy(), rg.weights.cpu().numpy()
    for shape in ((nd, 5), (3, nd, 5)):
        x = torch.zeros(*shape[:-2], ns, 5, device=DEV, requires_grad=True)
        g = torch.randn(*shape, generator=torch.Generator().manual_seed(SEED + len(shape)))
        grads = []
        for _ in range(2):
            x.grad = None
            rg(x).backward(g.to(DEV))
            grads.append(x.grad.clone())
        assert torch.equal(grads[0], grads[1])
        want, bound, _ = transpose_bound(ei, w32, g.numpy(), ns)
        assert (np.abs(grads[-1].cpu().numpy().astype(np.float64) - want) <= bound).all()
    assert not rg.weights.requires_grad


# ---- 8. partial coverage: the northern faces onto the whole lat-lon grid

def test_partial_coverage(ga):
    src, dst = "north5", "ll17x32"
    want = CR.overlaps_cached(src, dst)
    ei, area, da = want["edge_index"], want["area"], want["dst_area"]
    _, cover = CR.weights(ei, area, da)
    missing = cover < 1e-9
    assert missing.sum() > 100 and ((cover > 1e-3) & (cover < 0.999)).sum() > 10
    with pytest.raises(ValueError, match=rf"{int(missing.sum())} of 544 target cells"):
        ga.Regridder.conservative(CR.cells(src), CR.cells(dst), DEV)
    ns = CR.cells(src).shape[0]
    rows = np.bincount(ei[1], minlength=544)
    for normalize in ("covered", "cell"):
        rg = regridder(src, dst, normalize, "nan")
        assert np.abs(rg.coverage.cpu().numpy() - cover).max() <= 1e-12
        assert rg.uncovered.dtype == torch.bool and np.array_equal(rg.uncovered.cpu().numpy(), missing)
        assert np.array_equal(rg.edge_index.cpu().numpy(), ei)
        x = torch.ones(3, ns, 2, device=DEV, requires_grad=True)
        y = rg(x)
        assert torch.equal(torch.isnan(y).any(dim=-1), rg.uncovered[None, :].expand(3, -1))
        assert bool(torch.isnan(y[:, rg.uncovered]).all())
        got = y[0, ~rg.uncovered, 0].detach().double().cpu().numpy()
        scale = np.ones_like(cover) if normalize == "covered" else cover
        assert (np.abs(got - scale[~missing]) <= (rows[~missing] + 2) * U24).all()
        g = torch.ones_like(y)
        g[:, rg.uncovered] = float("nan")                            # whatever arrives at an uncovered row is dropped
        y.backward(g)
        assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
    assert float(regridder(src, dst, "cell", "nan").coverage.max()) <= 1.0 + 1e-12


# ---- 9. reproducibility and capture

def test_two_builds_are_bitwise_equal(ga):
    a = ga.cell_overlaps(CR.cells("ll17x32"), CR.cells("faces5"), DEV)
    b = ga.cell_overlaps(CR.cells("ll17x32"), CR.cells("faces5"), DEV)
    assert torch.equal(a[0], b[0]) and all(torch.equal(p.view(torch.int64), q.view(torch.int64)) for p, q in zip(a[1:], b[1:]))
    r1, r2 = (ga.Regridder.conservative(CR.cells("faces4"), CR.cells("rot4"), DEV, normalize="cell") for _ in range(2))
    assert torch.equal(r1.edge_index, r2.edge_index) and torch.equal(r1.weights, r2.weights)
    assert torch.equal(r1.coverage.view(torch.int64), r2.coverage.view(torch.int64))


def test_call_is_capturable_after_one_eager_call(ga):
    rg = ga.Regridder.conservative(CR.cells("faces3"), CR.cells("ll9x16"), DEV)
    x = field(180, 5, 3).to(DEV)
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
    fresh = field(180, 5, 3, seed=SEED + 1).to(DEV)
    static_x.copy_(fresh)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, rg(fresh))
    static_x.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ---- 10. validation

def test_validation_on_the_device_path(ga):
    ok = CR.cells("faces3")
    clockwise = ok[:, ::-1]
    nan = ok.copy()
    nan[3, 1, 0] = np.nan
    hemi = np.array([[[1.0, 0, 0.01], [-0.5, 0.8660254037844386, 0.01], [-0.5, -0.8660254037844386, 0.01]]])
    for bad in (clockwise, np.zeros((4, 9, 3)), nan, hemi):
        with pytest.raises(ValueError):
            ga.cell_areas(bad, DEV)
        with pytest.raises(ValueError):
            ga.cell_overlaps(ok, bad, DEV)
        with pytest.raises(ValueError):
            ga.Regridder.conservative(bad, ok, DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ga.Regridder.conservative(ok, ok, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        regridder("faces3", "ll9x16")(torch.zeros(180, 2))
    empty = ga.cell_overlaps(ok[:0], ok, DEV)                        # an empty side: nothing overlaps
    assert tuple(empty[0].shape) == (2, 0) and empty[3].numel() == 180
