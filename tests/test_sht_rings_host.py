"""Reduced Gaussian grids without a GPU: the ring tables and size checks of gwen_amd.spectral, and the numpy restatement
tests/sht_rings_ref.py checked against itself and against tests/sht_ref.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sht_ref as R  # noqa: E402
import sht_rings_ref as G  # noqa: E402

IRREGULAR = [1, 4, 7, 12, 18, 25, 25, 19, 12, 8, 5, 2]


def test_octahedral_ring_lengths():
    from gwen_amd.spectral import octahedral_nlon
    import gwen_amd
    o8 = octahedral_nlon(8)
    assert o8.dtype == np.int64
    assert o8.tolist() == [20, 24, 28, 32, 36, 40, 44, 48, 48, 44, 40, 36, 32, 28, 24, 20]
    assert int(o8.sum()) == 544
    assert int(octahedral_nlon(320).sum()) == 421120
    assert np.array_equal(o8, G.octahedral(8))
    assert gwen_amd.octahedral_nlon is octahedral_nlon
    with pytest.raises(ValueError):
        octahedral_nlon(0)


@pytest.mark.parametrize("rings, lmax, longitude, word", [
    ([], 0, "direct", "ring"),
    ([20, 24, 0, 24, 20], 2, "direct", "ring_nlon[2] = 0"),
    ([8] * 2049, 3, "direct", "2049"),
    ([20] * 4, 4, "direct", "lmax = 3"),
    ([2049] * 1025, 1024, "direct", "1024"),
    ([20, 24, 24, 20] * 4, 12, "direct", "25"),
    ([20, 24, 24, 20], 3, "fft", "fft"),
], ids=["empty", "zero-ring", "nlat", "lmax-nlat", "lmax-1023", "max-nlon", "fft"])
def test_check_rings_raises(rings, lmax, longitude, word):
    from gwen_amd.spectral import check_rings
    with pytest.raises(ValueError) as err:
        check_rings(rings, lmax, longitude)
    assert word in str(err.value)


def test_check_rings_accepts_and_returns_int64():
    import gwen_amd
    rings = gwen_amd.check_rings(IRREGULAR, 11)
    assert rings.dtype == np.int64 and rings.tolist() == IRREGULAR
    assert gwen_amd.check_rings(gwen_amd.octahedral_nlon(8), 11, "direct").size == 16
    with pytest.raises(ValueError):
        gwen_amd.check_rings(IRREGULAR, None)
    with pytest.raises(ValueError):
        gwen_amd.check_rings(IRREGULAR, 3, "bluestein")


@pytest.mark.parametrize("n, lmax", [(8, 7), (8, 11), (16, 15)])
def test_restatement_round_trip(n, lmax):
    rings = G.octahedral(n)
    c = np.random.default_rng(n + lmax).standard_normal((1, (lmax + 1) ** 2, 2))
    err = float(np.abs(G.analysis(G.synthesis(c, rings, lmax), rings, lmax) - c).max())
    print(f"O{n}, lmax {lmax} (M_j down to {int(G.orders(rings, lmax).min())}): round trip {err:.1e}")
    assert err <= 1e-12


def test_restatement_equals_the_regular_one_on_equal_rings():
    rings, geom = [18] * 9, ("gauss", 9, 18, 8)
    rng = np.random.default_rng(3)
    x, c = rng.standard_normal((2, 162, 3)), rng.standard_normal((2, 81, 3))
    assert np.abs(G.analysis(x, rings, 8) - R.analysis(x, *geom)).max() <= 1e-13
    assert np.abs(G.synthesis(c, rings, 8) - R.synthesis(c, *geom)).max() <= 1e-13
    assert (G.orders(rings, 8) == 8).all()
    assert np.array_equal(G.point_weights(rings), R.point_weights("gauss", 9, 18))


@pytest.mark.parametrize("rings", [G.octahedral(8), IRREGULAR, [18] * 9], ids=["o8", "irr", "regular"])
def test_restated_weights_sum_to_one(rings):
    q = G.point_weights(rings)
    assert q.shape == (int(np.sum(rings)),) and abs(q.sum() - 1.0) <= 1e-14
    pos = G.positions(rings)
    assert np.abs(np.linalg.norm(pos, axis=1) - 1.0).max() <= 1e-15
    assert pos[0, 1] == 0.0 and pos[0, 2] < 0 < pos[-1, 2]                  # longitude 0 first, south to north


def test_restated_adjoint_identities_on_the_irregular_rings():
    rings, lmax = IRREGULAR, 11
    assert G.orders(rings, lmax).tolist() == [0, 1, 3, 5, 8, 11, 11, 9, 5, 3, 2, 0]
    rng = np.random.default_rng(5)
    p, t = int(np.sum(rings)), (lmax + 1) ** 2
    x, h, u, v = (rng.standard_normal((2, p, 3)) for _ in range(4))
    c, g, gv, gd = (rng.standard_normal((2, t, 3)) for _ in range(4))

    def close(a, b, terms):
        assert abs(a - b) <= 1e-12 * terms, (a, b, terms)

    ax = G.analysis(x, rings, lmax)
    close((ax * g).sum(), (x * G.analysis_adjoint(g, rings, lmax)).sum(), np.abs(ax * g).sum())
    sc = G.synthesis(c, rings, lmax)
    close((sc * h).sum(), (c * G.synthesis_adjoint(h, rings, lmax)).sum(), np.abs(sc * h).sum())
    vort, div = G.vector_analysis(u, v, rings, lmax)
    hu, hv = G.vector_analysis_adjoint(gv, gd, rings, lmax)
    close((vort * gv).sum() + (div * gd).sum(), (u * hu).sum() + (v * hv).sum(),
          np.abs(vort * gv).sum() + np.abs(div * gd).sum())
    su, sv = G.vector_synthesis(gv, gd, rings, lmax)
    av, ad = G.vector_synthesis_adjoint(u, v, rings, lmax)
    close((su * u).sum() + (sv * v).sum(), (gv * av).sum() + (gd * ad).sum(),
          np.abs(su * u).sum() + np.abs(sv * v).sum())


def test_restated_vector_round_trip_on_o8():
    rings, lmax = G.octahedral(8), 7
    rng = np.random.default_rng(6)
    vort, div = rng.standard_normal((2, 1, 64, 2))
    vort[:, 0] = div[:, 0] = 0.0
    back = G.vector_analysis(*G.vector_synthesis(vort, div, rings, lmax), rings, lmax)
    assert np.abs(back[0] - vort).max() <= 1e-12 and np.abs(back[1] - div).max() <= 1e-12


# ---- the C entry validates its scalar fields before any HIP call ----------------------------------------------------

EINVAL, ERANGE, ENOSPACE = -1, -2, -3                                       # GWEN_E* (include/gwen_hip.h)


def rings_call(**over):
    """A gwen_sht_rings_call on O8, lmax 7, C 3, batch 2 with stand-in pointers that nothing dereferences."""
    from gwen_amd import _lib
    item = 8 * 16 * 15 * 3
    fields = dict(op=_lib.SHT_OP_ANALYSIS, adjoint=0, in0=0x1000, in1=0x1000, in_f64=0, out0=0x1000, out1=0x1000,
                  out_f64=1, nodes=0x1000, lat_w=0x1000, twiddle=0x1000, seed=0x1000, ring_nlon=0x1000, ring_start=0x1000,
                  batch=2, nlat=16, points=544, max_nlon=48, lmax=7, C=3, workspace=0x1000, workspace_bytes=item - 8,
                  stream=None)
    fields.update(over)
    return _lib.ShtRingsCall(**fields)


def test_rings_workspace_bytes(hip_lib):
    size = hip_lib.gwen_sht_rings_workspace_bytes
    assert size(0, 16, 544, 48, 7, 3) == 8 * 16 * 15 * 3 and size(1, 16, 544, 48, 7, 3) == 2 * 8 * 16 * 15 * 3
    assert size(0, 16, 544, 48, 11, 3) == 8 * 16 * 23 * 3
    assert size(0, 16, 544, 48, 7, 3) == hip_lib.gwen_sht_workspace_bytes(2, 16, 48, 7, 3)
    for bad in ((2, 16, 544, 48, 7, 3), (0, 0, 544, 48, 7, 3), (0, 2049, 4098, 2, 0, 1), (0, 16, 544, 48, 16, 3),
                (0, 1100, 2 ** 22, 2047, 1024, 1), (0, 16, 544, 48, 24, 3), (0, 16, 62, 48, 7, 3),
                (0, 16, 16 * 48 + 1, 48, 7, 3), (0, 16, 544, 48, 7, 0), (0, 16, 544, 48, -1, 3)):
        assert size(*bad) == 0, bad


def test_rings_transform_validates_before_any_device_call(hip_lib):
    import ctypes
    from gwen_amd import _lib
    run = hip_lib.gwen_sht_rings_transform
    assert run(None) == EINVAL
    # with every size right the workspace, one double short of an item, is what stops the call
    for op in (_lib.SHT_OP_ANALYSIS, _lib.SHT_OP_SYNTHESIS):
        assert run(ctypes.byref(rings_call(op=op))) == ENOSPACE
    item = 8 * 16 * 15 * 3
    for op in (_lib.SHT_OP_VECTOR_ANALYSIS, _lib.SHT_OP_VECTOR_SYNTHESIS):
        assert run(ctypes.byref(rings_call(op=op, workspace_bytes=2 * item - 8))) == ENOSPACE
    assert run(ctypes.byref(rings_call(batch=0))) == 0
    for over in (dict(op=4), dict(op=-1), dict(nlat=0), dict(nlat=2049), dict(lmax=16), dict(lmax=-1), dict(lmax=24),
                 dict(points=62), dict(points=16 * 48 + 1), dict(C=0), dict(batch=-1), dict(in_f64=2), dict(out_f64=-1),
                 dict(op=_lib.SHT_OP_VECTOR_ANALYSIS, adjoint=2), dict(ring_nlon=None), dict(ring_start=None),
                 dict(ring_nlon=0x1002), dict(ring_start=0x1004), dict(twiddle=0x1008), dict(twiddle=None),
                 dict(in0=None), dict(out0=None), dict(workspace=None), dict(nodes=None), dict(seed=None),
                 dict(op=_lib.SHT_OP_VECTOR_ANALYSIS, in1=None), dict(op=_lib.SHT_OP_VECTOR_SYNTHESIS, in0=None, in1=None)):
        assert run(ctypes.byref(rings_call(**over))) == EINVAL, over
    assert run(ctypes.byref(rings_call(op=_lib.SHT_OP_VECTOR_SYNTHESIS, in1=None, workspace_bytes=8))) == ENOSPACE
    for over in (dict(C=2 ** 31), dict(nlat=2, lmax=1, max_nlon=2 ** 31, points=2 ** 31 + 1),
                 dict(nlat=2048, lmax=7, max_nlon=2 ** 21, points=2 ** 31)):
        assert run(ctypes.byref(rings_call(**over))) == ERANGE, over
