"""ring_longitude="bluestein" without a GPU: the ring plans on both sides of the C ABI, the size checks, the host tables
of gwen_amd.spectral restated as a transform in numpy, and the refusals of gwen_sht_rings_fft_transform."""
import ctypes

import numpy as np
import pytest

IRREGULAR = [1, 4, 7, 12, 18, 25, 25, 19, 12, 8, 5, 2]
EINVAL, ERANGE, ENOSPACE = -1, -2, -3                                       # GWEN_E* (include/gwen_hip.h)


def test_ring_fft_plan_on_the_listed_values():
    import gwen_amd
    from gwen_amd import spectral
    assert gwen_amd.ring_fft_plan is spectral.ring_fft_plan
    assert spectral.RING_LONGITUDE == ("direct", "bluestein") and spectral.LONGITUDE == ("direct", "fft")
    plan = spectral.ring_fft_plan
    assert plan(28) == ("bluestein", 14, 27) and plan(19) == ("bluestein", 19, 40)
    assert plan(4088) == ("bluestein", 2044, 4096) and plan(2047) == ("bluestein", 2047, 4096)
    assert plan(44) == ("bluestein", 22, 45)
    assert plan(20) == ("mixed", 10, 0) and plan(25) == ("mixed", 25, 0) and plan(1) == ("mixed", 1, 0)
    assert plan(4096) == ("mixed", 2048, 0) and plan(3125) == ("mixed", 3125, 0)
    assert plan(4098)[0] is None and plan(2049)[0] is None and plan(0)[0] is None


def test_ring_fft_plan_equals_the_library_up_to_4200(hip_lib):
    from gwen_amd import _lib
    from gwen_amd.spectral import fft_supported, ring_fft_plan
    n, m = ctypes.c_int64(), ctypes.c_int64()
    kinds = set()
    for nlon in range(1, 4201):
        kind, pn, pm = ring_fft_plan(nlon)
        code = hip_lib.gwen_sht_ring_fft_plan(nlon, ctypes.byref(n), ctypes.byref(m))
        assert _lib.SHT_RING_KINDS[code] == kind, nlon
        kinds.add(kind)
        if kind is None:
            continue
        assert (n.value, m.value) == (pn, pm), nlon
        assert pn == (nlon // 2 if nlon % 2 == 0 else nlon)
        assert (kind == "mixed") == fft_supported(nlon)
        if kind == "bluestein":
            assert 2 * pn - 1 <= pm <= 4096 and fft_supported(pm)
            assert not any(fft_supported(k) for k in range(2 * pn - 1, pm)), nlon     # the smallest such M
    assert kinds == {"mixed", "bluestein", None}
    assert hip_lib.gwen_sht_ring_fft_plan(0, ctypes.byref(n), ctypes.byref(m)) == 0
    assert hip_lib.gwen_sht_ring_fft_plan(28, None, ctypes.byref(m)) == 0


def test_check_rings_takes_the_keyword():
    import gwen_amd
    rings = gwen_amd.check_rings(IRREGULAR, 11, "direct", "bluestein")
    assert rings.dtype == np.int64 and rings.tolist() == IRREGULAR
    assert gwen_amd.check_rings(gwen_amd.octahedral_nlon(8), 11, ring_longitude="bluestein").size == 16
    assert gwen_amd.check_rings(IRREGULAR, 11, ring_longitude="direct").tolist() == IRREGULAR
    with pytest.raises(ValueError) as err:
        gwen_amd.check_rings([2049, 4098, 4098, 2049], 3, ring_longitude="bluestein")
    assert "ring_nlon[0] = 2049" in str(err.value)
    with pytest.raises(ValueError) as err:
        gwen_amd.check_rings([4096, 4098, 4098, 4096], 3, ring_longitude="bluestein")
    assert "ring_nlon[1] = 4098" in str(err.value)
    assert gwen_amd.check_rings([2049, 4098, 4098, 2049], 3).size == 4              # the direct sums take them
    with pytest.raises(ValueError) as err:
        gwen_amd.check_rings(IRREGULAR, 11, ring_longitude="fft")
    assert "ring_longitude" in str(err.value) and "'fft'" in str(err.value)


def test_longitude_fft_on_a_reduced_grid_still_raises():
    import gwen_amd
    for make in (lambda **kw: gwen_amd.SphericalHarmonics.reduced(IRREGULAR, "cpu", lmax=11, **kw),
                 lambda **kw: gwen_amd.SphericalHarmonics.octahedral(8, "cpu", **kw)):
        with pytest.raises(ValueError, match="fft"):
            make(longitude="fft")
        with pytest.raises(ValueError, match="fft"):
            make(longitude="fft", ring_longitude="bluestein")
    with pytest.raises(ValueError, match="fft"):
        gwen_amd.check_rings(IRREGULAR, 11, "fft")


# ---- the host tables, as a transform -------------------------------------------------------------------------------------

def bluestein(z, tables, ring, sign):
    """The n-point DFT of ``z`` with ``exp(sign 2 pi i j k / n)`` as csrc/sht_fft.h runs it, from the tables of ``ring``."""
    kind, n, m, chirp_at, filter_at, conv_at = tables["plan"][ring, :6].tolist()
    assert kind == 2 and z.shape == (n,)
    c = tables["chirp"][chirp_at:chirp_at + n] @ np.array([1.0, 1.0j])
    big = tables["filter"][filter_at:filter_at + m] @ np.array([1.0, 1.0j])
    if sign > 0:
        c, big = np.conj(c), np.conj(big)
    a = np.zeros(m, dtype=np.complex128)
    a[:n] = z * c
    conv = m * np.fft.ifft(np.fft.fft(a) * big)                 # transform<-1>, times H, transform<+1>
    return conv[:n] * c


@pytest.mark.parametrize("nlon", [7, 14, 19, 22, 133, 2044, 2047])
def test_tables_restate_the_dft(nlon):
    """``nlon`` is the length of the complex FFT: that of the ring of ``2 nlon`` points, and of the ring of ``nlon``
    points where that is odd."""
    from gwen_amd.spectral import ring_fft_plan, ring_fft_tables
    rings = [2 * nlon] + ([nlon] if nlon % 2 else [])
    kinds = [ring_fft_plan(r) for r in rings]
    assert all(k[0] == "bluestein" and k[1] == nlon for k in kinds) and len({k[2] for k in kinds}) == 1
    tables = ring_fft_tables(rings + rings)
    plan = tables["plan"]
    assert plan.dtype == np.int32 and plan.shape == (2 * len(rings), 8)
    assert np.array_equal(plan[:len(rings)], plan[len(rings):])                       # one set a distinct length
    m = int(plan[0, 2])
    assert tables["max_points"] == m and tables["conv_twiddle"].shape == (m, 2)       # one table per distinct M
    assert tables["chirp"].shape == (len(rings) * nlon, 2) and tables["filter"].shape == (len(rings) * m, 2)
    k = np.arange(m)
    want = np.stack([np.cos(2 * np.pi * k / m), np.sin(2 * np.pi * k / m)], 1)
    assert np.abs(tables["conv_twiddle"] - want).max() <= 2e-16
    rng = np.random.default_rng(nlon)
    z = rng.standard_normal(nlon) + 1j * rng.standard_normal(nlon)
    scale = np.sqrt(nlon) * np.abs(z).max()
    for ring in range(len(rings)):
        fwd = np.abs(bluestein(z, tables, ring, -1) - np.fft.fft(z)).max()
        inv = np.abs(bluestein(z, tables, ring, +1) - nlon * np.fft.ifft(z)).max()
        print(f"n = {nlon}, M = {m}, ring of {rings[ring]}: forward {fwd / scale:.1e}, inverse {inv / scale:.1e} "
              f"sqrt(n) max |x|")
        assert fwd <= 1e-13 * scale and inv <= 1e-13 * scale


def test_tables_of_mixed_rings_and_offsets():
    from gwen_amd.spectral import octahedral_nlon, ring_fft_tables
    reg = ring_fft_tables([150] * 4)
    assert reg["plan"][:, :3].tolist() == [[1, 75, 0]] * 4 and reg["max_points"] == 75
    assert reg["chirp"].shape == (1, 2) and reg["filter"].shape == (1, 2) and reg["conv_twiddle"].shape == (1, 2)
    rings = octahedral_nlon(8)
    o8 = ring_fft_tables(rings)
    kinds = o8["plan"][:, 0].tolist()
    assert [r for r, k in zip(rings.tolist(), kinds) if k == 2] == [28, 44, 44, 28]
    assert o8["max_points"] == 45 and o8["chirp"].shape == (14 + 22, 2) and o8["filter"].shape == (27 + 45, 2)
    assert o8["conv_twiddle"].shape == (27 + 45, 2)
    assert np.array_equal(o8["plan"][2], o8["plan"][13]) and o8["plan"][2].tolist() == [2, 14, 27, 0, 0, 0, 0, 0]
    assert o8["plan"][6].tolist() == [2, 22, 45, 14, 27, 27, 0, 0]
    with pytest.raises(ValueError, match=r"ring_nlon\[1\] = 4098"):
        ring_fft_tables([20, 4098])


# ---- the C entry validates before any HIP call -------------------------------------------------------------------------

def fft_call(plan=0x1000, chirp=0x1000, filter=0x1000, conv_twiddle=0x1000, max_points=45, **over):
    """A gwen_sht_rings_fft_call on O8, lmax 7, C 3, batch 2 with stand-in pointers that nothing dereferences."""
    from gwen_amd import _lib
    item = 8 * 16 * 15 * 3
    fields = dict(op=_lib.SHT_OP_ANALYSIS, adjoint=0, in0=0x1000, in1=0x1000, in_f64=0, out0=0x1000, out1=0x1000,
                  out_f64=1, nodes=0x1000, lat_w=0x1000, twiddle=0x1000, seed=0x1000, ring_nlon=0x1000, ring_start=0x1000,
                  batch=2, nlat=16, points=544, max_nlon=48, lmax=7, C=3, workspace=0x1000, workspace_bytes=item - 8,
                  stream=None)
    fields.update(over)
    return _lib.ShtRingsFftCall(rings=_lib.ShtRingsCall(**fields), ring_plan=plan, chirp=chirp, filter=filter,
                                conv_twiddle=conv_twiddle, max_points=max_points)


def test_rings_fft_transform_validates_before_any_device_call(hip_lib):
    from gwen_amd import _lib
    run = hip_lib.gwen_sht_rings_fft_transform
    assert run(None) == EINVAL
    # with every size and pointer right the workspace, one double short of an item, is what stops the call
    for op in (_lib.SHT_OP_ANALYSIS, _lib.SHT_OP_SYNTHESIS):
        assert run(ctypes.byref(fft_call(op=op))) == ENOSPACE
    item = 8 * 16 * 15 * 3
    for op in (_lib.SHT_OP_VECTOR_ANALYSIS, _lib.SHT_OP_VECTOR_SYNTHESIS):
        assert run(ctypes.byref(fft_call(op=op, workspace_bytes=2 * item - 8))) == ENOSPACE
    assert run(ctypes.byref(fft_call(max_points=1))) == ENOSPACE and run(ctypes.byref(fft_call(max_points=4096))) == ENOSPACE
    assert run(ctypes.byref(fft_call(batch=0))) == 0
    for over in (dict(op=4), dict(op=-1), dict(nlat=0), dict(nlat=2049), dict(lmax=16), dict(lmax=-1), dict(lmax=24),
                 dict(points=62), dict(points=16 * 48 + 1), dict(C=0), dict(batch=-1), dict(in_f64=2), dict(out_f64=-1),
                 dict(op=_lib.SHT_OP_VECTOR_ANALYSIS, adjoint=2), dict(ring_nlon=None), dict(ring_start=None),
                 dict(ring_nlon=0x1002), dict(ring_start=0x1004), dict(twiddle=0x1008), dict(twiddle=None),
                 dict(in0=None), dict(out0=None), dict(workspace=None), dict(nodes=None), dict(seed=None),
                 dict(op=_lib.SHT_OP_VECTOR_ANALYSIS, in1=None), dict(op=_lib.SHT_OP_VECTOR_SYNTHESIS, in0=None, in1=None),
                 dict(plan=None), dict(chirp=None), dict(filter=None), dict(conv_twiddle=None), dict(plan=0x1008),
                 dict(chirp=0x1008), dict(filter=0x1008), dict(conv_twiddle=0x1008), dict(max_points=0),
                 dict(max_points=4097), dict(max_points=-1), dict(batch=0, max_points=0)):
        assert run(ctypes.byref(fft_call(**over))) == EINVAL, over
    assert run(ctypes.byref(fft_call(op=_lib.SHT_OP_VECTOR_SYNTHESIS, in1=None, workspace_bytes=8))) == ENOSPACE
    for over in (dict(C=2 ** 31), dict(nlat=2, lmax=1, max_nlon=2 ** 31, points=2 ** 31 + 1),
                 dict(nlat=2048, lmax=7, max_nlon=2 ** 21, points=2 ** 31)):
        assert run(ctypes.byref(fft_call(**over))) == ERANGE, over
