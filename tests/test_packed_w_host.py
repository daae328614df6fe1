"""Packed W of the narrow K4 / K5 forward through the C ABI: the size query, the argument checks of the pack entry point
and of the entry points that take images, the mode queries and the admission of the 80-row form.  CPU only: every call
below returns before the first HIP call (N = 0, or a refusal); the pointers handed over are never dereferenced."""
import ctypes as C

import pytest

EINVAL = -1
X3, F32, X6, F16X3 = 0, 1, 2, 3
WIDTHS = (16, 32, 64)
A16 = C.c_void_p(0x1000)                       # some 16-byte aligned address
ODD = C.c_void_p(0x1008)                       # and one that is not


def _layer(lib, fin=64, fout=64, exact=X6, rows=0, wp=None, packed=0, n=0, depth=0, mode=0):
    return lib.gwen_gcn_layer_tuned3_f32(None, None, None, None, None, None, None, n, fin, fout, fin, fout, 1, 0, 0, 0, exact,
                                         8, depth, rows, mode, wp, packed, None)


def _chain(lib, fin=64, f1=64, f2=32, pre=0, contract=X6, rows=0, w1p=None, w2p=None, packed=0, n=0, depth=0, mode=0):
    return lib.gwen_gcn_chain_tuned3_f32(None, None, None, None, None, None, None, None, n, fin, f1, f2, pre, 1, 1, 0, 0,
                                         contract, 8, depth, rows, mode, w1p, w2p, packed, None)


def test_size_query(hip_lib):
    for fin in WIDTHS:
        for fout in WIDTHS:
            assert hip_lib.gwen_gcn_packw_bytes(fin, fout, X3) == fin * fout * 2 * 2
            assert hip_lib.gwen_gcn_packw_bytes(fin, fout, X6) == fin * fout * 3 * 2
            assert hip_lib.gwen_gcn_packw_bytes(fin, fout, F32) == 0
            assert hip_lib.gwen_gcn_packw_bytes(fin, fout, F16X3) == 0
    for fin, fout in ((128, 64), (64, 128), (24, 64), (64, 8), (0, 64), (-16, 16), (256, 256)):
        assert hip_lib.gwen_gcn_packw_bytes(fin, fout, X6) == 0
    assert hip_lib.gwen_gcn_packw_bytes(64, 64, 7) == 0 and hip_lib.gwen_gcn_packw_bytes(64, 64, -1) == 0


def test_pack_arguments_are_checked(hip_lib):
    pack = hip_lib.gwen_gcn_packw_f32
    assert pack(None, 64, 64, X6, A16, None) == EINVAL                # no W
    assert pack(A16, 64, 64, X6, None, None) == EINVAL                # no image buffer
    assert pack(ODD, 64, 64, X6, A16, None) == EINVAL                 # misaligned
    assert pack(A16, 64, 64, X6, ODD, None) == EINVAL
    assert pack(A16, 128, 64, X6, A16, None) == EINVAL                # unsupported widths
    assert pack(A16, 64, 48, X3, A16, None) == EINVAL
    assert pack(A16, 64, 64, F32, A16, None) == EINVAL                # no bf16 split: no images
    assert pack(A16, 64, 64, F16X3, A16, None) == EINVAL


@pytest.mark.parametrize("packed", [-1, 3, 9])
def test_packed_outside_0_1_2_is_refused(hip_lib, packed):
    assert _layer(hip_lib, wp=A16, packed=packed) == EINVAL
    assert _chain(hip_lib, w1p=A16, w2p=A16, packed=packed) == EINVAL
    assert _chain(hip_lib, 64, 64, 0, 1, w1p=A16, packed=packed) == EINVAL


def test_layer_entry_point_checks_its_images(hip_lib):
    for exact in (X3, X6):
        assert _layer(hip_lib, exact=exact, wp=A16, packed=2) == 0        # N = 0: nothing to do
        assert _layer(hip_lib, exact=exact, wp=A16, packed=1) == 0
        assert _layer(hip_lib, exact=exact, wp=A16, packed=0) == 0
        assert _layer(hip_lib, exact=exact, wp=None, packed=0) == 0       # no images: the kernel splits
        assert _layer(hip_lib, exact=exact, wp=None, packed=1) == 0
        assert _layer(hip_lib, exact=exact, wp=None, packed=2) == EINVAL  # null images
        assert _layer(hip_lib, exact=exact, wp=ODD, packed=2) == EINVAL
    assert _layer(hip_lib, exact=F32, wp=A16, packed=2) == EINVAL          # wrong contraction: the fp32-input MFMA
    assert _layer(hip_lib, exact=F32, wp=A16, packed=0) == 0               # ... which the library's choice never packs
    for fin, fout in ((128, 64), (64, 128), (256, 256)):
        assert _layer(hip_lib, fin, fout, wp=A16, packed=2, rows=0) == EINVAL   # wide layers have no packed form
        assert _layer(hip_lib, fin, fout, wp=A16, packed=0) == 0
    assert _layer(hip_lib, 24, 64, wp=A16, packed=2) == EINVAL
    # the other checks of the entry point are those of gwen_gcn_layer_tuned2_f32
    assert _layer(hip_lib, wp=A16, packed=2, depth=3) == EINVAL
    assert _layer(hip_lib, wp=A16, packed=2, mode=3) == EINVAL
    assert _layer(hip_lib, wp=A16, packed=2, n=-1) == EINVAL


def test_chain_entry_point_checks_its_images(hip_lib):
    for c in (X3, X6):
        assert _chain(hip_lib, contract=c, w1p=A16, w2p=A16, packed=2) == 0
        assert _chain(hip_lib, contract=c, w1p=A16, w2p=A16, packed=0) == 0
        assert _chain(hip_lib, contract=c, packed=0) == 0
        assert _chain(hip_lib, contract=c, packed=1) == 0
        assert _chain(hip_lib, contract=c, packed=2) == EINVAL                      # null images
        assert _chain(hip_lib, contract=c, w1p=A16, packed=2) == EINVAL             # W2 has none
        assert _chain(hip_lib, contract=c, w2p=A16, packed=2) == EINVAL             # W1 has none
        assert _chain(hip_lib, contract=c, w1p=ODD, w2p=A16, packed=2) == EINVAL
        assert _chain(hip_lib, contract=c, w1p=A16, w2p=ODD, packed=2) == EINVAL
        assert _chain(hip_lib, 64, 32, 0, 1, contract=c, w1p=A16, packed=2) == 0    # activation first: one weight
        assert _chain(hip_lib, 64, 32, 0, 1, contract=c, packed=2) == EINVAL
        assert _chain(hip_lib, 64, 0, 0, 1, contract=c, w1p=A16, packed=2) == EINVAL   # the plain gather contracts nothing
        assert _chain(hip_lib, 64, 0, 0, 1, contract=c, w1p=A16, packed=0) == 0
    assert _chain(hip_lib, contract=F32, w1p=A16, w2p=A16, packed=2) == EINVAL     # K5 has no fp32-MFMA form
    assert _chain(hip_lib, 128, 128, 0, 1, contract=X3, w1p=A16, packed=2) == EINVAL   # unsupported widths for images
    assert _chain(hip_lib, 128, 128, 0, 1, contract=X3, w1p=A16, packed=0) == 0


def test_stack_launcher_checks_packed(hip_lib):
    fwd = hip_lib.gwen_gnn_forward_packed_f32
    for packed in (-1, 3):
        assert fwd(None, None, 0, None, None, None, 0, 1, None, None, None, 0, None, None, 8, None, packed) == EINVAL
    assert fwd(None, None, 0, None, None, None, 0, 1, None, None, None, 0, None, None, 8, None, 0) == EINVAL   # no graph


def test_mode_queries(hip_lib):
    for fin in WIDTHS:
        for fout in WIDTHS:
            for exact in (X3, X6):
                assert hip_lib.gwen_gcn_layer_packed_mode(fin, fout, exact) in (1, 2)
            assert hip_lib.gwen_gcn_layer_packed_mode(fin, fout, F32) == 1         # no images on the fp32-input MFMA
    assert hip_lib.gwen_gcn_layer_packed_mode(256, 64, X3) == 1                    # nor for wide layers
    assert hip_lib.gwen_gcn_layer_packed_mode(64, 64, 3) == 0 and hip_lib.gwen_gcn_layer_packed_mode(24, 64, X3) == 0
    for fin in WIDTHS:
        for f1 in WIDTHS:
            for c in (X3, X6):
                if hip_lib.gwen_gcn_chain_supported(fin, f1, 0, 1, c):
                    assert hip_lib.gwen_gcn_chain_packed_mode(fin, f1, 0, 1, c) in (1, 2)
                for f2 in WIDTHS:
                    want = (1, 2) if hip_lib.gwen_gcn_chain_supported(fin, f1, f2, 0, c) else (0,)
                    assert hip_lib.gwen_gcn_chain_packed_mode(fin, f1, f2, 0, c) in want
        assert hip_lib.gwen_gcn_chain_packed_mode(fin, 0, 0, 1, X3) == 1           # the plain gather reads no W
    assert hip_lib.gwen_gcn_chain_packed_mode(128, 128, 0, 1, X3) == 1
    assert hip_lib.gwen_gcn_chain_packed_mode(64, 64, 32, 0, F32) == 0
    # the c2 step's shapes: what was measured decides, and what ships is written down here
    shipped = {"layer": {(64, 64): 2, (32, 64): 1, (16, 32): 1}, "chain": {(64, 64, 32, 0): 2, (32, 16, 0, 1): 2}}
    for (fin, fout), mode in shipped["layer"].items():
        assert hip_lib.gwen_gcn_layer_packed_mode(fin, fout, X6) == mode
    for (fin, f1, f2, pre), mode in shipped["chain"].items():
        assert hip_lib.gwen_gcn_chain_packed_mode(fin, f1, f2, pre, X6) == mode


def test_80_row_blocks_exist_where_images_are_read(hip_lib):
    """80 rows are five gather passes at Fin = 64 and no whole number of passes at 32 or 16; the kernels that split W
    themselves have no such form, through the new entry points as through the old ones."""
    for fout in WIDTHS:
        assert _layer(hip_lib, 64, fout, rows=80, wp=A16, packed=2) == 0
        assert _layer(hip_lib, 64, fout, rows=80, wp=A16, packed=1) == EINVAL
        assert _layer(hip_lib, 64, fout, rows=80) == EINVAL
        assert _layer(hip_lib, 32, fout, rows=80, wp=A16, packed=2) == EINVAL
        assert _layer(hip_lib, 16, fout, rows=80, wp=A16, packed=2) == EINVAL
    assert hip_lib.gwen_gcn_layer_tuned2_f32(None, None, None, None, None, None, None, 0, 64, 64, 64, 64, 1, 0, 0, 0, X6, 8, 0,
                                             80, 0, None) == EINVAL
    for rows in (64, 96, 112, 128):                                        # the sizes there were stay, packed or not
        assert _layer(hip_lib, rows=rows, wp=A16, packed=2) == 0 and _layer(hip_lib, rows=rows) == 0
    for rows in (48, 100, 144):
        assert _layer(hip_lib, rows=rows, wp=A16, packed=2) == EINVAL
    assert hip_lib.gwen_gcn_chain_supported(64, 64, 32, 0, X6) == 1
    assert _chain(hip_lib, rows=80, w1p=A16, w2p=A16, packed=2) == 0
    assert _chain(hip_lib, rows=80, w1p=A16, w2p=A16, packed=1) == EINVAL
    assert _chain(hip_lib, rows=80) == EINVAL
    assert _chain(hip_lib, 64, 32, 0, 1, rows=80, w1p=A16, packed=2) == 0
    assert _chain(hip_lib, 32, 16, 0, 1, rows=80, w1p=A16, packed=2) == EINVAL
    assert _chain(hip_lib, 64, 0, 0, 1, rows=80) == EINVAL
    assert hip_lib.gwen_gcn_chain_tuned2_f32(None, None, None, None, None, None, None, None, 0, 64, 64, 32, 0, 1, 1, 0, 0, X6,
                                             8, 0, 80, 0, None) == EINVAL
    for rows in (64, 96, 112):
        assert _chain(hip_lib, rows=rows, w1p=A16, w2p=A16, packed=2) == 0 and _chain(hip_lib, rows=rows) == 0
    assert _chain(hip_lib, rows=128, w1p=A16, w2p=A16, packed=2) == EINVAL


def test_occupancy_queries_check_their_arguments(hip_lib):
    """gwen_gcn_{layer,chain}_blocks_per_cu: the checks of the tuned3 entry points, a result pointer and rows to launch."""
    v = C.c_int(-7)
    layer, chain = hip_lib.gwen_gcn_layer_blocks_per_cu, hip_lib.gwen_gcn_chain_blocks_per_cu
    la = (None, None, None, None, None, None, None)
    assert layer(*la, 100, 64, 64, 64, 64, 1, 0, 0, 0, X6, 8, 0, 0, 0, A16, 2, None) == EINVAL        # nowhere to store
    assert layer(*la, 0, 64, 64, 64, 64, 1, 0, 0, 0, X6, 8, 0, 0, 0, A16, 2, C.byref(v)) == EINVAL    # nothing to launch
    assert layer(*la, 100, 64, 64, 64, 64, 1, 0, 0, 0, X6, 8, 0, 0, 0, A16, 3, C.byref(v)) == EINVAL  # packed outside 0 .. 2
    assert layer(*la, 100, 64, 64, 64, 64, 1, 0, 0, 0, X6, 8, 0, 80, 0, None, 1, C.byref(v)) == EINVAL   # 80 rows: images only
    ca = la + (None,)
    assert chain(*ca, 100, 64, 64, 32, 0, 1, 1, 0, 0, X6, 8, 0, 0, 0, A16, A16, 2, None) == EINVAL
    assert chain(*ca, 0, 64, 64, 32, 0, 1, 1, 0, 0, X6, 8, 0, 0, 0, A16, A16, 2, C.byref(v)) == EINVAL
    assert chain(*ca, 100, 64, 64, 32, 0, 1, 1, 0, 0, X6, 8, 0, 0, 0, A16, None, 2, C.byref(v)) == EINVAL   # W2 has no image
    assert v.value == -7
