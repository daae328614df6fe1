"""Argument checks of the tuned K4 / K5 entry points (gwen_gcn_layer_tuned_f32, gwen_gcn_chain_tuned_f32) and the depth
queries through the C ABI.  CPU only: every call below returns before the first HIP call (N = 0, or a refusal)."""
import pytest

EINVAL = -1


def _layer(lib, depth, rows, fin=64, fout=64, n=0):
    return lib.gwen_gcn_layer_tuned_f32(None, None, None, None, None, None, None, n, fin, fout, fin, fout, 1, 0, 0, 0, 0, 8,
                                        depth, rows, None)


def _chain(lib, depth, rows, fin=64, f1=64, f2=32, pre=0, n=0):
    return lib.gwen_gcn_chain_tuned_f32(None, None, None, None, None, None, None, None, n, fin, f1, f2, pre, 1, 1, 0, 0, 0,
                                        8, depth, rows, None)


@pytest.mark.parametrize("depth", [-1, 3, 8])
def test_depth_outside_0_1_2_is_refused(hip_lib, depth):
    assert _layer(hip_lib, depth, 0) == EINVAL
    assert _chain(hip_lib, depth, 0) == EINVAL
    assert _chain(hip_lib, depth, 0, 64, 0, 0, 1) == EINVAL


@pytest.mark.parametrize("depth", [0, 1, 2])
def test_valid_depths_pass_the_check(hip_lib, depth):
    assert _layer(hip_lib, depth, 0) == 0                  # N = 0: nothing to do
    assert _chain(hip_lib, depth, 0) == 0
    assert _layer(hip_lib, depth, 0, 256, 256) == 0        # wide layers take the argument and run depth 1


def test_block_rows_are_whole_gather_passes(hip_lib):
    ok = {64: (0, 64, 96, 112, 128), 32: (0, 64, 96, 128), 16: (0, 64, 128)}
    for fin, good in ok.items():
        for rows in (-64, 0, 1, 16, 32, 48, 64, 80, 96, 112, 128, 192, 256):
            assert _layer(hip_lib, 1, rows, fin, 64) == (0 if rows in good else EINVAL), (fin, rows)
    okc = {64: (0, 64, 96, 112), 32: (0, 64, 96), 16: (0, 64)}
    for fin, good in okc.items():
        for rows in (-64, 0, 1, 16, 32, 48, 64, 80, 96, 112, 128, 192, 256):
            assert _chain(hip_lib, 2, rows, fin, 64, 32) == (0 if rows in good else EINVAL), (fin, rows)
            assert _chain(hip_lib, 2, rows, fin, 0, 0, 1) == (0 if rows in (0, 1024 // fin) else EINVAL), (fin, rows)
    assert _layer(hip_lib, 1, 128, 128, 128) == 0 and _layer(hip_lib, 1, 64, 128, 128) == EINVAL
    assert _chain(hip_lib, 1, 128, 128, 128, 0, 1) == 0 and _chain(hip_lib, 1, 96, 128, 128, 0, 1) == EINVAL


def test_depth_queries(hip_lib):
    for fin in (16, 32, 64):
        for fout in (16, 32, 64):
            for exact in (0, 1, 2):
                assert hip_lib.gwen_gcn_layer_depth(fin, fout, exact) in (1, 2)
    assert hip_lib.gwen_gcn_layer_depth(256, 64, 0) == 1
    assert hip_lib.gwen_gcn_layer_depth(64, 64, 3) == 0 and hip_lib.gwen_gcn_layer_depth(24, 64, 0) == 0
    assert hip_lib.gwen_gcn_chain_depth(64, 64, 32, 0, 0) in (1, 2)
    assert hip_lib.gwen_gcn_chain_depth(64, 0, 0, 1, 0) in (1, 2)
    assert hip_lib.gwen_gcn_chain_depth(64, 64, 32, 0, 1) == 0          # K5 has no fp32-MFMA form
