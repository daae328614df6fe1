"""The stack launcher's scratch (csrc/forward.hip): three activation buffers while the three fit the 256 MiB Infinity
Cache, two beyond that -- a third buffer of a large activation is real memory and buys nothing there.  Host only: the
size query makes no HIP call."""
from gwen_amd import _lib

N = 100002                                     # the c2 mesh
WIDTHS = [(64, 64), (64, 32), (32, 16), (16, 32), (32, 64), (64, 64)]


def _floats(lib, members):
    desc = (_lib.LayerDesc * len(WIDTHS))()
    for d, (fi, fo) in zip(desc, WIDTHS):
        d.fin, d.fout, d.relu, d.order, d.contract = fi, fo, 1, _lib.ORDER_AUTO, _lib.CONTRACT_BF16X6
    return int(lib.gwen_gnn_forward_scratch_floats(N, members, desc, len(WIDTHS)))


def test_scratch_is_three_buffers_in_the_cache_and_two_beyond(hip_lib):
    lib = _lib.lib()
    one = N * 64                               # floats of one member's widest activation (a multiple of 4)
    base = _floats(lib, 1) - 3 * one           # workspaces and padding besides the activation buffers
    assert 0 <= base < one
    for members in (1, 2, 3):                  # 3 x 76.8 MB = 230 MB: still inside 256 MiB
        assert _floats(lib, members) - 3 * members * one < members * one
        assert _floats(lib, members) >= 3 * members * one
    for members in (4, 16, 340):               # 3 x 102 MB is beyond it: the pair
        assert 2 * members * one <= _floats(lib, members) < 3 * members * one
