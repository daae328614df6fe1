"""The refusals of the pitch / member-stride arguments of the GCN entry points (include/gwen_hip.h), code for code.
CPU only, in the manner of tests/test_launcher_table_host.py: fake 16-byte aligned pointers, and every call is one the
launcher REFUSES, so it returns before the first HIP call (an accepted call with fake pointers would launch)."""
import pytest

from strided import LAYOUTS

EINVAL = -1
P, Q = 0x10000, 0x20000               # two distinct fake device pointers, 16-byte aligned
N = 640


@pytest.fixture(scope="module")
def L(hip_lib):
    return hip_lib


def _k2(L, ldh, ldo, F=64):
    return L.gwen_gcn_propagate_f32(P, P, P, P, None, Q, N, F, ldh, ldo, 3, N * F, N * F, 0, None)


def _k3(L, ldx, ldh, fin=64, fout=32):
    return L.gwen_gcn_linear_f32(P, P, None, Q, N, fin, fout, ldx, ldh, 0, 0, None, 0, None)


def _nn(L, ldx, ldw, ldh, fin=64, fout=32):
    return L.gwen_gcn_linear_nn_f32(P, P, None, Q, N, fin, fout, ldx, ldw, ldh, 0, 0, None, 0, None)


def _k4(L, ldx=64, ldo=32, msx=N * 64, mso=N * 32, fin=64, fout=32):
    return L.gwen_gcn_layer_tuned2_f32(None, P, P, P, P, None, Q, N, fin, fout, ldx, ldo, 3, msx, mso, 0, 0, 8, 0, 0, 0,
                                       None)


def _k5(L, form, msx, mso):
    fin, f1, f2, pre = {"chain": (64, 64, 32, 0), "pre": (64, 32, 0, 1), "gather": (64, 0, 0, 1)}[form]
    return L.gwen_gcn_chain_tuned2_f32(None, P, P, P, P if f1 else None, P if f2 else None, None, Q, N, fin, f1, f2, pre, 0,
                                       3, msx, mso, 0, 8, 0, 0, 0, None)


def _k8(L, ldo=128, msx=N * 64, mso=N * 128, fin=64, fout=128):
    return L.gwen_gcn_wide_layer_f32(P, P, P, P, P, None, Q, N, N, fin, fout, ldo, 3, msx, mso, 0, 128, 0, None)


def _k7(L, msx, mso, n=125, fin=64, fout=32):
    return L.gwen_gcn_small_layer_f32(P, P, P, None, None, Q, n, fin, fout, 3, msx, mso, 0, None, 0, 0, None)


def test_a_pitch_below_the_width_is_refused(L):
    assert _k2(L, 63, 64) == EINVAL and _k2(L, 64, 63) == EINVAL
    assert _k3(L, 63, 32) == EINVAL and _k3(L, 64, 31) == EINVAL
    assert _nn(L, 63, 32, 32) == EINVAL and _nn(L, 64, 31, 32) == EINVAL and _nn(L, 64, 32, 31) == EINVAL
    assert _k4(L, ldx=63) == EINVAL and _k4(L, ldo=31) == EINVAL and _k4(L, ldo=28) == EINVAL
    assert _k8(L, ldo=127) == EINVAL and _k8(L, ldo=124) == EINVAL
    for contract in (0, 1, 2):
        assert L.gwen_gcn_grad_weight_f32(P, P, Q, N, 64, 32, 31, 64, None, contract, None) == EINVAL      # ldg < Fout
        assert L.gwen_gcn_grad_weight_f32(P, P, Q, N, 64, 32, 32, 63, None, contract, None) == EINVAL      # ldx < Fin
        assert L.gwen_gcn_grad_weight_partial_f32(P, P, Q, N, 64, 32, 31, 64, contract, None) == EINVAL
        assert L.gwen_gcn_grad_weight_partial_f32(P, P, Q, N, 64, 32, 32, 63, contract, None) == EINVAL
        assert L.gwen_gcn_grad_weight_bias_partial_f32(P, P, Q, Q, N, 64, 64, 63, 64, contract, None) == EINVAL
        assert L.gwen_gcn_grad_weight_bias_partial_f32(P, P, Q, Q, N, 64, 64, 64, 63, contract, None) == EINVAL
    assert L.gwen_gcn_grad_bias_f32(P, Q, N, 64, 63, None, None) == EINVAL
    assert L.gwen_gcn_grad_bias_partial_f32(P, Q, N, 64, 63, None) == EINVAL


@pytest.mark.parametrize("off", [1, 2, 3])
def test_vector_kernels_refuse_strides_that_break_16_byte_alignment(L, off):
    """K4, K5, K8 (and K7) move 16-byte vectors at x + m * mstride_x and out + m * mstride_o + r * ldo."""
    assert _k4(L, ldo=32 + off) == EINVAL
    assert _k4(L, msx=N * 64 + off) == EINVAL
    assert _k4(L, mso=N * 32 + off) == EINVAL
    assert _k8(L, ldo=128 + off) == EINVAL
    assert _k8(L, msx=N * 64 + off) == EINVAL
    assert _k8(L, mso=N * 128 + off) == EINVAL
    for form, fw in (("chain", 32), ("pre", 32), ("gather", 64)):
        assert _k5(L, form, N * 64 + off, N * fw) == EINVAL
        assert _k5(L, form, N * 64, N * fw + off) == EINVAL          # the output side: stores at out + m * mstride_o
    assert _k7(L, 125 * 64 + off, 125 * 32) == EINVAL
    assert _k7(L, 125 * 64, 125 * 32 + off) == EINVAL


def test_fused_weight_and_bias_gradient_exists_on_the_dma_staged_kernel_only(L):
    """g, x 16-byte aligned with ldg, ldx multiples of 4; otherwise the caller takes the two separate launches."""
    for contract in (0, 2):
        assert L.gwen_gcn_grad_weight_bias_supported(64, 64, contract) == 1
        for g, x, ldg, ldx in ((P + 4, P, 64, 64), (P, P + 8, 64, 64), (P, P, 65, 64), (P, P, 64, 66)):
            assert L.gwen_gcn_grad_weight_bias_partial_f32(g, x, Q, Q, N, 64, 64, ldg, ldx, contract, None) == EINVAL


def test_k4_takes_contiguous_input_rows_only(L):
    assert _k4(L, ldx=68) == EINVAL and _k4(L, ldx=128) == EINVAL


def test_linear_nn_takes_the_weight_at_its_own_pitch_only(L):
    assert _nn(L, 64, 36, 32) == EINVAL and _nn(L, 64, 64, 32) == EINVAL


# ---------------------------------------------------------------------------------------------------------------------
# the layout helper itself (tests/strided.py), on the CPU: a torch "kernel" out = 2 x with the pitches it is handed
# ---------------------------------------------------------------------------------------------------------------------
M_, R_, F_ = 3, 37, 12


def _double(ar, x, o, ldx=None, msx=None, ldo=None, mso=None, rows=R_):
    import torch
    src = torch.as_strided(ar.buf, (M_, rows, F_), (msx or x.mstride, ldx or x.ld, 1), x.offset)
    torch.as_strided(ar.buf, (M_, rows, F_), (mso or o.mstride, ldo or o.ld, 1), o.offset).copy_(2 * src)


def _arena(lx, lo):
    import torch
    from strided import Arena, layout
    vals = torch.randn(M_, R_, F_, generator=torch.Generator().manual_seed(23))
    ar = Arena("cpu")
    x = ar.input(vals, layout(lx, M_, R_, F_, k=1, j=2))
    o = ar.output(M_, R_, F_, layout(lo, M_, R_, F_, k=2, j=1))
    return vals, ar.commit(), x, o


@pytest.mark.parametrize("lo", LAYOUTS)
@pytest.mark.parametrize("lx", LAYOUTS)
def test_layout_helper_accepts_a_right_kernel(lx, lo):
    import torch
    from strided import POISON, SENTINEL
    vals, ar, x, o = _arena(lx, lo)
    for op in (x, o):                                          # the extent is tight, the base aligned as the layout says
        assert op.extent == (M_ - 1) * op.mstride + (R_ - 1) * op.ld + F_
        assert op.view[-1, -1, -1].storage_offset() == op.offset + op.extent - 1
        assert (op.ptr - ar.buf.data_ptr()) % 16 == 4 * (op.layout.base % 4) and op.guard >= 64 * op.ld
    assert torch.equal(x.values(), vals) and bool((ar.buf == POISON).any())
    assert bool((o.view.view(torch.int32) == SENTINEL).all())
    _double(ar, x, o)
    ar.verify()
    assert torch.equal(o.values(), 2 * vals)
    ar.reset()
    assert bool((o.view.view(torch.int32) == SENTINEL).all())


@pytest.mark.parametrize("wrong", ["ldo", "mso", "mso_interleaved", "unwritten", "input_written"])
def test_layout_helper_catches_a_wrong_kernel(wrong):
    import torch
    lo = "interleaved" if wrong == "mso_interleaved" else "window" if wrong == "ldo" else "member_gap"
    vals, ar, x, o = _arena("row_pad", lo)
    if wrong == "ldo":
        _double(ar, x, o, ldo=F_)                              # Fout where ldo belongs
    elif wrong.startswith("mso"):
        _double(ar, x, o, mso=R_ * o.ld)                       # rows * ld where mstride_o belongs
    elif wrong == "unwritten":
        _double(ar, x, o, rows=R_ - 1)
    else:
        _double(ar, x, o)
        x.view[1, 2, 3] += 1.0
    with pytest.raises(AssertionError):
        ar.verify()
    assert int(torch.isnan(ar.buf).sum()) > 0


def test_layout_helper_makes_a_used_padding_value_visible():
    import torch
    vals, ar, x, o = _arena("row_pad", "packed")
    _double(ar, x, o, ldx=F_)                                  # Fin where ldx belongs: rows drift into the padding
    ar.verify()                                                # nothing outside the output is written ...
    assert not torch.equal(o.values(), 2 * vals)               # ... but the poison is in the result
    assert float(o.values().abs().max()) >= 2.0 ** 100
