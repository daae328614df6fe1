"""The reference's loss module restated (gwen_amd.loss_functions): fixtures, restatement, surface and argument checks --
everything that needs no GPU."""
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch
from torch import nn

import ref_losses_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ERANGE = -1, -2


def _generator():
    spec = importlib.util.spec_from_file_location("make_ref_losses_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_ref_losses_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fixtures():
    return R.load_fixtures()


def test_fixture_files_hold_every_case_and_fit_a_commit(fixtures):
    names = R.case_names(fixtures)
    assert len(names) == 22
    assert sum(n.startswith("crps") for n in names) == 7 and sum(n.startswith("varreg") for n in names) == 5
    for f in ("ref_losses.npz", "ref_losses_large.npz"):            # the limit holds per committed file: 1 MiB each
        assert os.path.getsize(os.path.join(R.GOLDEN, f)) < 2 ** 20
    for n in names:
        for key in ("x", "t", "meta", "value32", "value64", "grad32_x", "grad64_x", "grad32_t", "grad64_t"):
            assert f"{n}/{key}" in fixtures, (n, key)
        assert fixtures[f"{n}/x"].dtype == np.float32 and fixtures[f"{n}/grad64_x"].dtype == np.float64
    # the NaN cases are NaN, and nothing else is
    for n in names:
        nan = n in ("varreg_m1_nan", "masked_l1_all_zero", "masked_mse_all_zero")
        assert bool(np.isnan(fixtures[f"{n}/value64"]).all()) == nan, n
        assert bool(np.isnan(fixtures[f"{n}/value32"]).all()) == nan, n


def test_restatement_reproduces_the_reference_fp64(fixtures):
    """tests/ref_losses_ref.py against value64 / grad64 of every case, 1e-12 of the array's largest value."""
    for n in R.case_names(fixtures):
        got = R.restate(n, fixtures)
        for g, key in zip(got, ("value64", "grad64_x", "grad64_t")):
            want = fixtures[f"{n}/{key}"]
            g = np.asarray(g, np.float64).reshape(want.shape)
            assert np.array_equal(np.isnan(g), np.isnan(want)), (n, key)
            ok = ~np.isnan(want)
            if ok.any():
                scale = np.abs(want[ok]).max()
                assert np.abs(g[ok] - want[ok]).max() <= 1e-12 * (scale if scale > 0 else 1.0), (n, key)


def test_generator_reproduces_the_committed_files(fixtures):
    """The generator, run in memory, against the committed files.  Inputs, meta and the case list are bitwise the
    files' on any build, and the classes' signatures are the reference's own.  Under the torch build that wrote the
    files every array is bitwise the file's.  Under another build the fp64 results must agree to 1e-12 of the array's
    largest value (the restatement's tolerance: fp64 sums in another order), and the fp32 results -- another fp32
    evaluation of the same expression -- must lie within the bound the GPU comparisons use against the recorded fp64,
    max(4 max|ref32 - ref64|, 16 * 2^-24 max|ref64|); a build outside it means the fixtures are to be regenerated."""
    gen = _generator()
    if not gen.available():
        pytest.skip("no checkout of the reference on this machine")
    ref = gen.load_reference()
    from gwen_amd import loss_functions as LF
    for name in ("CRPSLoss", "EnsembleVarRegLoss", "MaskedLoss"):
        ours, theirs = getattr(LF, name), getattr(ref, name)
        for fn in ("__init__", "forward"):
            a, b = inspect.signature(getattr(ours, fn)), inspect.signature(getattr(theirs, fn))
            assert [(p.name, p.default) for p in a.parameters.values()] == \
                   [(p.name, p.default) for p in b.parameters.values()], (name, fn)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fresh = gen.generate()
    assert sorted(fresh) == sorted(fixtures)
    same_build = str(fixtures["torch"]) == torch.__version__
    for k, v in fresh.items():
        want = fixtures[k]
        if k == "torch":
            continue
        assert v.dtype == want.dtype and v.shape == want.shape, k
        key = k.split("/")[1]
        if same_build or key in ("x", "t", "mask", "meta"):
            assert v.tobytes() == want.tobytes(), k
            continue
        assert np.array_equal(np.isnan(v), np.isnan(want)), k
        ok = ~np.isnan(want)
        if not ok.any():
            continue
        ref64 = fixtures[k.replace("32", "64")].astype(np.float64)
        scale = float(np.abs(ref64[ok]).max())
        if "64" in key:
            assert float(np.abs(v[ok] - want[ok]).max()) <= 1e-12 * (scale if scale > 0 else 1.0), k
        else:
            bound = max(4.0 * float(np.abs(want[ok].astype(np.float64) - ref64[ok]).max()), 16.0 * 2.0 ** -24 * scale)
            assert float(np.abs(v[ok].astype(np.float64) - ref64[ok]).max()) <= bound, \
                f"{k}: torch {torch.__version__} is outside the recorded fp32 run's bound; regenerate the fixtures"


def test_import_line_and_signatures():
    from gwen_amd.loss_functions import CRPSLoss, EnsembleVarRegLoss, MaskedLoss
    import gwen_amd
    assert gwen_amd.CRPSLoss is CRPSLoss and gwen_amd.MaskedLoss is MaskedLoss
    assert gwen_amd.EnsembleVarRegLoss is EnsembleVarRegLoss

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    E = inspect.Parameter.empty
    assert params(CRPSLoss.__init__) == [("self", E)]
    assert params(CRPSLoss.forward) == [("self", E), ("outputs", E), ("target", E), ("dim", 0)]
    assert params(EnsembleVarRegLoss.__init__) == [("self", E), ("alpha", 0.1)]
    assert params(EnsembleVarRegLoss.forward) == [("self", E), ("outputs", E), ("target", E)]
    assert params(MaskedLoss.__init__) == [("self", E), ("loss_fn", E)]
    assert params(MaskedLoss.forward) == [("self", E), ("outputs", E), ("target", E), ("mask", E)]
    assert EnsembleVarRegLoss().alpha == 0.1 and isinstance(CRPSLoss(), nn.Module)
    fn = nn.L1Loss(reduction="none")
    assert MaskedLoss(fn).loss_fn is fn
    # the product does not lean on the oracle
    text = open(os.path.join(ROOT, "gwen_amd", "loss_functions.py")).read()
    assert "oracle" not in text


def test_argument_errors_in_order():
    from gwen_amd.loss_functions import CRPSLoss, EnsembleVarRegLoss, MaskedLoss
    crps, var, masked = CRPSLoss(), EnsembleVarRegLoss(), MaskedLoss(nn.L1Loss(reduction="none"))
    x5, t4 = torch.randn(4, 2, 1, 3, 5), torch.randn(2, 1, 3, 5)
    # ranks and shapes: ValueError, and the message names the limit
    with pytest.raises(ValueError, match="5-D"):
        crps(torch.randn(4, 2, 3, 5), torch.randn(2, 3, 5))
    with pytest.raises(ValueError, match="5-D"):
        crps(torch.randn(4, 2, 1, 1, 3, 5), torch.randn(2, 1, 1, 3, 5))
    with pytest.raises(ValueError, match="target must be"):
        crps(x5, torch.randn(2, 1, 3, 4))
    with pytest.raises(ValueError, match="at least 2 members"):
        crps(torch.randn(1, 2, 1, 3, 5), t4)
    with pytest.raises(ValueError, match="at least 2 members"):
        crps(torch.randn(4, 2, 1, 3, 5), torch.randn(4, 2, 3, 5), dim=2)
    with pytest.raises(ValueError, match="256"):
        crps(torch.randn(257, 1, 1, 1, 2), torch.randn(1, 1, 1, 2))
    with pytest.raises(ValueError):
        crps(x5, t4, dim=5)
    with pytest.raises(ValueError, match="2 dims"):
        var(torch.randn(7), torch.randn(7))
    with pytest.raises(ValueError, match="broadcast"):
        var(torch.randn(3, 5, 7), torch.randn(3, 5, 6))
    with pytest.raises(ValueError, match="shape"):
        masked(torch.randn(3, 7, 9), torch.randn(3, 7, 8), torch.ones(7, 9))
    with pytest.raises(ValueError, match="broadcast"):
        masked(torch.randn(3, 7, 9), torch.randn(3, 7, 9), torch.ones(7, 8))
    with pytest.raises(ValueError, match="requires grad"):
        masked(torch.randn(3, 7, 9), torch.randn(3, 7, 9), torch.ones(7, 9, requires_grad=True))
    # shapes come before dtypes, dtypes before devices
    with pytest.raises(ValueError):
        crps(torch.randn(4, 2, 3, 5, dtype=torch.float64), torch.randn(2, 3, 5))
    with pytest.raises(TypeError, match="float32"):
        crps(x5.double(), t4)
    with pytest.raises(TypeError, match="float32"):
        var(torch.randn(3, 5, 7), torch.randn(3, 1, 7).double())
    with pytest.raises(TypeError, match="float32"):
        masked(torch.randn(3, 7, 9).double(), torch.randn(3, 7, 9).double(), torch.ones(7, 9))
    with pytest.raises(TypeError, match="mask"):
        masked(torch.randn(3, 7, 9), torch.randn(3, 7, 9), torch.ones(7, 9, dtype=torch.int64))
    # CPU tensors: no fallback
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crps(x5, t4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        var(torch.randn(3, 5, 7), torch.randn(3, 1, 7))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        masked(torch.randn(3, 7, 9), torch.randn(3, 7, 9), torch.ones(7, 9, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MaskedLoss(nn.SmoothL1Loss(reduction="none"))(torch.randn(3, 7, 9), torch.randn(3, 7, 9), torch.ones(7, 9))


P = 1 << 20           # a pointer-like value that is never dereferenced: every call below returns before any HIP call


def test_gauss_crps_abi_rejects_bad_arguments(hip_lib):
    L = hip_lib
    fwd = lambda a, m, r, s, pred=P, tgt=P, loss=P, ws=P, n=1 << 30: \
        L.gwen_gauss_crps_f32(pred, tgt, a, m, r, s, loss, ws, n, None)               # noqa: E731
    bwd = lambda a, m, r, s, g=P, pred=P, tgt=P, gp=P, gt=P: \
        L.gwen_gauss_crps_bwd_f32(g, pred, tgt, a, m, r, s, gp, gt, None)              # noqa: E731
    assert L.gwen_gauss_crps_workspace_floats(1, 8, 4096, 1024) == 2 * 4
    assert L.gwen_gauss_crps_workspace_floats(3, 8, 1025, 1025) == 2 * 4
    for call in (fwd, bwd):
        for a, m, r, s in ((0, 8, 64, 8), (1, 8, 0, 1), (-1, 8, 64, 8), (1, 8, 64, 0), (1, 8, 64, -2)):
            assert call(a, m, r, s) == EINVAL, (a, m, r, s)
        for m in (0, 1, 257, 1 << 33):
            assert call(1, m, 64, 8) == EINVAL, m
        assert call(2, 8, 64, 48) == EINVAL                     # S does not divide R
        assert call(2, 8, 64, 128) == EINVAL                    # ... nor may a sample span two a
        assert call(1, 2, (1 << 33) + 1, 1) == ERANGE           # more points than the grid addresses
        assert call(1 << 20, 2, 1 << 20, 1 << 20) == ERANGE
        assert call(1 << 17, 256, 1 << 16, 1 << 16) == ERANGE   # 2^41 elements
        assert call(1 << 62, 2, 1 << 62, 1) == ERANGE           # products that overflow int64
    for a, m, r, s in ((0, 8, 64, 8), (1, 1, 64, 8), (1, 8, 64, 48), (1, 2, 1 << 34, 1)):
        assert L.gwen_gauss_crps_workspace_floats(a, m, r, s) == 0
    assert fwd(1, 8, 4096, 1024, n=7) == EINVAL                 # workspace too short
    for kw in ("pred", "tgt", "loss", "ws"):
        assert fwd(1, 8, 64, 8, **{kw: None}) == EINVAL, kw
        assert fwd(1, 8, 64, 8, **{kw: P + 2}) == EINVAL, kw    # not 4-byte aligned
    for kw in ("g", "pred", "tgt"):
        assert bwd(1, 8, 64, 8, **{kw: None}) == EINVAL, kw
    assert bwd(1, 8, 64, 8, gp=None, gt=None) == EINVAL        # one of the two gradients must be asked for
    for kw in ("g", "pred", "tgt", "gp", "gt"):
        assert bwd(1, 8, 64, 8, **{kw: P + 1}) == EINVAL, kw


def test_varreg_abi_rejects_bad_arguments(hip_lib):
    L = hip_lib
    call = lambda a, m, r, bc=0, pred=P, tgt=P, gp=P, gt=P, loss=P, ws=P, n=1 << 30: \
        L.gwen_varreg_l1_f32(pred, tgt, a, m, r, bc, 0.1, gp, gt, loss, ws, n, None)   # noqa: E731
    assert L.gwen_varreg_l1_workspace_floats(3, 5, 1000) == 2 * 3
    for a, m, r in ((0, 5, 7), (3, 0, 7), (3, 5, 0), (3, -5, 7), (3, 1 << 31, 7)):
        assert call(a, m, r) == EINVAL, (a, m, r)
        assert L.gwen_varreg_l1_workspace_floats(a, m, r) == 0
    assert call(3, 5, 7, bc=2) == EINVAL
    assert call(1, 2, (1 << 33) + 1) == ERANGE
    assert call(1 << 10, 1 << 10, 1 << 21) == ERANGE
    assert call(1 << 62, 2, 1 << 62) == ERANGE
    assert call(3, 5, 1000, n=5) == EINVAL
    for kw in ("pred", "tgt", "loss", "ws"):
        assert call(3, 5, 7, **{kw: None}) == EINVAL, kw
    for kw in ("pred", "tgt", "gp", "gt", "loss", "ws"):
        assert call(3, 5, 7, **{kw: P + 2}) == EINVAL, kw


def test_masked_mean_abi_rejects_bad_arguments(hip_lib):
    L = hip_lib
    call = lambda outer, inner, full=0, kind=0, out=P, tgt=P, mask=P, go=P, gt=P, loss=P, ws=P, n=1 << 30: \
        L.gwen_masked_mean_f32(out, tgt, mask, outer, inner, full, kind, go, gt, loss, ws, n, None)  # noqa: E731
    assert L.gwen_masked_mean_workspace_floats(15, 63) == 1 + 1024 + 1
    for outer, inner in ((0, 63), (15, 0), (-1, 63)):
        assert call(outer, inner) == EINVAL
        assert L.gwen_masked_mean_workspace_floats(outer, inner) == 0
    assert call(15, 63, full=2) == EINVAL and call(15, 63, kind=2) == EINVAL and call(15, 63, kind=-1) == EINVAL
    assert call(1 << 17, (1 << 16) + 1) == ERANGE
    assert call(1 << 62, 1 << 62) == ERANGE
    assert call(15, 63, n=1025) == EINVAL
    for kw in ("out", "tgt", "mask", "loss", "ws"):
        assert call(15, 63, **{kw: None}) == EINVAL, kw
    for kw in ("out", "tgt", "mask", "go", "gt", "loss", "ws"):
        assert call(15, 63, **{kw: P + 2}) == EINVAL, kw
