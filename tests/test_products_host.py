"""Ensemble products and rank histogram (gwen_amd.products) without a GPU: the fp64 restatements against numpy and
torch, argument validation on CPU tensors, the C ABI's refusals and the exported names."""
import numpy as np
import pytest
import torch

import products_ref as ref

Q = (0.0, 0.05, 0.1, 0.25, 1.0 / 3.0, 0.5, 0.9, 0.99, 1.0)


@pytest.mark.parametrize("m", [1, 2, 3, 5, 8, 17, 64])
def test_quantile_restatement_agrees_with_numpy_and_torch(m):
    g = torch.Generator().manual_seed(m)
    x = torch.randn(m, 40, 3, generator=g)
    got = ref.quantiles(x, Q)
    q64 = torch.tensor(Q, dtype=torch.float32).double()
    want_np = np.quantile(x.double().numpy(), q64.numpy(), axis=0, method="linear")
    want_t = torch.quantile(x.double(), q64, dim=0, interpolation="linear")
    assert float((got - torch.from_numpy(want_np)).abs().max()) <= 1e-13
    assert float((got - want_t).abs().max()) <= 1e-13
    # q = 0 / 1 copy the extremes, q = 0.5 with an odd count is the median
    assert torch.equal(got[0], x.double().amin(0)) and torch.equal(got[-1], x.double().amax(0))
    if m % 2 == 1:
        assert torch.equal(got[5], x.double().median(0).values)


def test_quantile_restatement_keeps_infinite_extremes():
    x = torch.tensor([[-float("inf")], [1.0], [float("inf")]]).reshape(3, 1, 1)
    got = ref.quantiles(x, (0.0, 0.5, 1.0)).reshape(3)
    assert got[0] == -float("inf") and got[1] == 1.0 and got[2] == float("inf")


def test_exceedance_restatement():
    x = torch.tensor([0.0, 1.0, 1.0, 2.0, float("nan")]).reshape(5, 1, 1).repeat(1, 2, 3)
    got = ref.exceedance(x, (1.0, -1.0, 2.0))
    assert got.shape == (3, 2, 3)
    assert torch.equal(got[:, 0, 0], torch.tensor([1.0, 4.0, 0.0], dtype=torch.float64) / 5)   # strict; NaN never
    per_channel = torch.tensor([[1.0, 0.0, 5.0]])
    assert torch.equal(ref.exceedance(x, per_channel)[0, 1], torch.tensor([1.0, 3.0, 0.0], dtype=torch.float64) / 5)
    want = (x.unsqueeze(0) > torch.tensor([1.0, -1.0, 2.0]).reshape(3, 1, 1, 1)).double().mean(1)
    assert torch.equal(got, want)


@pytest.mark.parametrize("m", [1, 4, 9])
def test_histogram_rows_sum_to_the_counted_weight(m):
    g = torch.Generator().manual_seed(m)
    quant = lambda t: torch.clamp(torch.round(t * 2) / 2, -2, 2)                      # noqa: E731
    x, y = quant(torch.randn(m, 500, 4, generator=g)), quant(torch.randn(500, 4, generator=g))
    y[3, 1] = float("nan")
    x[0, 7, 2] = float("nan")
    w = torch.rand(500, generator=g)
    for weights in (None, w):
        h = ref.rank_histogram(x, y, weights)
        assert h.shape == (4, m + 1)
        assert float((h.sum(1) - ref.counted_weight(x, y, weights)).abs().max()) <= 1e-10
    h = ref.rank_histogram(x, y)
    assert float(h.sum()) == pytest.approx(500 * 4 - 2)


def test_histogram_restatement_known_answers():
    x = torch.tensor([1.0, 2.0, 3.0]).reshape(3, 1, 1)
    h = lambda y: ref.rank_histogram(x, torch.tensor([[y]]))[0]                        # noqa: E731
    assert torch.equal(h(0.0), torch.tensor([1.0, 0, 0, 0], dtype=torch.float64))
    assert torch.equal(h(2.5), torch.tensor([0, 0, 1.0, 0], dtype=torch.float64))
    assert torch.equal(h(4.0), torch.tensor([0, 0, 0, 1.0], dtype=torch.float64))
    assert torch.equal(h(2.0), torch.tensor([0, 0.5, 0.5, 0], dtype=torch.float64))   # one tie: bins 1 and 2 share
    same = torch.zeros(3, 1, 1)
    assert torch.allclose(ref.rank_histogram(same, torch.zeros(1, 1))[0], torch.full((4,), 0.25, dtype=torch.float64))


def _cpu(m=4, n=10, c=6):
    return torch.randn(m, n, c), torch.randn(n, c)


def test_shape_and_argument_errors_come_first():
    from gwen_amd.products import (ensemble_products, ensemble_quantiles, exceedance_probability, rank_histogram)
    p, t = _cpu()
    with pytest.raises(ValueError):
        ensemble_products(p)                                     # nothing asked for
    with pytest.raises(ValueError):
        ensemble_products(p[0], mean=True)                       # no members axis
    with pytest.raises(ValueError):
        ensemble_products(torch.randn(65, 10, 6), mean=True)     # M = 65
    with pytest.raises(ValueError):
        ensemble_products(torch.randn(4, 0, 6), std=True)
    with pytest.raises(ValueError):
        ensemble_products("pred", mean=True)
    with pytest.raises(ValueError):
        ensemble_quantiles(p, (0.5, 1.5))                        # q outside [0, 1]
    with pytest.raises(ValueError):
        ensemble_quantiles(p, torch.tensor([-0.1]))
    with pytest.raises(ValueError):
        ensemble_quantiles(p, [float("nan")])
    with pytest.raises(ValueError):
        ensemble_quantiles(p, torch.linspace(0, 1, 33))          # Q over the limit
    with pytest.raises(ValueError):
        ensemble_quantiles(p, torch.rand(2, 2))
    with pytest.raises(ValueError):
        ensemble_quantiles(p, [])
    with pytest.raises(ValueError):
        exceedance_probability(p, torch.zeros(33))               # T over the limit
    with pytest.raises(ValueError):
        exceedance_probability(p, torch.zeros(2, 5))             # neither [T] nor [T, C]
    with pytest.raises(ValueError):
        exceedance_probability(p, torch.zeros(2, 6, 1))
    with pytest.raises(ValueError):
        exceedance_probability(p, ["a"])
    with pytest.raises(ValueError):
        rank_histogram(p, t[:, :5])
    with pytest.raises(ValueError):
        rank_histogram(p[0], t)
    with pytest.raises(ValueError):
        rank_histogram(p, t, node_weights=torch.ones(9))
    with pytest.raises(ValueError):
        rank_histogram(p, t, node_weights=[1.0] * 10)
    # a shape error wins over a dtype and a device error
    with pytest.raises(ValueError):
        ensemble_quantiles(p.double(), (2.0,))
    with pytest.raises(ValueError):
        rank_histogram(p.double(), t[:, :5])


def test_dtype_then_device_errors():
    from gwen_amd.products import ensemble_products, ensemble_quantiles, exceedance_probability, rank_histogram
    p, t = _cpu()
    with pytest.raises(TypeError):
        ensemble_products(p.double(), mean=True)
    with pytest.raises(TypeError):
        rank_histogram(p, t.double())
    with pytest.raises(TypeError):
        rank_histogram(p, t, node_weights=torch.ones(10, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ensemble_products(p, quantiles=(0.1, 0.5), thresholds=(0.0,), mean=True, std=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ensemble_quantiles(p, 0.5)                               # a bare number is one quantile
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        exceedance_probability(p, torch.zeros(3, 6, dtype=torch.float64))   # converted, not refused
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rank_histogram(p, t, node_weights=torch.ones(10, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rank_histogram(p[:1], t, normalize=False)


def test_validation_makes_no_library_call(monkeypatch):
    from gwen_amd import _lib, products

    def boom():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", boom)
    p, t = _cpu()
    with pytest.raises(ValueError):
        products.ensemble_quantiles(p, (1.5,))
    with pytest.raises(TypeError):
        products.rank_histogram(p, t.double())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        products.ensemble_products(p, quantiles=(0.5,), thresholds=(0.0,), mean=True, std=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        products.rank_histogram(p, t)


def test_names_are_exported():
    import gwen_amd
    for name in ("ensemble_products", "ensemble_quantiles", "exceedance_probability", "rank_histogram"):
        assert name in gwen_amd.__all__ and callable(getattr(gwen_amd, name))
    assert gwen_amd.products.MAX_QUANTILES == 32 and gwen_amd.products.MAX_THRESHOLDS == 32


def test_abi_refuses_bad_arguments_without_gpu(hip_lib):
    L = hip_lib
    x = 1024                                                     # a fake, aligned, never dereferenced address
    ok = (x, 4, 10, 8, x, 3, x, 2, 0, x, x, x, x, None)
    args = lambda **kw: tuple(kw.get(k, v) for k, v in zip(                          # noqa: E731
        ("pred", "M", "N", "C", "q", "Q", "thr", "T", "pc", "mean", "std", "quant", "prob", "st"), ok))
    for bad in (dict(M=0), dict(M=65), dict(N=0), dict(C=0), dict(Q=33), dict(T=33), dict(Q=-1), dict(pc=2),
                dict(pred=None), dict(q=None), dict(quant=None), dict(thr=None), dict(prob=None), dict(mean=x + 2),
                dict(Q=0, T=0, mean=None, std=None), dict(N=2 ** 41)):
        assert L.gwen_ens_products_f32(*args(**bad)) == -1, bad
    # the workspace of the rank histogram: chunks * C * (M + 1), chunks capped at 1024 and at 2^22 floats
    ws = L.gwen_ens_rank_hist_workspace_floats
    assert ws(4, 100, 8) == (100 + 31) // 32 * 8 * 5            # 256 / 8 = 32 rows a block
    assert ws(8, 200000, 16) == 1024 * 16 * 9
    assert ws(64, 200000, 256) == (2 ** 22 // (256 * 65)) * 256 * 65 <= 2 ** 22
    assert ws(64, 10, 2 ** 20) == 2 ** 20 * 65                  # one chunk at least
    assert ws(0, 10, 8) == 0 and ws(65, 10, 8) == 0 and ws(4, 0, 8) == 0
    hok = (x, x, x, 4, 100, 8, 1, x, x, ws(4, 100, 8), None)
    assert L.gwen_ens_rank_hist_f32(*hok[:9], ws(4, 100, 8) - 1, None) == -1
    for i, v in ((0, None), (1, None), (7, None), (8, None), (3, 65), (4, 0), (5, 0), (2, x + 1)):
        bad = list(hok)
        bad[i] = v
        assert L.gwen_ens_rank_hist_f32(*bad) == -1, (i, v)
