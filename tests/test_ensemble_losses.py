"""Ensemble CRPS (gwen_amd.losses) without a GPU: argument validation, the C ABI's refusals, the grid-cell areas and
the fp64 test reference itself."""
import math

import numpy as np
import pytest
import torch

from ensemble_ref import (count_difference, crps_points, crps_points_sorted, midrank_count_difference, pair_coef,
                          reference)


def _cpu(m=4, n=10, c=6):
    return torch.randn(m, n, c), torch.randn(n, c)


def test_shape_and_argument_errors_come_first():
    from gwen_amd.losses import ensemble_crps, ensemble_scores
    p, t = _cpu()
    with pytest.raises(ValueError):
        ensemble_crps(p[0], t)                                  # no members axis
    with pytest.raises(ValueError):
        ensemble_crps(p, t[:, :5])                              # target shape
    with pytest.raises(ValueError):
        ensemble_crps(p[:1], t)                                 # one member, alpha = 1
    with pytest.raises(ValueError):
        ensemble_crps(p[:1], t, alpha=0.5)
    with pytest.raises(ValueError):
        ensemble_crps(torch.randn(65, 10, 6), t)                # M = 65
    with pytest.raises(ValueError):
        ensemble_crps(p, t, alpha=1.5)
    with pytest.raises(ValueError):
        ensemble_crps(p, t, node_weights=torch.ones(9))
    with pytest.raises(ValueError):
        ensemble_crps(p, t, channel_weights=torch.ones(6, 1))
    with pytest.raises(ValueError):
        ensemble_crps(p, t, node_weights=torch.ones(10, requires_grad=True))
    with pytest.raises(ValueError):
        ensemble_crps(p, t, channel_weights=torch.ones(6, requires_grad=True))
    with pytest.raises(ValueError):
        ensemble_scores(torch.randn(4, 0, 6), torch.randn(0, 6))
    from gwen_amd.losses import EnsembleCRPSLoss
    with pytest.raises(ValueError):
        EnsembleCRPSLoss(alpha=-0.1)


def test_dtype_then_device_errors():
    from gwen_amd.losses import ensemble_crps, ensemble_scores
    p, t = _cpu()
    with pytest.raises(TypeError):
        ensemble_crps(p.double(), t)
    with pytest.raises(TypeError):
        ensemble_crps(p, t, node_weights=torch.ones(10, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ensemble_crps(p, t)                                     # fp32 on the CPU: no fallback
    with pytest.raises(RuntimeError):
        ensemble_scores(p[:1], t, alpha=0.0)                    # M = 1 with alpha = 0 is valid: only the device fails
    with pytest.raises(RuntimeError):
        ensemble_crps(p, t, node_weights=torch.ones(10, dtype=torch.bool))


def test_module_holds_weights_as_buffers_and_pickles():
    import pickle
    from gwen_amd import geodesic_mesh
    from gwen_amd.losses import EnsembleCRPSLoss
    areas = geodesic_mesh(2).face_areas()
    mod = EnsembleCRPSLoss(alpha=0.95, node_weights=areas, channel_weights=torch.ones(3))
    names = dict(mod.named_buffers())
    assert set(names) == {"node_weights", "channel_weights"}
    assert names["node_weights"].dtype == torch.float32 and names["node_weights"].shape == (80,)
    back = pickle.loads(pickle.dumps(mod))
    assert back.alpha == 0.95 and torch.equal(back.node_weights, mod.node_weights)
    assert EnsembleCRPSLoss().node_weights is None


def test_abi_refuses_bad_sizes_without_gpu(hip_lib):
    L = hip_lib
    ws = L.gwen_ens_crps_workspace_floats(4, 100, 8)
    assert ws == 2 + 8 + 3 * 8 * 100
    assert L.gwen_ens_crps_workspace_floats(4, 200000, 256) == 2 + 256 + 3 * 256 * 2048
    assert L.gwen_ens_crps_workspace_floats(0, 100, 8) == 0
    assert L.gwen_ens_crps_workspace_floats(65, 100, 8) == 0
    p = 256                                                     # aligned non-null host values: never dereferenced
    for m, n, c, w in ((0, 100, 8, ws), (65, 100, 8, ws), (4, 0, 8, ws), (4, 100, 0, ws), (4, 100, 8, ws - 1)):
        assert L.gwen_ens_crps_f32(p, p, None, None, m, n, c, 0.1, None, None, p, None, p, w, None) == -1
    # missing pred / target / loss / workspace, misaligned pointer
    assert L.gwen_ens_crps_f32(None, p, None, None, 4, 100, 8, 0.1, None, None, p, None, p, ws, None) == -1
    assert L.gwen_ens_crps_f32(p, p, None, None, 4, 100, 8, 0.1, None, None, None, None, p, ws, None) == -1
    assert L.gwen_ens_crps_f32(p, p, None, None, 4, 100, 8, 0.1, None, None, p, None, None, ws, None) == -1
    assert L.gwen_ens_crps_f32(p + 2, p, None, None, 4, 100, 8, 0.1, None, None, p, None, p, ws, None) == -1


@pytest.mark.parametrize("nu", [1, 4, 16])
def test_face_areas_cover_the_sphere(nu):
    from gwen_amd import geodesic_mesh
    m = geodesic_mesh(nu)
    a = m.face_areas()
    assert a.dtype == np.float64 and a.shape == (m.faces.shape[0],)
    assert abs(a.sum() - 4.0 * math.pi) <= 1e-9
    assert (a > 0).all()


def test_icosahedron_faces_are_equal():
    from gwen_amd import geodesic_mesh
    a = geodesic_mesh(1).face_areas()
    assert a.shape == (20,)
    np.testing.assert_allclose(a, 4.0 * math.pi / 20.0, rtol=1e-12)


def test_face_areas_follow_a_reordered_mesh():
    from gwen_amd import geodesic_mesh
    a, b = geodesic_mesh(6).face_areas(), geodesic_mesh(6, reorder="hilbert").face_areas()
    np.testing.assert_allclose(np.sort(a), np.sort(b), rtol=1e-12)


@pytest.mark.parametrize("m", [2, 3, 8, 33])
@pytest.mark.parametrize("alpha", [1.0, 0.95, 0.0])
def test_reference_pairwise_and_sorted_forms_agree(m, alpha):
    g = torch.Generator().manual_seed(m)
    x = torch.randn(m, 50, 3, generator=g, dtype=torch.float64)
    x[:, :20] = torch.round(x[:, :20] * 2) / 2                # ties
    y = torch.round(torch.randn(50, 3, generator=g, dtype=torch.float64) * 2) / 2
    a, b = crps_points(x, y, alpha), crps_points_sorted(x, y, alpha)
    assert torch.allclose(a, b, rtol=1e-12, atol=1e-12)
    assert torch.equal(midrank_count_difference(x), count_difference(x))


def test_reference_gradient_is_the_rank_formula():
    g = torch.Generator().manual_seed(5)
    m, alpha = 6, 0.95
    x = (torch.round(torch.randn(m, 30, 2, generator=g, dtype=torch.float64) * 2) / 2).requires_grad_()
    y = torch.round(torch.randn(30, 2, generator=g, dtype=torch.float64) * 2) / 2
    loss, _ = reference(x, y, alpha=alpha)
    loss.backward()
    k = pair_coef(m, alpha)
    want = (torch.sign(x.detach() - y) / m - 2 * k * count_difference(x.detach())) / (30 * 2)
    assert torch.allclose(x.grad, want, rtol=1e-12, atol=1e-15)
