"""Host and C-ABI side of K6's precision tiers (CPU only: nothing here launches a kernel)."""
import pickle

import pytest


def test_contract_entry_points_are_exported_and_bound(hip_lib):
    from gwen_amd import _lib
    for name in ("gwen_mlp2_contract_supported", "gwen_mlp2_contract_workspace_bytes", "gwen_mlp2_contract_f32",
                 "gwen_mlp2_bwd_contract_f32"):
        assert hasattr(hip_lib, name) and name in _lib.SIGNATURES


def test_contract_supported_and_workspace(hip_lib):
    from gwen_amd import _lib
    L = hip_lib
    for f in (32, 64, 128, 256):
        assert L.gwen_mlp2_contract_supported(f, _lib.CONTRACT_F16X3) == 1
        assert L.gwen_mlp2_contract_supported(f, _lib.CONTRACT_BF16X3) == 1
        assert L.gwen_mlp2_contract_supported(f, _lib.CONTRACT_F32) == 0
        assert L.gwen_mlp2_contract_supported(f, _lib.CONTRACT_BF16X6) == 0
        assert L.gwen_mlp2_contract_workspace_bytes(f, _lib.CONTRACT_BF16X3) == L.gwen_mlp2_workspace_bytes(f)
    for f in (0, 16, 48, 512):
        assert L.gwen_mlp2_contract_supported(f, _lib.CONTRACT_F16X3) == 0
        assert L.gwen_mlp2_contract_workspace_bytes(f, _lib.CONTRACT_F16X3) == -1
    # 256 channels: the fragment images plus one int32 exponent per output column of each matrix
    assert L.gwen_mlp2_contract_workspace_bytes(256, _lib.CONTRACT_F16X3) == 2 * 2 * 256 * 256 * 2 + 2 * 256 * 4
    assert L.gwen_mlp2_contract_workspace_bytes(64, _lib.CONTRACT_F16X3) == 0
    assert L.gwen_mlp2_contract_workspace_bytes(64, _lib.CONTRACT_F32) == -1


def test_contract_launches_refuse_before_touching_a_device(hip_lib):
    from gwen_amd import _lib
    L = hip_lib
    fake = 4096                                     # never dereferenced: the calls must return before any launch

    def fwd(F, contract):
        return L.gwen_mlp2_contract_f32(fake, fake, None, None, 0, 0, None, None, 0, 0, None, fake, None, None, fake, 10,
                                        F, 0, None, None, 0, None, 0, 0, contract, None, 0, None)

    def bwd(F, contract):
        return L.gwen_mlp2_bwd_contract_f32(fake, fake, fake, fake, fake, 10, F, fake, fake, fake, 10, F, contract, None,
                                            0, None)

    for c in (_lib.CONTRACT_F32, _lib.CONTRACT_BF16X6, 7, -1):
        assert fwd(64, c) == -1 and bwd(64, c) == -1
    assert fwd(48, _lib.CONTRACT_F16X3) == -1 and fwd(48, _lib.CONTRACT_BF16X3) == -1
    assert bwd(32, _lib.CONTRACT_F16X3) == -1 and bwd(128, _lib.CONTRACT_F16X3) == -1    # the backward launch: 64, 256


def test_unknown_precisions_are_refused():
    import torch
    from gwen_amd.forecaster import InteractionForecaster
    from gwen_amd.interaction import InteractionNet, mlp2
    for bad in ("fp32", "bf16x6", "bf16x3", None):
        with pytest.raises(ValueError, match="3xbf16"):
            InteractionNet(64, precision=bad)
    net = InteractionNet(64)
    with pytest.raises(ValueError):
        net.precision = "fp32"
    assert net.precision == "3xbf16"
    a, w = torch.zeros(4, 64), torch.zeros(64, 64)
    with pytest.raises(ValueError, match="f16x3"):
        mlp2(a, w, w, contract="bf16x6")
    with pytest.raises(ValueError):
        InteractionForecaster(4, 32, 1, precision="fp32")
    with pytest.raises(ValueError):
        InteractionForecaster(4, 32, 1).set_precision("bf16x6")


def test_precision_is_a_setting_not_state():
    import torch
    from gwen_amd.interaction import InteractionNet
    lo, hi = InteractionNet(64), InteractionNet(64, precision="f16x3")
    assert lo.precision == "3xbf16" and hi.precision == "f16x3"
    keys = ["edge_mlp.0.weight", "edge_mlp.0.bias", "edge_mlp.2.weight", "edge_mlp.2.bias",
            "node_mlp.0.weight", "node_mlp.0.bias", "node_mlp.2.weight", "node_mlp.2.bias"]
    assert list(lo.state_dict()) == keys and list(hi.state_dict()) == keys
    hi.load_state_dict(lo.state_dict(), strict=True)
    assert hi.precision == "f16x3"
    lo.load_state_dict(hi.state_dict(), strict=True)
    assert lo.precision == "3xbf16"
    assert all(torch.equal(a, b) for a, b in zip(lo.state_dict().values(), hi.state_dict().values()))
    again = pickle.loads(pickle.dumps(hi))
    assert again.precision == "f16x3" and list(again.state_dict()) == keys
    hi.precision = "3xbf16"
    assert pickle.loads(pickle.dumps(hi)).precision == "3xbf16"


def test_forecaster_set_precision_reaches_every_block():
    from gwen_amd.forecaster import InteractionForecaster
    m = InteractionForecaster(4, 32, 3)
    keys = list(m.state_dict())
    assert m.precision == "3xbf16"
    assert all(n.precision == "3xbf16" for n in (m.encoder, *m.processor, m.decoder))
    assert m.set_precision("f16x3") is m
    assert m.precision == "f16x3" and all(n.precision == "f16x3" for n in (m.encoder, *m.processor, m.decoder))
    assert list(m.state_dict()) == keys
    back = pickle.loads(pickle.dumps(m))
    assert back.precision == "f16x3" and all(n.precision == "f16x3" for n in (back.encoder, *back.processor, back.decoder))
    m2 = InteractionForecaster(4, 32, 3, precision="f16x3")
    m2.load_state_dict(InteractionForecaster(4, 32, 3).state_dict(), strict=True)
    assert m2.precision == "f16x3"
