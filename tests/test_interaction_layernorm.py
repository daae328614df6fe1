"""Host and C-ABI side of the InteractionNet block's LayerNorm option (CPU only: nothing here launches a kernel)."""
import pickle

import pytest
import torch

KEYS = ["edge_mlp.0.weight", "edge_mlp.0.bias", "edge_mlp.2.weight", "edge_mlp.2.bias",
        "node_mlp.0.weight", "node_mlp.0.bias", "node_mlp.2.weight", "node_mlp.2.bias"]
NORM_KEYS = ["edge_norm.weight", "edge_norm.bias", "node_norm.weight", "node_norm.bias"]


def test_off_by_default_and_four_keys_when_on():
    from gwen_amd.interaction import InteractionNet
    plain, off, on = InteractionNet(64), InteractionNet(64, layer_norm=False), InteractionNet(64, layer_norm=True)
    assert plain.layer_norm is False and off.layer_norm is False and on.layer_norm is True
    assert list(plain.state_dict()) == KEYS and list(off.state_dict()) == KEYS
    assert list(on.state_dict()) == KEYS + NORM_KEYS
    sd = on.state_dict()
    for k in ("edge_norm", "node_norm"):
        assert torch.equal(sd[k + ".weight"], torch.ones(64)) and torch.equal(sd[k + ".bias"], torch.zeros(64))
    assert isinstance(on.edge_norm, torch.nn.LayerNorm) and on.edge_norm.eps == 1e-5
    assert InteractionNet(32, layer_norm=True, norm_eps=1e-3).node_norm.eps == 1e-3
    assert len(list(on.parameters())) == 12 and len(list(plain.parameters())) == 8


def test_plain_state_dict_loads_with_strict_false():
    from gwen_amd.interaction import InteractionNet
    plain, on = InteractionNet(64), InteractionNet(64, layer_norm=True)
    res = on.load_state_dict(plain.state_dict(), strict=False)
    assert sorted(res.missing_keys) == sorted(NORM_KEYS) and not res.unexpected_keys
    assert all(torch.equal(on.state_dict()[k], plain.state_dict()[k]) for k in KEYS)
    assert torch.equal(on.edge_norm.weight, torch.ones(64)) and torch.equal(on.node_norm.bias, torch.zeros(64))
    with pytest.raises(RuntimeError):
        on.load_state_dict(plain.state_dict(), strict=True)


def test_pickle_keeps_the_setting_and_old_pickles_read_as_off():
    from gwen_amd.interaction import InteractionNet
    on = InteractionNet(64, precision="f16x3", layer_norm=True, norm_eps=1e-4)
    back = pickle.loads(pickle.dumps(on))
    assert back.layer_norm is True and back.precision == "f16x3" and back.edge_norm.eps == 1e-4
    assert list(back.state_dict()) == KEYS + NORM_KEYS
    assert pickle.loads(pickle.dumps(InteractionNet(64))).layer_norm is False
    old = InteractionNet(64)
    del old.__dict__["_layer_norm"]                       # a module pickled before the setting existed
    assert pickle.loads(pickle.dumps(old)).layer_norm is False


def test_forecaster_hands_the_option_to_every_block():
    from gwen_amd.forecaster import InteractionForecaster
    steps = 3
    off = InteractionForecaster(4, 32, steps)
    on = InteractionForecaster(4, 32, steps, layer_norm=True, norm_eps=1e-6)
    blocks = (on.encoder, *on.processor, on.decoder)
    assert len(blocks) == steps + 2 and all(b.layer_norm for b in blocks)
    assert all(b.edge_norm.eps == 1e-6 and b.node_norm.eps == 1e-6 for b in blocks)
    assert not any(b.layer_norm for b in (off.encoder, *off.processor, off.decoder))
    assert not any("norm" in k for k in off.state_dict())
    added = [k for k in on.state_dict() if k not in off.state_dict()]
    assert len(added) == 4 * (steps + 2) and all(k.rsplit(".", 2)[-2] in ("edge_norm", "node_norm") for k in added)
    # the embedders and the read-out stay plain Linears
    for name in ("grid_embed", "mesh_embed", "g2m_edge_embed", "mesh_edge_embed", "m2g_edge_embed", "readout"):
        assert type(getattr(on, name)) is torch.nn.Linear
    back = pickle.loads(pickle.dumps(on))
    assert all(b.layer_norm for b in (back.encoder, *back.processor, back.decoder))


def test_mlp2_refuses_bad_layer_norm_arguments():
    from gwen_amd.interaction import mlp2
    a, w = torch.zeros(4, 64), torch.zeros(64, 64)
    g, b = torch.ones(64), torch.zeros(64)
    with pytest.raises(ValueError, match="together"):
        mlp2(a, w, w, ln_weight=g)
    with pytest.raises(ValueError, match="together"):
        mlp2(a, w, w, ln_bias=b)
    with pytest.raises(ValueError, match=r"\[F\]"):
        mlp2(a, w, w, ln_weight=torch.ones(32), ln_bias=b)
    with pytest.raises(ValueError, match=r"\[F\]"):
        mlp2(a, w, w, ln_weight=g, ln_bias=torch.zeros(64, 1))
    with pytest.raises(RuntimeError, match="HIP device"):          # CPU tensors: no CPU fallback
        mlp2(a, w, w, ln_weight=g, ln_bias=b)


def test_layer_norm_op_refuses_bad_arguments(hip_lib):
    from gwen_amd import ops
    g, b = torch.ones(64), torch.zeros(64)
    with pytest.raises(ValueError):
        ops.layer_norm(torch.zeros(4, 6), torch.ones(6), torch.zeros(6))            # F % 4
    with pytest.raises(ValueError):
        ops.layer_norm(torch.zeros(4, 1028), torch.ones(1028), torch.zeros(1028))   # F > 1024
    with pytest.raises(ValueError):
        ops.layer_norm(torch.zeros(4, 64), torch.ones(32), b)
    with pytest.raises(ValueError):
        ops.layer_norm(torch.zeros(4, 64), g, b, res=torch.zeros(5, 64))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.layer_norm(torch.zeros(4, 64), g, b)


def test_new_entries_are_exported_and_bound(hip_lib):
    from gwen_amd import _lib
    for name in ("gwen_mlp2_ln_f32", "gwen_mlp2_ln_supported", "gwen_layer_norm_supported", "gwen_layer_norm_f32",
                 "gwen_layer_norm_bwd_chunks", "gwen_layer_norm_bwd_f32"):
        assert hasattr(hip_lib, name) and name in _lib.SIGNATURES


def test_supported_queries(hip_lib):
    from gwen_amd import _lib
    L = hip_lib
    for c in (_lib.CONTRACT_BF16X3, _lib.CONTRACT_F16X3):
        for f in (32, 128, 48, 512, 0):                           # no fused instantiation: the unfused route
            assert L.gwen_mlp2_ln_supported(f, c, _lib.MLP2_LN_EDGE) == 0
            assert L.gwen_mlp2_ln_supported(f, c, _lib.MLP2_LN_NODE) == 0
        for f in (64, 256):
            assert L.gwen_mlp2_ln_supported(f, c, 2) == 0 and L.gwen_mlp2_ln_supported(f, c, -1) == 0
            assert L.gwen_mlp2_ln_supported(f, c, _lib.MLP2_LN_EDGE) in (0, 1)
    for c in (_lib.CONTRACT_F32, _lib.CONTRACT_BF16X6, 7):
        assert L.gwen_mlp2_ln_supported(64, c, _lib.MLP2_LN_EDGE) == 0
    for f in (4, 36, 64, 256, 1000, 1024):
        assert L.gwen_layer_norm_supported(f) == 1
    for f in (0, -4, 6, 1028, 2048):
        assert L.gwen_layer_norm_supported(f) == 0
    assert L.gwen_layer_norm_bwd_chunks(0) == 0 and L.gwen_layer_norm_bwd_chunks(1) == 1
    assert L.gwen_layer_norm_bwd_chunks(256) == 1 and L.gwen_layer_norm_bwd_chunks(257) == 2
    assert L.gwen_layer_norm_bwd_chunks(-1) == -1


def test_new_launches_refuse_before_touching_a_device(hip_lib):
    from gwen_amd import _lib
    L = hip_lib
    fake = 4096                                     # never dereferenced: the calls must return before any launch

    def k6(F, contract, gamma=fake, beta=fake, **kw):
        a = dict(G1=None, idx1=None, G2=None, idx2=None, res=None, agg=None)
        a.update(kw)
        return L.gwen_mlp2_ln_f32(fake, fake, a["G1"], a["idx1"], 10, F, a["G2"], a["idx2"], 10, F, None, fake, None,
                                  a["res"], fake, 10, F, 0, fake if a["agg"] else None, fake if a["agg"] else None,
                                  1 if a["agg"] else 0, a["agg"], 5 if a["agg"] else 0, 0, contract, gamma, beta, 1e-5,
                                  None, 0, None)

    for c in (_lib.CONTRACT_F32, _lib.CONTRACT_BF16X6, 7, -1):
        assert k6(64, c) == -1
    for c in (_lib.CONTRACT_BF16X3, _lib.CONTRACT_F16X3):
        assert k6(48, c) == -1 and k6(512, c) == -1
        assert k6(64, c, gamma=fake, beta=None) == -1 and k6(64, c, gamma=None, beta=fake) == -1
        assert k6(64, c) == -1                                     # gamma on a launch shape without an instantiation
        # the block's launch shapes at 32 / 128 channels have none either: Python takes the unfused route
        assert k6(32, c, G1=fake, idx1=fake, G2=fake, idx2=fake, res=fake, agg=fake) == -1
        assert k6(128, c, G1=fake, res=2 * fake) == -1
    fwd = lambda rows, F, **kw: L.gwen_layer_norm_f32(                                            # noqa: E731
        fake, kw.get("gamma", fake), kw.get("beta", fake), kw.get("eps", 1e-5), None, kw.get("out", fake), rows, F,
        kw.get("rowptr"), kw.get("agg"), kw.get("n", 0), 0, None)
    bwd = lambda rows, F, **kw: L.gwen_layer_norm_bwd_f32(                                        # noqa: E731
        fake, fake, kw.get("gamma", fake), 1e-5, kw.get("gx", 2 * fake), None, rows, F, None)
    for f in (0, 6, 1028):
        assert fwd(10, f) == -1 and bwd(10, f) == -1
    assert fwd(-1, 64) == -1 and bwd(-1, 64) == -1
    assert fwd(10, 64, gamma=None) == -1 and fwd(10, 64, beta=None) == -1 and fwd(10, 64, out=None) == -1
    assert fwd(10, 64, eps=-1.0) == -1 and fwd(10, 64, agg=fake, n=3) == -1      # agg without rowptr
    assert fwd(10, 64, out=fake + 4) == -1                                       # alignment
    assert bwd(10, 64, gamma=None) == -1 and bwd(10, 64, gx=fake) == -1          # gx may not alias x
    assert fwd(0, 64) == 0 and bwd(0, 64) == 0                                   # nothing to do
