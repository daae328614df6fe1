"""Edge attention and the graph-transformer block, the part that needs no GPU: the C ABI's shape rule and argument
checks, the fp64 restatement the GPU tests measure against (written here) with its closed forms, and the modules'
constructors, state_dict keys and pickling.  BUILD-DEFINED, PARITY UNPINNED."""
import math
import pickle

import pytest
import torch
import torch.nn.functional as TF

import gwen_amd.attention  # noqa: F401  (the feature under test: without it nothing in this file runs)
from helpers import SEED

EINVAL = -1

# ---- the restatement -------------------------------------------------------------------------------------------------------
# Plain torch (index_add_ / scatter_reduce) in the dtype of its inputs -- fp64 as the reference, fp32 on the CPU as the
# yardstick of the GPU tests' bounds (tests/test_gpu_attention.py imports it from here).  Never imported from the library.
# Edge lists are ``src``, ``dst`` int64 [E] in ANY order; ``ee`` [E, F] in that same order.
FWD_FLOOR, GRAD_FLOOR, YARD = 2e-6, 1e-5, 4.0     # the project's fp32-class bounds; the factor over torch's own fp32 error


def attention_ref(q, k, v, src, dst, heads, ee=None, parts=False):
    nd, f = q.shape
    e, d = src.numel(), f // heads
    kk, vv = k[src], v[src]
    if ee is not None:
        kk, vv = kk + ee, vv + ee
    sc = (q[dst].view(e, heads, d) * kk.view(e, heads, d)).sum(-1) / math.sqrt(d)
    idx = dst.view(-1, 1).expand(e, heads)
    with torch.no_grad():                         # (the softmax does not depend on the shift)
        mx = torch.full((nd, heads), -math.inf, dtype=q.dtype).scatter_reduce(0, idx, sc, "amax", include_self=True)
    ex = torch.exp(sc - mx[dst])
    den = torch.zeros(nd, heads, dtype=q.dtype).index_add_(0, dst, ex)
    p = ex / den[dst]
    out = torch.zeros(nd, heads, d, dtype=q.dtype).index_add_(0, dst, p.unsqueeze(-1) * vv.view(e, heads, d))
    out = out.view(nd, f)
    return (out, sc, p) if parts else out


def act_fn(name):
    return {"none": lambda t: t, "relu": torch.relu, "silu": TF.silu}[name]


def block_ref(x_src, x_dst, e, src, dst, p, heads, act="silu", eps=1e-5, same=False):
    """GraphTransformer.forward's x_dst' (``p``: the block's state_dict in the dtype of the inputs)"""
    f = x_dst.size(1)
    ln = lambda x, n: TF.layer_norm(x, (f,), p[n + ".weight"], p[n + ".bias"], eps)                     # noqa: E731
    hs = ln(x_src, "norm1")
    hd = hs if same else ln(x_dst, "norm1")
    q = hd @ p["lin_q.weight"].t() + p["lin_q.bias"]
    kv = hs @ p["lin_kv.weight"].t() + p["lin_kv.bias"]
    ee = e @ p["lin_e.weight"].t()
    a = attention_ref(q, kv[:, :f], kv[:, f:], src, dst, heads, ee)
    x1 = x_dst + a @ p["lin_o.weight"].t() + p["lin_o.bias"]
    h = act_fn(act)(ln(x1, "norm2") @ p["mlp.0.weight"].t() + p["mlp.0.bias"])
    return x1 + h @ p["mlp.2.weight"].t() + p["mlp.2.bias"]


def interaction_ref(x_src, x_dst, e, src, dst, p, act="silu"):
    """the plain InteractionNet block (sum aggregation, no LayerNorm): x_dst' only (encoder / decoder of the forecaster)"""
    mlp = lambda x, a, b: act_fn(act)(x @ p[a + ".0.weight"].t() + p[a + ".0.bias"]) @ p[a + ".2.weight"].t() \
        + p[a + ".2.bias"]                                                                             # noqa: E731
    m = mlp(torch.cat([e, x_src[src], x_dst[dst]], dim=1), "edge_mlp", None)
    agg = torch.zeros(x_dst.size(0), m.size(1), dtype=m.dtype).index_add_(0, dst, m)
    return x_dst + mlp(torch.cat([x_dst, agg], dim=1), "node_mlp", None)


def forecaster_ref(sd, grid_x, mesh_pos, g2m, mesh_ei, m2g, f_g2m, f_mesh, f_m2g, steps, heads, act="silu"):
    """one step of InteractionForecaster(processor="transformer")"""
    sub = lambda prefix: {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}            # noqa: E731
    lin = lambda x, name: x @ sd[name + ".weight"].t() + sd[name + ".bias"]                             # noqa: E731
    vg, vm = lin(grid_x, "grid_embed"), lin(mesh_pos, "mesh_embed")
    e_g2m, e_m, e_m2g = lin(f_g2m, "g2m_edge_embed"), lin(f_mesh, "mesh_edge_embed"), lin(f_m2g, "m2g_edge_embed")
    vm = interaction_ref(vg, vm, e_g2m, g2m[0], g2m[1], sub("encoder."), act)
    for k in range(steps):
        vm = block_ref(vm, vm, e_m, mesh_ei[0], mesh_ei[1], sub(f"processor.{k}."), heads, act, same=True)
    vg = interaction_ref(vm, vg, e_m2g, m2g[0], m2g[1], sub("decoder."), act)
    return grid_x + lin(vg, "readout")


def row_err(got, want) -> float:
    """the largest per-row max |got - want| / max |want|"""
    g, w = got.double().cpu(), want.double().cpu()
    if w.numel() == 0:
        return 0.0
    return float(((g - w).abs().amax(dim=1) / w.abs().amax(dim=1).clamp(min=1e-300)).max())


@pytest.mark.parametrize("F,H,ok", [
    (32, 1, 1), (32, 8, 1), (32, 16, 0), (64, 1, 1), (64, 4, 1), (64, 16, 1), (64, 32, 0), (64, 3, 0), (64, 0, 0),
    (64, -2, 0), (96, 4, 0), (128, 8, 1), (128, 32, 1), (128, 64, 0), (256, 1, 1), (256, 8, 1), (256, 64, 1),
    (256, 128, 0), (512, 8, 0), (16, 4, 0), (0, 1, 0)])
def test_supported_table(hip_lib, F, H, ok):
    assert hip_lib.gwen_edge_attention_supported(F, H) == ok
    from gwen_amd.attention import attention_supported
    assert attention_supported(F, H) == bool(ok)


def test_zero_sized_calls_and_null_arguments_without_gpu(hip_lib):
    L = hip_lib
    # zero-sized: GWEN_OK before any HIP call
    assert L.gwen_edge_attention_f32(None, 64, None, 64, None, 64, None, None, None, 0, 5, 0, 64, 4, None, None, None) == 0
    assert L.gwen_edge_attention_bwd_target_f32(None, 64, None, 64, None, 64, None, None, None, None, None, None, 0, 5, 0,
                                                64, 4, None, None, None, None, None) == 0
    assert L.gwen_edge_attention_bwd_source_f32(None, None, None, None, 64, None, None, None, 0, 7, 0, 64, 4, None, 64,
                                                None, 64, None) == 0
    # null arguments with rows to do: GWEN_EINVAL before any HIP call
    assert L.gwen_edge_attention_f32(None, 64, None, 64, None, 64, None, None, None, 7, 5, 9, 64, 4, None, None,
                                     None) == EINVAL
    assert L.gwen_edge_attention_bwd_target_f32(None, 64, None, 64, None, 64, None, None, None, None, None, None, 7, 5, 9,
                                                64, 4, None, None, None, None, None) == EINVAL
    assert L.gwen_edge_attention_bwd_source_f32(None, None, None, None, 64, None, None, None, 5, 7, 9, 64, 4, None, 64,
                                                None, 64, None) == EINVAL
    # unsupported shapes, negative sizes, a row stride below F or no multiple of 4, a misaligned pointer
    assert L.gwen_edge_attention_f32(None, 64, None, 64, None, 64, None, None, None, 0, 5, 0, 64, 3, None, None,
                                     None) == EINVAL
    assert L.gwen_edge_attention_f32(None, 64, None, 64, None, 64, None, None, None, -1, 5, 0, 64, 4, None, None,
                                     None) == EINVAL
    for ldq, q in ((32, 64), (66, 64), (64, 68)):
        assert L.gwen_edge_attention_f32(q, ldq, 64, 64, 64, 64, None, 64, 64, 7, 5, 9, 64, 4, 128, 128, None) == EINVAL
    # sizes whose indices do not fit int32
    assert L.gwen_edge_attention_f32(64, 64, 64, 64, 64, 64, None, 64, 64, 7, 5, 2 ** 31, 64, 4, 128, 128, None) == -2
    assert L.gwen_edge_attention_bwd_source_f32(64, 64, 64, 64, 64, 64, 64, 64, 2 ** 31, 7, 9, 64, 4, 128, 64, 256, 64,
                                                None) == -2


# ---- closed forms of the restatement ------------------------------------------------------------------------------------
def _random_graph(ns, nd, e, seed=SEED):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, ns, (e,), generator=g), torch.randint(0, nd, (e,), generator=g)


def test_restatement_zero_keys_give_the_mean_of_v():
    ns, nd, F, H = 11, 9, 32, 8
    src, dst = _random_graph(ns, nd, 60)
    dst[dst == 4] = 5                                             # target 4 has no in-edge
    g = torch.Generator().manual_seed(SEED + 1)
    q = torch.randn(nd, F, generator=g, dtype=torch.float64)
    v = torch.randn(ns, F, generator=g, dtype=torch.float64)
    out = attention_ref(q, torch.zeros(ns, F, dtype=torch.float64), v, src, dst, H)
    deg = torch.zeros(nd, dtype=torch.float64).index_add_(0, dst, torch.ones(60, dtype=torch.float64))
    mean = torch.zeros(nd, F, dtype=torch.float64).index_add_(0, dst, v[src]) / deg.clamp(min=1).view(-1, 1)
    assert float((out - mean).abs().max()) < 1e-14
    assert deg[4] == 0 and float(out[4].abs().max()) == 0.0


def test_restatement_one_in_edge_gives_v_plus_ee():
    ns, nd, F, H = 6, 6, 64, 4
    src, dst = torch.tensor([2, 0, 5]), torch.tensor([1, 3, 4])
    g = torch.Generator().manual_seed(SEED + 2)
    q, k, v = (torch.randn(n, F, generator=g, dtype=torch.float64) for n in (nd, ns, ns))
    ee = torch.randn(3, F, generator=g, dtype=torch.float64)
    out = attention_ref(q, k, v, src, dst, H, ee)
    assert torch.equal(out[dst], v[src] + ee)
    assert float(out[[0, 2, 5]].abs().max()) == 0.0


def test_restatement_logit_gradients_sum_to_zero_per_target():
    """d loss / d sc summed over a target's in-edges is 0 for every head (the softmax is shift-invariant)."""
    ns, nd, F, H = 13, 7, 32, 4
    src, dst = _random_graph(ns, nd, 80)
    g = torch.Generator().manual_seed(SEED + 3)
    q, k, v = (torch.randn(n, F, generator=g, dtype=torch.float64, requires_grad=True) for n in (nd, ns, ns))
    ee = torch.randn(80, F, generator=g, dtype=torch.float64)
    out, sc, p = attention_ref(q, k, v, src, dst, H, ee, parts=True)
    sc.retain_grad()
    (out * torch.randn(nd, F, generator=g, dtype=torch.float64)).sum().backward()
    tot = torch.zeros(nd, H, dtype=torch.float64).index_add_(0, dst, sc.grad)
    assert float(tot.abs().max()) < 1e-13 * max(1.0, float(sc.grad.abs().max()))
    rows = torch.zeros(nd, H, dtype=torch.float64).index_add_(0, dst, p.detach())
    has = torch.zeros(nd, dtype=torch.bool).index_fill_(0, dst, True)
    assert float((rows[has] - 1).abs().max()) < 1e-14


# ---- modules ------------------------------------------------------------------------------------------------------------
BLOCK_KEYS = ["norm1.weight", "norm1.bias", "lin_q.weight", "lin_q.bias", "lin_kv.weight", "lin_kv.bias", "lin_e.weight",
              "lin_o.weight", "lin_o.bias", "norm2.weight", "norm2.bias", "mlp.0.weight", "mlp.0.bias", "mlp.2.weight",
              "mlp.2.bias"]
INET_KEYS = [f"{m}.{i}.{p}" for m in ("edge_mlp", "node_mlp") for i in (0, 2) for p in ("weight", "bias")]
EMBED_KEYS = [f"{m}.{p}" for m in ("grid_embed", "mesh_embed", "g2m_edge_embed", "mesh_edge_embed", "m2g_edge_embed")
              for p in ("weight", "bias")]


def test_block_constructor_errors(hip_lib):
    from gwen_amd import GraphTransformer
    for bad in [(64, 3), (64, 32), (96, 4), (64, 0), (64, 4.0)]:
        with pytest.raises(ValueError):
            GraphTransformer(*bad)
    with pytest.raises(ValueError):
        GraphTransformer(64, 4, activation="gelu")
    with pytest.raises(ValueError):
        GraphTransformer(64, 4, precision="fp16")
    net = GraphTransformer(64, 4)
    with pytest.raises(ValueError):
        net.precision = "bf16x6"
    net.precision = "f16x3"
    assert net.precision == "f16x3"


def test_block_state_dict_and_pickle(hip_lib):
    from gwen_amd import GraphTransformer
    torch.manual_seed(SEED)
    net = GraphTransformer(64, 4, precision="f16x3", norm_eps=1e-6)
    sd = net.state_dict()
    assert list(sd) == BLOCK_KEYS
    assert tuple(sd["lin_kv.weight"].shape) == (128, 64) and tuple(sd["lin_e.weight"].shape) == (64, 64)
    back = pickle.loads(pickle.dumps(net))
    assert list(back.state_dict()) == BLOCK_KEYS and back.precision == "f16x3" and back.heads == 4
    assert back.norm1.eps == 1e-6 and all(torch.equal(a, b) for a, b in zip(sd.values(), back.state_dict().values()))


def test_forecaster_keys(hip_lib):
    from gwen_amd import InteractionForecaster
    want = EMBED_KEYS + [f"encoder.{k}" for k in INET_KEYS] \
        + [f"processor.{i}.{k}" for i in range(2) for k in INET_KEYS] + [f"decoder.{k}" for k in INET_KEYS] \
        + ["readout.weight", "readout.bias"]
    assert list(InteractionForecaster(8, 64, 2).state_dict()) == want          # the default: unchanged
    assert list(InteractionForecaster(8, 64, 2, processor="interaction", heads=4).state_dict()) == want
    model = InteractionForecaster(8, 64, 2, processor="transformer", heads=4, noise_channels=16, layer_norm=True)
    norms = [f"{n}.{p}" for n in ("edge_norm", "node_norm") for p in ("weight", "bias")]
    want_t = EMBED_KEYS + [f"encoder.{k}" for k in INET_KEYS + norms] \
        + [f"processor.{i}.{k}" for i in range(2) for k in BLOCK_KEYS] + [f"decoder.{k}" for k in INET_KEYS + norms] \
        + ["readout.weight", "readout.bias", "noise_embed.weight"]
    assert list(model.state_dict()) == want_t
    assert all(b.heads == 4 and b.precision == "3xbf16" for b in model.processor)
    model.set_precision("f16x3")
    assert all(b.precision == "f16x3" for b in model.processor) and model.encoder.precision == "f16x3"
    back = pickle.loads(pickle.dumps(model))
    assert list(back.state_dict()) == want_t and back.processor_kind == "transformer"
    with pytest.raises(ValueError):
        InteractionForecaster(8, 64, 2, processor="gcn")
    with pytest.raises(ValueError):
        InteractionForecaster(8, 64, 2, processor="transformer", heads=3)


def _cpu_graph(ns, nd, src, dst):
    from gwen_amd import EdgeGraph
    order = torch.sort(dst, stable=True).indices
    rowptr = torch.zeros(nd + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(torch.bincount(dst, minlength=nd), 0).to(torch.int32)
    return EdgeGraph(ns, nd, src.numel(), rowptr, src[order].int(), dst[order].int(), order.int(), 0)


def test_argument_errors_on_the_cpu(hip_lib):
    from gwen_amd import GraphTransformer, edge_attention, edge_attention_kv
    src, dst = _random_graph(5, 6, 12)
    graph = _cpu_graph(5, 6, src, dst)
    q, k, v, ee = torch.randn(6, 64), torch.randn(5, 64), torch.randn(5, 64), torch.randn(12, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        edge_attention(q, k, v, graph, 4, ee)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        edge_attention_kv(q, torch.randn(5, 128), graph, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GraphTransformer(64, 4)(k, q, ee, graph)
