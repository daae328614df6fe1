"""Graph-transformer block on the fused edge-attention kernel (csrc/attention.hip).

BUILD-DEFINED, PARITY UNPINNED -- the reference's only graph layer is GCNConv (/root/reference/src/gwen/models_gnn.py:
118-130); it has no attention.  Semantics are PyG ``TransformerConv``'s with ``edge_dim`` (the processor the published
encode-process-decode weather models ship beside the InteractionNet one), restated in fp64 by the tests.  With H heads,
D = F / H and s(e) / d(e) the source / target of stored edge e:

    sc[e,h]  = (1 / sqrt(D)) sum_{c in head h} q[d(e),c] (k[s(e),c] + ee[e,c])
    p[e,h]   = softmax of sc[.,h] over the in-edges of d(e)          (running-maximum form: nothing overflows)
    out[d,c] = sum_{e into d} p[e,h(c)] (v[s(e),c] + ee[e,c])        (no in-edges: 0)

``edge_attention`` is that op: ONE launch forward (no [E, F] intermediate, no atomics), two launches backward -- pass T
per target (gq, gee and the per-edge P, DS [E, H]) and pass S per source over ``EdgeGraph.segments("src")`` (gk, gv) --
all in fixed summation orders: two runs are bitwise equal.  fp32 on every precision tier.

``GraphTransformer`` is the pre-norm block around it, with InteractionNet's call shape:

    hs, hd   = norm1(x_src), norm1(x_dst)                                   (once when x_src is x_dst)
    q        = lin_q(hd);  [k | v] = lin_kv(hs);  ee = lin_e(e)             (lin_e: no bias)
    x1       = x_dst + lin_o(edge_attention(q, k, v, graph, heads, ee))
    x_dst'   = x1 + mlp.2(act(mlp.0(norm2(x1))))

Edge features (``ee`` and ``e``) live in the graph's STORED order, as everywhere (``EdgeGraph.sort_edges``).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor, nn
from torch.autograd.function import once_differentiable

from . import _lib, ops
from .graph import _ptr, _stream
from .interaction import _ACT, EdgeGraph, _act_pair, _ew, _mlp2_contract, mlp2


def attention_supported(channels: int, heads: int) -> bool:
    """gwen_edge_attention_supported: channels in (32, 64, 128, 256), heads a power of two, channels / heads >= 4."""
    return bool(_lib.lib().gwen_edge_attention_supported(int(channels), int(heads)))


def _table(name: str, t: Tensor, rows: int, f: int) -> None:
    """A node table may be a column block of a wider row-major matrix (mlp2's rule for its gathered tables)."""
    if t.dim() != 2 or t.size(0) != rows or t.size(1) != f:
        raise ValueError(f"edge_attention: {name} must be [{rows}, {f}]; got {tuple(t.shape)}")
    if rows > 0 and (t.stride(1) != 1 or t.stride(0) % 4 or t.stride(0) < f or t.data_ptr() % 16):
        raise ValueError(f"edge_attention: {name} must have unit column stride and 16-byte aligned rows")


def _check(q: Tensor, k: Tensor, v: Optional[Tensor], graph: EdgeGraph, heads: int, ee: Optional[Tensor]) -> int:
    for name, t in (("q", q), ("k", k), ("v", v), ("ee", ee)):
        if t is not None:
            ops._require(t, name)
    if q.dim() != 2:
        raise ValueError(f"edge_attention: q must be [num_dst, F]; got {tuple(q.shape)}")
    f = q.size(1)
    if not isinstance(heads, int) or not attention_supported(f, heads):
        raise ValueError(f"edge_attention needs F in (32, 64, 128, 256) and heads a power of two with F / heads >= 4; "
                         f"got F = {f}, heads = {heads}")
    _table("q", q, graph.num_dst, f)
    if v is None:
        _table("kv", k, graph.num_src, 2 * f)
    else:
        _table("k", k, graph.num_src, f)
        _table("v", v, graph.num_src, f)
    if ee is not None and tuple(ee.shape) != (graph.num_edges, f):
        raise ValueError(f"edge_attention: ee must be [{graph.num_edges}, {f}] (stored edge order); got {tuple(ee.shape)}")
    return f


def _ld(t: Tensor, f: int) -> int:
    return t.stride(0) if t.size(0) > 1 else max(t.stride(0), f) // 4 * 4


def _forward(q: Tensor, k: Tensor, v: Tensor, ee: Optional[Tensor], graph: EdgeGraph, heads: int):
    f, dev = q.size(1), q.device
    out = torch.empty(graph.num_dst, f, dtype=torch.float32, device=dev)
    lse = torch.empty(graph.num_dst, heads, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().gwen_edge_attention_f32(
            _ptr(q), _ld(q, f), _ptr(k), _ld(k, f), _ptr(v), _ld(v, f), _ptr(ee), _ptr(graph.rowptr), _ptr(graph.src),
            graph.num_dst, graph.num_src, graph.num_edges, f, heads, _ptr(out), _ptr(lse), _stream(dev))
    _lib.check(rc, "gwen_edge_attention_f32")
    return out, lse


class _EdgeAttentionFunction(torch.autograd.Function):
    """``edge_attention`` with autograd: saves q, k, v, ee, out, lse; the backward is pass T and pass S of
    csrc/attention.hip (p is recomputed from lse; atomic-free, reproducible).  ``v`` None: ``k`` is the stacked
    [num_src, 2F] projection [k | v], and its gradient comes back as ONE [num_src, 2F] array."""

    @staticmethod
    def forward(ctx, graph: EdgeGraph, heads: int, q: Tensor, k: Tensor, v: Optional[Tensor], ee: Optional[Tensor]):
        f = q.size(1)
        kk, vv = (k[:, :f], k[:, f:]) if v is None else (k, v)
        out, lse = _forward(q, kk, vv, ee, graph, heads)
        ctx.graph, ctx.heads = graph, heads
        ctx.save_for_backward(q, k, v, ee, out, lse)
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        q, k, v, ee, out, lse = ctx.saved_tensors
        graph, heads = ctx.graph, ctx.heads
        f, dev = q.size(1), q.device
        n_dst, n_src, e = graph.num_dst, graph.num_src, graph.num_edges
        stacked = v is None
        kk, vv = (k[:, :f], k[:, f:]) if stacked else (k, v)
        g = g.contiguous()
        L = _lib.lib()
        gq = torch.empty(n_dst, f, dtype=torch.float32, device=dev)
        gee = None if ee is None else torch.empty_like(ee)
        p = torch.empty(e, heads, dtype=torch.float32, device=dev)
        ds = torch.empty(e, heads, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = L.gwen_edge_attention_bwd_target_f32(
                _ptr(q), _ld(q, f), _ptr(kk), _ld(kk, f), _ptr(vv), _ld(vv, f), _ptr(ee), _ptr(graph.rowptr),
                _ptr(graph.src), _ptr(g), _ptr(out), _ptr(lse), n_dst, n_src, e, f, heads, _ptr(gq), _ptr(gee),
                _ptr(p), _ptr(ds), _stream(dev))
        _lib.check(rc, "gwen_edge_attention_bwd_target_f32")
        need = ctx.needs_input_grad
        gk = gv = None
        if need[3] or (not stacked and need[4]):
            rowptr, col, _ = graph.segments("src")
            if stacked:
                gk = torch.empty(n_src, 2 * f, dtype=torch.float32, device=dev)
                ok, ov = gk[:, :f], gk[:, f:]
            else:
                ok = gk = torch.empty(n_src, f, dtype=torch.float32, device=dev)
                ov = gv = torch.empty(n_src, f, dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                rc = L.gwen_edge_attention_bwd_source_f32(
                    _ptr(rowptr), _ptr(col), _ptr(graph.dst), _ptr(q), _ld(q, f), _ptr(g), _ptr(p), _ptr(ds), n_src,
                    n_dst, e, f, heads, _ptr(ok), _ld(ok, f), _ptr(ov), _ld(ov, f), _stream(dev))
            _lib.check(rc, "gwen_edge_attention_bwd_source_f32")
        pick = lambda i, t: t if need[i] else None                                          # noqa: E731
        return None, None, pick(2, gq), pick(3, gk), None if stacked else pick(4, gv), pick(5, gee)


def _run(q: Tensor, k: Tensor, v: Optional[Tensor], graph: EdgeGraph, heads: int, ee: Optional[Tensor]) -> Tensor:
    f = _check(q, k, v, graph, heads, ee)
    if ee is not None:
        ee = ee.contiguous()
        if ee.data_ptr() % 16:
            raise ValueError("edge_attention: ee must be 16-byte aligned")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (q, k, v, ee)):
        return _EdgeAttentionFunction.apply(graph, heads, q, k, v, ee)
    kk, vv = (k[:, :f], k[:, f:]) if v is None else (k, v)
    return _forward(q, kk, vv, ee, graph, heads)[0]


def edge_attention(q: Tensor, k: Tensor, v: Tensor, graph: EdgeGraph, heads: int, ee: Optional[Tensor] = None) -> Tensor:
    """Multi-head attention of every target over its in-edges (module docstring): ``q`` [num_dst, F], ``k`` / ``v``
    [num_src, F], ``ee`` [E, F] in stored edge order or None (= 0) -> [num_dst, F].  fp32; F in (32, 64, 128, 256),
    ``heads`` a power of two with F / heads >= 4.  q, k, v may be column blocks of a wider row-major matrix (unit column
    stride, row stride a multiple of 4, 16-byte aligned).  Differentiable in q, k, v and ee."""
    if v is None:
        raise ValueError("edge_attention: v is required (edge_attention_kv takes the stacked [k | v])")
    return _run(q, k, v, graph, heads, ee)


def edge_attention_kv(q: Tensor, kv: Tensor, graph: EdgeGraph, heads: int, ee: Optional[Tensor] = None) -> Tensor:
    """``edge_attention(q, kv[:, :F], kv[:, F:], ..)`` for the stacked projection ``kv`` = [k | v] [num_src, 2F] of one K3
    launch: the same bits, and the backward writes gk | gv into ONE [num_src, 2F] array -- K3's backward reads it as is."""
    return _run(q, kv, None, graph, heads, ee)


class _ActFunction(torch.autograd.Function):
    """act(x) with autograd on gwen_act_pair_f32 (value and derivative from one pass) and gwen_ew_f32."""

    @staticmethod
    def forward(ctx, x: Tensor, act: str) -> Tensor:
        h, d = _act_pair(x.contiguous().clone(), act)
        ctx.save_for_backward(d)
        return h

    @staticmethod
    def backward(ctx, g: Tensor):
        (d,) = ctx.saved_tensors
        return _ew(_lib.EW_MUL, g.contiguous().clone(), d), None


class _FeedForwardFunction(torch.autograd.Function):
    """x1 + mlp.2(act(mlp.0(norm2(x1)))) with autograd.  The forward is the launch set the block takes without
    gradients -- the LayerNorm kernel and ONE K6 launch (mlp2 with the residual) -- so a training forward and an inference
    forward are the same bits; it saves x1 and the six parameters, nothing hidden-sized.  The backward forms the half
    again piece by piece (``GraphTransformer._feed_forward_pieces``: LayerNorm, K3, activation, K3, each with its own
    autograd Function on libgwen_hip.so) and differentiates that."""

    @staticmethod
    def forward(ctx, net, x1: Tensor, *params) -> Tensor:
        ctx.net = net
        ctx.save_for_backward(x1, *params)
        return net._feed_forward_fused(x1)

    @staticmethod
    @once_differentiable
    def backward(ctx, g: Tensor):
        x1, *params = ctx.saved_tensors
        needs = ctx.needs_input_grad[1:]
        with torch.enable_grad():
            xd = x1.detach().requires_grad_(needs[0])
            y = ctx.net._feed_forward_pieces(xd)
        wanted = [t for t, n in zip([xd, *ctx.net._feed_forward_parameters()], needs) if n]
        grads = iter(torch.autograd.grad(y, wanted, g, allow_unused=True))
        return (None,) + tuple(next(grads) if n else None for n in needs)


class GraphTransformer(nn.Module):
    """``forward(x_src, x_dst, e, graph, update_edges=True, ee=None) -> (x_dst', e)`` (module docstring); edges are not
    updated: ``e`` is returned as given (None with ``update_edges=False``, as InteractionNet).  ``ee=``: the edge term
    lin_e(e) computed by the caller (it depends on weights and static edge features only: the forecaster forms it
    once per rollout); ``lin_e`` is then skipped.

    Parameters: ``norm1, lin_q, lin_kv, lin_e, lin_o, norm2, mlp.0, mlp.2`` (lin_kv.weight [2F, F]: rows k, then v;
    lin_e has no bias).  ``precision`` ("3xbf16", the default, or "f16x3": fp32-class) governs every K3 / K6 contraction
    of the block, as in InteractionNet; the attention kernel, the LayerNorms and the residuals are fp32 on both.  A
    setting, not a parameter.  The feed-forward half is ONE K6 launch (mlp2 with the residual), with gradients too
    (``_FeedForwardFunction``: its backward forms the half again piece by piece), so the block computes the same bits
    with and without gradients; every other piece runs through its own autograd Function on libgwen_hip.so."""

    def __init__(self, channels: int, heads: int, activation: str = "silu", precision: str = "3xbf16",
                 norm_eps: float = 1e-5):
        super().__init__()
        if activation not in _ACT:
            raise ValueError("activation in (none, relu, silu)")
        if not isinstance(heads, int) or not attention_supported(channels, heads):
            raise ValueError(f"GraphTransformer needs channels in (32, 64, 128, 256) and heads a power of two with "
                             f"channels / heads >= 4; got channels = {channels}, heads = {heads}")
        self.channels, self.heads, self.activation = channels, heads, activation
        self.precision = precision
        f = channels
        self.norm1 = nn.LayerNorm(f, eps=norm_eps)
        self.lin_q = nn.Linear(f, f)
        self.lin_kv = nn.Linear(f, 2 * f)
        self.lin_e = nn.Linear(f, f, bias=False)
        self.lin_o = nn.Linear(f, f)
        self.norm2 = nn.LayerNorm(f, eps=norm_eps)
        a = {"none": nn.Identity, "relu": nn.ReLU, "silu": nn.SiLU}[activation]()
        self.mlp = nn.Sequential(nn.Linear(f, f), a, nn.Linear(f, f))

    @property
    def precision(self) -> str:
        return self.__dict__.get("_precision", "3xbf16")

    @precision.setter
    def precision(self, p: str) -> None:
        _mlp2_contract(p)
        self._precision = p

    def _lin(self, x: Tensor, m: nn.Linear, grad: bool) -> Tensor:
        """K3 on the block's precision; with autograd when gradients are needed."""
        if grad:
            return ops.linear_autograd(x, m.weight, m.bias, contract=self.precision)
        return ops.linear(x, m.weight, m.bias, contract=self.precision)

    def edge_term(self, e: Tensor) -> Tensor:
        """ee = lin_e(e) [E, F] (K3 on the block's precision; with autograd when gradients are needed)."""
        grad = torch.is_grad_enabled() and (e.requires_grad or self.lin_e.weight.requires_grad)
        return self._lin(e, self.lin_e, grad)

    def forward(self, x_src: Tensor, x_dst: Tensor, e: Optional[Tensor], graph: EdgeGraph, update_edges: bool = True,
                ee: Optional[Tensor] = None) -> Tuple[Tensor, Optional[Tensor]]:
        f = self.channels
        if x_src.shape != (graph.num_src, f) or x_dst.shape != (graph.num_dst, f) or \
                (e is not None and e.shape != (graph.num_edges, f)) or (e is None and ee is None):
            raise ValueError("x_src / x_dst / e do not match the graph and the channel count")
        grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad
                                               for t in (x_src, x_dst, e, ee, *self.parameters()))
        n1 = self.norm1
        if ee is None:
            ee = self._lin(e, self.lin_e, grad)
        if grad:
            hs = ops.layer_norm(x_src, n1.weight, n1.bias, n1.eps)
            hd = hs if x_src is x_dst else ops.layer_norm(x_dst, n1.weight, n1.bias, n1.eps)
        else:
            hs = ops.layer_norm_rows(x_src, n1.weight, n1.bias, n1.eps)[0]
            hd = hs if x_src is x_dst else ops.layer_norm_rows(x_dst, n1.weight, n1.bias, n1.eps)[0]
        q = self._lin(hd, self.lin_q, grad)
        kv = self._lin(hs, self.lin_kv, grad)
        att = edge_attention_kv(q, kv, graph, self.heads, ee)
        o = self._lin(att, self.lin_o, grad)
        if grad:
            x_new = _FeedForwardFunction.apply(self, x_dst + o, *self._feed_forward_parameters())
        else:
            x_new = self._feed_forward_fused(_ew(_lib.EW_ADD, o, x_dst.contiguous()))
        return x_new, (e if update_edges else None)

    def _feed_forward_parameters(self):
        return (self.norm2.weight, self.norm2.bias, self.mlp[0].weight, self.mlp[0].bias, self.mlp[2].weight,
                self.mlp[2].bias)

    def _feed_forward_fused(self, x1: Tensor) -> Tensor:
        """x1 + mlp.2(act(mlp.0(norm2(x1)))) without autograd: the LayerNorm kernel and ONE K6 launch."""
        n2 = self.norm2
        x1 = x1.contiguous()
        h2 = ops.layer_norm_rows(x1, n2.weight, n2.bias, n2.eps)[0]
        return mlp2(h2, self.mlp[0].weight, self.mlp[2].weight, self.mlp[2].bias, b1=self.mlp[0].bias, res=x1,
                    act=self.activation, contract=self.precision)[0]

    def _feed_forward_pieces(self, x1: Tensor) -> Tensor:
        """The same half under autograd, every piece through its own Function (the backward of ``_FeedForwardFunction``)."""
        n2 = self.norm2
        h = self._lin(ops.layer_norm(x1, n2.weight, n2.bias, n2.eps), self.mlp[0], True)
        if self.activation != "none":
            h = _ActFunction.apply(h, self.activation)
        return x1 + self._lin(h, self.mlp[2], True)
