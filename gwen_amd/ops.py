"""Tensor-level wrappers over the C ABI (include/gwen_hip.h) and the autograd Function of one layer.

torch is used for device memory, the current HIP stream and autograd bookkeeping only; every
arithmetic step of the layer runs in libgwen_hip.so.  The U-Net's raw ops, forward (csrc/conv.hip) and backward
(csrc/conv_bwd.hip: conv3x3_grad_weight, upsample2x_backward, norm_relu_backward, unpool2x2), are at the end.
"""
from __future__ import annotations

import ctypes
import math
import weakref
from typing import Optional

import torch
from torch import Tensor

from . import _lib
from .graph import GraphCSR, _ptr, _stream, _version_of


def _require(t: Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"gwen_amd: {name} must live on a HIP device (no CPU fallback)")
    if t.dtype != torch.float32:
        raise TypeError(f"gwen_amd: {name} must be float32 (got {t.dtype})")


def _rows2d(x: Tensor):
    """[N,F] or [M,N,F] -> (members, N, F)."""
    if x.dim() == 2:
        return 1, x.size(0), x.size(1)
    if x.dim() == 3:
        return x.size(0), x.size(1), x.size(2)
    raise ValueError(f"expected [N, F] or [members, N, F], got {tuple(x.shape)}")


AUTO_ORDERS = ("auto", "auto_x6", "auto_x3")


def contract_of_order(order: str) -> str:
    """Contraction of a layer run under ``order``: "auto" -> "f16x3" (the default: fp32-class on the kernel's own
    split -- K8 on two scaled fp16 images, every other kernel on bf16x6), "auto_x6" /
    "fused" -> "bf16x6" in every kernel, "auto_x3" / "fused_x3" -> "3xbf16", every other (explicit) order -> "fp32"."""
    if order == "auto":
        return "f16x3"
    if order in ("auto_x6", "fused"):
        return "bf16x6"
    if order in ("auto_x3", "fused_x3"):
        return "3xbf16"
    return "fp32"


def _contract_code(contract, exact: bool = True) -> int:
    if contract is None:
        return _lib.CONTRACT_F32 if exact else _lib.CONTRACT_BF16X3
    if contract not in _lib.CONTRACT_NAMES:
        raise ValueError(f'contract must be one of {sorted(_lib.CONTRACT_NAMES)}')
    return _lib.CONTRACT_NAMES[contract]


def _dense_code(contract, exact: bool = True) -> int:
    """K3 / K4 / K5 / K7: "f16x3" (fp32-class on the kernel's own split) is bf16x6 there."""
    return _lib.dense_contract(_contract_code(contract, exact))


def propagate(graph: GraphCSR, h: Tensor, bias: Optional[Tensor] = None, relu: bool = False,
              transposed: bool = False) -> Tensor:
    """K2: out[i] = act(sum_s val[s] * h[col[s]] + bias) over the CSR (or its transpose)."""
    _require(h, "h")
    h = h.contiguous()
    m, n_src, f = _rows2d(h)
    n = graph.num_nodes
    if not transposed and n_src != graph.source_nodes:
        raise ValueError(f"h has {n_src} rows but the graph has {graph.source_nodes} source nodes")
    if transposed:                        # A^T h: rows = this graph's sources, h has one row per target
        graph = graph.transposed_graph()
        n = graph.num_nodes
        if n_src != graph.source_nodes:
            raise ValueError(f"h has {n_src} rows but the transposed graph has {graph.source_nodes} sources")
    if bias is not None:
        _require(bias, "bias")
        bias = bias.contiguous()
    dev = h.device
    # long rows (hub nodes, complete graphs beyond K7's 256 nodes): the same kernel over the segment chain --
    # every 32-entry segment summed by its own lane group, then each row's partial sums in segment order
    levels = graph.long_row_levels()
    chain = levels if levels is not None else [(graph.rowptr, graph.col, graph.val, n, n_src)]
    cur = h
    for k, (rowptr, col, val, rows, cols) in enumerate(chain):
        last = k + 1 == len(chain)
        out = torch.empty(*h.shape[:-2], rows, f, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.lib().gwen_gcn_propagate_f32(
                _ptr(rowptr), _ptr(col), _ptr(val), _ptr(cur), _ptr(bias) if last else None, _ptr(out), rows, f,
                f, f, m, cols * f, rows * f, int(relu and last), _stream(dev))
        _lib.check(rc, "gwen_gcn_propagate_f32")
        cur = out
    return cur


def linear(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, relu: bool = False,
           exact: bool = True, contract: Optional[str] = None) -> Tensor:
    """K3: act(x @ weight^T + bias); x [..., Fin], weight [Fout, Fin].  ``contract``: "fp32" (fp32-input MFMA, a
    k-ordered fp32 fmaf chain), "bf16x6" (fp32-class split, what AUTO layers use) or "3xbf16" (the faster
    split); when None, ``exact`` picks between "fp32" (True) and "3xbf16" (False)."""
    _require(x, "x")
    _require(weight, "weight")
    x = x.contiguous()
    weight = weight.contiguous()
    fin, fout = weight.size(1), weight.size(0)
    if x.size(-1) != fin:
        raise ValueError(f"x has {x.size(-1)} features but weight expects {fin}")
    rows = math.prod(x.shape[:-1])
    out = torch.empty(*x.shape[:-1], fout, dtype=torch.float32, device=x.device)
    if bias is not None:
        _require(bias, "bias")
        bias = bias.contiguous()
    dev = x.device
    code = _dense_code(contract, exact)
    ws = None
    nws = 0 if code == _lib.CONTRACT_F32 else int(_lib.lib().gwen_gcn_linear_workspace_floats(rows, fin, fout))
    if nws > 0:
        ws = torch.empty(nws, dtype=torch.float32, device=dev)          # split-K partial products
    with torch.cuda.device(dev):
        rc = _lib.lib().gwen_gcn_linear_f32(_ptr(x), _ptr(weight), _ptr(bias), _ptr(out), rows, fin,
                                            fout, fin, fout, int(relu), code, _ptr(ws), nws,
                                            _stream(dev))
    _lib.check(rc, "gwen_gcn_linear_f32")
    return out


def linear_nn(x: Tensor, weight_t: Tensor, contract: Optional[str] = None) -> Tensor:
    """K3 with the weight operand as stored by the OTHER product: x [..., K] @ weight_t [K, N] (row-major), no transposing
    copy -- the backward's g_x = g W with W = the layer's [out, in] weight.  Split contractions ("3xbf16", "bf16x6",
    "f16x3"); "fp32" / None transposes and takes the exact kernel."""
    _require(x, "x")
    _require(weight_t, "weight_t")
    code = _dense_code(contract, True)
    # (tall inputs -- mesh-sized rows -- keep the transposed form: their weights are small and K3 runs them on K8's pipeline)
    if code == _lib.CONTRACT_F32 or math.prod(x.shape[:-1]) >= 16384:
        return linear(x, weight_t.t().contiguous(), contract=contract)
    x = x.contiguous()
    weight_t = weight_t.contiguous()
    k, n = weight_t.shape
    if x.size(-1) != k:
        raise ValueError(f"x has {x.size(-1)} features but weight_t has {k} rows")
    rows = math.prod(x.shape[:-1])
    out = torch.empty(*x.shape[:-1], n, dtype=torch.float32, device=x.device)
    dev = x.device
    nws = int(_lib.lib().gwen_gcn_linear_workspace_floats(rows, k, n))
    ws = torch.empty(nws, dtype=torch.float32, device=dev) if nws > 0 else None
    with torch.cuda.device(dev):
        rc = _lib.lib().gwen_gcn_linear_nn_f32(_ptr(x), _ptr(weight_t), None, _ptr(out), rows, k, n, k, n, n, 0, code,
                                               _ptr(ws), nws, _stream(dev))
    _lib.check(rc, "gwen_gcn_linear_nn_f32")
    return out


class LinearFunction(torch.autograd.Function):
    """Differentiable K3: y = act(x W^T + b) with the backward on the same library -- g_x = g W (K3), g_W = g^T x and
    g_b = column sums of g (the fixed-order reductions of K4's backward).  ``act``: "none" or "relu"."""

    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor, bias: Optional[Tensor], relu: bool, contract: str) -> Tensor:
        y = linear(x, weight, bias, relu, contract=contract)
        ctx.relu, ctx.contract, ctx.has_bias = relu, contract, bias is not None
        ctx.save_for_backward(x, weight, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, g: Tensor):
        x, weight, y = ctx.saved_tensors
        g = g.contiguous()
        if ctx.relu:
            g = relu_backward(y, g)
        gx = linear_nn(g, weight, ctx.contract) if ctx.needs_input_grad[0] else None
        gw = grad_weight(g, x, ctx.contract) if ctx.needs_input_grad[1] else None
        gb = grad_bias(g) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        return gx, gw, gb, None, None


def linear_autograd(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, relu: bool = False,
                    contract: str = "bf16x6") -> Tensor:
    """K3 with autograd (``LinearFunction``)."""
    return LinearFunction.apply(x, weight, bias, relu, contract)


def layer_supported(fin: int, fout: int) -> bool:
    return bool(_lib.lib().gwen_gcn_layer_supported(fin, fout))


def layer_fused(graph: GraphCSR, x: Tensor, weight: Tensor, bias: Optional[Tensor] = None,
                relu: bool = False, exact: bool = False, contract: Optional[str] = None,
                depth: int = 0, block_rows: int = 0, index_mode: int = 0, store_mode: int = 0,
                row_stores: int = 0) -> Tensor:
    """K4: act((A~ x) W^T + b) in one launch (widths in {16,32,64,128,256}).  ``contract``: "bf16x6", "3xbf16" or
    "fp32"; when None, ``exact`` picks between "fp32" (True) and "3xbf16" (False).  ``depth`` (gather passes in
    flight per wave: 1 or 2) and ``block_rows`` (64 / 96 / 112 / 128 where the widths allow) are scheduling choices
    that change no value; 0 = the library's.  So is ``index_mode`` (1: every lane loads its row's indices and weights;
    2: one record load per row, broadcast in the lane group -- widths up to 64 on a uniform layout only)
    and ``store_mode`` (1: plain output stores; 3: the same stores written through -- widths up to 64 on a bf16 split and a
    uniform layout only; 2 and 4 are reserved) and ``row_stores`` (1: the written-through tile leaves as the MFMA holds it;
    2: as whole rows through an LDS out tile -- only where the store mode is 3) (gwen_gcn_layer_tuned5_f32)."""
    _require(x, "x")
    _require(weight, "weight")
    x = x.contiguous()
    weight = weight.contiguous()
    m, n_src, fin = _rows2d(x)
    n = graph.num_nodes
    fout = weight.size(0)
    if n_src != graph.source_nodes or weight.size(1) != fin:
        raise ValueError("shape mismatch between x, weight and the graph")
    if n_src * fin * 4 >= (1 << 32):
        raise ValueError("x is too large for K4's 32-bit row offsets")
    if bias is not None:
        _require(bias, "bias")
        bias = bias.contiguous()
    out = torch.empty(*x.shape[:-2], n, fout, dtype=torch.float32, device=x.device)
    dev = x.device
    g_rowptr, g_col, g_val = graph.grouped()
    with torch.cuda.device(dev):
        rc = _lib.lib().gwen_gcn_layer_tuned5_f32(
            _ptr(g_rowptr), _ptr(g_col), _ptr(g_val), _ptr(x), _ptr(weight), _ptr(bias),
            _ptr(out), n, fin, fout, fin, fout, m, n_src * fin, n * fout, int(relu),
            _dense_code(contract, exact), graph.entries(), int(depth), int(block_rows), int(index_mode), None, 0,
            _stream(dev), int(store_mode), int(row_stores))
    _lib.check(rc, "gwen_gcn_layer_tuned5_f32")
    return out


layer = layer_fused


def wide_supported(fin: int, fout: int) -> bool:
    return bool(_lib.lib().gwen_gcn_wide_supported(fin, fout))


def wide_preferred(graph: GraphCSR, x: Tensor, fin: int, fout: int, contract: str = "3xbf16") -> bool:
    """Would the stack launcher run this AUTO layer as K8?  (Same rule, so training and inference agree.)"""
    m, n_src, _ = _rows2d(x)
    code = _lib.wide_contract(fin, fout, _contract_code(contract))
    if not _lib.lib().gwen_gcn_wide_preferred(graph.num_nodes, m, fin, fout) or \
            not _lib.lib().gwen_gcn_wide_contract_supported(fin, fout, code):
        return False
    tiles = graph.tiles()
    return tiles is not None and (code != _lib.CONTRACT_BF16X6 or tiles[3] <= 128)


def wide_layer(graph: GraphCSR, x: Tensor, weight: Tensor, bias: Optional[Tensor] = None,
               relu: bool = False, contract: str = "f16x3") -> Tensor:
    """K8: act((A~ x) W^T + b), tile-staged through LDS (widths in {64,128,256}, graphs that tile:
    ``graph.tiles()``).  ``contract``: "f16x3" (the library default: fp32-class on two scaled fp16 images, ONE launch
    at every width), "bf16x6" (graphs whose tile unions stay
    within 128 rows; 256 -> 256 as two 256 -> 128 launches) or "3xbf16" -- the bf16 splits term for term K4's
    arithmetic."""
    _require(x, "x")
    _require(weight, "weight")
    x = x.contiguous()
    weight = weight.contiguous()
    m, n_src, fin = _rows2d(x)
    n = graph.num_nodes
    fout = weight.size(0)
    if n_src != graph.source_nodes or weight.size(1) != fin:
        raise ValueError("shape mismatch between x, weight and the graph")
    tiles = graph.tiles()
    if tiles is None or not wide_supported(fin, fout):
        raise ValueError("K8 needs a graph that tiles (rows of at most 8 entries, <= 192 distinct sources per "
                         "64 rows) and widths in {64, 128, 256}")
    if bias is not None:
        _require(bias, "bias")
        bias = bias.contiguous()
    out = torch.empty(*x.shape[:-2], n, fout, dtype=torch.float32, device=x.device)
    dev = x.device
    t_rows, t_lid, t_val, umax = tiles
    with torch.cuda.device(dev):
        rc = _lib.lib().gwen_gcn_wide_layer_f32(
            _ptr(t_rows), _ptr(t_lid), _ptr(t_val), _ptr(x), _ptr(weight), _ptr(bias), _ptr(out),
            n, n_src, fin, fout, fout, m, n_src * fin, n * fout, int(relu), umax,
            _lib.wide_contract(fin, fout, _contract_code(contract)), _stream(dev))
    _lib.check(rc, "gwen_gcn_wide_layer_f32")
    return out


def small_layer(graph: GraphCSR, x: Tensor, weight: Tensor, bias: Optional[Tensor] = None,
                relu: bool = False, packed: Optional[Tensor] = None, contract: str = "3xbf16") -> Tensor:
    """K7: act(A~ (x W^T) + b) in one launch on a graph of at most 256 nodes (dense adjacency).
    ``packed``: the weight's ``gwen_amd.forward.pack_weight`` image (streamed instead of ``weight``; "3xbf16"
    only).  ``contract``: "3xbf16" or "bf16x6"."""
    _require(x, "x")
    _require(weight, "weight")
    x, weight = x.contiguous(), weight.contiguous()
    m, n_src, fin = _rows2d(x)
    n, fout = graph.num_nodes, weight.size(0)
    dense = graph.dense()
    code = _dense_code(contract)
    if dense is None or not _lib.lib().gwen_gcn_small_supported(n, fin, fout, code):
        raise ValueError("K7 needs a square graph of at most 256 nodes, Fin % 32 == 0, Fout % 16 == 0")
    if n_src != n or weight.size(1) != fin:
        raise ValueError("shape mismatch between x, weight and the graph")
    if bias is not None:
        _require(bias, "bias")
        bias = bias.contiguous()
    dev = x.device
    out = torch.empty(*x.shape[:-2], n, fout, dtype=torch.float32, device=dev)
    nws = int(_lib.lib().gwen_gcn_small_workspace_floats(n, m, fin, fout))
    ws = torch.empty(nws, dtype=torch.float32, device=dev) if nws > 0 else None
    with torch.cuda.device(dev):
        rc = _lib.lib().gwen_gcn_small_layer_f32(_ptr(dense), _ptr(x), _ptr(weight), _ptr(packed), _ptr(bias), _ptr(out),
                                                 n, fin, fout, m, n * fin, n * fout, int(relu), _ptr(ws),
                                                 nws, code, _stream(dev))
    _lib.check(rc, "gwen_gcn_small_layer_f32")
    return out


def chain(graph: GraphCSR, x: Tensor, w1: Optional[Tensor], w2: Optional[Tensor], bias: Optional[Tensor],
          relu: bool, pre: bool, contract: str = "3xbf16", depth: int = 0, block_rows: int = 0,
          index_mode: int = 0, store_mode: int = 0) -> Tensor:
    """K5.  pre=False: act((A~ x) w1^T + bias) w2^T;  pre=True: act(A~ x + bias) w1^T  (inference only); pre=True
    with w1 = None: act(A~ x + bias), the propagation on the grouped layout.  ``contract``: "3xbf16" or "bf16x6".
    ``depth`` / ``block_rows`` / ``index_mode`` / ``store_mode``: as ``layer_fused`` (gwen_gcn_chain_tuned4_f32); they change
    no value."""
    _require(x, "x")
    x = x.contiguous()
    m, n, fin = _rows2d(x)
    f1 = 0 if w1 is None else w1.size(0)
    f2 = 0 if w2 is None else w2.size(0)
    fw = f2 or f1 or fin
    out = torch.empty(*x.shape[:-1], fw, dtype=torch.float32, device=x.device)
    g_rowptr, g_col, g_val = graph.grouped()
    dev = x.device
    with torch.cuda.device(dev):
        rc = _lib.lib().gwen_gcn_chain_tuned4_f32(
            _ptr(g_rowptr), _ptr(g_col), _ptr(g_val), _ptr(x), None if w1 is None else _ptr(w1.contiguous()),
            None if w2 is None else _ptr(w2.contiguous()), None if bias is None else _ptr(bias.contiguous()),
            _ptr(out), n, fin, f1, f2, int(pre), int(relu), m, n * fin, n * fw, _dense_code(contract),
            graph.entries(), int(depth), int(block_rows), int(index_mode), None, None, 0, _stream(dev), int(store_mode))
    _lib.check(rc, "gwen_gcn_chain_tuned4_f32")
    return out


def _grad_workspace(rows: int, fin: int, fout: int, dev) -> Tensor:
    n = int(_lib.lib().gwen_gcn_grad_workspace_floats(rows, fin, fout))
    return torch.empty(n, dtype=torch.float32, device=dev)


def grad_weight(g: Tensor, x: Tensor, contract: Optional[str] = None) -> Tensor:
    """grad_W [Fout, Fin] = g^T @ x over all leading rows.  ``contract``: the contraction of the layer the gradient
    belongs to -- None / "fp32": exact fp32 products; "bf16x6" / "f16x3" / "3xbf16": the split contractions where the
    widths allow (multiples of 64: 2.7 - 3.7 x faster at 256 channels), the fp32 MFMA elsewhere."""
    g = g.contiguous(); x = x.contiguous()
    fout, fin = g.size(-1), x.size(-1)
    rows = math.prod(g.shape[:-1])
    out = torch.empty(fout, fin, dtype=torch.float32, device=g.device)
    ws = _grad_workspace(rows, fin, fout, g.device)
    with torch.cuda.device(g.device):
        rc = _lib.lib().gwen_gcn_grad_weight_f32(_ptr(g), _ptr(x), _ptr(out), rows, fin, fout, fout,
                                                 fin, _ptr(ws), _contract_code(contract), _stream(g.device))
    _lib.check(rc, "gwen_gcn_grad_weight_f32")
    return out


def grad_bias(g: Tensor) -> Tensor:
    g = g.contiguous()
    f = g.size(-1)
    rows = math.prod(g.shape[:-1])
    out = torch.empty(f, dtype=torch.float32, device=g.device)
    ws = _grad_workspace(rows, f, 1, g.device)
    with torch.cuda.device(g.device):
        rc = _lib.lib().gwen_gcn_grad_bias_f32(_ptr(g), _ptr(out), rows, f, f, _ptr(ws),
                                               _stream(g.device))
    _lib.check(rc, "gwen_gcn_grad_bias_f32")
    return out


class _ReduceTask(ctypes.Structure):          # gwen_reduce_task (include/gwen_hip.h)
    _fields_ = [("partial", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("count", ctypes.c_int64),
                ("nchunks", ctypes.c_int64)]


class GradBatch:
    """Many grad_weight / grad_bias reductions whose fixed-order finishes share ONE launch
    (gwen_reduce_chunks_batched, up to 32 per launch) instead of one each: stage 1 of every reduction is launched
    at once, the returned tensors are complete after ``finish()``.  Same chunking and summation order per reduction
    whatever else is in the batch (deterministic, run to run bitwise)."""

    def __init__(self) -> None:
        self._tasks: list = []
        self._keep: list = []
        self._dev = None

    def _add(self, partial: Tensor, out: Tensor, count: int, nch: int) -> None:
        self._tasks.append((partial.data_ptr(), out.data_ptr(), count, nch))
        self._keep += [partial, out]

    def grad_weight(self, g: Tensor, x: Tensor, contract: Optional[str] = None) -> Tensor:
        g = g.contiguous(); x = x.contiguous()
        fout, fin = g.size(-1), x.size(-1)
        rows = math.prod(g.shape[:-1])
        dev = self._dev = g.device
        out = torch.empty(fout, fin, dtype=torch.float32, device=dev)
        if rows == 0:
            return out.zero_()
        code = _contract_code(contract)
        nch = int(_lib.lib().gwen_gcn_grad_weight_chunks(rows, fin, fout, code))
        dst = out if nch == 1 else torch.empty(nch * fout * fin, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.lib().gwen_gcn_grad_weight_partial_f32(_ptr(g), _ptr(x), _ptr(dst), rows, fin, fout, fout, fin,
                                                             code, _stream(dev))
        _lib.check(rc, "gwen_gcn_grad_weight_partial_f32")
        if nch > 1:
            self._add(dst, out, fout * fin, nch)
        return out

    def grad_weight_bias(self, g: Tensor, x: Tensor, contract: Optional[str] = None):
        """(g^T x, column sums of g): ONE stage-1 launch where the weight gradient runs on the LDS-staged split kernel (the
        g tile is in LDS anyway), the two separate launches elsewhere."""
        g = g.contiguous(); x = x.contiguous()
        fout, fin = g.size(-1), x.size(-1)
        rows = math.prod(g.shape[:-1])
        code = _contract_code(contract)
        L = _lib.lib()
        if rows == 0 or not L.gwen_gcn_grad_weight_bias_supported(fin, fout, code) or g.data_ptr() % 16 \
                or x.data_ptr() % 16:
            return self.grad_weight(g, x, contract), self.grad_bias(g)
        dev = self._dev = g.device
        gw = torch.empty(fout, fin, dtype=torch.float32, device=dev)
        gb = torch.empty(fout, dtype=torch.float32, device=dev)
        nch = int(L.gwen_gcn_grad_weight_chunks(rows, fin, fout, code))
        pw = gw if nch == 1 else torch.empty(nch * fout * fin, dtype=torch.float32, device=dev)
        pb = gb if nch == 1 else torch.empty(nch * fout, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = L.gwen_gcn_grad_weight_bias_partial_f32(_ptr(g), _ptr(x), _ptr(pw), _ptr(pb), rows, fin, fout, fout, fin,
                                                         code, _stream(dev))
        _lib.check(rc, "gwen_gcn_grad_weight_bias_partial_f32")
        if nch > 1:
            self._add(pw, gw, fout * fin, nch)
            self._add(pb, gb, fout, nch)
        return gw, gb

    def grad_bias(self, g: Tensor) -> Tensor:
        g = g.contiguous()
        f = g.size(-1)
        rows = math.prod(g.shape[:-1])
        dev = self._dev = g.device
        out = torch.empty(f, dtype=torch.float32, device=dev)
        if rows == 0:
            return out.zero_()
        nch = int(_lib.lib().gwen_gcn_grad_chunks(rows))
        dst = out if nch == 1 else torch.empty(nch * f, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.lib().gwen_gcn_grad_bias_partial_f32(_ptr(g), _ptr(dst), rows, f, f, _stream(dev))
        _lib.check(rc, "gwen_gcn_grad_bias_partial_f32")
        if nch > 1:
            self._add(dst, out, f, nch)
        return out

    def finish(self) -> None:
        cap = 32                                             # GWEN_MAX_REDUCE_TASKS
        for i in range(0, len(self._tasks), cap):
            part = self._tasks[i:i + cap]
            arr = (_ReduceTask * len(part))(*[_ReduceTask(*t) for t in part])
            with torch.cuda.device(self._dev):
                rc = _lib.lib().gwen_reduce_chunks_batched(ctypes.cast(arr, ctypes.c_void_p), len(part),
                                                           _stream(self._dev))
            _lib.check(rc, "gwen_reduce_chunks_batched")
        self._tasks, self._keep = [], []


def _layer_norm_args(x: Tensor, weight: Tensor, bias: Tensor, res: Optional[Tensor]) -> None:
    if x.dim() != 2 or not _lib.lib().gwen_layer_norm_supported(x.size(-1)):
        raise ValueError(f"layer_norm needs [rows, F] with F a multiple of 4 up to 1024; got {tuple(x.shape)}")
    f = x.size(-1)
    if tuple(weight.shape) != (f,) or tuple(bias.shape) != (f,):
        raise ValueError("layer_norm: weight and bias must be [F]")
    if res is not None and res.shape != x.shape:
        raise ValueError("layer_norm: res must have the shape of x")
    for name, t in (("x", x), ("weight", weight), ("bias", bias), ("res", res)):
        if t is not None:
            _require(t, name)


def layer_norm_rows(x: Tensor, weight: Tensor, bias: Tensor, eps: float = 1e-5, res: Optional[Tensor] = None,
                    rowptr: Optional[Tensor] = None, n_dst: int = 0, mean: bool = False, want_out: bool = True):
    """gwen_layer_norm_f32 without autograd: (out, agg) with out = (res +) LN(x) and -- given the ``rowptr`` of
    target-sorted rows -- agg[d] = sum / mean of LN(x) over target d's rows in stored order, from the same pass."""
    _layer_norm_args(x, weight, bias, res)
    x, weight, bias = x.contiguous(), weight.contiguous(), bias.contiguous()
    res = None if res is None else res.contiguous()
    rows, f = x.shape
    dev = x.device
    out = torch.empty_like(x) if want_out else None
    agg = torch.empty(n_dst, f, dtype=torch.float32, device=dev) if rowptr is not None else None
    with torch.cuda.device(dev):
        rc = _lib.lib().gwen_layer_norm_f32(_ptr(x), _ptr(weight), _ptr(bias), eps, _ptr(res), _ptr(out), rows, f,
                                            _ptr(rowptr), _ptr(agg), n_dst, int(mean), _stream(dev))
    _lib.check(rc, "gwen_layer_norm_f32")
    return out, agg


def layer_norm_backward(x: Tensor, g: Tensor, weight: Tensor, eps: float, batch: Optional["GradBatch"] = None,
                        want_params: bool = True):
    """gwen_layer_norm_bwd_f32: (g_x, grad_weight | grad_bias as ONE [2 F] tensor, or None) for y = LN(x) and the
    gradient ``g`` of y.  The parameter gradients are per-chunk partials finished in a fixed order -- with ``batch`` in
    that GradBatch's one finish launch (complete after its ``finish()``), else here."""
    x, g, weight = x.contiguous(), g.contiguous(), weight.contiguous()
    rows, f = x.shape
    dev = x.device
    gx = torch.empty_like(x)
    gp = torch.zeros(2 * f, dtype=torch.float32, device=dev) if want_params else None
    if rows == 0:
        return gx, gp
    nch = int(_lib.lib().gwen_layer_norm_bwd_chunks(rows))
    part = None
    if want_params:
        part = gp if nch == 1 else torch.empty(nch * 2 * f, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().gwen_layer_norm_bwd_f32(_ptr(x), _ptr(g), _ptr(weight), eps, _ptr(gx), _ptr(part), rows, f,
                                                _stream(dev))
    _lib.check(rc, "gwen_layer_norm_bwd_f32")
    if want_params and nch > 1:
        own = batch is None
        batch = GradBatch() if own else batch
        batch._dev = dev
        batch._add(part, gp, 2 * f, nch)
        if own:
            batch.finish()
    return gx, gp


class LayerNormFunction(torch.autograd.Function):
    """y = (res +) LN(x) on csrc/layernorm.hip, forward and backward (atomic-free: two runs are bitwise equal)."""

    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor, bias: Tensor, eps: float, res: Optional[Tensor]) -> Tensor:
        out, _ = layer_norm_rows(x, weight, bias, eps, res)
        ctx.save_for_backward(x, weight)
        ctx.eps, ctx.has_res = eps, res is not None
        return out

    @staticmethod
    def backward(ctx, g: Tensor):
        x, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        f = x.size(-1)
        g = g.contiguous()
        gx, gp = layer_norm_backward(x.detach(), g, weight.detach(), ctx.eps, want_params=need[1] or need[2])
        return (gx if need[0] else None, gp[:f] if need[1] else None, gp[f:] if need[2] else None, None,
                g if ctx.has_res and need[4] else None)


def layer_norm(x: Tensor, weight: Tensor, bias: Tensor, eps: float = 1e-5, res: Optional[Tensor] = None) -> Tensor:
    """``(res +) torch.nn.functional.layer_norm(x, [F], weight, bias, eps)`` for fp32 ``[rows, F]`` (F a multiple of 4 up
    to 1024): biased variance, formed from deviations about the mean; with autograd (x, weight, bias, res)."""
    _layer_norm_args(x, weight, bias, res)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, weight, bias, res)):
        return LayerNormFunction.apply(x, weight, bias, eps, res)
    return layer_norm_rows(x, weight, bias, eps, res)[0]


def relu_backward(y: Tensor, g: Tensor) -> Tensor:
    y = y.contiguous(); g = g.contiguous()
    out = torch.empty_like(g)
    with torch.cuda.device(g.device):
        rc = _lib.lib().gwen_relu_backward_f32(_ptr(y), _ptr(g), _ptr(out), g.numel(),
                                               _stream(g.device))
    _lib.check(rc, "gwen_relu_backward_f32")
    return out


def _propagate_transposed(graph: GraphCSR, g: Tensor, contract: Optional[str]) -> Tensor:
    """A~^T g for the backward.  Small square graphs with wide rows (the reference's member graphs: 125 nodes x 1024 ..
    16 384 features) on a split precision: ONE dense product D^T g (K3 with g as the [K, N] operand, as the forward's K7
    contracts D h) instead of K2 walking the 125-entry rows (53.6 -> 10 us at 16 384 features); everything else: K2."""
    if g.dim() == 2 and g.size(-1) >= 256 and contract in ("3xbf16", "bf16x6", "f16x3"):
        d = graph.dense_transposed_square()
        if d is not None:
            return linear_nn(d, g, contract)
    return propagate(graph, g, transposed=True)


class GCNLayerFunction(torch.autograd.Function):
    """act(A~ (x W^T) + b): forward and backward entirely on the HIP kernels.

    ``order``: "auto" picks "small" = K7 on graphs of at most 256 nodes (one launch, dense adjacency),
    else "fused" = K4, one launch, whenever the widths allow; otherwise the
    two linear maps run as two launches, transform-first (x W^T, then aggregate at width Fout -- what
    PyG does) when Fout <= Fin, aggregate-first (A~ x at width Fin, then the projection with the
    bias/ReLU epilogue) when Fin < Fout, so the gather always runs at the narrower width.
    All three equal the reference's result up to fp32 rounding order (A~ is linear).
    """

    @staticmethod
    def forward(ctx, x: Tensor, weight: Tensor, bias: Optional[Tensor], graph: GraphCSR,
                relu: bool, order: str, packed: Optional[Tensor] = None) -> Tensor:
        fout, fin = weight.shape
        # one precision rule for both host paths (this Function and the stack launcher, forward.hip): an AUTO
        # layer contracts with its split ("auto": f16x3 = K8's scaled fp16 split / bf16x6 in every other kernel,
        # "auto_x6": bf16x6, "auto_x3": 3xbf16) whatever kernels it resolves to;
        # explicit orders ("transform_first", "aggregate_first", "fused_exact") use the exact fp32-input MFMA
        contract = contract_of_order(order)
        if order in AUTO_ORDERS:
            if graph.dense() is not None and _lib.lib().gwen_gcn_small_supported(graph.num_nodes, fin, fout,
                                                                                 _dense_code(contract)):
                order = "small"              # K7: the reference's member graphs (<= 256 nodes)
            elif graph.long_row_levels() is not None:
                # rows far beyond 8 entries: the fused kernels walk a row serially, the segment chain does not
                order = "aggregate_first" if fin < fout else "transform_first"
            elif wide_preferred(graph, x, fin, fout, contract):
                order = "wide"               # K8: K4's arithmetic, tile-staged (same backward)
            elif layer_supported(fin, fout):
                order = "fused"
            else:
                order = "aggregate_first" if fin < fout else "transform_first"
        if order == "small":
            out = small_layer(graph, x, weight, bias, relu, packed=packed if contract == "3xbf16" else None,
                              contract=contract)
            saved_in = x
        elif order == "wide":
            out = wide_layer(graph, x, weight, bias, relu, contract=contract)
            saved_in = x
        elif order in ("fused", "fused_x3", "fused_exact"):
            out = layer_fused(graph, x, weight, bias, relu, contract=contract)          # ("f16x3" is bf16x6 in K4)
            saved_in = x
        elif order == "transform_first":
            h = linear(x, weight, contract=contract)
            out = propagate(graph, h, bias, relu)
            saved_in = x
        elif order == "aggregate_first":
            agg = propagate(graph, x)
            out = linear(agg, weight, bias, relu, contract=contract)
            saved_in = agg
        else:
            raise ValueError(f"unknown order {order!r}")
        ctx.graph, ctx.relu, ctx.order, ctx.has_bias = graph, relu, order, bias is not None
        ctx.contract = contract          # the backward contracts on the layer's own precision ("f16x3": bf16x6 in K3)
        ctx.save_for_backward(saved_in, weight, out if relu else None)
        return out

    @staticmethod
    def backward(ctx, grad_out: Tensor):
        saved_in, weight, out = ctx.saved_tensors
        g = grad_out.contiguous()
        if ctx.relu:
            g = relu_backward(out, g)
        gb = grad_bias(g) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        gx = gw = None
        if ctx.order in ("transform_first", "fused", "fused_x3", "fused_exact", "small", "wide"):   # out = act(A~ x W^T + b) either way
            gh = _propagate_transposed(ctx.graph, g, ctx.contract)  # A~^T g
            if ctx.needs_input_grad[1]:
                gw = grad_weight(gh, saved_in, ctx.contract)       # gh^T x
            if ctx.needs_input_grad[0]:
                gx = linear_nn(gh, weight, ctx.contract)                                 # gh W (split-K, W as stored)
        else:
            if ctx.needs_input_grad[1]:
                gw = grad_weight(g, saved_in, ctx.contract)        # g^T (A~ x)
            if ctx.needs_input_grad[0]:
                gagg = linear_nn(g, weight, ctx.contract)                                # g W
                gx = _propagate_transposed(ctx.graph, gagg, ctx.contract)   # A~^T (g W)
        return gx, gw, gb, None, None, None, None


def gcn_layer(x: Tensor, weight: Tensor, bias: Optional[Tensor], graph: GraphCSR,
              relu: bool = False, order: str = "auto", packed: Optional[Tensor] = None) -> Tensor:
    _require(x, "x")
    _require(weight, "weight")
    if x.device != weight.device or x.device != graph.device:
        raise RuntimeError("x, weight and the graph must be on the same device")
    return GCNLayerFunction.apply(x, weight, bias, graph, relu, order, packed)


# ---- U-Net kernels (csrc/conv.hip): channels-last activations [B, H, W, C], a channel slice of a wider buffer allowed ----

def _nhwc(t: Tensor, name: str):
    """(B, H, W, C, row pitch) of a channels-last activation: dense over B, H, W with the channels contiguous inside
    rows of ``pitch >= C`` elements -- a contiguous tensor or a slice ``buf[..., c0:c1]`` of one."""
    _require(t, name)
    if t.dim() != 4:
        raise ValueError(f"{name} must be channels-last [B, H, W, C], got {tuple(t.shape)}")
    b, h, w, c = t.shape
    if t.numel() == 0:
        return b, h, w, c, max(c, 1)
    ld = t.stride(2) if w > 1 else (t.stride(1) if h > 1 else (t.stride(0) if b > 1 else c))
    ok = (c == 1 or t.stride(3) == 1) and ld >= c and (w == 1 or t.stride(2) == ld) \
        and (h == 1 or t.stride(1) == w * ld) and (b == 1 or t.stride(0) == h * w * ld)
    if not ok:
        raise ValueError(f"{name} must be channels-last rows with one pitch (a contiguous tensor or a channel slice of "
                         f"one); got shape {tuple(t.shape)}, strides {t.stride()}")
    return b, h, w, c, ld


def _affine_pair(affine, c: int, dev):
    if affine is None:
        return None, None
    s, t = affine
    for name, v in (("affine scale", s), ("affine shift", t)):
        _require(v, name)
        if tuple(v.shape) != (c,) or v.device != dev:
            raise ValueError(f"{name} must be [{c}] on {dev}")
    return s.contiguous(), t.contiguous()


_CONV_PACKED: dict = {}   # id(weight) -> (weak reference, {(contract, transposed): (key, image)}); repacked when the version moves


def conv3x3_pack(weight: Tensor, transposed: bool = False, contract: Optional[str] = None) -> Tensor:
    """The packed image of a 3x3 weight (gwen_conv3x3_pack_f32), cached per weight ``_version`` as the K4 / K5 packed W
    is: ``weight`` [Cout, Cin, 3, 3] (Conv2d) or, ``transposed``, [Cin, Cout, 3, 3] (ConvTranspose2d)."""
    _require(weight, "weight")
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError(f"weight must be [., ., 3, 3], got {tuple(weight.shape)}")
    code = _dense_code(contract or "bf16x6")
    cout, cin = (weight.size(1), weight.size(0)) if transposed else (weight.size(0), weight.size(1))
    ver = _version_of(weight)
    key = (weight.data_ptr(), ver, tuple(weight.shape), weight.device)
    ident, slot = id(weight), (code, bool(transposed))
    entry = _CONV_PACKED.get(ident)
    if entry is not None and entry[0]() is not weight:           # the id of a weight that went away, reused
        entry = None
    hit = None if entry is None else entry[1].get(slot)
    if ver is not None and hit is not None and hit[0] == key:
        return hit[1]
    nbytes = int(_lib.lib().gwen_conv3x3_pack_bytes(cin, cout, code))
    if nbytes == 0:
        raise ValueError(f"conv3x3: channels must be in [1, 2048] and the contract a split one; got Cin {cin}, Cout "
                         f"{cout}, contract {contract!r}")
    w = weight.detach().contiguous()
    img = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=weight.device)
    with torch.cuda.device(weight.device):
        rc = _lib.lib().gwen_conv3x3_pack_f32(_ptr(w), cin, cout, int(transposed), code, _ptr(img), _stream(weight.device))
    _lib.check(rc, "gwen_conv3x3_pack_f32")
    # the entry lives as long as the weight object does (an id may be reused afterwards: the weak reference tells);
    # one image per (contraction, layout) of it, so two tiers on one weight do not repack each other
    if entry is None:
        entry = (weakref.ref(weight, lambda _r, i=ident: _CONV_PACKED.pop(i, None)), {})
        _CONV_PACKED[ident] = entry
    entry[1][slot] = (key, img)
    return img


def conv3x3(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, transposed: bool = False, pool: bool = False,
            affine=None, relu: bool = False, contract: Optional[str] = None, out: Optional[Tensor] = None,
            argmax: bool = False):
    """3x3 / stride 1 / padding 1 convolution of channels-last ``x`` [B, H, W, Cin] (gwen_conv3x3_f32): conv + bias, then
    ``pool`` (2x2 / stride 2 max, floor rule), then ``affine`` = (scale, shift) per output channel, then ReLU, in one
    launch.  ``transposed``: ``weight`` is a ConvTranspose2d's [Cin, Cout, 3, 3].  ``contract``: "bf16x6" (default,
    fp32-class; "f16x3" means it too) or "3xbf16".  ``out``: where to write, [B, Ho, Wo, Cout], a channel slice allowed.
    ``argmax`` (with ``pool`` only; gwen_conv3x3_argmax_f32): returns ``(out, argmax, pre)`` -- the same bits in ``out``,
    the window's winner as uint8 [B, Ho, Wo, Cout] (0 .. 3 in the order (0,0) (0,1) (1,0) (1,1), torch's rule) and the
    pooled value + bias before the affine and the ReLU: what the backward keeps."""
    if argmax and not pool:
        raise ValueError("conv3x3: argmax needs pool=True")
    b, h, w, cin, ldx = _nhwc(x, "x")
    img = conv3x3_pack(weight, transposed, contract)
    cout, wcin = (weight.size(1), weight.size(0)) if transposed else (weight.size(0), weight.size(1))
    if wcin != cin:
        raise ValueError(f"x has {cin} channels but weight expects {wcin}")
    dev = x.device
    if weight.device != dev:
        raise RuntimeError("x and weight must be on the same device")
    if bias is not None:
        _require(bias, "bias")
        if tuple(bias.shape) != (cout,):
            raise ValueError(f"bias must be [{cout}]")
        bias = bias.detach().contiguous()
    s, t = _affine_pair(affine, cout, dev)
    ho, wo = (h // 2, w // 2) if pool else (h, w)
    if out is None:
        out = torch.empty(b, ho, wo, cout, dtype=torch.float32, device=dev)
    ob, oh, ow, oc, ldo = _nhwc(out, "out")
    if (ob, oh, ow, oc) != (b, ho, wo, cout) or out.device != dev:
        raise ValueError(f"out must be [{b}, {ho}, {wo}, {cout}] on {dev}, got {tuple(out.shape)}")
    flags = (_lib.CONV_AFFINE if affine is not None else 0) | (_lib.CONV_RELU if relu else 0) | (_lib.CONV_POOL if pool else 0)
    # the slices' raw sums (low resolutions); -1: they would reach 4 GiB, and the launcher answers GWEN_ERANGE
    nws = max(int(_lib.lib().gwen_conv3x3_workspace_floats(b, h, w, cin, cout, flags)), 0)
    ws = torch.empty(nws, dtype=torch.float32, device=dev) if nws > 0 else None
    if argmax:
        am = torch.empty(b, ho, wo, cout, dtype=torch.uint8, device=dev)
        pre = torch.empty(b, ho, wo, cout, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.lib().gwen_conv3x3_argmax_f32(_ptr(x), _ptr(img), _ptr(bias), _ptr(s), _ptr(t), _ptr(out), b, h, w,
                                                    cin, cout, ldx, ldo, flags, _dense_code(contract or "bf16x6"),
                                                    _ptr(ws), nws, _ptr(am), _ptr(pre), cout, _stream(dev))
        _lib.check(rc, "gwen_conv3x3_argmax_f32")
        return out, am, pre
    with torch.cuda.device(dev):
        rc = _lib.lib().gwen_conv3x3_f32(_ptr(x), _ptr(img), _ptr(bias), _ptr(s), _ptr(t), _ptr(out), b, h, w, cin, cout,
                                         ldx, ldo, flags, _dense_code(contract or "bf16x6"), _ptr(ws), nws, _stream(dev))
    _lib.check(rc, "gwen_conv3x3_f32")
    return out


def upsample2x(x: Tensor, affine=None, relu: bool = False, out: Optional[Tensor] = None) -> Tensor:
    """Bilinear x2 with align_corners=True of channels-last ``x`` [B, H, W, C] (gwen_upsample2x_f32), then ``affine`` =
    (scale, shift) per channel, then ReLU.  ``out``: [B, 2H, 2W, C], a channel slice of a wider buffer allowed."""
    b, h, w, c, ldx = _nhwc(x, "x")
    dev = x.device
    s, t = _affine_pair(affine, c, dev)
    if out is None:
        out = torch.empty(b, 2 * h, 2 * w, c, dtype=torch.float32, device=dev)
    ob, oh, ow, oc, ldo = _nhwc(out, "out")
    if (ob, oh, ow, oc) != (b, 2 * h, 2 * w, c) or out.device != dev:
        raise ValueError(f"out must be [{b}, {2 * h}, {2 * w}, {c}] on {dev}, got {tuple(out.shape)}")
    flags = (_lib.CONV_AFFINE if affine is not None else 0) | (_lib.CONV_RELU if relu else 0)
    with torch.cuda.device(dev):
        rc = _lib.lib().gwen_upsample2x_f32(_ptr(x), _ptr(s), _ptr(t), _ptr(out), b, h, w, c, ldx, ldo, flags, _stream(dev))
    _lib.check(rc, "gwen_upsample2x_f32")
    return out


def channel_stats(x: Tensor):
    """(mean, biased variance) per channel over every row of channels-last ``x`` [..., C] (a channel slice allowed), as
    fp64 tensors [C] (gwen_channel_stats_f64: fp64 sums in a fixed order) -- train-mode BatchNorm's statistics."""
    if x.dim() != 4:
        _require(x, "x")
        if x.dim() != 2 or (x.size(1) > 1 and x.stride(1) != 1) or x.stride(0) < x.size(1):
            raise ValueError(f"channel_stats needs [rows, C] rows or channels-last [B, H, W, C]; got {tuple(x.shape)}")
        rows, c, ld = x.size(0), x.size(1), (x.stride(0) if x.size(0) > 1 else x.size(1))
    else:
        b, h, w, c, ld = _nhwc(x, "x")
        rows = b * h * w
    dev = x.device
    nbytes = int(_lib.lib().gwen_channel_stats_workspace_bytes(rows, c))
    if nbytes == 0:
        raise ValueError(f"channel_stats needs at least one row and 1 <= C <= 2048; got rows {rows}, C {c}")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    stats = torch.empty(2, c, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().gwen_channel_stats_f64(_ptr(x), rows, c, ld, _ptr(stats[0]), _ptr(stats[1]), _ptr(ws), nbytes,
                                               _stream(dev))
    _lib.check(rc, "gwen_channel_stats_f64")
    return stats[0], stats[1]


def affine_relu_(x: Tensor, scale: Tensor, shift: Tensor) -> Tensor:
    """x <- max(0, x * scale[c] + shift[c]) in place on channels-last ``x`` [B, H, W, C] (a channel slice allowed):
    gwen_affine_relu_f32, the finish of train-mode BatchNorm + ReLU."""
    b, h, w, c, ld = _nhwc(x, "x")
    s, t = _affine_pair((scale, shift), c, x.device)
    with torch.cuda.device(x.device):
        rc = _lib.lib().gwen_affine_relu_f32(_ptr(x), _ptr(s), _ptr(t), b * h * w, c, ld, _stream(x.device))
    _lib.check(rc, "gwen_affine_relu_f32")
    return x


# ---- U-Net backward (csrc/conv_bwd.hip) ----

def conv3x3_grad_weight_plan(b: int, h: int, w: int, cin: int, cout: int):
    """(channel tiles of 16 x 16 per block, pixel chunks) of ``conv3x3_grad_weight`` at these shapes."""
    tiles, chunks = ctypes.c_int(0), ctypes.c_int64(0)
    _lib.check(_lib.lib().gwen_conv3x3_grad_weight_plan(b, h, w, cin, cout, ctypes.byref(tiles), ctypes.byref(chunks)),
               "gwen_conv3x3_grad_weight_plan")
    return tiles.value, chunks.value


def conv3x3_grad_weight(g: Tensor, x: Tensor, transposed: bool = False, contract: Optional[str] = None) -> Tensor:
    """The 3x3 weight gradient (gwen_conv3x3_grad_weight_f32): ``g`` [B, H, W, Cout] the gradient of the convolution's
    output, ``x`` [B, H, W, Cin] its input, both channels-last, channel slices allowed.  Returns the layer's weight
    shape: [Cout, Cin, 3, 3], or ``transposed`` a ConvTranspose2d's [Cin, Cout, 3, 3].  ``contract`` as ``conv3x3``."""
    b, h, w, cout, ldg = _nhwc(g, "g")
    xb, xh, xw, cin, ldx = _nhwc(x, "x")
    if (xb, xh, xw) != (b, h, w) or x.device != g.device:
        raise ValueError(f"g {tuple(g.shape)} and x {tuple(x.shape)} must agree in [B, H, W] and device")
    dev = g.device
    gw = torch.empty((cin, cout, 3, 3) if transposed else (cout, cin, 3, 3), dtype=torch.float32, device=dev)
    code = _dense_code(contract or "bf16x6")
    nws = max(int(_lib.lib().gwen_conv3x3_grad_weight_workspace_floats(b, h, w, cin, cout)), 0)
    ws = torch.empty(nws, dtype=torch.float32, device=dev) if nws > 0 else None
    with torch.cuda.device(dev):
        rc = _lib.lib().gwen_conv3x3_grad_weight_f32(_ptr(g), _ptr(x), _ptr(gw), b, h, w, cin, cout, ldg, ldx,
                                                     int(transposed), code, _ptr(ws), nws, _stream(dev))
    _lib.check(rc, "gwen_conv3x3_grad_weight_f32")
    return gw


def upsample2x_backward(g: Tensor, mask_from: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """The adjoint of ``upsample2x`` (gwen_upsample2x_backward_f32, a gather): ``g`` [B, 2H, 2W, C] -> [B, H, W, C].
    ``mask_from``: a tensor of g's shape; g counts only where it is > 0 (the ReLU after the upsample)."""
    b, h2, w2, c, ldg = _nhwc(g, "g")
    if h2 % 2 or w2 % 2:
        raise ValueError(f"g must be [B, 2H, 2W, C], got {tuple(g.shape)}")
    h, w = h2 // 2, w2 // 2
    dev = g.device
    ldm = c
    if mask_from is not None:
        mb, mh, mw, mc, ldm = _nhwc(mask_from, "mask_from")
        if (mb, mh, mw, mc) != (b, h2, w2, c) or mask_from.device != dev:
            raise ValueError(f"mask_from must have g's shape {tuple(g.shape)}, got {tuple(mask_from.shape)}")
    if out is None:
        out = torch.empty(b, h, w, c, dtype=torch.float32, device=dev)
    ob, oh, ow, oc, ldo = _nhwc(out, "out")
    if (ob, oh, ow, oc) != (b, h, w, c) or out.device != dev:
        raise ValueError(f"out must be [{b}, {h}, {w}, {c}] on {dev}, got {tuple(out.shape)}")
    with torch.cuda.device(dev):
        rc = _lib.lib().gwen_upsample2x_backward_f32(_ptr(g), _ptr(mask_from), _ptr(out), b, h, w, c, ldg, ldm, ldo,
                                                     _stream(dev))
    _lib.check(rc, "gwen_upsample2x_backward_f32")
    return out


def norm_relu_backward(g_y: Tensor, y: Tensor, pre: Tensor, weight: Tensor, mean: Tensor, rstd: Tensor, train: bool):
    """Backward of ``y = relu(weight * xhat + bias)``, ``xhat = (pre - mean) * rstd`` per channel over channels-last
    [B, H, W, C] tensors (channel slices allowed): ``(g_pre, g_weight, g_bias)`` (gwen_norm_relu_backward_f32).
    ``mean`` / ``rstd``: fp64 [C], the batch's (``train``) or the running ones.  g_weight and g_bias come back as fp64
    [C] (fp64 sums in a fixed two-stage order, as ``channel_stats``); g_pre is fp32, contiguous."""
    b, h, w, c, ldg = _nhwc(g_y, "g_y")
    dev = g_y.device
    lds = []
    for name, t in (("y", y), ("pre", pre)):
        tb, th, tw, tc, ld = _nhwc(t, name)
        if (tb, th, tw, tc) != (b, h, w, c) or t.device != dev:
            raise ValueError(f"{name} must have g_y's shape {tuple(g_y.shape)}, got {tuple(t.shape)}")
        lds.append(ld)
    _require(weight, "weight")
    for name, t in (("mean", mean), ("rstd", rstd)):
        if t.dtype != torch.float64 or tuple(t.shape) != (c,) or t.device != dev:
            raise ValueError(f"{name} must be a float64 [{c}] tensor on {dev}")
    if tuple(weight.shape) != (c,) or weight.device != dev:
        raise ValueError(f"weight must be [{c}] on {dev}")
    rows = b * h * w
    nbytes = int(_lib.lib().gwen_channel_stats_workspace_bytes(rows, c))
    if nbytes == 0:
        raise ValueError(f"norm_relu_backward needs at least one row and 1 <= C <= 2048; got rows {rows}, C {c}")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    sums = torch.empty(2, c, dtype=torch.float64, device=dev)
    g_pre = torch.empty(b, h, w, c, dtype=torch.float32, device=dev)
    weight, mean, rstd = weight.detach().contiguous(), mean.contiguous(), rstd.contiguous()
    with torch.cuda.device(dev):
        rc = _lib.lib().gwen_norm_relu_backward_f32(_ptr(g_y), _ptr(y), _ptr(pre), _ptr(weight), _ptr(mean), _ptr(rstd),
                                                    _ptr(g_pre), _ptr(sums), rows, c, ldg, lds[0], lds[1], c,
                                                    int(bool(train)), _ptr(ws), nbytes, _stream(dev))
    _lib.check(rc, "gwen_norm_relu_backward_f32")
    return g_pre, sums[1], sums[0]


def unpool2x2(g_p: Tensor, argmax: Tensor, h: int, w: int) -> Tensor:
    """The 2x2 max-pool's backward (gwen_unpool2x2_f32): ``g_p`` [B, h // 2, w // 2, C] goes to each window's winner
    (``argmax`` of ``conv3x3(..., argmax=True)``) in a zero-filled [B, h, w, C]."""
    b, hp, wp, c, ldg = _nhwc(g_p, "g_p")
    if (hp, wp) != (h // 2, w // 2):
        raise ValueError(f"g_p must be [B, {h // 2}, {w // 2}, C], got {tuple(g_p.shape)}")
    if argmax.dtype != torch.uint8 or tuple(argmax.shape) != (b, hp, wp, c) or argmax.device != g_p.device:
        raise ValueError(f"argmax must be a uint8 tensor of g_p's shape {tuple(g_p.shape)} on its device")
    argmax = argmax.contiguous()
    dev = g_p.device
    out = torch.empty(b, h, w, c, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().gwen_unpool2x2_f32(_ptr(g_p), _ptr(argmax), _ptr(out), b, h, w, c, ldg, c, _stream(dev))
    _lib.check(rc, "gwen_unpool2x2_f32")
    return out
