"""GWEN's GNN model surface, same names as /root/reference/src/gwen/models_gnn.py.

``GNNConfig`` (:86-103), ``DownConvLayers`` (:106-157), ``UpConvLayers`` (:160-212),
``GCNConvLayers`` (:215-258), ``GNNModel`` (:268-303) and ``loss_func`` (:261-265), with identical
attribute names, so a reference ``state_dict`` (20 tensors) loads with
``strict=True`` in both directions and ``GNNModel.forward(x, edge_index)`` drops into the reference's
train/eval loops (:365, :444).

MI355X-side differences: the graph is prepared once per forward (not once per layer), the ReLU the
reference applies after a layer is fused into that layer's last kernel, and ``x`` may carry a
leading ensemble-member axis ``[members, N, C]`` that shares one prepared graph.
The train/eval drivers, MLflow logging and NeighborLoader of the reference file are host
orchestration and out of scope.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass

import torch
from torch import Tensor, nn

from .forward import StackForward, pack_weight, stack_apply
from .gcn_conv import GCNConv
from .graph import GraphCSR, default_cache

logger = logging.getLogger("gwen_amd")


@dataclass
class GNNConfig(dict):
    """Configuration parameters for the GNN model (models_gnn.py:86-103)."""

    nodes_in: int
    nodes_out: int
    channels_in: int
    channels_out: int
    hidden_feats: int


class DownConvLayers(nn.Module):
    """conv1..conv5 declared, conv1..conv3 used (models_gnn.py:118-130, :147-151)."""

    def __init__(self, gnn_configs: GNNConfig):
        super().__init__()
        h = gnn_configs.hidden_feats
        self.conv1 = GCNConv(gnn_configs.channels_in, h)
        self.conv2 = GCNConv(h, h // 2)
        self.conv3 = GCNConv(h // 2, h // 4)
        self.conv4 = GCNConv(h // 4, h // 8)
        self.conv5 = GCNConv(h // 8, h // 16)

    def forward(self, x: Tensor, edge_index) -> Tensor:
        try:
            x = self.conv1(x, edge_index, relu=True)
            x = self.conv2(x, edge_index, relu=True)
            x = self.conv3(x, edge_index, relu=True)
        except Exception as e:
            logger.error("Error occurred while performing forward pass in DownConvLayers: %s", e)
            raise
        return x


class UpConvLayers(nn.Module):
    """upconv1..upconv5 declared, upconv3..upconv5 used (models_gnn.py:172-184, :202-206)."""

    def __init__(self, gnn_configs: GNNConfig):
        super().__init__()
        h = gnn_configs.hidden_feats
        self.upconv1 = GCNConv(h // 16, h // 8)
        self.upconv2 = GCNConv(h // 8, h // 4)
        self.upconv3 = GCNConv(h // 4, h // 2)
        self.upconv4 = GCNConv(h // 2, h)
        self.upconv5 = GCNConv(h, gnn_configs.channels_out)

    def forward(self, x: Tensor, edge_index) -> Tensor:
        try:
            x = self.upconv3(x, edge_index, relu=True)
            x = self.upconv4(x, edge_index, relu=True)
            x = self.upconv5(x, edge_index)
        except Exception as e:
            logger.error("Error occurred while performing forward pass in UpConvLayers: %s", e)
            raise
        return x


class GCNConvLayers(nn.Module):
    """down stack then up stack (models_gnn.py:235-236, :252-253)."""

    def __init__(self, gnn_configs: GNNConfig):
        super().__init__()
        self.down_conv_layers = DownConvLayers(gnn_configs)
        self.up_conv_layers = UpConvLayers(gnn_configs)

    def forward(self, x: Tensor, edge_index) -> Tensor:
        x = self.down_conv_layers(x, edge_index)
        x = self.up_conv_layers(x, edge_index)
        return x


class _MaskedL1(torch.autograd.Function):
    """gwen_masked_l1_f32: the loss value and its gradient in one pass over (output, target)."""

    @staticmethod
    def forward(ctx, output: Tensor, target: Tensor, mask: Tensor) -> Tensor:
        from . import _lib
        from .graph import _ptr, _stream
        o, t = output.contiguous(), target.contiguous()
        m = mask.contiguous()                            # bool [N] (loss_func sends nothing else here)
        n, c = o.size(-2), o.size(-1)
        members = o.numel() // (n * c) if n * c else 0
        dev = o.device
        grad = torch.empty_like(o) if ctx.needs_input_grad[0] else None
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        nws = int(_lib.lib().gwen_masked_l1_workspace_floats())
        ws = torch.empty(nws, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.lib().gwen_masked_l1_f32(_ptr(o), _ptr(t), _ptr(m.view(torch.uint8)), members, n, c, _ptr(grad),
                                               _ptr(loss), _ptr(ws), nws, _stream(dev))
        _lib.check(rc, "gwen_masked_l1_f32")
        ctx.save_for_backward(*([grad] if grad is not None else []))
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        saved = ctx.saved_tensors
        return (saved[0] * g if saved else None), None, None


def loss_func(output: Tensor, target: Tensor, target_mask: Tensor) -> Tensor:
    """L1 on the masked rows (models_gnn.py:261-265): the mean of |output - target| over the rows the mask
    selects.  The reference writes it with boolean indexing, ``l1_loss(output[mask], target[mask])``, which on
    a device costs a nonzero() + sort + two gathers and a host synchronisation per step (~100 us of the c2
    training step); the same mean as a masked sum needs neither.  Only the summation order differs.
    BOOL masks (what the reference's dataset produces, utils.py:205) take that path: fp32 tensors on the GPU
    (channels a multiple of 4, target without a gradient) in ONE fused pass that yields the value and the gradient
    (gwen_masked_l1_f32: 3 launches instead of ~14), other bool-masked inputs as tensor ops.  Any other mask --
    an integer INDEX tensor selects (and may repeat) rows -- is the reference's own expression."""
    if output.dim() < 2 or output.shape != target.shape or target_mask.dtype != torch.bool \
            or target_mask.dim() != 1 or target_mask.numel() != output.size(-2):
        return torch.nn.functional.l1_loss(output[target_mask], target[target_mask])
    if (output.is_cuda and output.dtype == torch.float32 and target.dtype == torch.float32 and not target.requires_grad
            and output.size(-1) % 4 == 0):
        return _MaskedL1.apply(output, target, target_mask)
    m = target_mask.to(output.dtype).unsqueeze(-1)                  # [N, 1] (broadcasts over a members axis)
    picked = m.sum() * output.size(-1) * (output.numel() // (output.size(-1) * output.size(-2)))
    return ((output - target).abs() * m).sum() / picked


class GNNModel(nn.Module):
    """``forward(x, edge_index) -> [N, channels_out]`` (models_gnn.py:292-303)."""

    def __init__(self, gnn_configs: GNNConfig) -> None:
        super().__init__()
        self.conv_layers = GCNConvLayers(gnn_configs)
        self.activation = torch.nn.ReLU()
        self._packed = {}        # layer index -> (weight identity/version, packed image) for K7
        self._packw = {}         # the same for K4 / K5 (StackForward's packw_cache)

    def __getstate__(self):      # derived data: keep the module picklable (mp.spawn, mlflow) and small
        state = self.__dict__.copy()
        state["_packed"] = {}
        state["_packw"] = {}
        return state

    def _packed_weights(self, graph: GraphCSR):
        """Fragment-ordered weight images for K7 (small graphs, e.g. the reference's member graphs):
        packed once per weight VERSION, so the eval loop re-uses them across batches and time steps
        although every batch brings a new edge_index (models_gnn.py:351-360).  None on large graphs."""
        if graph.dense() is None:
            return None
        out = []
        for i, (w, _, _, order) in enumerate(self.stack()):
            key = (w.data_ptr(), w._version, tuple(w.shape))
            hit = self._packed.get(i)
            if hit is None or hit[0] != key:
                hit = (key, pack_weight(w) if order == "auto_x3" else None)     # the packed images are 3xbf16's
                self._packed[i] = hit
            out.append(hit[1])
        return out

    def set_precision(self, precision: str) -> "GNNModel":
        """"f16x3" (default), "bf16x6", "3xbf16" or "fp32" for every layer (``GCNConv.precision``); returns self."""
        for mod in self.modules():
            if isinstance(mod, GCNConv):
                mod.precision = precision
        return self

    def prepare(self, edge_index: Tensor, num_nodes: int) -> GraphCSR:
        """Prepare (or fetch) the normalised graph all six layers share."""
        return default_cache().get(edge_index, num_nodes, None, add_self_loops=True,
                                   improved=False, normalize=True)

    def stack(self):
        """The six layers the forward uses, in order, as (weight, bias, relu, order)."""
        d, u = self.conv_layers.down_conv_layers, self.conv_layers.up_conv_layers
        used = [(d.conv1, True), (d.conv2, True), (d.conv3, True), (u.upconv3, True),
                (u.upconv4, True), (u.upconv5, False)]
        return [(c.lin.weight, c.bias, relu, c.order) for c, relu in used]

    def forward(self, x: Tensor, edge_index) -> Tensor:
        if not isinstance(edge_index, GraphCSR):
            edge_index = self.prepare(edge_index, x.size(-2))
        needs_grad = torch.is_grad_enabled() and (
            x.requires_grad or any(p.requires_grad for p in self.parameters()))
        if needs_grad:
            # training: the whole stack as one autograd node (one host call per direction) on graphs beyond
            # K7's size; the per-layer autograd Functions on the reference's small member graphs
            if edge_index.dense() is None and edge_index.long_row_levels() is None and \
                    all(b is not None for _, b, _, _ in self.stack()):
                return stack_apply(x, edge_index, self.stack())
            return self.conv_layers(x, edge_index)
        # inference: the whole stack from one host call (gwen_gnn_forward_f32)
        return StackForward(self.stack(), edge_index, self._packed_weights(edge_index),
                            getattr(self, "_packw", None)).run(x)
