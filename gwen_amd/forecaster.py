"""Encode-process-decode forecaster on InteractionNet blocks (BASELINE config c5).

BUILD-DEFINED, PARITY UNPINNED -- the reference has neither grid/mesh graphs nor edge MLPs nor a
rollout (its model is six GCNConv calls, /root/reference/src/gwen/models_gnn.py:
135-157,:189-212).  BASELINE.json's north_star names "the InteractionNet/GraphConv edge-MLP +
scatter-add node-aggregation block that propagates atmospheric state over the grid->mesh->grid graphs
each rollout step"; this module is that loop, with semantics of this build's own choosing (restated on
the CPU in oracle/interaction_oracle.py):

    vg  = grid_x  Wg^T + bg                 vm = mesh_pos Wm^T + bm              (embedders, K3)
    e_* = edge_feat_* We_*^T + be_*         edge_feat = [length, dx, dy, dz] of the edge
    vm      = Encoder(vg, vm, e_g2m)        InteractionNet, grid -> mesh   (gwen_amd/interaction.py, K6)
    vm, e_m = Processor_k(vm, vm, e_m)      InteractionNet, mesh -> mesh,  k = 1..steps
    vg      = Decoder(vm, vg, e_m2g)        InteractionNet, mesh -> grid
    (``processor="transformer"``: the processor blocks are ``attention.GraphTransformer``s instead -- multi-head attention
     over a mesh node's in-edges with the edge term ee_k = lin_e_k(e_m), a static embedding like e_m itself)
    grid_y  = grid_x + vg Wo^T + bo                                          (residual read-out, K3)

The grid is the set of triangle centres of the geodesic mesh; every cell is linked with its three
corner vertices (gwen_amd/g2m.py) -- or, with ``prepare(..., grid_pos=)``, any point set on the sphere, linked to the
mesh by radius (grid -> mesh) and by containing face (mesh -> grid) (gwen_amd/gridgraph.py).  Static embeddings (vm, e_*) depend on the weights only and are
computed once per ``forward`` / ``rollout`` call.  Trainable (``interaction._InteractionNetFunction``), over several lead
times with ``rollout(grad=True)`` (gwen_amd/checkpoint.py: one step's activations at a time).  A leading members axis
``[members, N_grid, C]`` runs as ONE launch set over the block-diagonal graph (``ForecastGraphs.batched``).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch
from torch import Tensor, nn

from . import forcings as forcings_mod
from . import noise as noise_mod
from . import ops
from .g2m import grid_mesh_edges
from .attention import GraphTransformer
from .checkpoint import checkpointed_step
from .interaction import EdgeGraph, InteractionNet, interaction_graph
from .mesh import Mesh


def edge_features(pos_src: np.ndarray, pos_dst: np.ndarray, edge_index: np.ndarray) -> np.ndarray:
    """[E, 4] float32: chord length and displacement (target - source) of every edge."""
    d = pos_dst[edge_index[1]] - pos_src[edge_index[0]]
    return np.concatenate([np.linalg.norm(d, axis=1, keepdims=True), d], axis=1).astype(np.float32)


@dataclass
class ForecastGraphs:
    g2m: EdgeGraph
    mesh: EdgeGraph
    m2g: EdgeGraph
    mesh_pos: Tensor        # [Nm, 3]
    f_g2m: Tensor           # [E, 4] each, in the STORED edge order of its graph
    f_mesh: Tensor
    f_m2g: Tensor
    _batched: dict = None   # members -> ForecastGraphs of the block-diagonal graphs
    members: int = 1        # copies of the graphs these are (mesh latent row r = node r % Nm of member r // Nm)
    grid_latlon: Tensor = None   # [N, 2] float64 radians (lat, lon) of ONE member's grid points: members share them
    grid_static: Tensor = None   # [N, S] fp32 static fields of ONE member's grid points, or None

    def batched(self, members: int) -> "ForecastGraphs":
        """Graphs and static inputs of ``members`` independent copies (EdgeGraph.batched): the c5 path rolls
        every local member through ONE launch set per step."""
        if members == 1:
            return self
        if self._batched is None:
            self._batched = {}
        if members not in self._batched:
            rep = lambda t: t.repeat(members, 1)                                   # noqa: E731
            self._batched[members] = ForecastGraphs(
                self.g2m.batched(members), self.mesh.batched(members), self.m2g.batched(members),
                rep(self.mesh_pos), rep(self.f_g2m), rep(self.f_mesh), rep(self.f_m2g), members=members,
                grid_latlon=self.__dict__.get("grid_latlon"), grid_static=self.__dict__.get("grid_static"))
        return self._batched[members]

    @property
    def mesh_nodes(self) -> int:
        """Mesh nodes of ONE member."""
        return self.mesh_pos.size(0) // self.__dict__.get("members", 1)

    @property
    def grid_nodes(self) -> int:
        """Grid points of ONE member: the rows of the ``grid_x`` these graphs take."""
        return self.g2m.num_src // self.__dict__.get("members", 1)


class InteractionForecaster(nn.Module):
    """``precision`` ("3xbf16", the default, or "f16x3": fp32-class) applies to every contraction of the model -- the
    blocks (``InteractionNet.precision``) and the embedding / read-out ``Linear``s; ``set_precision`` changes it.  Not
    part of ``state_dict()``.  A captured step (``GraphedStep``, ``ensemble_forecast``) keeps the precision it was
    captured with.

    ``noise_channels`` K > 0 (8, 16, 32 or 64) adds latent noise: once per step, between the encoder and the
    processor, ``vm += z Wz^T`` with z drawn per member, node and step from a ``noise.NoiseStream`` passed as ``noise=``
    (``noise_embed`` = Wz, an ``nn.Linear(K, hidden, bias=False)``, zero-initialised: a fresh noisy model computes what
    its deterministic self computes).  Without ``noise=`` the step is deterministic (z = 0).  Every call that takes a
    stream leaves it ``n_steps`` draws further on; member m at step t of a call that starts at draw d gets
    z(seed, 0, d + t, m, node, k), whichever path runs it.

    ``layer_norm=True`` (off by default; ``norm_eps``): the encoder, every processor block and the decoder normalise both
    MLP outputs (``InteractionNet(layer_norm=True)``: m_e = LN(MLP_e(..)), x' = x + LN(MLP_n(..))); the embedders and the
    read-out stay plain ``Linear``s.

    ``processor="transformer"`` (default "interaction"; ``heads``, 8 by default): the ``steps`` processor blocks are
    ``attention.GraphTransformer(hidden, heads)``s over the mesh graph -- pre-norm attention with an edge term and a
    feed-forward half; they carry their own LayerNorms (``norm_eps``), whatever ``layer_norm`` says, which then applies
    to the encoder and the decoder only.  Each block's edge term ``lin_e(e_m)`` depends on weights only and joins the
    static embeddings: a rollout step holds no edge-sized dense product.  Mesh edges are not updated.  Encoder and
    decoder stay InteractionNet; everything else (members, noise, graphed rollouts, ``set_precision``) works alike.

    Inputs that are never predicted (all off by default), added to the grid embedding in one launch per step
    (``forcings.embed``): ``vg = grid_embed(grid_x) + static_embed(grid_static) + forcing_embed(f)``.
    ``static_channels`` S > 0: ``graphs.grid_static`` [N, S] (``prepare(..., grid_static=)``: orography, land-sea mask, ...),
    the same for every member and every step; its embedding joins the static embeddings.  ``solar=True``: the 5 solar /
    time channels of ``forcings.solar`` at the time of a ``forcings.ForcingClock`` passed as ``clock=``, evaluated at
    ``graphs.grid_latlon``.  ``forcing_channels`` Fg > 0: given fields (SST, boundary data) passed as ``forcing=``, [N, Fg]
    for one step and [n_steps, N, Fg] for a rollout.  f = [solar, given], at most 64 columns.  Every call that takes a
    clock leaves it ``n_steps`` steps further on.  A model that needs a clock, a forcing or a static field and is not
    given one raises ``ValueError``."""

    def __init__(self, grid_channels: int, hidden: int, steps: int = 4, activation: str = "silu",
                 aggr: str = "sum", precision: str = "3xbf16", noise_channels: int = 0, layer_norm: bool = False,
                 norm_eps: float = 1e-5, processor: str = "interaction", heads: int = 8, static_channels: int = 0,
                 solar: bool = False, forcing_channels: int = 0):
        super().__init__()
        if processor not in ("interaction", "transformer"):
            raise ValueError(f"processor must be 'interaction' or 'transformer', got {processor!r}")
        self.processor_kind = processor
        self.grid_channels, self.hidden, self.steps = grid_channels, hidden, steps
        self.grid_embed = nn.Linear(grid_channels, hidden)
        self.mesh_embed = nn.Linear(3, hidden)
        self.g2m_edge_embed = nn.Linear(4, hidden)
        self.mesh_edge_embed = nn.Linear(4, hidden)
        self.m2g_edge_embed = nn.Linear(4, hidden)
        ln = {"layer_norm": True, "norm_eps": norm_eps} if layer_norm else {}        # (off: the blocks as they were)
        self.layer_norm = bool(layer_norm)
        self.encoder = InteractionNet(hidden, activation, aggr, **ln)
        if processor == "transformer":
            self.heads = heads
            self.processor = nn.ModuleList([GraphTransformer(hidden, heads, activation, norm_eps=norm_eps)
                                            for _ in range(steps)])
        else:
            self.processor = nn.ModuleList([InteractionNet(hidden, activation, aggr, **ln) for _ in range(steps)])
        self.decoder = InteractionNet(hidden, activation, aggr, **ln)
        self.readout = nn.Linear(hidden, grid_channels)
        self.set_precision(precision)
        if noise_channels not in (0,) + noise_mod.INJECT_CHANNELS:
            raise ValueError(f"noise_channels must be 0 or one of {noise_mod.INJECT_CHANNELS}, got {noise_channels}")
        self.noise_channels = noise_channels
        if noise_channels:
            self.noise_embed = nn.Linear(noise_channels, hidden, bias=False)
            nn.init.zeros_(self.noise_embed.weight)
        width = forcings_mod.SOLAR_CHANNELS * bool(solar) + forcing_channels
        if static_channels < 0 or forcing_channels < 0 or width > forcings_mod.MAX_CHANNELS or \
                (width == 0 and static_channels > forcings_mod.MAX_CHANNELS):
            raise ValueError(f"static_channels >= 0 and 0 <= 5 solar + forcing_channels <= {forcings_mod.MAX_CHANNELS} "
                             f"expected, got {static_channels}, {solar}, {forcing_channels}")
        if (static_channels or width) and hidden % 4:
            raise ValueError(f"static fields and forcings need hidden % 4 == 0, got {hidden}")
        self.static_channels, self.solar, self.forcing_channels = static_channels, bool(solar), forcing_channels
        if static_channels:
            self.static_embed = nn.Linear(static_channels, hidden, bias=False)
        if width:
            self.forcing_embed = nn.Linear(width, hidden, bias=False)

    def set_precision(self, p: str) -> "InteractionForecaster":
        """The contraction of the encoder, the processors, the decoder and the six embedding / read-out layers."""
        for net in (self.encoder, *self.processor, self.decoder):
            net.precision = p                                # (validates p: "3xbf16" or "f16x3")
        self.precision = p
        return self

    @staticmethod
    def prepare(mesh: Mesh, device, grid_pos=None, radius: Optional[float] = None,
                grid_static=None) -> ForecastGraphs:
        """``grid_pos=None``: the grid is the mesh's own triangle centres.  ``grid_pos`` ``[N, 3]`` (any points on the
        sphere: ``gridgraph.latlon_grid``, ``gridgraph.sphere_points`` of ICON cell centres, ...): the grid <-> mesh
        graphs come from ``gridgraph.grid_graphs`` -- every grid point sends to the mesh nodes within ``radius`` (default
        0.6 x the longest mesh edge) and receives from the corners of the mesh face that contains it.
        ``grid_latlon`` is always filled from the grid's unit vectors (on the default grid: of the face centres);
        ``grid_static`` [N, S]: the static fields of a model with ``static_channels=S``."""
        if grid_pos is not None:
            return _prepare_on_grid(mesh, device, grid_pos, radius, grid_static)
        if radius is not None:
            raise ValueError("radius applies to grid_pos; the default grid is linked to the corners of its own faces")
        g2m, m2g = grid_mesh_edges(mesh)
        n_mesh, n_grid = mesh.num_nodes, mesh.faces.shape[0]
        cell = mesh.pos[mesh.faces].mean(axis=1)
        cell /= np.linalg.norm(cell, axis=1, keepdims=True)
        gs = (interaction_graph(torch.from_numpy(g2m).to(device), n_grid, n_mesh),
              interaction_graph(torch.from_numpy(mesh.edge_index).to(device), n_mesh, n_mesh),
              interaction_graph(torch.from_numpy(m2g).to(device), n_mesh, n_grid))
        feats = (edge_features(cell, mesh.pos, g2m), edge_features(mesh.pos, mesh.pos, mesh.edge_index),
                 edge_features(mesh.pos, cell, m2g))
        fs = [g.sort_edges(torch.from_numpy(f).to(device)) for g, f in zip(gs, feats)]
        return ForecastGraphs(*gs, torch.from_numpy(mesh.pos.astype(np.float32)).to(device), *fs,
                              **_grid_fields(cell, grid_static, device))

    def _lin(self, x: Tensor, m: nn.Linear) -> Tensor:
        """K3 on the model's precision, as the blocks around it ("3xbf16": bf16x3; "f16x3": K3's fp32-class split);
        with autograd when gradients are needed (ops.LinearFunction: the backward runs on K3 and the gradient
        reductions too)."""
        prec = self.__dict__.get("precision", "3xbf16")        # (a model pickled before the setting existed)
        if torch.is_grad_enabled() and (x.requires_grad or m.weight.requires_grad):
            return ops.linear_autograd(x, m.weight, m.bias, contract=prec)
        if prec == "3xbf16":
            return ops.linear(x, m.weight, m.bias, exact=False)
        return ops.linear(x, m.weight, m.bias, contract=prec)

    def _static(self, graphs: ForecastGraphs):
        lin = self._lin
        static = (lin(graphs.mesh_pos, self.mesh_embed), lin(graphs.f_g2m, self.g2m_edge_embed),
                  lin(graphs.f_mesh, self.mesh_edge_embed), lin(graphs.f_m2g, self.m2g_edge_embed))
        if self.__dict__.get("processor_kind", "interaction") == "transformer":      # (a model pickled before: interaction)
            static += ([net.edge_term(static[2]) for net in self.processor],)        # every block's ee = lin_e(e_m)
        S, width = self._forcing_widths()
        if S and width:                                       # (S alone: the static fields ARE the forcing columns)
            static += (lin(self._grid_static(graphs, S), self.static_embed),)        # base [N, hidden], members share it
        return static

    def _forcing_widths(self):
        """(static channels, forcing columns 5 solar + Fg); a model pickled before the settings existed: (0, 0)."""
        d = self.__dict__
        return d.get("static_channels", 0), forcings_mod.SOLAR_CHANNELS * d.get("solar", False) + d.get("forcing_channels", 0)

    @staticmethod
    def _grid_static(graphs: ForecastGraphs, S: int) -> Tensor:
        gs = graphs.__dict__.get("grid_static")
        if gs is None or gs.size(1) != S:
            raise ValueError(f"the model has static_channels={S}: prepare(..., grid_static=[N, {S}]) "
                             f"(got {None if gs is None else tuple(gs.shape)})")
        return gs

    def _forced(self, vg: Tensor, graphs: ForecastGraphs, base: Optional[Tensor], clock, forcing) -> Tensor:
        """vg + static_embed(grid_static) + forcing_embed([solar, forcing]): one launch, in place without autograd."""
        S, width = self._forcing_widths()
        d = self.__dict__
        sol, Fg = d.get("solar", False), d.get("forcing_channels", 0)
        if sol and clock is None:
            raise ValueError("the model has solar=True: pass clock= (a forcings.ForcingClock)")
        if Fg and (forcing is None or forcing.dim() != 2 or forcing.size(1) != Fg):
            raise ValueError(f"the model has forcing_channels={Fg}: pass forcing= [N, {Fg}] per step "
                             f"(got {None if forcing is None else tuple(forcing.shape)})")
        if width:
            wf, given = self.forcing_embed.weight, forcing if Fg else None
        else:
            wf, given = self.static_embed.weight, self._grid_static(graphs, S)
        grad = torch.is_grad_enabled() and (vg.requires_grad or wf.requires_grad
                                            or (base is not None and base.requires_grad))
        return forcings_mod.embed(vg, clock if sol else None, graphs.grid_latlon if sol else None, given, wf, base,
                                  graphs.grid_nodes, out=None if grad else vg)

    def _step(self, grid_x: Tensor, graphs: ForecastGraphs, static, out: Optional[Tensor] = None,
              noise: Optional["noise_mod.NoiseStream"] = None, member0: int = 0,
              clock: Optional["forcings_mod.ForcingClock"] = None, forcing: Optional[Tensor] = None) -> Tensor:
        """One step; with ``noise``: the latent noise of members ``member0 ..`` at the stream's draw, which the step
        then advances by one (in stream order: captured with the step).  ``clock`` / ``forcing``: the time of the solar
        forcings, which the step then advances by one ``dt``, and the given forcing fields [N, Fg] of this step."""
        vm, e_g2m, e_m, e_m2g, *ees = static
        S, width = self._forcing_widths()
        base = ees.pop() if S and width else None
        vg = self._lin(grid_x, self.grid_embed)
        if S or width:
            vg = self._forced(vg, graphs, base, clock, forcing)
        if clock is not None:
            clock.advance(1)
        vm, _ = self.encoder(vg, vm, e_g2m, graphs.g2m, update_edges=False)
        if noise is not None:
            if self.__dict__.get("noise_channels", 0):             # (a model pickled before the setting existed: 0)
                wz = self.noise_embed.weight
                grad = torch.is_grad_enabled() and (vm.requires_grad or wz.requires_grad)
                vm = noise_mod.inject(vm, wz, noise, graphs.mesh_nodes, member0, out=None if grad else vm)
            noise.advance(1)
        if ees:                                                    # processor="transformer": attention blocks
            for net, ee in zip(self.processor, ees[0]):
                vm, _ = net(vm, vm, e_m, graphs.mesh, ee=ee)
        else:
            for net in self.processor:
                vm, e_m = net(vm, vm, e_m, graphs.mesh)
        vg, _ = self.decoder(vm, vg, e_m2g, graphs.m2g, update_edges=False)
        delta = self._lin(vg, self.readout)
        return grid_x + delta if out is None else torch.add(grid_x, delta, out=out)      # (out: GraphedStep's buffers)

    def forward(self, grid_x: Tensor, graphs: ForecastGraphs, noise: Optional["noise_mod.NoiseStream"] = None,
                member0: int = 0, clock: Optional["forcings_mod.ForcingClock"] = None,
                forcing: Optional[Tensor] = None) -> Tensor:
        """``grid_x`` [N_grid, C] or [members, N_grid, C] (members share graphs and weights: one launch set
        over the block-diagonal graph).  ``noise``: latent noise of members ``member0 ..`` (advances the stream by 1).
        ``clock``, ``forcing`` [N_grid, Fg]: the forcings, shared by the members (advances the clock by 1)."""
        if grid_x.dim() == 3:
            m = grid_x.size(0)
            gb = graphs.batched(m)
            return self._step(grid_x.reshape(-1, grid_x.size(-1)), gb, self._static(gb), noise=noise,
                              member0=member0, clock=clock, forcing=forcing).view_as(grid_x)
        return self._step(grid_x, graphs, self._static(graphs), noise=noise, member0=member0, clock=clock,
                          forcing=forcing)

    def rollout(self, grid_x: Tensor, graphs: ForecastGraphs, n_steps: int,
                graphed: bool = False, noise: Optional["noise_mod.NoiseStream"] = None,
                member0: int = 0, clock: Optional["forcings_mod.ForcingClock"] = None,
                forcing: Optional[Tensor] = None, grad: bool = False, checkpoint: bool = True) -> List[Tensor]:
        """Autoregressive: state_{t+1} = forward(state_t); returns the n_steps states.
        ``graphed``: capture ONE step (its ~26 launches) into a hipGraph and replay it per step -- the
        launchers allocate and synchronise nothing, so the step is capturable as is; worth it when the
        host cannot keep ahead of the device (64 channels: 1.31 -> 1.14 ms per step; 128: 2.71 -> 2.39).
        ``clock``: the time of step 0's forcings (left ``n_steps`` steps on); ``forcing`` [n_steps, N, Fg]: step t's
        given fields.

        ``grad=True``: the states take part in autograd (train on a loss over several lead times).  ``grid_x`` is then
        [N, C] or [members, N, C] (one launch set over the block-diagonal graph, as ``forward``), the static embeddings are
        computed once per call, under autograd, and the stream and the clock end ``n_steps`` further on; the backward does
        not move them.  ``checkpoint`` (default): every step keeps its input state only and its backward runs the step's
        forward again (``checkpoint.checkpointed_step``) -- one step's activations alive at a time, for one more forward
        per step.  ``checkpoint=False``: the plain chain of steps, every step's saved tensors alive until the backward
        (for comparison and small models).  Not with ``graphed``: a captured step holds the static embeddings of the
        weights at capture time and no autograd graph."""
        _check_forcing_steps(forcing, n_steps)
        states, cur = [], grid_x
        kw = {} if noise is None else {"noise": noise, "member0": member0}
        if clock is not None:
            kw["clock"] = clock
        per_step = (lambda t: {}) if forcing is None else (lambda t: {"forcing": forcing[t]})      # noqa: E731
        if grad:
            if graphed:
                raise ValueError("rollout: grad=True cannot replay a captured step (graphed=True): it holds the static "
                                 "embeddings of the weights at capture time")
            if grid_x.dim() == 3:
                graphs = graphs.batched(grid_x.size(0))
                cur = grid_x.reshape(-1, grid_x.size(-1))
            static = self._static(graphs)
            for t in range(n_steps):
                if checkpoint:
                    cur = checkpointed_step(self, cur, graphs, static, **kw, **per_step(t))
                else:
                    cur = self._step(cur, graphs, static, **kw, **per_step(t))
                states.append(cur.view_as(grid_x) if grid_x.dim() == 3 else cur)
            return states
        with torch.no_grad():
            if graphed:
                step = GraphedStep(self, graphs, grid_x, **kw, **per_step(0))
                for t in range(n_steps):
                    cur = step(cur, **per_step(t))           # (one of the step's two buffers: the next call reads it in place)
                    states.append(cur.clone())
                return states
            static = self._static(graphs)
            for t in range(n_steps):
                cur = self._step(cur, graphs, static, **kw, **per_step(t))
                states.append(cur)
        return states


def _check_forcing_steps(forcing: Optional[Tensor], n_steps: int) -> None:
    if forcing is not None and (forcing.dim() != 3 or forcing.size(0) != n_steps):
        raise ValueError(f"forcing must be [n_steps = {n_steps}, N, Fg], got {tuple(forcing.shape)}")


def _prepare_on_grid(mesh: Mesh, device, grid_pos, radius: Optional[float], grid_static=None) -> ForecastGraphs:
    """``InteractionForecaster.prepare`` for given grid points: edges from ``gridgraph.grid_graphs`` (built on the device),
    features ``[length, dx, dy, dz]`` over the normalised points, as on the default grid."""
    from . import gridgraph
    grid = gridgraph.unit_vectors(grid_pos, "grid_pos")
    g2m_t, m2g_t, _ = gridgraph.grid_graphs(mesh, grid_pos, device, radius)
    n_mesh, n_grid = mesh.num_nodes, grid.shape[0]
    gs = (interaction_graph(g2m_t, n_grid, n_mesh),
          interaction_graph(torch.from_numpy(mesh.edge_index).to(device), n_mesh, n_mesh),
          interaction_graph(m2g_t, n_mesh, n_grid))
    feats = (edge_features(grid, mesh.pos, g2m_t.cpu().numpy()), edge_features(mesh.pos, mesh.pos, mesh.edge_index),
             edge_features(mesh.pos, grid, m2g_t.cpu().numpy()))
    fs = [g.sort_edges(torch.from_numpy(f).to(device)) for g, f in zip(gs, feats)]
    return ForecastGraphs(*gs, torch.from_numpy(mesh.pos.astype(np.float32)).to(device), *fs,
                          **_grid_fields(grid, grid_static, device))


def _grid_fields(grid: np.ndarray, grid_static, device) -> dict:
    """``grid_latlon`` (lat = atan2(z, hypot(x, y)), lon = atan2(y, x) of the unit vectors, float64 radians) and
    ``grid_static`` of a ``ForecastGraphs``."""
    g = np.asarray(grid, dtype=np.float64)
    latlon = np.stack([np.arctan2(g[:, 2], np.hypot(g[:, 0], g[:, 1])), np.arctan2(g[:, 1], g[:, 0])], axis=1)
    if grid_static is not None:
        grid_static = torch.as_tensor(grid_static, dtype=torch.float32)
        if grid_static.dim() != 2 or grid_static.size(0) != g.shape[0]:
            raise ValueError(f"grid_static must be [{g.shape[0]}, S], got {tuple(grid_static.shape)}")
        grid_static = grid_static.to(device).contiguous()
    return {"grid_latlon": torch.from_numpy(latlon).to(device), "grid_static": grid_static}


def ensemble_forecast(model, graphs: ForecastGraphs, x_members: Tensor,
                      n_steps: int, num_members: int, group=None, graphed: bool = True,
                      batched: bool = True, step_cache: dict = None, gather: bool = True,
                      noise=None, member0: Optional[int] = None, clock=None, forcing: Optional[Tensor] = None) -> Tensor:
    """BASELINE config c5: this rank's members ``[members_local, N_grid, C]`` are rolled out ``n_steps``
    steps (independent members, replicated graph and weights), then every rank's final states are gathered
    ONCE (``ensemble.gather_members``: RCCL all-gather over xGMI under the "nccl" backend).  Returns
    ``[num_members, N_grid, C]`` on every rank.

    ``batched`` (default): all local members advance together -- ONE launch set per step over the
    block-diagonal graph (``ForecastGraphs.batched``), captured once and replayed when ``graphed``.
    ``batched=False``: one member after the other (the same arithmetic; kept for comparison).
    ``step_cache``: a dict the captured step lives in between calls (capture costs one eager step plus the
    capture itself; the static embeddings inside it are those of the weights at capture time).
    ``gather=False`` returns this rank's final states ``[members_local, N_grid, C]`` without the collective.
    ``noise`` (a ``noise.NoiseStream``): latent noise.  This rank's first member is ``member0``, by default
    ``ensemble.member_range(num_members, rank, world)[0]``; every rank holds the same seed and the same draw, so member m
    gets the same noise on any rank and in any path.  The stream ends ``n_steps`` draws further on, on every rank, also
    on one that holds no member (the member-by-member path rewinds it between members).  Cost: ``member0`` is a kernel
    argument, so the graphed member-by-member path with ``noise`` captures one step per member (an eager warm-up step
    and two graph captures each) -- on every call unless ``step_cache`` keeps them; the batched path captures once.
    ``clock`` (a ``forcings.ForcingClock``), ``forcing`` [n_steps, N_grid, Fg]: the forcings of a model that takes them,
    shared by the members.  The clock ends ``n_steps`` steps further on, on every rank (rewound between members on the
    member-by-member path, like the noise).
    ``model`` needs ``_static(graphs)`` and ``_step(x, graphs, static)`` (InteractionForecaster; with ``noise``, also the
    ``noise=`` and ``member0=`` keywords of its ``_step``; with ``clock`` / ``forcing``, those keywords)."""
    from . import ensemble
    m_local = x_members.size(0)
    if noise is not None and member0 is None:
        dist = torch.distributed
        on = dist.is_available() and dist.is_initialized()
        rank, world = (dist.get_rank(group), dist.get_world_size(group)) if on else (0, 1)
        member0 = ensemble.member_range(num_members, rank, world)[0]
    _check_forcing_steps(forcing, n_steps)
    kw = {} if noise is None else {"noise": noise}
    if clock is not None:
        kw["clock"] = clock
    per_step = (lambda t: {}) if forcing is None else (lambda t: {"forcing": forcing[t]})      # noqa: E731

    def captured(g, x0, m0):
        if step_cache is None:
            return GraphedStep(model, g, x0, **kw, **per_step(0), **({} if noise is None else {"member0": m0}))
        key = (id(model), id(g), tuple(x0.shape)) + (() if noise is None else (id(noise), m0)) + \
            (() if clock is None else (id(clock),))
        if key not in step_cache:
            step_cache[key] = GraphedStep(model, g, x0, **kw, **per_step(0),
                                          **({} if noise is None else {"member0": m0}))
        return step_cache[key]

    def one_step(x, g, static, m0, t):
        return model._step(x, g, static, **kw, **per_step(t), **({} if noise is None else {"member0": m0}))

    with torch.no_grad():
        if m_local == 0:
            local = x_members.new_empty((0,) + tuple(x_members.shape[1:]))
            if noise is not None:
                noise.advance(n_steps)                       # a rank without members keeps the others' draw
            if clock is not None:
                clock.advance(n_steps)
        elif batched:
            gb = graphs.batched(m_local)
            cur = x_members.reshape(-1, x_members.size(-1))
            if graphed:
                step = captured(gb, cur, member0)
                for t in range(n_steps):             # (the step alternates between its two state buffers: no copies)
                    cur = step(cur, **per_step(t))
                cur = cur.clone()
            else:
                static = model._static(gb)
                for t in range(n_steps):
                    cur = one_step(cur, gb, static, member0, t)
            local = cur.view_as(x_members)
        else:
            finals = []
            static = None if graphed else model._static(graphs)
            step = captured(graphs, x_members[0], None) if graphed and noise is None else None
            for m in range(m_local):
                m0 = None if noise is None else member0 + m
                if clock is not None and m > 0:
                    clock.advance(-n_steps)                  # every member starts at the call's time
                if noise is not None:
                    if m > 0:
                        noise.advance(-n_steps)              # every member starts at the call's draw
                    if graphed:                              # (member0 is a kernel argument: one capture per member)
                        step = captured(graphs, x_members[0], m0)
                cur = x_members[m]
                for t in range(n_steps):
                    cur = step(cur, **per_step(t)) if step is not None else one_step(cur, graphs, static, m0, t)
                finals.append(cur.clone() if step is not None else cur)
            local = torch.stack(finals)
    if not gather:
        return local
    return ensemble.gather_members(local, num_members, group)


class GraphedStep:
    """One forecaster step captured into hipGraphs (``torch.cuda.CUDAGraph``) over TWO state buffers -- the graph A -> B
    and the graph B -> A -- so that an autoregressive rollout replays them alternately without copying the state (one
    capture over a fixed input / output pair cost two state-sized copies per step: 2 % of the c5 rollout).  ``step(x)``
    copies ``x`` into the next input buffer unless it IS that buffer (the previous call's result), replays, and returns the
    output buffer -- valid until the call AFTER the next one (clone it to keep it longer).

    ``noise``: the captured step injects the latent noise of members ``member0 ..`` at the stream's draw and advances it,
    so every replay draws fresh noise (the warm-up step's advance is taken back).

    ``clock``: the captured step reads the clock's time and advances it, so every replay sees the next time (the warm-up's
    advance is taken back too).  ``forcing`` [N, Fg]: the given fields live in a fixed buffer that ``step(x, forcing=f_t)``
    copies into before the replay."""

    def __init__(self, model: InteractionForecaster, graphs: ForecastGraphs, grid_x: Tensor, noise=None,
                 member0: int = 0, clock=None, forcing: Optional[Tensor] = None):
        self.bufs = [grid_x.detach().clone(), torch.empty_like(grid_x)]
        self.graphs = graphs                                 # the captured graphs hold raw pointers into these:
        self.noise = noise                                   # (and into the noise state)
        self.clock = clock                                   # (and into the clock)
        self.forcing = None if forcing is None else forcing.detach().clone().contiguous()
        self.cur = 0                                         # the buffer the next call reads
        kw = {} if noise is None else {"noise": noise, "member0": member0}
        if clock is not None:
            kw["clock"] = clock
        if forcing is not None:
            kw["forcing"] = self.forcing
        with torch.no_grad():                                # keep every tensor they read alive
            static = self._static = model._static(graphs)
            model._step(self.bufs[0], graphs, static, out=self.bufs[1], **kw)  # warm-up: occupancy queries, tilings, caches
            if noise is not None:
                noise.advance(-1)
            if clock is not None:
                clock.advance(-1)
            torch.cuda.synchronize(grid_x.device)
            self.replays = []
            for i in (0, 1):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    model._step(self.bufs[i], graphs, static, out=self.bufs[1 - i], **kw)
                self.replays.append(g)

    def __call__(self, x: Tensor, forcing: Optional[Tensor] = None) -> Tensor:
        if forcing is not None:
            if self.forcing is None:
                raise ValueError("the step was captured without forcing=")
            self.forcing.copy_(forcing)
        src = self.bufs[self.cur]
        if x.data_ptr() != src.data_ptr():
            src.copy_(x)
        self.replays[self.cur].replay()
        self.cur ^= 1
        return self.bufs[self.cur]
