"""gwen_amd -- MI355X-native implementation of GWEN's GCNConv-stack hot path.

Public surface mirrors /root/reference/src/gwen/models_gnn.py (GNNConfig, DownConvLayers,
UpConvLayers, GCNConvLayers, GNNModel, loss_func) plus the ``GCNConv`` layer it imports from
torch-geometric (:19).  Kernels live in libgwen_hip.so (include/gwen_hip.h); build it with
``python -m gwen_amd.build``.
"""
from . import attention, checkpoint, forcings, forecaster, g2m, gridgraph, interaction, loss_functions, losses, noise, ops
from . import products, regrid, sfno, spectral
from .attention import GraphTransformer, edge_attention, edge_attention_kv
from .checkpoint import checkpointed_step
from .forward import GraphedForward, KernelEvents, StackForward, event_bracket_overhead
from .gcn_conv import GCNConv, Linear
from .forecaster import InteractionForecaster
from .interaction import EdgeGraph, InteractionNet, interaction_graph
from .losses import EnsembleCRPSLoss, ensemble_crps, ensemble_scores
from .loss_functions import CRPSLoss, EnsembleVarRegLoss, MaskedLoss
from .noise import NoiseStream
from .forcings import ForcingClock
from .products import ensemble_products, ensemble_quantiles, exceedance_probability, rank_histogram
from .gridgraph import containing_faces, grid_graphs, latlon_grid, radius_edges, sphere_points
from .regrid import (Regridder, cell_areas, cell_overlaps, latlon_cells, mesh_cells, mesh_dual_cells,
                     nearest_neighbours)
from .spectral import SphericalHarmonics, check_rings, octahedral_nlon, ring_fft_plan
from .sfno import SFNO, SFNOBlock, SpectralConv, spectral_conv, spectral_conv_supported
from .graph import GraphCSR, GraphCache, default_cache, prepare_graph
from .mesh import Mesh, complete_graph, geodesic_mesh
from .models_gnn import (DownConvLayers, GCNConvLayers, GNNConfig, GNNModel, UpConvLayers,
                         loss_func)
from .models_cnn import BaseNet, Decoder, Encoder, UNet

__all__ = [
    "GCNConv", "Linear", "GraphedForward", "KernelEvents", "StackForward", "event_bracket_overhead", "GraphCSR", "GraphCache", "default_cache", "prepare_graph", "Mesh",
    "complete_graph", "geodesic_mesh", "DownConvLayers", "GCNConvLayers", "GNNConfig", "GNNModel",
    "UpConvLayers", "loss_func", "InteractionNet", "InteractionForecaster", "EdgeGraph", "interaction_graph",
    "EnsembleCRPSLoss", "ensemble_crps", "ensemble_scores", "NoiseStream", "GraphTransformer", "edge_attention", "edge_attention_kv",
    "ensemble_products", "ensemble_quantiles", "exceedance_probability", "rank_histogram",
    "sphere_points", "latlon_grid", "radius_edges", "containing_faces", "grid_graphs", "ForcingClock",
    "Regridder", "nearest_neighbours", "mesh_cells", "mesh_dual_cells", "latlon_cells", "cell_areas", "cell_overlaps", "checkpointed_step", "CRPSLoss", "EnsembleVarRegLoss", "MaskedLoss",
    "SphericalHarmonics", "octahedral_nlon", "check_rings", "ring_fft_plan", "SFNO", "SFNOBlock", "SpectralConv", "spectral_conv", "spectral_conv_supported",
    "BaseNet", "Encoder", "Decoder", "UNet",
]
__version__ = "0.1.0"
