"""cgat_amd -- MI355X (gfx950) implementation of the hyllios/CGAT edge-attention hot path.

`CGAtNet` and the layer classes keep the reference's constructor / forward API and
state_dict layout, so `--version cgat_amd` plugs into the reference LightningModule
(lightning_module.py:165-176).  Importing this package loads libcgat_hip.so and raises if
it is missing: there is no CPU or PyTorch-eager fallback.
"""
from . import _lib  # noqa: F401  (loads the shared library, fails loudly)
from .hypernet import H_Net, H_Net_0, HyperFC
from .mlp import ResidualNetwork, Rezero, SimpleNetwork
from .nets import CGAtNet, GATConvEdges, GATConvNodes, MHAttention, MultiHeadNetwork
from .roost import MessageLayer, Roost, WeightedAttention
from .graph import GraphBatch, synthetic_batch
from .collate import PackedDataset
from .optim import FusedAdam, FusedAdamW, FusedLamb, FusedSGD, L1Loss, MSELoss, RobustL1, RobustL2, criterion_with_metrics, cyclical_lr
from .ops import get_bilinear_mode, set_bilinear_mode, set_validate_indices, set_edge_storage, get_edge_storage
from .ops import set_fused_inference, get_fused_inference
from .ops import set_fused_edge_combine, get_fused_edge_combine
from .ops import set_fused_attention_dropout, get_fused_attention_dropout
from .ops import IndexedEdgeAttr, set_indexed_edge_attr, get_indexed_edge_attr
from .ops import set_indexed_edge_training, get_indexed_edge_training
from .ops import set_indexed_vector_attention, get_indexed_vector_attention
from .trainer import DataParallelTrainer, Normalizer
from .chunked import set_max_edges_per_pass
from .capture import GraphedStep
from . import neighbors
from .neighbors import NeighborTables, neighbor_tables, dataset_dict_from_structures, synthetic_structures
from . import debug
from . import gp
from .gp import (GPHead, bound_and_gradient, collapsed_bound, deep_kernel_gradient, kmeans_inducing_points,
                 latent_adjoints, predictive_backward)

__all__ = ["CGAtNet", "GATConvNodes", "GATConvEdges", "MultiHeadNetwork", "MHAttention", "H_Net", "H_Net_0",
           "HyperFC", "SimpleNetwork", "ResidualNetwork", "Rezero", "Roost", "MessageLayer", "WeightedAttention",
           "GraphBatch", "synthetic_batch", "PackedDataset", "FusedAdamW", "FusedLamb", "RobustL1", "RobustL2", "cyclical_lr",
           "FusedSGD", "FusedAdam", "L1Loss", "MSELoss", "criterion_with_metrics", "set_bilinear_mode", "get_bilinear_mode",
           "set_validate_indices", "DataParallelTrainer", "Normalizer", "set_max_edges_per_pass",
           "set_edge_storage", "get_edge_storage", "set_fused_inference", "get_fused_inference", "set_fused_edge_combine",
           "get_fused_edge_combine", "set_fused_attention_dropout", "get_fused_attention_dropout", "IndexedEdgeAttr", "set_indexed_edge_attr",
           "get_indexed_edge_attr", "set_indexed_edge_training", "get_indexed_edge_training", "set_indexed_vector_attention",
           "get_indexed_vector_attention", "GraphedStep", "debug", "neighbors", "NeighborTables", "neighbor_tables",
           "dataset_dict_from_structures", "synthetic_structures", "gp", "GPHead", "bound_and_gradient", "collapsed_bound",
           "deep_kernel_gradient", "kmeans_inducing_points", "latent_adjoints", "predictive_backward"]
