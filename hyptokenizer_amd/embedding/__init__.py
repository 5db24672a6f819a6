"""The reference's ``embedding`` package: ``lorentz_model`` and ``poincare_ball``, served by the gfx950 kernels,
``graph_embedding``: training a Lorentz table on a graph (edge-softmax loss, negative sampler, training loop), ``graph_metrics``:
how well such a table reconstructs its graph (mean rank, mAP), and ``pooling``: the Lorentz centroid of bags of table rows
(sentence points from token rows)."""
from . import graph_embedding, graph_metrics, lorentz_model, poincare_ball, pooling  # noqa: F401
from .graph_embedding import NegativeSampler, edge_softmax_loss, fit_graph_embedding  # noqa: F401
from .graph_metrics import NeighborRankCounts, neighbor_rank_counts, reconstruction_metrics  # noqa: F401
from .pooling import HyperbolicEmbeddingBag, lorentz_centroid  # noqa: F401

__all__ = ["lorentz_model", "poincare_ball", "graph_embedding", "graph_metrics", "pooling", "edge_softmax_loss", "NegativeSampler",
           "fit_graph_embedding", "neighbor_rank_counts", "reconstruction_metrics", "NeighborRankCounts", "lorentz_centroid",
           "HyperbolicEmbeddingBag"]
