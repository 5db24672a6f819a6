"""The reference's ``embedding`` package: ``lorentz_model`` and ``poincare_ball``, served by the gfx950 kernels,
``graph_embedding``: training a Lorentz table on a graph (edge-softmax loss, negative sampler, training loop), ``graph_metrics``:
how well such a table reconstructs its graph (mean rank, mAP), ``hyperbolicity``: Gromov's delta of a graph metric or of a
table's distances and the curvature it suggests, and ``pooling``: the Lorentz centroid of bags of table rows
(sentence points from token rows), and ``entailment_cones``: a directed hierarchy loss on a Lorentz table (Ganea et al. 2018),
the cone energy of pairs, the transitive closure of a graph and the statistics of a trained hierarchy."""
from . import entailment_cones  # noqa: F401
from . import graph_embedding, graph_metrics, hyperbolicity, lorentz_model, poincare_ball, pooling  # noqa: F401
from .entailment_cones import cone_energy, cone_stats, entailment_cone_loss, transitive_closure  # noqa: F401
from .graph_embedding import NegativeSampler, edge_softmax_loss, fit_graph_embedding  # noqa: F401
from .graph_metrics import NeighborRankCounts, neighbor_rank_counts, reconstruction_metrics  # noqa: F401
from .hyperbolicity import (GromovDelta, curvature_estimate, embedding_hyperbolicity, graph_hyperbolicity,  # noqa: F401
                            gromov_delta)
from .pooling import HyperbolicEmbeddingBag, lorentz_centroid  # noqa: F401

__all__ = ["lorentz_model", "poincare_ball", "graph_embedding", "graph_metrics", "pooling", "edge_softmax_loss", "NegativeSampler",
           "fit_graph_embedding", "neighbor_rank_counts", "reconstruction_metrics", "NeighborRankCounts", "lorentz_centroid",
           "HyperbolicEmbeddingBag", "hyperbolicity", "GromovDelta", "gromov_delta", "graph_hyperbolicity", "embedding_hyperbolicity",
           "curvature_estimate", "entailment_cones", "entailment_cone_loss", "cone_energy", "cone_stats", "transitive_closure"]
