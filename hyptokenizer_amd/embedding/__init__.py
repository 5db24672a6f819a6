"""The reference's ``embedding`` package: ``lorentz_model`` and ``poincare_ball``, served by the gfx950 kernels, and
``graph_embedding``: training a Lorentz table on a graph (edge-softmax loss, negative sampler, training loop)."""
from . import graph_embedding, lorentz_model, poincare_ball  # noqa: F401
from .graph_embedding import NegativeSampler, edge_softmax_loss, fit_graph_embedding  # noqa: F401

__all__ = ["lorentz_model", "poincare_ball", "graph_embedding", "edge_softmax_loss", "NegativeSampler", "fit_graph_embedding"]
