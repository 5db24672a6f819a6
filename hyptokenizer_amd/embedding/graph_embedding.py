"""Embedding a graph in a Lorentz table: the edge-softmax loss of Nickel & Kiela (2017, 2018) as one fused HIP kernel pair,
a reproducible negative sampler and a small training loop on the Riemannian optimisers.

``edge_softmax_loss(table, index)`` -- ``table`` is fp32 ``[V, d + 1]`` on a HIP device, rows on the hyperboloid of
``sign_convention="lorentz"``; ``index`` int64 ``[B, 2 + K]`` holds per sample the anchor, the positive and ``K`` negatives.
With ``d_k = distance(anchor, partner_k)`` (``k = 0`` the positive) the loss of a sample is
``d_0 + log sum_k exp(-d_k)``, the positive inside the sum.  A negative outside ``[0, V)`` (``-1`` is the mask
``NegativeSampler`` writes) is left out of the sum; a sample whose anchor or positive is outside is left out altogether.
A partner that is the anchor itself (same index) is at distance exactly 0.

The gradient is the Euclidean one ``optim.RiemannianSGD`` / ``RiemannianAdam`` consume, by default as an uncoalesced sparse
COO tensor ``[V, d + 1]`` with one entry per slot of ``index``: their sparse path coalesces it and steps only the rows it
names.  Where the argument ``u`` of ``acosh`` is ``<= 1`` (coincident rows, the anchor against itself) the slot's
gradient is ZERO -- on purpose not the derivative of ``lorentz_model.distance``, which is infinite there and would turn the
whole sample into NaN; the true distance has no derivative at 0 and 0 is the subgradient that leaves coincident points
alone.  Two calls on the same inputs return the same bits (no atomics).

Only ``"lorentz"`` is served: under ``"reference"`` every distance is 0 and the loss is the constant ``log(1 + K)``.
There is no CPU fallback: off a HIP device the functions raise ``HypMergeUnavailable``.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, Hashable, List

import numpy as np
import torch

from ..engine import _f, _ptr, _require_cuda
# noqa below: other modules, tests and tools import these names from here
from ..graph import MAX_SAMPLER_NODES as MAX_NODES, Graph, GraphHandle, graph_arrays as _graph_arrays, sorted_symmetric_csr  # noqa: F401
from ._index_loss import check_index, index_loss
from ._table import MAX_WIDTH, MIN_WIDTH, check_table, ld as _ld  # noqa: F401


# ---- the loss -------------------------------------------------------------------------------------------------------------
def _check_loss_args(table: torch.Tensor, index: torch.Tensor, c: float, reduction: str, sign_convention: str) -> None:
    if sign_convention != "lorentz":
        raise ValueError(f"edge_softmax_loss: sign_convention must be 'lorentz', got {sign_convention!r} (under 'reference' "
                         "every distance is 0 and the loss is constant)")
    if reduction not in ("mean", "sum", "none"):
        raise ValueError(f"edge_softmax_loss: reduction must be 'mean', 'sum' or 'none', got {reduction!r}")
    check_table("edge_softmax_loss", table)
    check_index("edge_softmax_loss", index)
    if not (float(c) > 0.0 and np.isfinite(float(c))):
        raise ValueError(f"edge_softmax_loss: curvature must be positive and finite, got {c}")


def edge_softmax_loss(table: torch.Tensor, index: torch.Tensor, c: float = 1.0, reduction: str = "mean", *,
                      sparse_grad: bool = True, validate: bool = True, sign_convention: str = "lorentz") -> torch.Tensor:
    """The loss described in the module docstring: ``[B]`` for ``reduction="none"``, their sum, or their sum divided by the
    number of live samples (``"mean"``; 0 when there is none).

    ``sparse_grad=True`` leaves an uncoalesced sparse COO gradient ``[V, d + 1]`` on ``table`` whose indices are
    ``index.reshape(-1)``, a skipped slot replaced by its anchor (by 0 in a skipped sample) with a zero value row;
    ``sparse_grad=False`` lets torch densify it.  ``validate=True`` checks the anchors and positives against ``[0, V)`` with
    one synchronising read and raises ``ValueError``; ``validate=False`` reads nothing back and such samples are skipped."""
    _check_loss_args(table, index, c, reduction, sign_convention)
    return index_loss("edge_softmax_loss", table, index, "hm_edge_loss_fwd", "hm_edge_loss_bwd", (_f(c),), (), reduction, sparse_grad,
                      validate)


# ---- the sampler ----------------------------------------------------------------------------------------------------------
class NegativeSampler(GraphHandle):
    """``num_negatives`` nodes per (anchor, positive) pair, uniform over ``[0, V)`` except the anchor and its neighbours, from
    Philox4x32-10 keyed by ``seed`` with counter (sample, slot, attempt, step): ``sample(pairs, step)`` is a pure function
    of its arguments and ``seed``, whatever the device does.  A slot whose ``max_tries`` candidates were all rejected is
    ``-1``, the mask of ``edge_softmax_loss``.  ``graph`` is as ``GraphPaths`` accepts it."""

    PREFIX = "hm_negsample"
    CANONICAL = True
    NODE_LIMIT, NODE_LIMIT_TEXT = MAX_NODES, "2^31 - 1"

    def __init__(self, graph, num_negatives: int, seed: int = 0, device=None, max_tries: int = 32):
        if num_negatives < 0 or not (1 <= max_tries <= 65536):
            raise ValueError("NegativeSampler: num_negatives must be >= 0 and max_tries in 1..65536")
        self.num_negatives, self.max_tries = int(num_negatives), int(max_tries)
        self.seed = int(seed) & ((1 << 64) - 1)
        super().__init__(graph, device)

    def sample(self, pairs: torch.Tensor, step: int) -> torch.Tensor:
        """``pairs`` int64 ``[B, 2]`` on the sampler's device -> ``index`` int64 ``[B, 2 + num_negatives]``."""
        if pairs.dtype != torch.int64 or pairs.dim() != 2 or pairs.shape[1] != 2:
            raise ValueError(f"NegativeSampler.sample: pairs must be int64 [B, 2], got {pairs.dtype} {tuple(pairs.shape)}")
        if not (0 <= int(step) < (1 << 32)):
            raise ValueError(f"NegativeSampler.sample: step {step} is outside [0, 2^32)")
        _require_cuda(pairs)
        pairs = pairs.contiguous()
        out = torch.empty((pairs.shape[0], 2 + self.num_negatives), dtype=torch.int64, device=pairs.device)
        with torch.cuda.device(self.device):
            self._check(self._L.hm_negsample_sample(self._h, _ptr(pairs), pairs.shape[0], self.num_negatives, self.seed, int(step),
                                                    self.max_tries, _ptr(out), self._stream()))
        return out


# ---- the loop -------------------------------------------------------------------------------------------------------------
@dataclass
class GraphEmbeddingResult:
    table: torch.Tensor                                       # fp32 [V, dim + 1] on the device, rows on the hyperboloid
    node_names: List[Hashable]
    node_mapping: Dict[Hashable, int]                         # {name: row}, as compute_distortion takes it
    loss_history: List[float] = field(default_factory=list)   # mean loss per sample of every epoch


def init_table(num_nodes: int, dim: int, init_scale: float, seed: int, device) -> torch.Tensor:
    """Uniform spatial entries in ``+-init_scale`` under a CPU generator seeded by ``seed``, lifted to the hyperboloid."""
    gen = torch.Generator().manual_seed(int(seed))
    s = (torch.rand((num_nodes, dim), generator=gen, dtype=torch.float32) * 2.0 - 1.0) * float(init_scale)
    return torch.cat([torch.sqrt(1.0 + (s * s).sum(-1, keepdim=True)), s], -1).to(device)


def fit_graph_embedding(graph, dim: int, *, epochs: int, batch_size: int = 1024, num_negatives: int = 50, lr: float = 0.3,
                        burn_in_epochs: int = 0, burn_in_factor: float = 0.1, optimizer: str = "rsgd", init_scale: float = 1e-3,
                        seed: int = 0, c: float = 1.0, device=None, log_every: int = 0, objective: str = "softmax",
                        margin: float = 0.01, aperture_k: float = 0.1, closure: bool = False) -> GraphEmbeddingResult:
    """Embed ``graph`` (as ``GraphPaths`` accepts it) in ``dim`` hyperbolic dimensions.

    Positives are every edge in both directions; an epoch visits them in the order of a ``torch.randperm`` under a CPU
    generator seeded by ``seed``, ``batch_size`` at a time; batch number ``step`` (counted from 0 over the whole run) draws
    its negatives with ``NegativeSampler.sample(pairs, step)``.  The first ``burn_in_epochs`` epochs run at
    ``lr * burn_in_factor``.  The loss of every batch is summed on the device and read back once per epoch.

    ``objective="cones"`` trains a directed hierarchy with ``entailment_cones.entailment_cone_loss`` instead (DESIGN.md 5.21;
    ``margin``, ``aperture_k``; ``c`` is not used, angles do not depend on it).  Positives are the graph's edges as directed
    pairs, first column the parent, or their transitive closure when ``closure=True``.  The sampler is built on those pairs
    and stays undirected: a negative is neither an ancestor nor a descendant of its anchor.  Batch ``step`` corrupts the child
    (``apex="anchor"`` on ``sample(pairs, 2 step)``) and the parent (``apex="partner"`` on ``sample(pairs[:, [1, 0]],
    2 step + 1)``); the sum of the two losses is stepped once."""
    from ..optim import RiemannianAdam, RiemannianSGD
    if objective not in ("softmax", "cones"):
        raise ValueError(f"fit_graph_embedding: objective must be 'softmax' or 'cones', got {objective!r}")
    if optimizer not in ("rsgd", "radam"):
        raise ValueError(f"fit_graph_embedding: optimizer must be 'rsgd' or 'radam', got {optimizer!r}")
    if not (MIN_WIDTH <= dim + 1 <= MAX_WIDTH):
        raise ValueError(f"fit_graph_embedding: dim must lie in {MIN_WIDTH - 1}..{MAX_WIDTH - 1}, got {dim}")
    if epochs < 0 or batch_size < 1:
        raise ValueError("fit_graph_embedding: epochs must be >= 0 and batch_size >= 1")
    cones = objective == "cones"
    graph = Graph.of(graph, "NegativeSampler")
    if cones:
        from .entailment_cones import directed_pairs, entailment_cone_loss
        graph = Graph(graph.node_names, directed_pairs(graph, closure))
    sampler = NegativeSampler(graph, num_negatives, seed=seed, device=device)
    try:
        dev = sampler.device
        e = sampler.edges[sampler.edges[:, 0] != sampler.edges[:, 1]]
        positives = torch.from_numpy(np.ascontiguousarray(e) if cones else np.concatenate([e, e[:, ::-1]], 0).copy()).to(dev)
        table = torch.nn.Parameter(init_table(sampler.n, dim, init_scale, seed, dev))
        opt = (RiemannianSGD([table], lr=lr) if optimizer == "rsgd" else RiemannianAdam([table], lr=lr))
        gen = torch.Generator().manual_seed(int(seed))
        history: List[float] = []
        step = 0
        for epoch in range(epochs):
            for group in opt.param_groups:
                group["lr"] = lr * burn_in_factor if epoch < burn_in_epochs else lr
            order = torch.randperm(positives.shape[0], generator=gen).to(dev)
            total = torch.zeros((), dtype=torch.float32, device=dev)
            for b0 in range(0, positives.shape[0], batch_size):
                batch = positives[order[b0:b0 + batch_size]]
                if cones:
                    kw = dict(margin=margin, aperture_k=aperture_k, reduction="sum", validate=False)
                    loss = (entailment_cone_loss(table, sampler.sample(batch, 2 * step), apex="anchor", **kw) +
                            entailment_cone_loss(table, sampler.sample(batch[:, [1, 0]], 2 * step + 1), apex="partner", **kw))
                else:
                    loss = edge_softmax_loss(table, sampler.sample(batch, step), c, "sum", validate=False)
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
                total += loss.detach()
                step += 1
            history.append(float(total.item()) / max(positives.shape[0], 1))
            if log_every and (epoch + 1) % log_every == 0:
                print(f"epoch {epoch + 1}/{epochs}: loss {history[-1]:.6f}", flush=True)
    finally:
        sampler.close()
    names = sampler.node_names
    return GraphEmbeddingResult(table.detach(), names, {name: k for k, name in enumerate(names)}, history)
