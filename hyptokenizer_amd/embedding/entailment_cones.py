"""Entailment cones on a Lorentz table: a directed hierarchy loss as one fused HIP kernel pair, the cone energy of given pairs,
the transitive closure of a directed graph and the statistics of a trained hierarchy.

Ganea, Becigneul & Hofmann (ICML 2018): every point carries a cone that opens away from the origin, and ``v`` entails ``u``
(``u`` is above ``v``) when ``v`` lies inside ``u``'s cone.  For an apex row ``a`` (the parent) and a child row ``b`` on the unit
hyperboloid of ``sign_convention="lorentz"``::

    u    = a0 b0 - sum_s a_s b_s          n = sqrt(sum_s a_s^2)          w = sqrt(u^2 - 1)
    A    = (b0 - a0 u) / (n w)            cosine of the exterior angle at a between the ray from the origin and the geodesic to b
    ext  = acos(clamp(A, -A_MAX, A_MAX))  A_MAX = 1 - 2^-20
    aper = asin(min(2 K / n, S_MAX))      K = aperture_k, S_MAX = 1 - 2^-10: the half aperture of a's cone
    E    = max(0, ext - aper)             the cone energy of (a, b): 0 inside the cone

On the ball, with ``p = x_s / (1 + x0)``, these are the paper's ``Xi`` and ``psi`` (eqs. 26 and 28).  Angles do not depend on
curvature, so there is no ``c``.

``entailment_cone_loss(table, index)`` takes the ``[B, 2 + K]`` index of ``edge_softmax_loss`` (anchor, positive, K negatives)
and returns per sample ``E_0 + sum_k max(0, margin - E_k)`` over the live negatives.  ``apex="anchor"``: the anchor is the
parent and the partners candidate children (the negatives corrupt the child); ``apex="partner"``: every partner is an apex and
the anchor the child (the caller passes ``(child, parent, parents'...)``; the negatives corrupt the parent).  The rules of
``edge_softmax_loss`` hold: a negative outside ``[0, V)`` is skipped, a sample whose anchor or positive is outside is skipped
whole.  A partner that is the anchor itself, a slot with ``u <= 1`` and an apex at the origin are *flat*: ``E = 0`` and no
gradient (a flat negative contributes the constant ``margin``).  A clamped factor is a constant (on a table of width 2, a
line, every ``A`` is +-1 and counts as clamped), a negative inside the cone contributes ``margin`` with no gradient.  The
gradient is the Euclidean one of these expressions, by default the uncoalesced sparse COO tensor the Riemannian optimisers
consume.  Two calls on the same inputs return the same bits (no atomics).
There is no CPU fallback: off a HIP device the functions raise ``HypMergeUnavailable``.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from ..engine import _f, _require_cuda
from ..graph import Graph
from ._index_loss import check_index, forward, index_loss
from ._table import check_table

ROLES = {"anchor": 0, "partner": 1}
_FWD, _BWD, _SLOT = "hm_cone_loss_fwd", "hm_cone_loss_bwd", (4,)


def _check_args(who: str, table: torch.Tensor, index: torch.Tensor, margin: float, aperture_k: float, apex: str, reduction: str,
                sign_convention: str) -> None:
    if sign_convention != "lorentz":
        raise ValueError(f"{who}: sign_convention must be 'lorentz', got {sign_convention!r}")
    if reduction not in ("mean", "sum", "none"):
        raise ValueError(f"{who}: reduction must be 'mean', 'sum' or 'none', got {reduction!r}")
    if apex not in ROLES:
        raise ValueError(f"{who}: apex must be 'anchor' or 'partner', got {apex!r}")
    check_table(who, table)
    check_index(who, index)
    if not (float(aperture_k) > 0.0 and np.isfinite(float(aperture_k))):
        raise ValueError(f"{who}: aperture_k must be positive and finite, got {aperture_k}")
    if not (float(margin) >= 0.0 and np.isfinite(float(margin))):
        raise ValueError(f"{who}: margin must be non-negative and finite, got {margin}")


def entailment_cone_loss(table: torch.Tensor, index: torch.Tensor, *, margin: float = 0.01, aperture_k: float = 0.1,
                         apex: str = "anchor", reduction: str = "mean", sparse_grad: bool = True, validate: bool = True,
                         sign_convention: str = "lorentz") -> torch.Tensor:
    """The loss described in the module docstring: ``[B]`` for ``reduction="none"``, their sum, or their sum divided by the
    number of live samples (``"mean"``; 0 when there is none).  ``margin`` is Ganea's gamma, ``aperture_k`` their K.

    ``sparse_grad``, ``validate`` and the COO layout of the gradient are those of ``edge_softmax_loss``: indices
    ``index.reshape(-1)``, a skipped slot replaced by its anchor (by 0 in a skipped sample) with a zero value row."""
    _check_args("entailment_cone_loss", table, index, margin, aperture_k, apex, reduction, sign_convention)
    return index_loss("entailment_cone_loss", table, index, _FWD, _BWD, (_f(aperture_k), _f(margin), ROLES[apex]), _SLOT, reduction,
                      sparse_grad, validate)


def cone_energy(table: torch.Tensor, parents: torch.Tensor, children: torch.Tensor, *, aperture_k: float = 0.1) -> torch.Tensor:
    """``[N]`` energies ``E(parents[i], children[i])``, no gradient: the forward kernel with K = 0.  A pair with an index
    outside ``[0, V)`` has energy 0."""
    if parents.dim() != 1 or parents.shape != children.shape:
        raise ValueError(f"cone_energy: parents and children must be int64 [N], got {tuple(parents.shape)} and {tuple(children.shape)}")
    index = torch.stack([parents, children], 1)
    _check_args("cone_energy", table, index, 0.0, aperture_k, "anchor", "none", "lorentz")
    _require_cuda(table, index)
    return forward(_FWD, table.detach(), index.contiguous(), (_f(aperture_k), 0.0, 0), _SLOT)[0]


def transitive_closure(n: int, edges) -> np.ndarray:
    """int64 ``[M, 2]`` (ancestor, descendant) pairs of the directed graph on ``n`` nodes with ``edges`` ``[E, 2]`` (first
    column the parent): every pair joined by a directed path, once, sorted by (ancestor, descendant), self-pairs dropped
    (a node on a cycle reaches itself; that pair says nothing).

    A host routine: one breadth-first search per node over a CSR of the out-edges, O(n (n + E)) time in the worst case and
    O(n + E) memory beside the M pairs of the result -- meant for taxonomies (WordNet's noun closure has 7 * 10^5 pairs), not
    for dense graphs."""
    return _closure(Graph(range(n), np.asarray(edges, dtype=np.int64).reshape(-1, 2), "transitive_closure"))


def _closure(graph: Graph) -> np.ndarray:
    n = graph.n
    row_ptr, col = graph.out_csr()
    out = []
    seen = np.zeros(n, bool)
    for root in range(n):
        if row_ptr[root] == row_ptr[root + 1]:
            continue
        seen[:] = False
        frontier = np.unique(col[row_ptr[root]:row_ptr[root + 1]])
        reached = []
        while frontier.size:
            seen[frontier] = True
            reached.append(frontier)
            nxt = np.concatenate([col[row_ptr[f]:row_ptr[f + 1]] for f in frontier])
            frontier = np.unique(nxt[~seen[nxt]])
        desc = np.sort(np.concatenate(reached))
        desc = desc[desc != root]
        out.append(np.stack([np.full(desc.size, root, np.int64), desc], 1))
    return np.concatenate(out, 0) if out else np.zeros((0, 2), np.int64)


def cone_stats(table: torch.Tensor, edges, *, aperture_k: float = 0.1) -> Dict[str, float]:
    """How well ``table`` orders the directed ``edges`` ``[E, 2]`` (first column the parent, rows of ``table``): the mean cone
    energy of the edges and the share with ``E == 0``, and the same two numbers for the reversed edges.  A trained hierarchy
    has the first pair low / high and the second the other way round."""
    e = torch.as_tensor(np.asarray(edges, dtype=np.int64).reshape(-1, 2)).to(table.device)
    fwd = cone_energy(table, e[:, 0].contiguous(), e[:, 1].contiguous(), aperture_k=aperture_k)
    rev = cone_energy(table, e[:, 1].contiguous(), e[:, 0].contiguous(), aperture_k=aperture_k)
    m = max(int(e.shape[0]), 1)
    return {"num_edges": int(e.shape[0]), "aperture_k": float(aperture_k),
            "mean_energy": float(fwd.double().sum()) / m, "share_inside": float((fwd == 0).sum()) / m,
            "reversed_mean_energy": float(rev.double().sum()) / m, "reversed_share_inside": float((rev == 0).sum()) / m}


def directed_pairs(graph, closure: bool) -> np.ndarray:
    """The positives of ``fit_graph_embedding(objective="cones")``: the graph's edges as (parent, child) rows, self-loops
    dropped, or their transitive closure."""
    g = Graph.of(graph, "directed_pairs")
    return _closure(g) if closure else g.edges[g.edges[:, 0] != g.edges[:, 1]]
