"""Graph reconstruction of a Lorentz table -- mean rank and mean average precision (Nickel & Kiela 2017, section 4.1; 2018,
section 4) -- as one fused HIP walk over the pair tiles, without a ``[nodes, V]`` distance slab.

For every node ``u`` all other nodes are ranked by their distance to ``u`` and the question is where the graph neighbours of
``u`` land.  ``D[u, v]`` is the canonical fp32 distance at ``c = 1`` (the bits of ``lorentz_model.batch_distance``); ranks
take no curvature, since a division by ``sqrt(c)`` could merge distinct fp32 distances into ties.  A *slot* is a directed edge
``e = (u, o)`` with ``o`` in ``N(u)``, taken for every node (or for the nodes of ``nodes=``) in CSR order.  Per slot, int32::

    less_all[e]  = #{ v != u    : D[u,v] <  D[u,o] }
    equal_all[e] = #{ v != u    : D[u,v] == D[u,o] }      (>= 1: v = o)
    less_nb[e]   = #{ v in N(u) : D[u,v] <  D[u,o] }
    equal_nb[e]  = #{ v in N(u) : D[u,v] == D[u,o] }      (>= 1)

NaN orders as in ``multimodal.retrieval``: greater than every number, equal to NaN.  From the counts::

    rank[e]      = 1 + less_all[e] - less_nb[e]                       (position among the non-neighbours, ties optimistic)
    precision[e] = (less_nb[e] + equal_nb[e]) / (less_all[e] + equal_all[e])
    mean_rank    = sum_e rank[e] / #slots                             (exact int64 sum, one float64 division)
    AP(u)        = mean over o in N(u) of precision[(u, o)];   mAP = mean of AP(u) over the evaluated nodes with deg(u) > 0

``precision`` is scikit-learn's ``average_precision_score(labels, -dist)`` restated: that function puts a threshold at
every distinct score and sums ``(R_k - R_{k-1}) P_k`` over them, with ``R_k = tp_k / deg(u)`` and ``P_k = tp_k / (tp_k + fp_k)``
counted over everything at or before threshold ``k``.  ``R_k - R_{k-1}`` is the number of neighbours tied at threshold ``k``
divided by ``deg(u)``, so each such neighbour ``o`` contributes ``P_k / deg(u)`` with ``tp_k = less_nb + equal_nb`` and
``tp_k + fp_k = less_all + equal_all``: the mean of ``precision`` over the neighbours.

Only ``sign_convention="lorentz"`` is served (under ``"reference"`` every distance is 0).  There is no CPU fallback: off a HIP
device the functions raise ``HypMergeUnavailable``.  Nothing here is differentiable.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Hashable, Optional

import numpy as np
import torch

from .. import _lib
from ..engine import _ptr, _require_cuda, _stream_of
from ..graph import MAX_SAMPLER_NODES as MAX_NODES, Graph, select_nodes, sorted_symmetric_csr
from ._table import check_table, ld as _ld


@dataclass
class NeighborRankCounts:
    """What ``neighbor_rank_counts`` returns, all on the table's device, ``[slots]`` unless noted."""
    anchors: torch.Tensor                                     # int32: the node u of slot e = (u, o)
    pivots: torch.Tensor                                      # int32: the neighbour o
    less_all: torch.Tensor                                    # int32, the four counts of the module docstring
    equal_all: torch.Tensor
    less_nb: torch.Tensor
    equal_nb: torch.Tensor
    segments: torch.Tensor                                    # int64 [nodes + 1]: the slots of evaluated node g are segments[g] .. segments[g + 1] - 1
    slot_segment: torch.Tensor                                # int32: the g of every slot

    @property
    def num_slots(self) -> int:
        return int(self.anchors.shape[0])


def set_walk_layout(layout: int) -> None:
    """Test / tuning hook (results never depend on it): the tile layout of the all-keys walk from now on, process-wide.
    0 = the default (layout 1 below 97 columns, layout 2 from there on), 1 = anchor and partner rows in LDS, 2 = anchor rows in registers and partner rows as 16-byte LDS
    broadcasts."""
    _lib.check(_lib.load().hm_debug_recon_layout(int(layout)))


def _check_count_args(table: torch.Tensor, row_ptr: torch.Tensor, col: torch.Tensor, nodes: Optional[torch.Tensor]) -> None:
    who = "neighbor_rank_counts"
    check_table(who, table)
    v = table.shape[0]
    if not 1 <= v <= MAX_NODES:
        raise ValueError(f"{who}: the table must have between 1 and 2^31 - 1 rows, got {v}")
    if row_ptr.dtype != torch.int64 or row_ptr.dim() != 1 or row_ptr.shape[0] != v + 1:
        raise ValueError(f"{who}: row_ptr must be int64 [V + 1] = [{v + 1}], got {row_ptr.dtype} {tuple(row_ptr.shape)}")
    if col.dtype != torch.int32 or col.dim() != 1:
        raise ValueError(f"{who}: col must be int32 [nnz], got {col.dtype} {tuple(col.shape)}")
    if col.shape[0] > MAX_NODES:
        raise ValueError(f"{who}: nnz must stay below 2^31, got {col.shape[0]}")
    if nodes is not None:
        if nodes.dtype != torch.int64 or nodes.dim() != 1:
            raise ValueError(f"{who}: nodes must be int64 [n], got {nodes.dtype} {tuple(nodes.shape)}")
        select_nodes(nodes, v, who, what="row")


def neighbor_rank_counts(table: torch.Tensor, row_ptr: torch.Tensor, col: torch.Tensor, nodes: Optional[torch.Tensor] = None, *,
                         validate: bool = True) -> NeighborRankCounts:
    """The four counts of the module docstring for every slot of the CSR ``(row_ptr int64 [V + 1], col int32 [nnz])``, or for
    the slots of the rows ``nodes`` (int64, in range, free of repeats, any order) in the order given.

    The CSR has no self-loops and its rows are sorted and free of repeats (what ``sorted_symmetric_csr`` builds); it need not
    be symmetric.  ``table`` is fp32 ``[V, d + 1]`` with unit last stride and is read in place whatever its row stride.
    ``validate=True`` checks with one synchronising read that ``row_ptr`` starts at 0, never decreases and ends at ``nnz`` and
    that ``col`` stays inside ``[0, V)``; without it a slot that names a row outside the table gets -1 in all four counts.
    Working memory is 32 bytes per slot (28 of them returned) and a few vectors of the length of ``nodes``; nothing of size
    ``V`` times anything is allocated.  Two calls return the same bits."""
    _check_count_args(table, row_ptr, col, nodes)
    _require_cuda(table, row_ptr, col, *(() if nodes is None else (nodes,)))
    dev = table.device
    if row_ptr.device != dev or col.device != dev or (nodes is not None and nodes.device != dev):
        raise ValueError("neighbor_rank_counts: the table, row_ptr, col and nodes must live on the same device")
    x = table.detach()
    row_ptr, col = row_ptr.contiguous(), col.contiguous()
    v, d1 = x.shape
    nnz = col.shape[0]
    if validate:
        ok = (row_ptr[0] == 0) & (row_ptr[-1] == nnz) & (row_ptr[1:] >= row_ptr[:-1]).all()
        if nnz > 0:
            ok = ok & (col.min() >= 0) & (col.max() < v)
        if not bool(ok):
            raise ValueError(f"neighbor_rank_counts: not a CSR over [0, {v}): row_ptr must run from 0 to nnz without decreasing "
                             "and col must stay in range")
    if nodes is None:
        n_seg = v
        deg = row_ptr[1:] - row_ptr[:-1]
    else:
        nodes = nodes.contiguous()
        n_seg = nodes.shape[0]
        deg = row_ptr[nodes + 1] - row_ptr[nodes]
    segments = torch.zeros(n_seg + 1, dtype=torch.int64, device=dev)
    torch.cumsum(deg, 0, out=segments[1:])
    del deg
    n_slots = int(segments[-1])                               # the one read the allocation needs
    if n_slots > MAX_NODES:
        raise ValueError(f"neighbor_rank_counts: {n_slots} slots, the limit is 2^31 - 1")
    ints = torch.empty((7, n_slots), dtype=torch.int32, device=dev)
    scratch = torch.empty(n_slots, dtype=torch.float32, device=dev)
    anchors, pivots, slot_seg, less_all, equal_all, less_nb, equal_nb = ints.unbind(0)
    L = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(L.hm_recon_slots(_ptr(row_ptr), _ptr(col), v, nnz, _ptr(nodes), n_seg, _ptr(segments), n_slots, _ptr(anchors),
                                    _ptr(pivots), _ptr(slot_seg), _stream_of(x)))
        _lib.check(L.hm_recon_counts(_ptr(x), _ld(x), v, d1, _ptr(anchors), _ptr(pivots), _ptr(slot_seg), _ptr(segments), n_slots,
                                     n_seg, _ptr(less_all), _ptr(equal_all), _ptr(less_nb), _ptr(equal_nb), _ptr(scratch),
                                     _stream_of(x)))
    return NeighborRankCounts(anchors, pivots, less_all, equal_all, less_nb, equal_nb, segments, slot_seg)


def metrics_from_counts(counts: NeighborRankCounts) -> Dict[str, float]:
    """``{"mean_rank", "map", "num_pairs", "num_nodes"}`` of the counts, reduced in float64 on the device; one read of three
    numbers reaches the host.  ``num_nodes`` counts the evaluated nodes with at least one neighbour.  Without a slot both
    numbers are ``nan``."""
    s = counts.num_slots
    if s == 0:
        return {"mean_rank": float("nan"), "map": float("nan"), "num_pairs": 0, "num_nodes": 0}
    rank_sum = (counts.less_all - counts.less_nb).sum(dtype=torch.int64) + s      # below 2^53: exact as a float64
    deg = (counts.segments[1:] - counts.segments[:-1])
    live = (deg > 0).sum()
    # mAP = (1 / live) sum_e precision[e] / deg(anchor of e): the mean of the per-node means as one sum in a fixed order
    terms = (counts.less_nb + counts.equal_nb).double()
    terms /= (counts.less_all + counts.equal_all).double()
    terms /= deg.double()[counts.slot_segment.long()]
    m_ap = terms.sum() / live.double()
    rank_sum, m_ap, live = torch.stack([rank_sum.double(), m_ap, live.double()]).tolist()
    # the one division of the mean rank is Python's: correctly rounded, which a tensor divided by a scalar need not be
    return {"mean_rank": rank_sum / float(s), "map": m_ap, "num_pairs": s, "num_nodes": int(live)}


def reconstruction_metrics(table: torch.Tensor, graph, *, node_mapping: Optional[Dict[Hashable, int]] = None, nodes=None,
                           sign_convention: str = "lorentz") -> Dict[str, float]:
    """Mean rank and mAP of the graph's edges under the table's distances: ``{"mean_rank", "map", "num_pairs", "num_nodes"}``.

    ``graph`` is whatever ``NegativeSampler`` accepts: both directions of every edge count, self-loops and repeats are
    dropped.  Node ``k`` of the graph is row ``k`` of ``table``, or row ``node_mapping[name]`` (``{name: row}``, as
    ``compute_distortion`` takes it; the rows must be distinct): rows of the table that belong to no node then rank as
    non-neighbours.  ``nodes`` (a sequence or tensor of graph node indices, in range and free of repeats) restricts the
    evaluation to the slots of those nodes; every node is still a candidate in their rankings."""
    if sign_convention != "lorentz":
        raise ValueError(f"reconstruction_metrics: sign_convention must be 'lorentz', got {sign_convention!r} (under 'reference' "
                         "every distance is 0 and every rank is 1)")
    g = Graph.of(graph, "reconstruction_metrics")
    names, edges, n = g.node_names, g.edges, g.n
    if table.dim() != 2:
        raise ValueError(f"reconstruction_metrics: the table must be [V, d + 1], got shape {tuple(table.shape)}")
    v = table.shape[0]
    if node_mapping is None:
        if n != v:
            raise ValueError(f"reconstruction_metrics: the graph has {n} nodes and the table {v} rows; pass node_mapping")
        rows = None
    else:
        try:
            rows = np.array([int(node_mapping[name]) for name in names], dtype=np.int64)
        except KeyError as exc:
            raise ValueError(f"reconstruction_metrics: node_mapping has no row for node {exc.args[0]!r}") from None
        if rows.size and (rows.min() < 0 or rows.max() >= v):
            raise ValueError(f"reconstruction_metrics: node_mapping names a row outside [0, {v})")
        if np.unique(rows).size != rows.size:
            raise ValueError("reconstruction_metrics: node_mapping sends two nodes to one row")
        edges = rows[edges] if edges.size else edges
    if nodes is not None:
        sel = g.select(nodes, "reconstruction_metrics")
        sel = sel if rows is None else rows[sel]
    elif rows is not None:
        sel = rows
    else:
        sel = None
    _check_count_args(table, torch.empty(v + 1, dtype=torch.int64), torch.empty(0, dtype=torch.int32), None)
    _require_cuda(table)
    row_ptr, col = g.csr(True) if rows is None else sorted_symmetric_csr(v, edges)
    dev = table.device
    counts = neighbor_rank_counts(table, torch.from_numpy(row_ptr).to(dev), torch.from_numpy(col).to(dev),
                                  None if sel is None else torch.from_numpy(np.ascontiguousarray(sel)).to(dev), validate=False)
    return metrics_from_counts(counts)
