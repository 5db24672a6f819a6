"""Shortest-path lengths and connected components of an undirected graph on a HIP device (``hm_graph_*``, hm_graph.hip).

``GraphPaths`` replaces the per-pair ``nx.shortest_path_length`` of the reference's ``scripts/eval_hierarchy.py`` by one
bit-parallel multi-source BFS over all pairs of a call.  The graph is whatever ``graph.Graph.of`` accepts
(DESIGN.md 5.22).  Edges are taken as undirected; self-loops and repeated edges are harmless; a node without edges is legal.

There is no CPU fallback: on a non-HIP device the constructor raises ``HypMergeUnavailable``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict

import numpy as np
import torch

from .graph import MAX_PATH_NODES as MAX_NODES, GraphHandle, symmetric_csr  # noqa: F401  (tests and tools import them from here)


def _indices(x, what: str) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    a = np.asarray(x)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"GraphPaths: {what} must hold integer node indices")
    a = a.astype(np.int64).reshape(-1)
    if a.size and (a.min() < -(1 << 31) or a.max() >= (1 << 31)):
        raise ValueError(f"GraphPaths: {what} out of the int32 range")
    return np.ascontiguousarray(a.astype(np.int32))


class GraphPaths(GraphHandle):
    """One graph on a HIP device, as ``graph.Graph.of`` accepts it; ``graph`` is that ``Graph``.  ``node_names`` is the list
    of nodes in index order and ``index`` maps a node to its index; the three methods take node INDICES (tensors or
    sequences) and return tensors on the device."""

    PREFIX = "hm_graph"

    def components(self) -> torch.Tensor:
        """int32 ``[n]``: the smallest node index of every node's connected component."""
        labels = torch.empty(self.n, dtype=torch.int32, device=self.device)
        count = C.c_int64(0)
        self._check(self._L.hm_graph_components(self._h, C.c_void_p(labels.data_ptr()), C.byref(count), self._stream()))
        self.n_components = count.value
        return labels

    def path_lengths(self, src, dst) -> torch.Tensor:
        """int32 ``[P]``: edges on a shortest path from ``src[p]`` to ``dst[p]``; 0 where they are the same node, -1 where no
        path exists.  One BFS serves every pair of the call."""
        s, d = _indices(src, "src"), _indices(dst, "dst")
        if s.shape != d.shape:
            raise ValueError("GraphPaths.path_lengths: src and dst differ in length")
        out = torch.empty(max(s.size, 1), dtype=torch.int32, device=self.device)
        self._check(self._L.hm_graph_pair_lengths(self._h, C.c_void_p(s.ctypes.data), C.c_void_p(d.ctypes.data), s.size,
                                                  C.c_void_p(out.data_ptr()), self._stream()))
        return out[:s.size]

    def distance_rows(self, src, cols=None) -> torch.Tensor:
        """int16 ``[S, M]``: path length from ``src[s]`` to ``cols[m]`` (``cols`` omitted: to every node, M = n); -1 where
        no path exists."""
        s = _indices(src, "src")
        c = None if cols is None else _indices(cols, "cols")
        m = self.n if c is None else c.size
        out = torch.empty((s.size, m), dtype=torch.int16, device=self.device)
        if s.size == 0 or m == 0:
            return out
        self._check(self._L.hm_graph_distance_rows(self._h, C.c_void_p(s.ctypes.data), s.size,
                                                   C.c_void_p(c.ctypes.data) if c is not None else None, m,
                                                   C.c_void_p(out.data_ptr()), m, self._stream()))
        return out

    def last_stats(self) -> Dict[str, int]:
        """Of the last call: BFS levels (component iterations) that did work, kernel launches, passes, words per node."""
        v = [C.c_int64(0) for _ in range(4)]
        self._check(self._L.hm_graph_last_stats(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("levels", "launches", "passes", "words"), (x.value for x in v)))
