"""Shortest-path lengths and connected components of an undirected graph on a HIP device (``hm_graph_*``, hm_graph.hip).

``GraphPaths`` replaces the per-pair ``nx.shortest_path_length`` of the reference's ``scripts/eval_hierarchy.py`` by one
bit-parallel multi-source BFS over all pairs of a call.  The graph is any object with ``.nodes()`` and
``.edges()`` (a networkx graph; networkx itself is never imported here), or a tuple ``(node_names, edges)`` with ``edges``
an integer array ``[E, 2]`` of node positions.  A node's index is its position in ``.nodes()`` order.  Edges are taken as
undirected; self-loops and repeated edges are harmless; a node without edges is legal.

There is no CPU fallback: on a non-HIP device the constructor raises ``HypMergeUnavailable``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Hashable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._handle import DeviceHandle

MAX_NODES = 1 << 24


def symmetric_csr(n: int, edges: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(row_ptr int64[n + 1], col int32[2 E]) of the undirected graph: both directions of every edge, rows in node
    order."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    if edges.size and (edges.min() < 0 or edges.max() >= n):
        raise ValueError(f"GraphPaths: an edge names a node outside [0, {n})")
    src = np.concatenate([edges[:, 0], edges[:, 1]])
    dst = np.concatenate([edges[:, 1], edges[:, 0]])
    order = np.argsort(src, kind="stable")
    row_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=row_ptr[1:])
    return row_ptr, np.ascontiguousarray(dst[order].astype(np.int32))


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


class GraphPaths(DeviceHandle):
    """One graph on a HIP device.  ``node_names`` is the list of nodes in index order and ``index`` maps a node to its
    index; the three methods take node INDICES (tensors or sequences) and return tensors on the device."""

    PREFIX = "hm_graph"

    def __init__(self, graph, device=None):
        if isinstance(graph, tuple) and len(graph) == 2:
            names, edges = list(graph[0]), np.asarray(graph[1], dtype=np.int64)
            if edges.ndim == 2 and edges.shape[1] != 2 and edges.shape[0] == 2:
                edges = edges.T
        else:
            names = list(graph.nodes())
            index = {name: k for k, name in enumerate(names)}
            edges = np.array([(index[e[0]], index[e[1]]) for e in graph.edges()], dtype=np.int64).reshape(-1, 2)
        self.n = len(names)
        if self.n < 1:
            raise ValueError("GraphPaths: a graph without nodes")
        if self.n > MAX_NODES:                   # the library refuses it as well; checked before a handle exists
            raise ValueError(f"GraphPaths: {self.n} nodes, the limit is 2^24")
        self.node_names: List[Hashable] = names
        self.index: Dict[Hashable, int] = {name: k for k, name in enumerate(names)}
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        super().__init__(device)
        row_ptr, col = symmetric_csr(self.n, edges)
        self.nnz = int(row_ptr[-1])
        self._check(self._L.hm_graph_set_csr(self._h, C.c_void_p(row_ptr.ctypes.data), C.c_void_p(col.ctypes.data), self.n,
                                             self._stream()))

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
