"""One graph, normalised once: ``Graph`` (node names, integer edges, the three host CSR forms, the check of a node selection)
and ``GraphHandle``, the base of the device objects that upload one of those forms.

A graph is given as a ``Graph``, as a tuple ``(node_names, edges)`` with ``edges`` an integer array ``[E, 2]`` of node
positions (``[2, E]`` is transposed), or as any object with ``.nodes()`` and ``.edges()`` (a networkx graph; networkx itself
is never imported here).  A node's index is its position in ``node_names``.  Everything here is host work in numpy.
"""
from __future__ import annotations

import ctypes as C
from functools import cached_property
from typing import Dict, Hashable, Iterable, List, Tuple

import numpy as np
import torch

from ._handle import DeviceHandle

MAX_PATH_NODES = 1 << 24                 # hm_graph: GraphPaths
MAX_SAMPLER_NODES = (1 << 31) - 1        # hm_negsample and the reconstruction walk: int32 node indices

Csr = Tuple[np.ndarray, np.ndarray]      # (row_ptr int64 [n + 1], col int32 [nnz])


def select_nodes(nodes, n: int, who: str, unique: bool = True, what: str = "node") -> np.ndarray:
    """``nodes`` (a tensor or a sequence of indices) as int64 ``[k]``, every one inside ``[0, n)`` and, with ``unique``, none
    twice."""
    sel = torch.as_tensor(nodes).detach().cpu().reshape(-1).numpy().astype(np.int64)
    if sel.size and (sel.min() < 0 or sel.max() >= n):
        raise ValueError(f"{who}: nodes names a {what} outside [0, {n})")
    if unique and np.unique(sel).size != sel.size:
        raise ValueError(f"{who}: nodes must be free of repeats")
    return sel


def _rows(n: int, src: np.ndarray) -> np.ndarray:
    row_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=row_ptr[1:])
    return row_ptr


class Graph:
    """``node_names`` (index order), ``index`` (name -> index), ``n`` and ``edges`` int64 ``[E, 2]``, every entry inside
    ``[0, n)``; ``who`` names the caller in the message when one is not.  The CSR forms are built on first use and kept."""

    def __init__(self, names: Iterable[Hashable], edges, who: str = "Graph"):
        self.node_names: List[Hashable] = list(names)
        self.n = len(self.node_names)
        edges = np.asarray(edges, dtype=np.int64)
        if edges.ndim == 2 and edges.shape[1] != 2 and edges.shape[0] == 2:
            edges = edges.T
        self.edges = edges.reshape(-1, 2)
        if self.edges.size and (self.edges.min() < 0 or self.edges.max() >= self.n):
            raise ValueError(f"{who}: an edge names a node outside [0, {self.n})")

    @classmethod
    def of(cls, x, who: str = "Graph") -> "Graph":
        if isinstance(x, Graph):
            return x
        if isinstance(x, tuple) and len(x) == 2:
            return cls(x[0], x[1], who)
        return cls._named(x.nodes(), x.edges(), who)

    @classmethod
    def from_named_edges(cls, pairs, who: str = "Graph") -> "Graph":
        """The graph of a list of (name, name) edges: nodes are numbered in order of first appearance."""
        pairs = list(pairs)
        return cls._named(dict.fromkeys(name for pair in pairs for name in pair), pairs, who)

    @classmethod
    def _named(cls, names, pairs, who: str) -> "Graph":
        names = list(names)
        index = {name: k for k, name in enumerate(names)}
        g = cls(names, np.array([(index[e[0]], index[e[1]]) for e in pairs], dtype=np.int64).reshape(-1, 2), who)
        g.index = index
        return g

    @cached_property
    def index(self) -> Dict[Hashable, int]:
        return {name: k for k, name in enumerate(self.node_names)}

    def csr(self, canonical: bool = False) -> Csr:
        """The undirected graph, both directions of every edge.  ``canonical=False``: rows in node order, within a row the
        order of the edge list (first the edges that start at the node, then those that end there), repeats and self-loops
        kept -- what a BFS needs.  ``canonical=True``: self-loops dropped, every row sorted and free of repeats -- what a
        binary search in a row needs."""
        return self._canonical_csr if canonical else self._stable_csr

    def out_csr(self) -> Csr:
        """The directed graph: row ``u`` holds the ``v`` of every edge ``(u, v)``, in the order of the edge list."""
        return self._out_csr

    @cached_property
    def _stable_csr(self) -> Csr:
        src = np.concatenate([self.edges[:, 0], self.edges[:, 1]])
        dst = np.concatenate([self.edges[:, 1], self.edges[:, 0]])
        order = np.argsort(src, kind="stable")
        return _rows(self.n, src), np.ascontiguousarray(dst[order].astype(np.int32))

    @cached_property
    def _canonical_csr(self) -> Csr:
        n = self.n
        edges = self.edges[self.edges[:, 0] != self.edges[:, 1]]
        key = np.unique(np.concatenate([edges[:, 0] * n + edges[:, 1], edges[:, 1] * n + edges[:, 0]]))
        return _rows(n, key // n), np.ascontiguousarray((key % n).astype(np.int32))

    @cached_property
    def _out_csr(self) -> Csr:
        order = np.argsort(self.edges[:, 0], kind="stable")
        return _rows(self.n, self.edges[:, 0]), np.ascontiguousarray(self.edges[order, 1].astype(np.int32))

    def select(self, nodes, who: str, unique: bool = True) -> np.ndarray:
        """``select_nodes`` against this graph's ``n``."""
        return select_nodes(nodes, self.n, who, unique)


def symmetric_csr(n: int, edges) -> Csr:
    """``Graph.csr(False)`` of ``edges`` ``[E, 2]`` on the nodes ``0 .. n - 1``."""
    return Graph(range(n), np.asarray(edges, dtype=np.int64).reshape(-1, 2), "GraphPaths").csr(False)


def sorted_symmetric_csr(n: int, edges) -> Csr:
    """``Graph.csr(True)`` of ``edges`` ``[E, 2]`` on the nodes ``0 .. n - 1``."""
    return Graph(range(n), np.asarray(edges, dtype=np.int64).reshape(-1, 2), "NegativeSampler").csr(True)


def graph_arrays(graph) -> Tuple[List[Hashable], np.ndarray]:
    """(node names in index order, edges int64 ``[E, 2]``) of a graph in any accepted form."""
    g = Graph.of(graph)
    return g.node_names, g.edges


class GraphHandle(DeviceHandle):
    """A library handle that holds one CSR form of a graph on a HIP device: ``<PREFIX>_set_csr`` takes ``csr(CANONICAL)``
    of ``Graph.of(graph)``, refused above ``NODE_LIMIT`` nodes.  Argument errors come before the device is looked at."""

    CANONICAL = False
    NODE_LIMIT, NODE_LIMIT_TEXT = MAX_PATH_NODES, "2^24"

    def __init__(self, graph, device=None):
        who = type(self).__name__
        g = Graph.of(graph, who)
        if g.n < 1:
            raise ValueError(f"{who}: a graph without nodes")
        if g.n > self.NODE_LIMIT:                # the library refuses it as well; checked before a handle exists
            raise ValueError(f"{who}: {g.n} nodes, the limit is {self.NODE_LIMIT_TEXT}")
        row_ptr, col = g.csr(self.CANONICAL)
        self.graph, self.n, self.nnz = g, g.n, int(row_ptr[-1])
        self.node_names, self.index, self.edges = g.node_names, g.index, g.edges
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        super().__init__(device)
        self._check(getattr(self._L, self.PREFIX + "_set_csr")(self._h, C.c_void_p(row_ptr.ctypes.data), C.c_void_p(col.ctypes.data),
                                                                self.n, self._stream()))
