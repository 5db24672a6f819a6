"""CPU truth and golden loaders shared by the hierarchy-distortion tests (test_distortion_golden.py without a GPU,
test_gpu_distortion.py with one) and by the golden generator.  Pure Python: no networkx.

  adjacency(n, edges)          neighbour lists of the undirected graph (self-loops and repeated edges kept: harmless)
  bfs_lengths(adj, src)        path length from src to every node, -1 where there is no path
  component_labels(n, edges)   union-find: the smallest node index of every node's component
  Graph                        the duck type GraphPaths and eval_hierarchy take: .nodes(), .edges()
  load(golden_dir, mode)       the cases of g14_distortion_<mode>
  rng_hash()                   sha256 of random.getstate(), as the goldens record it
"""
from __future__ import annotations

import hashlib
import json
import os
import random
from collections import deque

import numpy as np

SIGN_MODE = {"reference": 0, "lorentz": 1}
MODES = ("reference", "lorentz")


def adjacency(n: int, edges) -> list:
    adj = [[] for _ in range(n)]
    for a, b in np.asarray(edges, np.int64).reshape(-1, 2).tolist():
        adj[a].append(b)
        adj[b].append(a)
    return adj


def bfs_lengths(adj: list, src: int) -> list:
    dist = [-1] * len(adj)
    dist[src] = 0
    queue = deque([src])
    while queue:
        v = queue.popleft()
        for u in adj[v]:
            if dist[u] < 0:
                dist[u] = dist[v] + 1
                queue.append(u)
    return dist


def component_labels(n: int, edges) -> list:
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    for a, b in np.asarray(edges, np.int64).reshape(-1, 2).tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)          # the smaller index stays root: the root is the component's minimum
    return [find(v) for v in range(n)]


class Graph:
    """Nodes in index order and an edge list of node names: what ``.nodes()`` / ``.edges()`` of a graph object give."""

    def __init__(self, names, edges):
        self._names = list(names)
        self._edges = [(self._names[a], self._names[b]) for a, b in np.asarray(edges, np.int64).reshape(-1, 2).tolist()]

    def nodes(self):
        return list(self._names)

    def edges(self):
        return list(self._edges)

    def number_of_nodes(self):
        return len(self._names)

    def number_of_edges(self):
        return len(self._edges)


class Case:
    """One recorded run of the reference: its graph (shared among the runs on it), inputs and results."""

    def __init__(self, meta: dict, graphs: dict, z):
        name = meta["name"]
        self.name = name
        self.meta = meta
        self.graph_name = meta["graph"]
        shared = graphs[self.graph_name]
        self.nodes = shared["nodes"]
        self.vocab = shared["vocab"]
        self.mapping = [(k, int(v)) for k, v in shared["mapping"]]
        self.seed, self.curvature, self.num_pairs = meta["seed"], meta["curvature"], meta["num_pairs"]
        self.edges = z[f"{self.graph_name}__edges"].astype(np.int64)
        self.emb = z[f"{self.graph_name}__emb"]
        self.tried = z[f"{name}__tried"].astype(np.int64)        # [T, 3]: node a, node b, path length or -1
        self.ratios = z[f"{name}__ratios"]
        self.n = len(self.nodes)
        self.index = {v: k for k, v in enumerate(self.nodes)}

    @property
    def accepted(self) -> np.ndarray:
        return self.tried[self.tried[:, 2] >= 0]

    def graph(self) -> Graph:
        return Graph(self.nodes, self.edges)

    def __repr__(self):
        return f"Case({self.name})"


_CACHE: dict = {}


def load(golden_dir: str, mode: str) -> list:
    key = (golden_dir, mode)
    if key not in _CACHE:
        meta = json.load(open(os.path.join(golden_dir, f"g14_distortion_{mode}.json")))
        z = np.load(os.path.join(golden_dir, f"g14_distortion_{mode}.npz"))
        _CACHE[key] = [Case(c, meta["graphs"], z) for c in meta["cases"]]
    return _CACHE[key]


_TRUTH: dict = {}


def truth(case: Case) -> dict:
    """{"adj", "labels", "rows": all-pairs path lengths int64 [n, n]} of a case's graph, computed once."""
    if case.graph_name not in _TRUTH:
        adj = adjacency(case.n, case.edges)
        rows = np.array([bfs_lengths(adj, v) for v in range(case.n)], np.int64)
        _TRUTH[case.graph_name] = {"adj": adj, "labels": component_labels(case.n, case.edges), "rows": rows}
    return _TRUTH[case.graph_name]


def rng_hash() -> str:
    return hashlib.sha256(repr(random.getstate()).encode()).hexdigest()
