#!/usr/bin/env python
"""Measure the hierarchy-distortion evaluation at WordNet size and write profiles/hierarchy_distortion_probe.json.

Graph: a synthetic tree-with-extras of WordNet's noun-hypernym SHAPE (about 82 000 nodes, 84 000 edges, depth 15-20).  The
WordNet figures (82 115 noun synsets, 84 428 hypernym edges) are from memory, not measured on the real graph: node k > 0
hangs under a node of a level chosen so that the level sizes grow and shrink as a hypernym tree's do, and 2 300 nodes get a
second parent one level up (multiple inheritance).  Vocabulary 50 000 tokens, d = 100, num_pairs = 10 000.

Recorded: stream time of components, of the BFS and of the gathered distance (an event pair around the whole call, median
of REPEATS: for the two graph calls that interval holds their host side too -- sort and dedup of the sources, the staging
copy, the reads of the control block between chunks of levels), BFS levels / launches / passes / words per node, wall time of compute_distortion and of the exhaustive mode (on a subset of
EXHAUSTIVE_NODES mapped nodes, stated in the file), and the same 10 000 pairs through a networkx loop when networkx
imports (else through a pure-Python BFS per pair).  No threshold: the file says what was measured, also where the GPU
path loses.

Usage: python tools/hierarchy_distortion_probe.py [--out profiles/hierarchy_distortion_probe.json]
"""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import time
from collections import deque

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hyptokenizer_amd.embedding.lorentz_model import distance  # noqa: E402
from hyptokenizer_amd.graph_paths import GraphPaths  # noqa: E402
from hyptokenizer_amd.scripts import eval_hierarchy as EH  # noqa: E402
from hyptokenizer_amd.synthetic import lorentz_table  # noqa: E402

N_NODES, N_EXTRA, VOCAB, D, NUM_PAIRS, REPEATS = 82115, 2300, 50000, 100, 10000, 5
EXHAUSTIVE_NODES = 8192
# share of the nodes per depth level (root = level 0), roughly a hypernym tree's profile
LEVEL_SHARE = [0.00002, 0.0001, 0.0005, 0.003, 0.012, 0.04, 0.09, 0.15, 0.19, 0.18, 0.14, 0.09, 0.055, 0.028, 0.013, 0.006, 0.002, 0.0008]


class SyntheticGraph:
    def __init__(self, names, edges):
        self.names, self.edge_index = names, edges

    def nodes(self):
        return self.names

    def edges(self):
        names = self.names
        return [(names[a], names[b]) for a, b in self.edge_index]

    def number_of_nodes(self):
        return len(self.names)

    def number_of_edges(self):
        return len(self.edge_index)


def wordnet_shaped_graph(seed: int = 0):
    """(graph, depth of its tree)"""
    rs = np.random.RandomState(seed)
    sizes = [max(1, int(round(s * N_NODES))) for s in LEVEL_SHARE]
    sizes[0] = 1
    sizes[8] += N_NODES - sum(sizes)
    level_start = np.concatenate([[0], np.cumsum(sizes)])
    edges = []
    for lv in range(1, len(sizes)):
        lo, hi = level_start[lv - 1], level_start[lv]
        parents = rs.randint(lo, hi, sizes[lv])
        edges += list(zip(parents.tolist(), range(level_start[lv], level_start[lv + 1])))
    for child in rs.randint(level_start[3], N_NODES, N_EXTRA).tolist():         # a second parent one level up
        lv = int(np.searchsorted(level_start, child, side="right")) - 1
        edges.append((int(rs.randint(level_start[lv - 1], level_start[lv])), child))
    names = [f"w{k}.n.01" for k in range(N_NODES)]
    return SyntheticGraph(names, edges), len(sizes) - 1


def event_ms(fn, repeats=REPEATS):
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def host_loop_seconds(graph: SyntheticGraph, pairs):
    """The reference's per-pair loop: networkx when it imports, else a pure-Python BFS per pair."""
    try:
        import networkx as nx
        g = nx.Graph()
        g.add_nodes_from(graph.nodes())
        g.add_edges_from(graph.edges())
        t0 = time.perf_counter()
        lengths = [nx.shortest_path_length(g, a, b) for a, b in pairs]
        return "networkx " + nx.__version__, time.perf_counter() - t0, lengths
    except ImportError:
        index = {v: k for k, v in enumerate(graph.nodes())}
        adj = [[] for _ in index]
        for a, b in graph.edge_index:
            adj[a].append(b)
            adj[b].append(a)
        t0 = time.perf_counter()
        lengths = []
        for a, b in pairs:
            src, dst = index[a], index[b]
            dist = {src: 0}
            queue = deque([src])
            while queue and dst not in dist:
                v = queue.popleft()
                for u in adj[v]:
                    if u not in dist:
                        dist[u] = dist[v] + 1
                        queue.append(u)
            lengths.append(dist[dst])
        return "pure-Python BFS per pair", time.perf_counter() - t0, lengths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hierarchy_distortion_probe.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    graph, depth = wordnet_shaped_graph()
    rs = random.Random(1)
    vocab = [f"w{k}" for k in rs.sample(range(N_NODES), VOCAB)]
    emb = lorentz_table(VOCAB, D, seed=3, scale=0.3).to(dev)
    mapping = EH.create_node_mapping(graph, vocab)
    out = {"graph": {"nodes": N_NODES, "edges": graph.number_of_edges(), "tree_depth": depth,
                     "note": "synthetic, WordNet noun-hypernym shape; the WordNet figures are from memory"},
           "vocab": VOCAB, "d": D, "num_pairs": NUM_PAIRS, "mapped_nodes": len(mapping), "device": torch.cuda.get_device_name(0)}

    gp = GraphPaths(graph, dev)
    labels = gp.components()
    out["components"] = {"stream_ms": event_ms(gp.components), **gp.last_stats(), "n_components": gp.n_components}
    comp = labels.cpu().numpy()
    label_of = {v: int(comp[gp.index[v]]) for v in mapping}
    EH.set_seeds(42)
    pairs = EH.sample_node_pairs(list(mapping), label_of, NUM_PAIRS)
    src = [gp.index[a] for a, _ in pairs]
    dst = [gp.index[b] for _, b in pairs]
    lengths = gp.path_lengths(src, dst)
    t0 = time.perf_counter()
    gp.path_lengths(src, dst)
    torch.cuda.synchronize()
    bfs_wall = time.perf_counter() - t0
    out["bfs"] = {"stream_ms": event_ms(lambda: gp.path_lengths(src, dst)), "wall_ms": bfs_wall * 1e3, **gp.last_stats(),
                  "distinct_sources": len(set(src)), "max_length": int(lengths.max().item()),
                  "bit_array_bytes": 3 * N_NODES * gp.last_stats()["words"] * 8}
    i = torch.tensor([mapping[a] for a, _ in pairs], device=dev)
    j = torch.tensor([mapping[b] for _, b in pairs], device=dev)
    out["distance"] = {"stream_ms": event_ms(lambda: distance(emb[i], emb[j], 1.0, sign_convention="lorentz"))}
    gp.close()

    EH.set_seeds(42)
    t0 = time.perf_counter()
    ratios, stats = EH.compute_distortion(graph, emb, mapping, num_pairs=NUM_PAIRS, device=dev, sign_convention="lorentz")
    out["compute_distortion"] = {"wall_s": time.perf_counter() - t0, "stats": stats}

    sub = dict(list(mapping.items())[:EXHAUSTIVE_NODES])
    t0 = time.perf_counter()
    ex = EH.compute_distortion_exhaustive(graph, emb, sub, device=dev, source_batch=1024, sign_convention="lorentz")
    out["exhaustive"] = {"wall_s": time.perf_counter() - t0, "mapped_nodes_used": len(sub), "source_batch": 1024, "stats": ex}

    how, seconds, host_lengths = host_loop_seconds(graph, pairs)
    out["host_loop"] = {"what": how, "wall_s": seconds, "agrees_with_gpu": host_lengths == lengths.cpu().tolist()}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
