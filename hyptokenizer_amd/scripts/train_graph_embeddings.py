#!/usr/bin/env python
"""Embed a graph in hyperbolic space: ``fit_graph_embedding`` (edge-softmax loss, negative sampler and Riemannian
optimiser, all on the HIP device) from the command line.

``--graph-path`` is the pickle ``scripts/eval_hierarchy.py`` reads (``load_wordnet_graph``), or a text file with one edge per
line, two node names separated by a tab; node indices are then the order of first appearance.  Writes ``embeddings.pt`` (fp32
``[V, dim + 1]``), ``nodes.json`` (node names in row order) and ``train_log.json`` (hyper-parameters and the mean loss of every
epoch) to ``--output-dir``; with ``--eval-pairs N > 0`` also ``distortion_stats.json`` from ``compute_distortion`` over N
sampled pairs; with ``--eval-reconstruction`` also ``reconstruction_stats.json``: ``reconstruction_metrics`` (mean rank and mAP
of the graph's edges) of the trained table and, under ``"initial"``, of the table training started from; with
``--eval-hyperbolicity N > 0`` also ``hyperbolicity_stats.json``: Gromov's delta, its relative form and the curvature estimate
 of the graph metric and of the trained table's distances on the same sample of N nodes.
``--objective cones`` trains a directed hierarchy with the entailment-cone loss instead (an edge's first node is
the parent; ``--margin``, ``--aperture-k``; ``--closure`` trains on the transitive closure of the edges) and records those
options in ``train_log.json``; ``--eval-cones`` writes ``cone_stats.json``: ``cone_stats`` of the graph's edges under the
trained table and, under ``"initial"``, under the table training started from.  The reference has no counterpart: it never
trains its embeddings.
"""
from __future__ import annotations

import json
import logging
import os
from typing import Dict

import torch
import typer

from hyptokenizer_amd.embedding.entailment_cones import cone_stats, directed_pairs
from hyptokenizer_amd.embedding.graph_embedding import GraphEmbeddingResult, fit_graph_embedding, init_table
from hyptokenizer_amd.embedding.graph_metrics import reconstruction_metrics
from hyptokenizer_amd.embedding.hyperbolicity import curvature_estimate, embedding_hyperbolicity, graph_hyperbolicity
from hyptokenizer_amd.graph import Graph
from hyptokenizer_amd.graph_paths import GraphPaths
from hyptokenizer_amd.scripts.eval_hierarchy import compute_distortion, load_wordnet_graph, set_seeds

logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(name)s - %(levelname)s - %(message)s")
logger = logging.getLogger(__name__)


EdgeListGraph = Graph.from_named_edges                      # a list of (name, name) edges -> Graph


def load_edge_list(path: str) -> Graph:
    """One edge per line, two node names separated by a tab; empty lines and lines starting with ``#`` are skipped."""
    edges = []
    with open(path, "r", encoding="utf-8") as f:
        for no, line in enumerate(f, 1):
            line = line.rstrip("\n")
            if not line.strip() or line.startswith("#"):
                continue
            parts = line.split("\t")
            if len(parts) != 2 or not parts[0] or not parts[1]:
                raise ValueError(f"{path}:{no}: expected two tab-separated node names")
            edges.append((parts[0], parts[1]))
    return Graph.from_named_edges(edges)


def load_graph(graph_path: str) -> Graph:
    """Normalised once: training and every evaluation below share the one ``Graph`` and the CSR forms it keeps."""
    if graph_path.endswith((".tsv", ".txt")):
        return load_edge_list(graph_path)
    return Graph.of(load_wordnet_graph(graph_path))


def train_graph_embeddings(graph_path: str, output_dir: str, dim: int = 10, epochs: int = 50, batch_size: int = 1024,
                           num_negatives: int = 50, lr: float = 0.3, burn_in_epochs: int = 10, burn_in_factor: float = 0.1,
                           optimizer: str = "rsgd", init_scale: float = 1e-3, seed: int = 0, curvature: float = 1.0,
                           eval_pairs: int = 0, log_every: int = 1, eval_reconstruction: bool = False,
                           eval_hyperbolicity: int = 0, objective: str = "softmax", margin: float = 0.01, aperture_k: float = 0.1,
                           closure: bool = False, eval_cones: bool = False) -> GraphEmbeddingResult:
    graph = load_graph(graph_path)
    params = dict(dim=dim, epochs=epochs, batch_size=batch_size, num_negatives=num_negatives, lr=lr, burn_in_epochs=burn_in_epochs,
                  burn_in_factor=burn_in_factor, optimizer=optimizer, init_scale=init_scale, seed=seed, c=curvature)
    if objective != "softmax":                                # the log of a softmax run keeps the keys it always had
        params.update(objective=objective, margin=margin, aperture_k=aperture_k, closure=closure)
    result = fit_graph_embedding(graph, log_every=log_every, **params)
    os.makedirs(output_dir, exist_ok=True)
    torch.save(result.table.cpu(), os.path.join(output_dir, "embeddings.pt"))
    with open(os.path.join(output_dir, "nodes.json"), "w") as f:
        json.dump([str(n) for n in result.node_names], f)
    with open(os.path.join(output_dir, "train_log.json"), "w") as f:
        json.dump(dict(params, graph_path=graph_path, nodes=len(result.node_names), loss_history=result.loss_history), f, indent=4)
    logger.info(f"Saved embeddings of {len(result.node_names)} nodes to {output_dir}")
    if eval_pairs > 0:
        set_seeds(seed)
        _, stats = compute_distortion(graph, result.table, result.node_mapping, num_pairs=eval_pairs, curvature=curvature,
                                      device=result.table.device, sign_convention="lorentz")
        with open(os.path.join(output_dir, "distortion_stats.json"), "w") as f:
            json.dump(stats, f, indent=4)
    if eval_reconstruction:
        table0 = init_table(len(result.node_names), dim, init_scale, seed, result.table.device)
        stats = reconstruction_metrics(result.table, graph, node_mapping=result.node_mapping)
        stats["initial"] = reconstruction_metrics(table0, graph, node_mapping=result.node_mapping)
        with open(os.path.join(output_dir, "reconstruction_stats.json"), "w") as f:
            json.dump(stats, f, indent=4)
        logger.info(f"Reconstruction: mean rank {stats['mean_rank']:.3f}, mAP {stats['map']:.4f} over {stats['num_pairs']} pairs")
    if eval_hyperbolicity > 0:
        with open(os.path.join(output_dir, "hyperbolicity_stats.json"), "w") as f:
            json.dump(hyperbolicity_stats(graph, result, eval_hyperbolicity, seed, curvature), f, indent=4)
    if eval_cones:
        edges = directed_pairs(graph, closure=False)          # rows: fit_graph_embedding numbers the nodes in the same order
        stats = cone_stats(result.table, edges, aperture_k=aperture_k)
        stats["initial"] = cone_stats(init_table(len(result.node_names), dim, init_scale, seed, result.table.device), edges,
                                      aperture_k=aperture_k)
        with open(os.path.join(output_dir, "cone_stats.json"), "w") as f:
            json.dump(stats, f, indent=4)
        logger.info(f"Cones: mean energy {stats['mean_energy']:.4f} ({stats['share_inside']:.3f} inside) over {stats['num_edges']} "
                    f"edges, reversed {stats['reversed_mean_energy']:.4f} ({stats['reversed_share_inside']:.3f} inside)")
    return result


def hyperbolicity_stats(graph, result: GraphEmbeddingResult, num_samples: int, seed: int, curvature: float) -> Dict[str, object]:
    """Gromov's delta of the graph metric and of the trained table's distances on one node sample: the sample the graph side
    keeps (its largest component among the drawn nodes), mapped to table rows."""
    paths = GraphPaths(graph, device=result.table.device)
    g = graph_hyperbolicity(paths, num_samples=num_samples, seed=seed)
    rows = [result.node_mapping[paths.node_names[int(k)]] for k in g.nodes_used]
    t = embedding_hyperbolicity(result.table, nodes=rows, num_samples=len(rows), base_points=g.base_positions.tolist(), seed=seed,
                                c=curvature)

    def side(h):
        return {"delta": h.delta, "delta_rel": h.delta_rel, "diameter": h.diameter, "n_used": h.n_used,
                # null: no diameter; "inf": delta 0, a tree fits every curvature (strict JSON has no infinity)
                "curvature_estimate": None if h.delta_rel != h.delta_rel else
                ("inf" if h.delta_rel == 0.0 else curvature_estimate(h.delta_rel)),
                "witness": list(h.witness)}
    stats = {"num_samples": int(num_samples), "seed": int(seed), "graph": side(g), "embedding": side(t)}
    logger.info(f"Hyperbolicity: graph delta {g.delta} (relative {g.delta_rel:.4f}), embedding delta {t.delta:.4f} "
                f"(relative {t.delta_rel:.4f}) on {g.n_used} nodes")
    return stats


def main(
    graph_path: str = "data/processed/wordnet_graph.gpk",
    output_dir: str = "results/graph_embedding",
    dim: int = 10,
    epochs: int = 50,
    batch_size: int = 1024,
    num_negatives: int = 50,
    lr: float = 0.3,
    burn_in_epochs: int = 10,
    burn_in_factor: float = 0.1,
    optimizer: str = "rsgd",
    init_scale: float = 1e-3,
    seed: int = 0,
    curvature: float = 1.0,
    eval_pairs: int = 0,
    eval_reconstruction: bool = False,
    eval_hyperbolicity: int = 0,
    objective: str = "softmax",
    margin: float = 0.01,
    aperture_k: float = 0.1,
    closure: bool = False,
    eval_cones: bool = False,
) -> None:
    """Train hyperbolic embeddings of a graph."""
    train_graph_embeddings(graph_path=graph_path, output_dir=output_dir, dim=dim, epochs=epochs, batch_size=batch_size,
                           num_negatives=num_negatives, lr=lr, burn_in_epochs=burn_in_epochs, burn_in_factor=burn_in_factor,
                           optimizer=optimizer, init_scale=init_scale, seed=seed, curvature=curvature, eval_pairs=eval_pairs,
                           eval_reconstruction=eval_reconstruction, eval_hyperbolicity=eval_hyperbolicity, objective=objective,
                           margin=margin, aperture_k=aperture_k, closure=closure, eval_cones=eval_cones)


if __name__ == "__main__":
    typer.run(main)
