#!/usr/bin/env python
"""Evaluate the hierarchy distortion of tokenizer embeddings against a WordNet graph.

Function surface of the reference's ``scripts/eval_hierarchy.py`` (same six names, arguments, defaults and output
files), with ``sign_convention=`` / ``--sign-convention`` (reference | lorentz) as ``train_hyperbolic_tokenizer.py`` has
it.  The reference samples node pairs, divides the hyperbolic distance of the two tokens by the pair's graph distance and
reports mean / median / min / max / std of the ratios.  What differs is where the work happens:

* graph distances: one ``GraphPaths.path_lengths`` call (a bit-parallel multi-source BFS on the HIP device) for all sampled
  pairs, instead of one ``nx.shortest_path_length`` per pair;
* connectivity: the sampler retries on component labels computed once on the device, and consumes Python's global RNG
  exactly as the reference's try / except loop does (``sample_node_pairs``);
* distances: one gathered ``lorentz_model.distance`` call instead of one call and one ``.item()`` per pair;
* ``create_node_mapping`` looks words up in one ``{token: first index}`` dict instead of ``vocab.index`` per node.

Deviations, documented: ``load_wordnet_graph`` uses ``pickle.load`` (the reference calls ``nx.read_gpickle``, which
networkx 3 no longer has, on a file its own builder writes with plain ``pickle``; networkx is needed only to unpickle);
``sample_node_pairs`` raises ``ValueError`` when no component holds two mapped nodes, where the reference never returns.

``compute_distortion_exhaustive`` is additive: the same ratio over EVERY connected pair of mapped nodes.
"""
from __future__ import annotations

import json
import logging
import os
import pickle
import random
from collections import Counter
from typing import Any, Dict, Hashable, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch
import typer

from hyptokenizer_amd.embedding.lorentz_model import batch_distance, distance
from hyptokenizer_amd.graph import Graph
from hyptokenizer_amd.graph_paths import GraphPaths

logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(name)s - %(levelname)s - %(message)s")
logger = logging.getLogger(__name__)


def set_seeds(seed: int = 42) -> None:
    """Reference ``:35-46``."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def load_wordnet_graph(graph_path: str):
    """Reference ``:49-62``, with ``pickle.load`` in place of ``nx.read_gpickle`` (see the module docstring)."""
    logger.info(f"Loading WordNet graph from {graph_path}")
    with open(graph_path, "rb") as f:
        graph = pickle.load(f)
    logger.info(f"Loaded graph with {graph.number_of_nodes()} nodes and {graph.number_of_edges()} edges")
    return graph


def create_node_mapping(graph, vocab: List[str]) -> Dict[str, int]:
    """Reference ``:65-89``: node name -> vocabulary index of the word before the first ``'.'``, for the words the
    vocabulary holds; key order is ``graph.nodes()`` order and the index is the word's FIRST occurrence, as
    ``vocab.index`` gives it."""
    first: Dict[str, int] = {}
    for k, token in enumerate(vocab):
        first.setdefault(token, k)
    mapping: Dict[str, int] = {}
    nodes = Graph.of(graph).node_names
    for node in nodes:
        k = first.get(node.split(".")[0])
        if k is not None:
            mapping[node] = k
    logger.info(f"Created mapping for {len(mapping)}/{len(nodes)} nodes")
    return mapping


def sample_node_pairs(valid_nodes: Sequence[Hashable], labels: Mapping[Hashable, int], num_pairs: int) -> List[Tuple[Hashable, Hashable]]:
    """The reference's sampling loop (``:124-136``) on the host: ``random.sample(valid_nodes, 2)``, drawn again while
    the two nodes lie in different components (``labels[node]`` = component label), where the reference catches
    ``NetworkXNoPath``.  It draws from Python's global RNG exactly as often as the reference does, so the pairs and the
    RNG state afterwards are the reference's.  Raises ``ValueError`` when no component holds two valid nodes."""
    valid_nodes = list(valid_nodes)
    if num_pairs > 0 and (not valid_nodes or max(Counter(labels[v] for v in valid_nodes).values()) < 2):
        raise ValueError("sample_node_pairs: no connected component holds two mapped nodes; no pair can be sampled")
    pairs = []
    for _ in range(num_pairs):
        while True:
            a, b = random.sample(valid_nodes, 2)
            if labels[a] == labels[b]:
                pairs.append((a, b))
                break
    return pairs


def _stats(ratios: np.ndarray) -> Dict[str, float]:
    return {
        "mean": float(np.mean(ratios)),
        "median": float(np.median(ratios)),
        "min": float(np.min(ratios)),
        "max": float(np.max(ratios)),
        "std": float(np.std(ratios)),
        "num_pairs": len(ratios),
    }


def _device(device) -> torch.device:
    if device is None:
        return torch.device("cuda" if torch.cuda.is_available() else "cpu")
    return torch.device(device)


def compute_distortion(graph, embeddings: torch.Tensor, node_mapping: Dict[str, int], num_pairs: int = 10000,
                       curvature: float = 1.0, device: Optional[torch.device] = None,
                       sign_convention: Optional[str] = None) -> Tuple[np.ndarray, Dict[str, float]]:
    """Reference ``:92-172``: (distortion ratios float64 ``[num_pairs]``, statistics)."""
    device = _device(device)
    paths = GraphPaths(graph, device)
    try:
        valid_nodes = list(node_mapping.keys())
        logger.info(f"Sampling from {len(valid_nodes)} valid nodes")
        comp = paths.components().cpu().numpy()
        labels = {node: int(comp[paths.index[node]]) for node in valid_nodes}
        pairs = sample_node_pairs(valid_nodes, labels, num_pairs)
        logger.info(f"Sampled {len(pairs)} node pairs")
        graph_dist = paths.path_lengths([paths.index[a] for a, _ in pairs], [paths.index[b] for _, b in pairs])
        emb = embeddings.detach().to(device)
        i = torch.tensor([node_mapping[a] for a, _ in pairs], dtype=torch.long, device=device)
        j = torch.tensor([node_mapping[b] for _, b in pairs], dtype=torch.long, device=device)
        emb_dist = distance(emb[i], emb[j], c=curvature, sign_convention=sign_convention)
        # the reference divides a Python float (the fp32 distance widened) by a Python int: float64 division, on the host
        ratios = emb_dist.double().cpu().numpy() / graph_dist.cpu().numpy().astype(np.float64)
    finally:
        paths.close()
    stats = _stats(ratios)
    logger.info(f"Computed distortion statistics: {stats}")
    return ratios, stats


def compute_distortion_exhaustive(graph, embeddings: torch.Tensor, node_mapping: Dict[str, int], curvature: float = 1.0,
                                  device: Optional[torch.device] = None, source_batch: int = 1024,
                                  sign_convention: Optional[str] = None) -> Dict[str, float]:
    """The distortion ratio over EVERY unordered pair of distinct mapped nodes that a path connects, instead of a sample.

    Per batch of ``source_batch`` mapped nodes: ``GraphPaths.distance_rows`` to all mapped nodes, ``batch_distance`` of
    the batch's embeddings against all mapped nodes' (by column slices), and float64 sum, sum of squares, min, max and
    count kept on the device.  Returns ``mean``, ``min``, ``max``, ``std`` (population, as ``np.std``) and ``num_pairs``.
    There is NO ``median``: it would need every ratio at once, which is what this function avoids."""
    device = _device(device)
    if source_batch < 1:
        raise ValueError("compute_distortion_exhaustive: source_batch must be positive")
    paths = GraphPaths(graph, device)
    try:
        valid_nodes = list(node_mapping.keys())
        node_idx = [paths.index[v] for v in valid_nodes]
        nv = len(valid_nodes)
        emb = embeddings.detach().to(device)
        rows_emb = emb[torch.tensor([node_mapping[v] for v in valid_nodes], dtype=torch.long, device=device)]
        total = torch.zeros((), dtype=torch.float64, device=device)
        total_sq = torch.zeros((), dtype=torch.float64, device=device)
        lo = torch.full((), float("inf"), dtype=torch.float64, device=device)
        hi = torch.full((), float("-inf"), dtype=torch.float64, device=device)
        count = torch.zeros((), dtype=torch.int64, device=device)
        position = torch.arange(nv, device=device)
        col_step = 8192
        for r0 in range(0, nv, source_batch):
            r1 = min(nv, r0 + source_batch)
            hops = paths.distance_rows(node_idx[r0:r1], node_idx)                     # int16 [B, nv]
            for c0 in range(r0 + 1, nv, col_step):                                    # columns after the batch's first row
                c1 = min(nv, c0 + col_step)
                g = hops[:, c0:c1]
                keep = (g > 0) & (position[c0:c1][None, :] > position[r0:r1][:, None])
                d = batch_distance(rows_emb[r0:r1], rows_emb[c0:c1], c=curvature, sign_convention=sign_convention)
                ratio = d.double() / g.double()
                picked = ratio[keep]
                if picked.numel() == 0:
                    continue
                total += picked.sum()
                total_sq += (picked * picked).sum()
                lo = torch.minimum(lo, picked.min())
                hi = torch.maximum(hi, picked.max())
                count += picked.numel()
    finally:
        paths.close()
    n = int(count.item())
    if n == 0:
        raise ValueError("compute_distortion_exhaustive: no connected pair of mapped nodes")
    mean = total.item() / n
    var = max(total_sq.item() / n - mean * mean, 0.0)
    return {"mean": mean, "min": lo.item(), "max": hi.item(), "std": var ** 0.5, "num_pairs": n}


def evaluate_hierarchy(embeddings_path: str, vocab_path: str, graph_path: str, output_path: str, num_pairs: int = 10000,
                       curvature: float = 1.0, seed: int = 42, sign_convention: Optional[str] = None) -> Dict[str, float]:
    """Reference ``:175-246``: writes the ratios to ``output_path`` (.npy) and the statistics to ``<stem>_stats.json``."""
    set_seeds(seed)
    device = _device(None)
    logger.info(f"Using device: {device}")
    embeddings = torch.load(embeddings_path, map_location=device)
    if isinstance(embeddings, torch.nn.Parameter):
        embeddings = embeddings.data
    logger.info(f"Loaded embeddings with shape {embeddings.shape}")
    with open(vocab_path, "r") as f:
        vocab = json.load(f)
    logger.info(f"Loaded vocabulary with {len(vocab)} tokens")
    graph = Graph.of(load_wordnet_graph(graph_path))
    node_mapping = create_node_mapping(graph, vocab)
    ratios, stats = compute_distortion(graph=graph, embeddings=embeddings, node_mapping=node_mapping, num_pairs=num_pairs,
                                       curvature=curvature, device=device, sign_convention=sign_convention)
    out_dir = os.path.dirname(output_path)
    if out_dir:                                   # a bare file name has no directory to make
        os.makedirs(out_dir, exist_ok=True)
    np.save(output_path, ratios)
    logger.info(f"Saved distortion ratios to {output_path}")
    stats_path = os.path.splitext(output_path)[0] + "_stats.json"
    with open(stats_path, "w") as f:
        json.dump(stats, f, indent=4)
    logger.info(f"Saved statistics to {stats_path}")
    return stats


def main(
    embeddings_path: str = "results/hyperbolic/v50000/embeddings.pt",
    vocab_path: str = "results/hyperbolic/v50000/vocab.json",
    graph_path: str = "data/processed/wordnet_graph.gpk",
    output_path: str = "results/hyperbolic/v50000/hierarchy_distortion.npy",
    num_pairs: int = 10000,
    curvature: float = 1.0,
    seed: int = 42,
    sign_convention: str = "reference",
) -> None:
    """Evaluate hierarchy distortion of embeddings."""
    evaluate_hierarchy(embeddings_path=embeddings_path, vocab_path=vocab_path, graph_path=graph_path, output_path=output_path,
                       num_pairs=num_pairs, curvature=curvature, seed=seed, sign_convention=sign_convention)


if __name__ == "__main__":
    typer.run(main)
