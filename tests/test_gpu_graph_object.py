"""One ``Graph`` handed to ``GraphPaths``, ``NegativeSampler`` and ``reconstruction_metrics`` gives, bit for bit, what the raw
``(names, edges)`` tuple gives to fresh instances of the same three."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

N = 63
TREE = [((k - 1) // 2, k) for k in range(1, N)]                        # 62 edges
CHORDS = [(7, 12), (20, 45), (3, 60), (31, 62), (15, 16)]
EDGES = TREE + CHORDS + [(9, 9), (3, 1)]                               # a self-loop, and the tree edge (1, 3) once more
CHOSEN = [0, 1, 9, 15, 16, 31, 45, 62]


def test_graph_object_and_tuple_give_the_same_bits():
    from hyptokenizer_amd.embedding.graph_embedding import NegativeSampler
    from hyptokenizer_amd.embedding.graph_metrics import reconstruction_metrics
    from hyptokenizer_amd.graph import Graph
    from hyptokenizer_amd.graph_paths import GraphPaths
    from hyptokenizer_amd.synthetic import lorentz_table
    names = [f"n{k}" for k in range(N)]
    edges = np.array(EDGES, np.int64)
    table = lorentz_table(N, 4, seed=3, scale=0.5).to(DEV)
    assert table.shape == (N, 5)
    pairs = torch.from_numpy(edges).to(DEV)
    src = [a for a in CHOSEN for _ in CHOSEN]
    dst = [b for _ in CHOSEN for b in CHOSEN]
    results = []
    for graph in (Graph.of((names, edges)), (names, edges.copy())):
        paths, sampler = GraphPaths(graph, DEV), NegativeSampler(graph, 5, seed=11, device=DEV)
        try:
            # by hand: the BFS form keeps both directions of all 69 edges, the sampler's form those of the 62 + 5 distinct
            # edges that are no loop
            assert (paths.n, sampler.n) == (N, N) and paths.nnz == 2 * 69 == 138 and sampler.nnz == 2 * 67 == 134
            assert paths.node_names == names and sampler.index["n62"] == 62
            got = {"components": paths.components(), "lengths": paths.path_lengths(src, dst), "rows": paths.distance_rows(CHOSEN),
                   "step0": sampler.sample(pairs, 0), "step1": sampler.sample(pairs, 1)}
            got = {k: v.cpu().numpy() for k, v in got.items()}
        finally:
            paths.close()
            sampler.close()
        got["metrics"] = reconstruction_metrics(table, graph)
        results.append(got)
    ours, raw = results
    for key in ("components", "lengths", "rows", "step0", "step1"):
        assert ours[key].dtype == raw[key].dtype and np.array_equal(ours[key], raw[key]), key
    assert set(ours["metrics"]) == {"mean_rank", "map", "num_pairs", "num_nodes"}
    for key, value in ours["metrics"].items():
        assert np.float64(value).tobytes() == np.float64(raw["metrics"][key]).tobytes(), key
    # and the answers are answers: one component, 64 lengths with a zero diagonal that agree with the rows, negatives drawn
    assert not ours["components"].any() and ours["lengths"].shape == (64,) and ours["rows"].shape == (8, N)
    assert np.array_equal(ours["lengths"].reshape(8, 8), ours["rows"][:, CHOSEN].astype(np.int32))
    assert not ours["lengths"].reshape(8, 8).diagonal().any() and ours["lengths"].reshape(8, 8)[0, 7] == 5
    assert ours["step0"].shape == (69, 7) and not np.array_equal(ours["step0"], ours["step1"])
    assert ours["metrics"]["num_pairs"] == 134 and ours["metrics"]["num_nodes"] == N
