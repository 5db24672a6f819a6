"""``hyptokenizer_amd.graph`` without a GPU: every accepted form of a graph normalises to the same ``Graph``, the three CSR
forms equal a builder written here from Python adjacency lists (it shares no code with the package), ``select`` is the check
of a node selection, and the two device objects refuse a bad graph before they look at the device."""
import numpy as np
import pytest
import torch

from hyptokenizer_amd.graph import Graph, select_nodes

# (number of nodes, edges): a path, a star, a graph with a self-loop, a repeated edge, an edge in both orientations and an
# isolated node (5), no edge at all, a single node
GRAPHS = {
    "path": (5, [(0, 1), (1, 2), (2, 3), (3, 4)]),
    "star": (7, [(0, 1), (0, 2), (3, 0), (0, 4), (5, 0), (0, 6)]),
    "untidy": (6, [(0, 1), (2, 2), (1, 3), (1, 3), (3, 4), (4, 3), (2, 0)]),
    "no_edges": (3, []),
    "one_node": (1, []),
}


class Named:
    """The duck type: ``.nodes()`` and ``.edges()`` over node names."""

    def __init__(self, names, edges):
        self._names, self._edges = names, [(names[a], names[b]) for a, b in edges]

    def nodes(self):
        return iter(self._names)

    def edges(self):
        return iter(self._edges)


def names_of(n):
    return [f"v{k}" for k in range(n)]


def flat(rows):
    """Adjacency lists -> (row_ptr, col) with plain loops."""
    row_ptr, col = [0], []
    for row in rows:
        col.extend(row)
        row_ptr.append(len(col))
    return np.array(row_ptr, np.int64), np.array(col, np.int32)


def expected(n, edges):
    stable = [[b for a, b in edges if a == v] + [a for a, b in edges if b == v] for v in range(n)]
    canonical = [sorted({b for a, b in edges if a == v and b != v} | {a for a, b in edges if b == v and a != v}) for v in range(n)]
    out = [[b for a, b in edges if a == v] for v in range(n)]
    return flat(stable), flat(canonical), flat(out)


def same_csr(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("kind", list(GRAPHS))
def test_every_input_form_gives_the_same_graph(kind):
    n, edges = GRAPHS[kind]
    names = names_of(n)
    e2 = np.array(edges, np.int64).reshape(-1, 2)
    forms = [Graph.of((names, e2)), Graph.of((names, np.ascontiguousarray(e2.T))), Graph.of((tuple(names), [list(e) for e in edges])),
             Graph.of(Named(names, edges))]
    for g in forms:
        assert g.n == n and g.node_names == names and g.index == {name: k for k, name in enumerate(names)}
        assert g.edges.dtype == np.int64 and g.edges.shape == (len(edges), 2) and np.array_equal(g.edges, e2)
        assert Graph.of(g) is g


@pytest.mark.parametrize("kind", list(GRAPHS))
def test_csr_forms_equal_adjacency_lists(kind):
    n, edges = GRAPHS[kind]
    stable, canonical, out = expected(n, edges)
    g = Graph.of((names_of(n), edges))
    assert same_csr(g.csr(), stable) and same_csr(g.csr(canonical=False), stable)
    assert same_csr(g.csr(canonical=True), canonical)
    assert same_csr(g.out_csr(), out)
    assert g.csr(True) is g.csr(True) and g.csr(False) is g.csr(False) and g.out_csr() is g.out_csr()     # built once
    # the names the forms had before Graph existed are the same builders
    from hyptokenizer_amd.embedding.graph_embedding import sorted_symmetric_csr
    from hyptokenizer_amd.graph_paths import symmetric_csr
    assert same_csr(symmetric_csr(n, np.array(edges, np.int64).reshape(-1, 2)), stable)
    assert same_csr(sorted_symmetric_csr(n, np.array(edges, np.int64).reshape(-1, 2)), canonical)


def test_what_the_untidy_graph_is_there_for():
    n, edges = GRAPHS["untidy"]
    g = Graph.of((names_of(n), edges))
    row_ptr, col = g.csr(False)
    assert int(row_ptr[-1]) == 2 * len(edges) and col[row_ptr[2]:row_ptr[3]].tolist() == [2, 0, 2]       # the loop twice
    row_ptr, col = g.csr(True)
    assert int(row_ptr[-1]) == 8 and col[row_ptr[3]:row_ptr[4]].tolist() == [1, 4] and row_ptr[5] == row_ptr[6]


def test_edge_range_message_names_the_caller():
    with pytest.raises(ValueError, match=r"^somebody: an edge names a node outside \[0, 3\)$"):
        Graph.of((list("abc"), [[0, 3]]), "somebody")
    with pytest.raises(ValueError, match="^Graph: an edge"):
        Graph.of((list("abc"), [[-1, 0]]))
    with pytest.raises(ValueError):
        Graph.of(([], [[0, 0]]))
    assert Graph.of(([], [])).n == 0


def test_select():
    g = Graph.of((names_of(5), GRAPHS["path"][1]))
    for nodes in ([3, 0, 4], torch.tensor([3, 0, 4]), torch.tensor([3, 0, 4], dtype=torch.int32), np.array([3, 0, 4])):
        got = g.select(nodes, "t")
        assert got.dtype == np.int64 and got.tolist() == [3, 0, 4]
    for empty in ([], torch.zeros(0, dtype=torch.int64)):
        got = g.select(empty, "t")
        assert got.dtype == np.int64 and got.shape == (0,)
    with pytest.raises(ValueError, match=r"^t: nodes names a node outside \[0, 5\)$"):
        g.select([0, 5], "t")
    with pytest.raises(ValueError, match="outside"):
        g.select(torch.tensor([-1, 2]), "t")
    with pytest.raises(ValueError, match="^t: nodes must be free of repeats$"):
        g.select([2, 1, 2], "t")
    assert g.select([2, 1, 2], "t", unique=False).tolist() == [2, 1, 2]
    with pytest.raises(ValueError, match=r"^t: nodes names a row outside \[0, 2\)$"):
        select_nodes([2], 2, "t", what="row")


def test_from_named_edges_numbers_nodes_by_first_appearance():
    g = Graph.from_named_edges([("dog", "animal"), ("cat", "animal"), ("animal", "thing"), ("cat", "cat")])
    assert g.node_names == ["dog", "animal", "cat", "thing"] and g.index["thing"] == 3
    assert g.edges.tolist() == [[0, 1], [2, 1], [1, 3], [2, 2]]
    assert Graph.from_named_edges([]).n == 0
    from hyptokenizer_amd.scripts.train_graph_embeddings import EdgeListGraph
    assert EdgeListGraph([("b", "a")]).node_names == ["b", "a"]


def test_a_bad_graph_is_refused_before_the_device():
    from hyptokenizer_amd.embedding.graph_embedding import NegativeSampler
    from hyptokenizer_amd.engine import HypMergeUnavailable
    from hyptokenizer_amd.graph_paths import GraphPaths
    bad, good = (list("abc"), [[0, 3]]), (list("abc"), [[0, 1], [1, 2]])
    with pytest.raises(ValueError, match="^GraphPaths: an edge names a node outside"):
        GraphPaths(bad, device="cpu")
    with pytest.raises(ValueError, match="^NegativeSampler: an edge names a node outside"):
        NegativeSampler(bad, 4, device="cpu")
    with pytest.raises(HypMergeUnavailable):
        GraphPaths(good, device="cpu")
    with pytest.raises(HypMergeUnavailable):
        NegativeSampler(good, 4, device="cpu")
    with pytest.raises(HypMergeUnavailable):                    # a Graph is taken as it is
        GraphPaths(Graph.of(good), device="cpu")
