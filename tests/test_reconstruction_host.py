"""Graph reconstruction, the part that needs no GPU: the entry points exist and refuse bad arguments before a device is
touched, the Python layer raises what it documents, and the truth of tests/reconstruction_cases.py agrees with its
restatement by sorting and with what the definitions say on inputs small enough to work out by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import graph_embedding_cases as GC
import reconstruction_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("hm_recon_slots", "hm_recon_counts", "hm_debug_recon_layout")


# ---- 1. the C ABI ------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_listed():
    from hyptokenizer_amd import _lib
    L = _lib.load()
    with open(os.path.join(ROOT, "include", "hypmerge.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name)
    assert L.hm_abi_version() == 3


def test_bad_arguments_are_refused_without_a_device():
    from hyptokenizer_amd import _lib
    L = _lib.load()
    E = _lib.HM_E_ARG
    P = C.c_void_p(4096)                                        # never dereferenced: every call below fails or has no slot
    big = 1 << 31

    def counts(x=P, ld=11, v=100, d1=11, anchor=P, pivot=P, seg=P, seg_ptr=P, slots=5, n_seg=2, la=P, ea=P, ln=P, en=P, u=P):
        return L.hm_recon_counts(x, ld, v, d1, anchor, pivot, seg, seg_ptr, slots, n_seg, la, ea, ln, en, u, None)

    for name in ("x", "anchor", "pivot", "seg", "seg_ptr", "la", "ea", "ln", "en", "u"):
        assert counts(**{name: None}) == E, name
    assert counts(d1=1) == E and counts(d1=130, ld=130) == E and counts(ld=10) == E
    assert counts(slots=-1) == E and counts(n_seg=-1) == E and counts(slots=big) == E
    assert counts(v=0) == E and counts(v=-1) == E and counts(v=big) == E
    assert counts(n_seg=0) == E                                 # slots without a segment
    assert b"hm_recon_counts" in L.hm_last_error(None)
    assert counts(slots=0) == _lib.HM_OK and counts(slots=0, n_seg=0, d1=2, ld=2) == _lib.HM_OK
    assert counts(slots=0, v=big - 1, d1=129, ld=200, anchor=None, la=None, u=None) == _lib.HM_OK

    def slots(row_ptr=P, col=P, v=100, nnz=7, nodes=None, n_seg=2, seg_ptr=P, n=5, a=P, p=P, s=P):
        return L.hm_recon_slots(row_ptr, col, v, nnz, nodes, n_seg, seg_ptr, n, a, p, s, None)

    for name in ("row_ptr", "col", "seg_ptr", "a", "p", "s"):
        assert slots(**{name: None}) == E, name
    assert slots(v=0) == E and slots(v=big) == E and slots(nnz=-1) == E and slots(n_seg=-1) == E and slots(n=-1) == E
    assert slots(n_seg=0) == E
    assert b"hm_recon_slots" in L.hm_last_error(None)
    assert slots(n=0) == _lib.HM_OK and slots(n=0, col=None, a=None, p=None, s=None, nnz=0) == _lib.HM_OK
    assert L.hm_debug_recon_layout(-1) == E and L.hm_debug_recon_layout(3) == E
    for layout in (1, 2, 0):
        assert L.hm_debug_recon_layout(layout) == _lib.HM_OK


# ---- 2. the Python layer -----------------------------------------------------------------------------------------------------
def test_python_layer_raises_what_it_documents():
    from hyptokenizer_amd.embedding import neighbor_rank_counts, reconstruction_metrics
    from hyptokenizer_amd.engine import HypMergeUnavailable
    n, edges = GC.tree_graph(15)
    x = torch.from_numpy(RC.table(n, 5))
    row_ptr, col = (torch.from_numpy(a) for a in RC.csr("tree", n))
    bad = [lambda: neighbor_rank_counts(x.double(), row_ptr, col),                   # a wrong dtype
           lambda: neighbor_rank_counts(torch.zeros(n, 1), row_ptr, col),             # a width outside 2..129
           lambda: neighbor_rank_counts(torch.zeros(n, 130), row_ptr, col),
           lambda: neighbor_rank_counts(torch.zeros(5, n).t(), row_ptr, col),         # no unit stride in the last dimension
           lambda: neighbor_rank_counts(x.reshape(-1), row_ptr, col),
           lambda: neighbor_rank_counts(x, row_ptr.int(), col),
           lambda: neighbor_rank_counts(x, row_ptr[:-1], col),
           lambda: neighbor_rank_counts(x, row_ptr, col.long()),
           lambda: neighbor_rank_counts(x, row_ptr, col, torch.tensor([0, 1], dtype=torch.int32)),
           lambda: neighbor_rank_counts(x, row_ptr, col, torch.tensor([0, n])),       # out of range
           lambda: neighbor_rank_counts(x, row_ptr, col, torch.tensor([-1, 2])),
           lambda: neighbor_rank_counts(x, row_ptr, col, torch.tensor([3, 1, 3])),    # a repeat
           lambda: reconstruction_metrics(x, (list(range(n)), edges), sign_convention="reference"),
           lambda: reconstruction_metrics(x[:-1], (list(range(n)), edges)),           # fewer rows than nodes, no mapping
           lambda: reconstruction_metrics(x, (list(range(n)), edges), node_mapping={k: 0 for k in range(n)}),
           lambda: reconstruction_metrics(x, (list(range(n)), edges), node_mapping={k: k for k in range(n - 1)}),
           lambda: reconstruction_metrics(x, (list(range(n)), edges), node_mapping={k: k + 1 for k in range(n)}),
           lambda: reconstruction_metrics(x, (list(range(n)), edges), nodes=[0, n]),
           lambda: reconstruction_metrics(x, (list(range(n)), edges), nodes=[2, 2]),
           lambda: reconstruction_metrics(x.double(), (list(range(n)), edges)),
           lambda: reconstruction_metrics(x, (list(range(n)), np.array([[0, n]])))]
    for k, fn in enumerate(bad):
        with pytest.raises(ValueError):
            fn()
            pytest.fail(f"case {k} raised nothing")
    with pytest.raises(HypMergeUnavailable):                    # valid arguments on the CPU: there is no fallback
        neighbor_rank_counts(x, row_ptr, col)
    with pytest.raises(HypMergeUnavailable):
        neighbor_rank_counts(x, row_ptr, col, torch.tensor([4, 0, 9]))
    with pytest.raises(HypMergeUnavailable):
        reconstruction_metrics(x, (list(range(n)), edges))
    with pytest.raises(HypMergeUnavailable):
        reconstruction_metrics(x, (list(range(n)), edges), node_mapping={k: n - 1 - k for k in range(n)}, nodes=[1, 0])


def test_cli_has_the_flag_off_by_default():
    import inspect
    from hyptokenizer_amd.scripts import train_graph_embeddings as T
    for fn in (T.main, T.train_graph_embeddings):
        assert inspect.signature(fn).parameters["eval_reconstruction"].default is False


# ---- 3. the truth itself -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", RC.KINDS)
def test_truth_equals_the_sort_restatement(oracle, kind):
    n, d1 = 41, 6
    x = GC.table(d1, seed=5, rows=n, scales=GC.WELL).numpy()
    dist = RC.distances(oracle, x)
    off = dist[~np.eye(n, dtype=bool)].reshape(n, n - 1)
    assert all(np.unique(r).size == n - 1 for r in off)        # no ties: the two forms must agree
    row_ptr, col = RC.csr(kind, n)
    t = RC.truth_counts(dist, row_ptr, col)
    ranks, precs = RC.sorted_ranks(dist, row_ptr, col)
    assert np.array_equal(1 + t["less_all"].astype(np.int64) - t["less_nb"], ranks)
    assert np.array_equal((t["less_nb"].astype(np.float64) + t["equal_nb"]) / (t["less_all"].astype(np.float64) + t["equal_all"]), precs)
    assert (t["equal_all"] == 1).all() and (t["equal_nb"] == 1).all()
    assert t["segments"].tolist() == row_ptr.tolist() and np.array_equal(t["pivots"], col)
    m = RC.metrics(t)
    assert m["num_pairs"] == col.size and m["num_nodes"] == int((np.diff(row_ptr) > 0).sum())
    assert m["mean_rank"] == ranks.sum() / ranks.size and 0.0 < m["map"] <= 1.0
    # a subset in another order: the slots of those nodes, in that order
    nodes = np.array([7, 0, n - 1, 3])
    sub = RC.truth_counts(dist, row_ptr, col, nodes)
    pick = np.concatenate([np.arange(row_ptr[u], row_ptr[u + 1]) for u in nodes]).astype(np.int64)
    for key in ("anchors", "pivots", "less_all", "equal_all", "less_nb", "equal_nb"):
        assert np.array_equal(sub[key], t[key][pick]), key


def test_a_path_along_a_geodesic_is_reconstructed_perfectly(oracle):
    n = 12
    x = RC.geodesic_path_table(n, 4)
    row_ptr, col = RC.csr("path", n)
    m = RC.metrics(RC.truth_counts(RC.distances(oracle, x), row_ptr, col))
    assert m == {"mean_rank": 1.0, "map": 1.0, "num_pairs": 2 * (n - 1), "num_nodes": n}


def test_duplicated_rows_give_the_documented_tie_counts(oracle):
    # rows 1 and 2 coincide, row 3 is far away; edges 0 - 1 and 1 - 3
    g = RC.geodesic_path_table(8, 3)
    x = np.stack([g[0], g[2], g[2], g[7]])
    row_ptr, col = RC.sorted_symmetric_csr(4, np.array([[0, 1], [1, 3]]))
    t = RC.truth_counts(RC.distances(oracle, x), row_ptr, col)
    assert t["anchors"].tolist() == [0, 1, 1, 3] and t["pivots"].tolist() == [1, 0, 3, 1]
    # (0, 1): rows 1 and 2 tie, nothing is closer.  (1, 0): the twin at distance 0 comes first.  (1, 3): the twin and row 0.
    # (3, 1): rows 1 and 2 tie again, row 0 is farther.
    assert t["less_all"].tolist() == [0, 1, 2, 0] and t["equal_all"].tolist() == [2, 1, 1, 2]
    assert t["less_nb"].tolist() == [0, 0, 1, 0] and t["equal_nb"].tolist() == [1, 1, 1, 1]
    m = RC.metrics(t)
    assert m["mean_rank"] == (1 + 2 + 2 + 1) / 4               # ties are counted in the neighbour's favour
    assert m["map"] == pytest.approx((0.5 + (0.5 + 2 / 3) / 2 + 0.5) / 3, rel=1e-15)
    # a NaN row: greater than every number as a bystander, equal to itself as a pivot
    x[2] = np.nan
    t = RC.truth_counts(RC.distances(oracle, x), *RC.sorted_symmetric_csr(4, np.array([[0, 1], [0, 2]])))
    assert t["anchors"].tolist() == [0, 0, 1, 2] and t["pivots"].tolist() == [1, 2, 0, 0]
    assert t["less_all"].tolist() == [0, 2, 0, 0] and t["equal_all"].tolist() == [1, 1, 1, 3]
    assert t["less_nb"].tolist() == [0, 1, 0, 0] and t["equal_nb"].tolist() == [1, 1, 1, 1]


def test_no_slots_means_nan():
    m = RC.metrics(RC.truth_counts(np.zeros((3, 3), np.float32), np.zeros(4, np.int64), np.zeros(0, np.int32)))
    assert np.isnan(m["mean_rank"]) and np.isnan(m["map"]) and m["num_pairs"] == 0 and m["num_nodes"] == 0


def test_float64_training_loop_reconstructs_the_tree(oracle):
    first, last = RC.e2e_tables_float64()
    assert np.array_equal(first, GC.e2e_init().numpy())
    # under float64 distances: the figures the feature was specified with
    before, after = RC.e2e_truth_metrics(oracle, first, float64=True), RC.e2e_truth_metrics(oracle, last, float64=True)
    print("float64 distances: before", repr(before), "after", repr(after))
    assert (before["mean_rank"], before["map"]) == pytest.approx(RC.E2E_RECON_FLOAT64[0], rel=1e-9)
    assert (after["mean_rank"], after["map"]) == pytest.approx(RC.E2E_RECON_FLOAT64[1], rel=1e-9)
    assert round(before["mean_rank"], 2) == 34.54 and round(before["map"], 4) == 0.0601
    assert round(after["mean_rank"], 3) == 1.048 and round(after["map"], 3) == 0.985
    assert before["num_pairs"] == after["num_pairs"] == 124 and after["num_nodes"] == 63
    # under the canonical fp32 distance (the truth): the initial table's near-coincident rows tie, the trained one is the same
    before, after = RC.e2e_truth_metrics(oracle, first), RC.e2e_truth_metrics(oracle, last)
    print("canonical fp32: before", repr(before), "after", repr(after))
    assert (before["mean_rank"], before["map"]) == pytest.approx(RC.E2E_RECON_TRUTH[0], rel=1e-9)
    assert (after["mean_rank"], after["map"]) == pytest.approx(RC.E2E_RECON_TRUTH[1], rel=1e-9)
    assert RC.E2E_RECON_TRUTH[1] == RC.E2E_RECON_FLOAT64[1] and before["mean_rank"] < RC.E2E_RECON_FLOAT64[0][0]
