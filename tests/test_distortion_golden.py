"""Hierarchy-distortion checks that need no GPU: the pure-Python truth of hierarchy_cases.py reproduces every path length
and connectivity verdict the reference recorded, ``create_node_mapping`` and ``sample_node_pairs`` reproduce its mapping,
its pairs and its RNG state, and the ratios rebuilt from the oracle's canonical distances lie within the project's pinned
distance parity of the reference's."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

import hierarchy_cases as HC

# README "Numerical parity": distances are pinned to the reference's at <= 1e-5; a ratio is distance / g
DISTANCE_PARITY = 1e-5


def test_goldens_cover_the_required_cases(golden_dir):
    for mode in HC.MODES:
        cases = HC.load(golden_dir, mode)
        by = {c.name: c for c in cases}
        assert {by[f"tree_s{k}"].meta["distinct_sources"] for k in (1, 63, 64, 65, 130)} == {1, 63, 64, 65, 130}
        assert by["forest"].meta["retries"] > 0 and (by["forest"].tried[:, 2] < 0).any()
        assert by["path70"].tried[:, 2].max() > 40 and by["path70"].n == 70
        assert by["star100"].n == 101
        assert len({v for _, v in by["synsets"].mapping}) < len(by["synsets"].mapping) < by["synsets"].n
        assert all(c.n <= 300 and len(c.ratios) == c.num_pairs == len(c.accepted) for c in cases)


@pytest.mark.parametrize("mode", HC.MODES)
def test_truth_reproduces_every_recorded_path_length(golden_dir, mode):
    for case in HC.load(golden_dir, mode):
        t = HC.truth(case)
        a, b, want = case.tried.T
        assert t["rows"][a, b].tolist() == want.tolist(), case
        labels = np.array(t["labels"])
        assert ((labels[a] == labels[b]) == (want >= 0)).all(), case
        assert (np.array([min(np.nonzero(labels == lab)[0]) for lab in labels]) == labels).all()      # label = smallest member


@pytest.mark.parametrize("mode", HC.MODES)
def test_create_node_mapping_equals_the_reference(golden_dir, mode):
    from hyptokenizer_amd.scripts.eval_hierarchy import create_node_mapping
    for case in HC.load(golden_dir, mode):
        got = create_node_mapping(case.graph(), case.vocab)
        assert list(got.items()) == case.mapping, case


@pytest.mark.parametrize("mode", HC.MODES)
def test_sampler_reproduces_pairs_and_rng_state(golden_dir, mode):
    from hyptokenizer_amd.scripts.eval_hierarchy import sample_node_pairs, set_seeds
    for case in HC.load(golden_dir, mode):
        labels = dict(zip(case.nodes, HC.truth(case)["labels"]))
        set_seeds(case.seed)
        pairs = sample_node_pairs([k for k, _ in case.mapping], labels, case.num_pairs)
        assert [[case.index[a], case.index[b]] for a, b in pairs] == case.accepted[:, :2].tolist(), case
        assert HC.rng_hash() == case.meta["rng_hash"], case


def test_sampler_refuses_a_graph_without_a_connected_pair():
    from hyptokenizer_amd.scripts.eval_hierarchy import sample_node_pairs
    state = random.getstate()
    with pytest.raises(ValueError, match="no connected component"):
        sample_node_pairs(["a", "b", "c"], {"a": 0, "b": 1, "c": 2}, 5)
    with pytest.raises(ValueError):
        sample_node_pairs([], {}, 1)
    assert random.getstate() == state                      # refused before a single draw
    assert sample_node_pairs(["a", "b"], {"a": 0, "b": 1}, 0) == []


@pytest.mark.parametrize("mode", HC.MODES)
def test_ratios_from_canonical_distances_lie_within_the_pinned_parity(oracle, golden_dir, mode):
    for case in HC.load(golden_dir, mode):
        mapping = dict(case.mapping)
        acc = case.accepted
        i = [mapping[case.nodes[a]] for a in acc[:, 0]]
        j = [mapping[case.nodes[b]] for b in acc[:, 1]]
        d = oracle.distance(case.emb[i], case.emb[j], case.curvature, HC.SIGN_MODE[mode])
        g = acc[:, 2].astype(np.float64)
        ratios = d.astype(np.float64) / g
        err = np.abs(ratios - case.ratios) * g
        print(case.name, mode, "max |ratio - ref| * g =", err.max())
        assert err.max() <= DISTANCE_PARITY, case
        if mode == "reference":
            assert not case.ratios.any()                   # every distance of the reference as shipped is 0.0
        else:
            assert case.ratios.min() >= 0 and case.ratios.max() > 0
        for key, fn in (("mean", np.mean), ("median", np.median), ("min", np.min), ("max", np.max), ("std", np.std)):
            assert case.meta["stats"][key] == float(fn(case.ratios)), (case, key)
        assert case.meta["stats"]["num_pairs"] == case.num_pairs


def test_symmetric_csr_of_the_python_layer():
    from hyptokenizer_amd.graph_paths import symmetric_csr
    row_ptr, col = symmetric_csr(5, np.array([[0, 1], [3, 1], [1, 1], [0, 1]]))
    assert row_ptr.tolist() == [0, 2, 7, 7, 8, 8] and row_ptr.dtype == np.int64 and col.dtype == np.int32
    assert col[0:2].tolist() == [1, 1] and sorted(col[2:7].tolist()) == [0, 0, 1, 1, 3] and col[7] == 1      # the self-loop twice
    with pytest.raises(ValueError):
        symmetric_csr(3, np.array([[0, 3]]))
    row_ptr, col = symmetric_csr(2, np.zeros((0, 2), np.int64))
    assert row_ptr.tolist() == [0, 0, 0] and col.size == 0


def test_header_and_library_export_the_entry_points():
    from hyptokenizer_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "hypmerge.h")).read()
    L = _lib.load()
    for name in ("hm_graph_create", "hm_graph_destroy", "hm_graph_set_csr", "hm_graph_components", "hm_graph_pair_lengths",
                 "hm_graph_distance_rows", "hm_graph_last_stats"):
        assert f"int {name}(" in header
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name)
    assert L.hm_abi_version() == 3


def test_argument_errors_come_back_without_a_device():
    from hyptokenizer_amd import _lib
    from hyptokenizer_amd.engine import HypMergeUnavailable
    from hyptokenizer_amd.graph_paths import GraphPaths
    from hyptokenizer_amd.scripts import eval_hierarchy as EH
    L = _lib.load()
    E = _lib.HM_E_ARG
    p = C.c_void_p(64)                                     # never dereferenced: every call below fails on its handle
    assert L.hm_graph_create(None, 0) == E
    assert L.hm_graph_set_csr(None, p, p, 4, None) == E and L.hm_graph_components(None, p, None, None) == E
    assert L.hm_graph_pair_lengths(None, p, p, 1, p, None) == E and L.hm_graph_distance_rows(None, p, 1, None, 0, p, 4, None) == E
    assert L.hm_graph_last_stats(None, None, None, None, None) == E
    assert b"hm_graph" in L.hm_last_error(None)
    assert L.hm_debug_set_default_knob(b"graph_pass_words", -1.0, 0) == E
    assert L.hm_debug_set_default_knob(b"graph_chunk_levels", 0.0, 0) == E
    assert L.hm_debug_set_default_knob(b"graph_pass_words", 2.0, 0) == 0 and L.hm_debug_set_default_knob(b"graph_pass_words", 0.0, 1) == 0
    names, edges = ["a", "b", "c"], np.array([[0, 1]])
    with pytest.raises(HypMergeUnavailable):
        GraphPaths((names, edges), device="cpu")
    with pytest.raises(ValueError):
        GraphPaths(([], np.zeros((0, 2), np.int64)), device="cpu")
    emb = torch.zeros(3, 5)
    emb[:, 0] = 1
    with pytest.raises(HypMergeUnavailable):
        EH.compute_distortion(HC.Graph(names, edges), emb, {"a": 0, "b": 1}, num_pairs=2, device=torch.device("cpu"))
    with pytest.raises(HypMergeUnavailable):
        EH.compute_distortion_exhaustive(HC.Graph(names, edges), emb, {"a": 0, "b": 1}, device=torch.device("cpu"))
