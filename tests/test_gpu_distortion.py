"""Hierarchy distortion on the GPU: the graph kernels (components, pair lengths, distance rows) against the pure-Python
truth of hierarchy_cases.py as exact integers on every golden graph, and ``scripts/eval_hierarchy.py`` against the
reference's recorded runs and the oracle's canonical distances."""
import ctypes as C
import json
import os
import pickle
import random

import numpy as np
import pytest
import torch

import hierarchy_cases as HC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASE_NAMES = [c.name for c in HC.load(GOLDEN, "lorentz")]
GRAPH_NAMES = [n for n in CASE_NAMES if not n.startswith("tree_s") or n == "tree_s130"]     # the tree runs share one graph
DISTANCE_PARITY = 1e-5            # README "Numerical parity": distances within 1e-5 of the reference's


def _case(name, mode="lorentz"):
    return next(c for c in HC.load(GOLDEN, mode) if c.name == name)


def _paths(case):
    from hyptokenizer_amd.graph_paths import GraphPaths
    return GraphPaths(case.graph(), DEV)


def _check_kernels(case, gp):
    t = HC.truth(case)
    rows = t["rows"]
    labels = gp.components()
    assert labels.dtype == torch.int32 and labels.device.type == "cuda"
    assert labels.cpu().tolist() == t["labels"], case
    assert gp.n_components == len(set(t["labels"]))
    # every pair the reference tried (unreachable ones included), each node with itself, every tried pair a second time
    a = np.concatenate([case.tried[:, 0], np.arange(case.n), case.tried[:, 0]])
    b = np.concatenate([case.tried[:, 1], np.arange(case.n), case.tried[:, 1]])
    got = gp.path_lengths(torch.from_numpy(a), b.tolist())
    assert got.dtype == torch.int32 and got.cpu().tolist() == rows[a, b].tolist(), case
    assert got[len(case.tried):len(case.tried) + case.n].eq(0).all()
    # all sources against all nodes, then a column list with a repeated node and sources in another order
    full = gp.distance_rows(np.arange(case.n))
    assert full.dtype == torch.int16 and full.shape == (case.n, case.n)
    assert np.array_equal(full.cpu().numpy().astype(np.int64), rows), case
    src = [case.n - 1, 0, case.n // 2, 0]
    cols = list(range(0, case.n, 3)) + [1, 1]
    part = gp.distance_rows(src, torch.tensor(cols))
    assert np.array_equal(part.cpu().numpy().astype(np.int64), rows[np.ix_(src, cols)]), case
    return gp.last_stats()


@pytest.mark.parametrize("name", GRAPH_NAMES)
def test_graph_kernels_agree_with_the_truth(name):
    case = _case(name)
    gp = _paths(case)
    try:
        _check_kernels(case, gp)
        if name == "path70":
            assert HC.truth(case)["rows"].max() == 69               # deeper than one chunk of levels and than 64
        if name == "forest":
            assert (HC.truth(case)["rows"] < 0).any()
        assert gp.path_lengths([], []).numel() == 0 and gp.distance_rows([], None).shape == (0, case.n)
    finally:
        gp.close()


@pytest.mark.parametrize("name", ["tree_s130", "forest", "path70"])
def test_forced_multi_pass_runs_give_the_same_answers(name):
    """One word per node and pass (64 sources) and three levels per chunk: the tree's 130 distinct sources take three
    passes, its 300 rows five."""
    from hyptokenizer_amd import _lib
    L = _lib.load()
    case = _case(name)
    _lib.check(L.hm_debug_set_default_knob(b"graph_pass_words", 1.0, 0))
    _lib.check(L.hm_debug_set_default_knob(b"graph_chunk_levels", 3.0, 0))
    try:
        gp = _paths(case)
    finally:
        _lib.check(L.hm_debug_set_default_knob(b"graph_pass_words", 0.0, 1))
        _lib.check(L.hm_debug_set_default_knob(b"graph_chunk_levels", 0.0, 1))
    try:
        stats = _check_kernels(case, gp)
        assert stats["words"] == 1
        gp.distance_rows(np.arange(case.n))
        assert gp.last_stats()["passes"] == (case.n + 63) // 64
        acc = case.accepted
        gp.path_lengths(acc[:, 0], acc[:, 1])
        assert gp.last_stats()["passes"] == (case.meta["distinct_sources"] + 63) // 64
    finally:
        gp.close()


@pytest.mark.parametrize("mode", HC.MODES)
def test_compute_distortion_equals_reference_pairs_and_canonical_ratios(oracle, monkeypatch, mode):
    from hyptokenizer_amd.scripts import eval_hierarchy as EH
    seen = {}
    real = EH.sample_node_pairs

    def spy(valid_nodes, labels, num_pairs):
        seen["pairs"] = real(valid_nodes, labels, num_pairs)
        return seen["pairs"]

    monkeypatch.setattr(EH, "sample_node_pairs", spy)
    for case in HC.load(GOLDEN, mode):
        mapping = EH.create_node_mapping(case.graph(), case.vocab)
        assert list(mapping.items()) == case.mapping
        EH.set_seeds(case.seed)
        ratios, stats = EH.compute_distortion(case.graph(), torch.from_numpy(case.emb), mapping, num_pairs=case.num_pairs,
                                              curvature=case.curvature, device=DEV, sign_convention=mode)
        assert HC.rng_hash() == case.meta["rng_hash"], case
        acc = case.accepted
        assert [[case.index[a], case.index[b]] for a, b in seen["pairs"]] == acc[:, :2].tolist(), case
        i = [mapping[case.nodes[a]] for a in acc[:, 0]]
        j = [mapping[case.nodes[b]] for b in acc[:, 1]]
        g = acc[:, 2].astype(np.float64)
        want = oracle.distance(case.emb[i], case.emb[j], case.curvature, HC.SIGN_MODE[mode]).astype(np.float64) / g
        assert ratios.dtype == np.float64 and np.array_equal(ratios.view(np.uint64), want.view(np.uint64)), case
        assert stats == {"mean": float(np.mean(want)), "median": float(np.median(want)), "min": float(np.min(want)),
                         "max": float(np.max(want)), "std": float(np.std(want)), "num_pairs": case.num_pairs}
        assert list(stats.keys()) == list(case.meta["stats"].keys())
        err = np.abs(ratios - case.ratios) * g
        print(case.name, mode, "max |ratio - ref| * g =", err.max())
        assert err.max() <= DISTANCE_PARITY, case


@pytest.mark.parametrize("mode", HC.MODES)
def test_evaluate_hierarchy_writes_both_files(tmp_path, monkeypatch, mode):
    from hyptokenizer_amd.scripts import eval_hierarchy as EH
    case = _case("forest", mode)
    torch.save(torch.from_numpy(case.emb), tmp_path / "embeddings.pt")
    json.dump(case.vocab, open(tmp_path / "vocab.json", "w"))
    pickle.dump(case.graph(), open(tmp_path / "graph.gpk", "wb"))
    out = tmp_path / "sub" / "dir" / "distortion.npy"
    stats = EH.evaluate_hierarchy(str(tmp_path / "embeddings.pt"), str(tmp_path / "vocab.json"), str(tmp_path / "graph.gpk"), str(out),
                                  num_pairs=case.num_pairs, curvature=case.curvature, seed=case.seed, sign_convention=mode)
    ratios = np.load(out)
    assert np.abs(ratios - case.ratios).max() <= DISTANCE_PARITY and HC.rng_hash() == case.meta["rng_hash"]
    text = open(tmp_path / "sub" / "dir" / "distortion_stats.json").read()
    assert json.loads(text) == stats and text == json.dumps(stats, indent=4)
    assert stats["num_pairs"] == case.num_pairs and stats["mean"] == float(np.mean(ratios))
    monkeypatch.chdir(tmp_path)                             # a bare file name: no directory to make
    EH.main(embeddings_path="embeddings.pt", vocab_path="vocab.json", graph_path="graph.gpk", output_path="bare.npy",
            num_pairs=case.num_pairs, curvature=case.curvature, seed=case.seed, sign_convention=mode)
    assert np.array_equal(np.load(tmp_path / "bare.npy"), ratios) and json.load(open(tmp_path / "bare_stats.json")) == stats


@pytest.mark.parametrize("name,mode,batch", [("forest", "lorentz", 50), ("synsets", "lorentz", 1024), ("synsets", "reference", 64),
                                             ("star100", "lorentz", 33)])
def test_exhaustive_mode_equals_numpy_over_all_connected_pairs(name, mode, batch):
    from hyptokenizer_amd.embedding.lorentz_model import batch_distance
    from hyptokenizer_amd.scripts import eval_hierarchy as EH
    case = _case(name, mode)
    mapping = dict(case.mapping)
    got = EH.compute_distortion_exhaustive(case.graph(), torch.from_numpy(case.emb), mapping, curvature=case.curvature, device=DEV,
                                           source_batch=batch, sign_convention=mode)
    valid = [case.index[k] for k in mapping]
    rows = HC.truth(case)["rows"][np.ix_(valid, valid)]
    e = torch.from_numpy(case.emb[[mapping[k] for k in mapping]]).to(DEV)
    d = batch_distance(e, e, case.curvature, sign_convention=mode).cpu().numpy().astype(np.float64)
    iu = np.triu_indices(len(valid), 1)
    keep = rows[iu] > 0
    ratios = d[iu][keep] / rows[iu][keep].astype(np.float64)
    assert "median" not in got and list(got.keys()) == ["mean", "min", "max", "std", "num_pairs"]
    assert got["num_pairs"] == int(keep.sum()) > 0
    assert got["min"] == ratios.min() and got["max"] == ratios.max()
    print(name, mode, got, float(np.mean(ratios)), float(np.std(ratios)))
    assert got["mean"] == pytest.approx(float(np.mean(ratios)), rel=1e-10, abs=0)
    assert got["std"] == pytest.approx(float(np.std(ratios)), rel=1e-10, abs=0)


def test_a_level_beyond_int16_is_refused_only_where_a_listed_node_reaches_it():
    """A path of 33 000 nodes from its first node: node 32 767 is the last one an int16 row can hold."""
    from hyptokenizer_amd import _lib
    from hyptokenizer_amd.graph_paths import GraphPaths
    n = 33000
    gp = GraphPaths((range(n), np.stack([np.arange(n - 1), np.arange(1, n)], 1)), DEV)
    try:
        assert gp.distance_rows([0], [32767, 5, 0]).cpu().tolist() == [[32767, 5, 0]]      # nodes further out are not listed
        assert gp.last_stats()["levels"] == n
        with pytest.raises(_lib.HypMergeError) as exc:
            gp.distance_rows([0], [5, 32768])
        assert exc.value.status == _lib.HM_E_CAPACITY and "int16" in str(exc.value)
        assert gp.path_lengths([0, n - 1], [n - 1, 1]).cpu().tolist() == [n - 1, n - 2]      # int32: no such limit
    finally:
        gp.close()


def test_argument_errors():
    from hyptokenizer_amd import _lib
    from hyptokenizer_amd.engine import HypMergeUnavailable
    from hyptokenizer_amd.graph_paths import GraphPaths
    case = _case("cycles")
    with pytest.raises(HypMergeUnavailable):
        GraphPaths(case.graph(), torch.device("cpu"))
    gp = _paths(case)
    try:
        for call in (lambda: gp.path_lengths([0, case.n], [1, 2]), lambda: gp.path_lengths([0], [-1]),
                     lambda: gp.distance_rows([case.n]), lambda: gp.distance_rows([0], [0, case.n])):
            with pytest.raises(_lib.HypMergeError) as exc:
                call()
            assert exc.value.status == _lib.HM_E_ARG and "out of range" in str(exc.value)
        with pytest.raises(ValueError):
            gp.path_lengths([0, 1], [2])
        with pytest.raises(ValueError):
            gp.path_lengths([0.5], [1.0])
        row_ptr = np.zeros(4, np.int64)
        too_many = (1 << 24) + 1                             # refused before row_ptr is read
        assert gp._L.hm_graph_set_csr(gp._h, C.c_void_p(row_ptr.ctypes.data), None, too_many, None) == _lib.HM_E_ARG
        bad = np.array([0, 2, 1, 1], np.int64)
        assert gp._L.hm_graph_set_csr(gp._h, C.c_void_p(bad.ctypes.data), C.c_void_p(row_ptr.ctypes.data), 3, None) == _lib.HM_E_ARG
        col = np.array([0, 3], np.int32)
        ok_ptr = np.array([0, 1, 2, 2], np.int64)
        assert gp._L.hm_graph_set_csr(gp._h, C.c_void_p(ok_ptr.ctypes.data), C.c_void_p(col.ctypes.data), 3, None) == _lib.HM_E_ARG
        assert gp.path_lengths([0], [0]).tolist() == [0]     # the refused calls left the graph as it was
    finally:
        gp.close()
    with pytest.raises(ValueError):
        GraphPaths((["a", "b"], np.array([[0, 2]])), DEV)
