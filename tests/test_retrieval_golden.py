"""Retrieval checks that need no GPU: the rank rule of retrieval_cases.py on the oracle's canonical distances reproduces the
reference's recorded recalls exactly, the C ABI exports the two entry points and refuses bad arguments without touching a
device, and the Python layer validates its arguments."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import retrieval_cases as RC

MODES = ("reference", "lorentz")


def _load(golden_dir, mode):
    meta = json.load(open(os.path.join(golden_dir, f"g12_retrieval_{mode}.json")))
    return meta, np.load(os.path.join(golden_dir, f"g12_retrieval_{mode}.npz"))


@pytest.mark.parametrize("mode", MODES)
def test_goldens_cover_the_required_shapes(golden_dir, mode):
    meta, z = _load(golden_dir, mode)
    cases = meta["cases"]
    assert {c["B"] for c in cases} >= {10, 12, 40, 200, 500}
    assert {c["d"] for c in cases} >= {1, 8, 64, 128}
    assert any(c["k_values"] == [1, 5, 10] for c in cases) and any(c["k_values"] != [1, 5, 10] for c in cases)
    assert any(c["ties"] for c in cases) or any(c["name"].endswith("ties") for c in meta["dropped"])
    for c in cases:
        assert z[f"{c['name']}__text"].shape == (c["B"], c["d"] + 1) == z[f"{c['name']}__image"].shape
        if mode == "lorentz":
            assert 0.0 < c["recall"]["r@1_text2image"] < 1.0 and 0.0 < c["recall"]["r@1_image2text"] < 1.0


@pytest.mark.parametrize("mode", MODES)
def test_rank_rule_on_canonical_distances_equals_the_reference(oracle, golden_dir, mode):
    meta, z = _load(golden_dir, mode)
    assert meta["cases"]
    for c in meta["cases"]:
        a, b = z[f"{c['name']}__text"], z[f"{c['name']}__image"]
        D = oracle.batch_distance(a, b, 1.0, RC.SIGN_MODE[mode])
        got = RC.recall_truth(D, c["k_values"])
        assert list(got.keys()) == list(c["recall"].keys()), c["name"]
        for key, want in c["recall"].items():
            assert got[key] == want, (c["name"], key, got[key], want)
        assert list(z[f"{c['name']}__recall"]) == list(c["recall"].values())
        if mode == "reference":                         # every distance is 0: rank i, recall min(k, B) / B
            assert not D.any()
            for k in c["k_values"]:
                assert got[f"r@{k}_text2image"] == min(k, c["B"]) / c["B"] == got[f"r@{k}_image2text"]


def test_truth_orders_nan_and_ties_by_index():
    nan = np.nan
    D = np.array([[1.0, 1.0, 0.5, nan],
                  [2.0, 2.0, 2.0, 2.0],
                  [nan, 0.0, nan, nan],
                  [3.0, nan, 1.0, 1.0]], np.float32)
    t2i, i2t = RC.ranks_truth(D)
    assert t2i.tolist() == [1, 1, 2, 1]                 # row 2: NaN diagonal, one number before it, NaN at j = 0 ties first
    assert i2t.tolist() == [0, 2, 3, 0]
    dist, idx = RC.knn_truth(D, 3)
    assert idx.tolist() == [[2, 0, 1], [0, 1, 2], [1, -1, -1], [2, 3, 0]]
    assert np.isinf(dist[2, 1:]).all() and dist[2, 0] == 0.0
    _, idx = RC.knn_truth(D, 2, exclude_self=True)
    assert idx.tolist() == [[2, 1], [0, 2], [1, -1], [2, 0]]


def test_header_and_library_export_the_entry_points():
    from hyptokenizer_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "hypmerge.h")).read()
    L = _lib.load()
    for name in ("hm_retrieval_ranks", "hm_knn", "hm_debug_retrieval_layout"):
        assert f"int {name}(" in header
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name)
    assert L.hm_abi_version() == 3


def test_argument_errors_come_back_without_a_device():
    from hyptokenizer_amd import _lib
    L = _lib.load()
    E = _lib.HM_E_ARG
    p = C.c_void_p(64)                                  # never dereferenced: every call below fails its argument check
    ranks = lambda zt=p, zi=p, n=8, ldt=9, ldi=9, d1=9, sign=1, r1=p, r2=p: L.hm_retrieval_ranks(zt, zi, n, ldt, ldi, d1, sign, r1, r2, None)  # noqa: E731
    assert ranks(zt=None) == E and ranks(zi=None) == E and ranks(r1=None, r2=None) == E
    assert ranks(n=0) == E and ranks(n=-3) == E and ranks(n=65537) == E
    assert ranks(d1=1, ldt=9) == E and ranks(d1=130, ldt=130, ldi=130) == E
    assert ranks(ldt=8) == E and ranks(ldi=8) == E and ranks(sign=2) == E
    assert b"hm_retrieval_ranks" in L.hm_last_error(None)
    knn = lambda q=p, nq=8, kk=p, nk=16, ldq=9, ldk=9, d1=9, c=1.0, sign=1, k=4, ex=0, d=p, i=p: L.hm_knn(q, nq, kk, nk, ldq, ldk, d1, c, sign, k, ex, d, i, None)  # noqa: E731
    assert knn(q=None) == E and knn(kk=None) == E and knn(d=None) == E and knn(i=None) == E
    assert knn(nq=0) == E and knn(nk=0) == E and knn(nq=(1 << 20) + 1) == E and knn(nk=(1 << 20) + 1) == E
    assert knn(d1=1) == E and knn(d1=130, ldq=130, ldk=130) == E and knn(ldq=8) == E and knn(ldk=8) == E
    assert knn(k=0) == E and knn(k=129, nk=1000) == E and knn(k=17) == E
    assert knn(c=0.0) == E and knn(c=float("nan")) == E and knn(sign=5) == E
    assert b"hm_knn" in L.hm_last_error(None)
    assert L.hm_debug_retrieval_layout(3) == E and L.hm_debug_retrieval_layout(-1) == E
    assert [L.hm_debug_retrieval_layout(v) for v in (1, 2, 0)] == [0, 0, 0]


def test_python_layer_validates_before_it_needs_a_device():
    from hyptokenizer_amd.engine import HypMergeUnavailable
    from hyptokenizer_amd.multimodal import compute_recall_at_k, hyperbolic_knn, retrieval_ranks
    from hyptokenizer_amd.multimodal import retrieval as R
    assert R.compute_recall_at_k is compute_recall_at_k
    x = torch.zeros(6, 5)
    x[:, 0] = 1
    with pytest.raises(ValueError, match="k = 7.*B = 6"):
        compute_recall_at_k(x, x, [1, 7])
    with pytest.raises(ValueError):
        compute_recall_at_k(x, x[:5])
    with pytest.raises(ValueError):
        retrieval_ranks(x, torch.zeros(6, 4))
    with pytest.raises(ValueError):
        retrieval_ranks(torch.zeros(6, 130), torch.zeros(6, 130))
    with pytest.raises(ValueError):
        retrieval_ranks(torch.zeros(0, 5), torch.zeros(0, 5))
    with pytest.raises(ValueError, match="128"):
        hyperbolic_knn(x, torch.zeros(200, 5), 129)
    with pytest.raises(ValueError, match="N = 6"):
        hyperbolic_knn(x, x, 7)
    with pytest.raises(ValueError):
        hyperbolic_knn(x, x, 0)
    with pytest.raises(ValueError):
        hyperbolic_knn(x, torch.zeros(6, 4), 1)
    with pytest.raises(ValueError):
        hyperbolic_knn(x, x, 1, c=0.0)
    y = torch.zeros(12, 5)
    y[:, 0] = 1
    for fn in (lambda: compute_recall_at_k(y, y), lambda: retrieval_ranks(x, x), lambda: hyperbolic_knn(x, y, 2),
               lambda: hyperbolic_knn(x, x, 2, exclude_self=True, sign_convention="reference")):
        with pytest.raises(HypMergeUnavailable):
            fn()
