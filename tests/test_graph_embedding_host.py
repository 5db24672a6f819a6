"""Graph embedding, the part that needs no GPU: the truth of tests/graph_embedding_cases.py agrees with the closed form of
DESIGN.md 5.17, the sampler restatement has the properties the sampler is built for, the entry points exist and refuse bad
arguments before a device is touched, and the Python layer raises what it documents."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import graph_embedding_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("hm_edge_loss_fwd", "hm_edge_loss_bwd", "hm_debug_edge_loss_form", "hm_negsample_create", "hm_negsample_destroy", "hm_negsample_check_csr",
           "hm_negsample_set_csr", "hm_negsample_sample")


# ---- 1. the truth itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d1,b,k,c", [(2, 3, 1, 1.0), (5, 37, 5, 1.0), (17, 37, 50, 0.5), (66, 3, 5, 2.0), (129, 37, 1, 1.0)])
def test_autograd_gradient_of_the_truth_is_the_closed_form(d1, b, k, c):
    x, idx, g = GC.table(d1).double(), GC.index_case(b, k), GC.upstream(b).double()
    _, want = GC.evaluate(GC.table(d1), idx, c, GC.upstream(b), torch.float64)
    loss, a, ok, live = GC.loss_terms(x, idx, c)
    got = GC.closed_form_grad(x, idx, a, g).numpy()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # the anchor against itself and the masked slots carry no weight; a fully masked negative set leaves loss 0
    part = idx[:, 1:]
    assert bool((a[part == idx[:, :1]] == 0).all()) and bool((a[~live] == 0).all())
    alone = live.sum(1) == 1
    assert float(loss[alone].abs().max() if alone.any() else 0.0) < 1e-12


def test_loss_is_d0_plus_logsumexp_and_skips_what_it_documents():
    x = GC.table(5).double()
    idx = torch.tensor([[0, 1, 2, 3], [0, 1, -1, 3], [0, 1, GC.V, 3], [0, -1, 2, 3], [GC.V, 1, 2, 3]])
    loss, a, ok, live = GC.loss_terms(x, idx, 1.0)
    d = lambda i, j: float(torch.acosh(-GC.ldot(x[i], x[j])))  # noqa: E731
    want0 = d(0, 1) + np.log(sum(np.exp(-d(0, j)) for j in (1, 2, 3)))
    want1 = d(0, 1) + np.log(sum(np.exp(-d(0, j)) for j in (1, 3)))
    assert abs(float(loss[0]) - want0) < 1e-12 and abs(float(loss[1]) - want1) < 1e-12 and float(loss[2]) == float(loss[1])
    assert float(loss[3]) == 0.0 and float(loss[4]) == 0.0 and ok.tolist() == [True, True, True, False, False]
    assert GC.reduce(loss.numpy(), idx, GC.V, "mean") == loss.numpy().sum() / 3


def test_float64_training_loop_descends_epoch_by_epoch():
    before, after, history = GC.e2e_loop_float64()
    assert (before, after) == pytest.approx(GC.E2E_FLOAT64, rel=1e-9)
    steps = [before] + history
    assert all(b < a for a, b in zip(steps[:-1], steps[1:]))
    assert before - after > 2.0


# ---- 2. the sampler restatement --------------------------------------------------------------------------------------------
def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(w) for w in GC.philox4x32_10(ctr, key)) == want


@pytest.mark.parametrize("graph", ["path", "star", "complete"])
def test_sampler_restatement_properties(graph):
    n, edges = {"path": GC.path_graph, "star": GC.star_graph, "complete": GC.complete_graph}[graph](12)
    adj = GC.adjacency_sets(n, edges)
    pairs = np.array([(a, b) for a in range(n) for b in sorted(adj[a])], dtype=np.int64)
    out = GC.sample_reference(n, edges, pairs, 7, seed=11, step=4)
    assert out.shape == (len(pairs), 9) and np.array_equal(out[:, :2], pairs)
    neg = out[:, 2:]
    if graph == "complete":
        assert (neg == -1).all()
        return
    for row in out:
        for c in row[2:]:
            assert c == -1 or (0 <= c < n and c != row[0] and c not in adj[row[0]])
    if graph == "path":
        assert (neg >= 0).all()                                 # at most 3 of 12 nodes are refused: 32 tries always find one
    else:
        assert (neg[pairs[:, 0] == 0] == -1).all()              # the hub is adjacent to everything
    # row b depends only on (seed, b, step): any subset of the batch, in any order, gives the same rows
    perm = np.random.RandomState(0).permutation(len(pairs))[:9]
    again = GC.sample_reference(n, edges, pairs[perm], 7, seed=11, step=4, rows=perm)
    assert np.array_equal(again, out[perm])
    assert not np.array_equal(GC.sample_reference(n, edges, pairs, 7, seed=11, step=5), out)
    assert not np.array_equal(GC.sample_reference(n, edges, pairs, 7, seed=12, step=4), out)


def test_sorted_symmetric_csr():
    from hyptokenizer_amd.embedding.graph_embedding import sorted_symmetric_csr
    n, edges = GC.random_sparse_graph(50, seed=3)
    row_ptr, col = sorted_symmetric_csr(n, edges)
    adj = GC.adjacency_sets(n, edges)
    assert row_ptr[0] == 0 and row_ptr[-1] == col.size and col.dtype == np.int32 and row_ptr.dtype == np.int64
    for v in range(n):
        assert col[row_ptr[v]:row_ptr[v + 1]].tolist() == sorted(adj[v] - {v})
    assert row_ptr[n] == row_ptr[n - 1]                         # the isolated last node
    with pytest.raises(ValueError):
        sorted_symmetric_csr(3, np.array([[0, 3]]))
    row_ptr, col = sorted_symmetric_csr(1, np.zeros((0, 2), np.int64))
    assert row_ptr.tolist() == [0, 0] and col.size == 0


# ---- 3. the C ABI ------------------------------------------------------------------------------------------------------------
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
    P = C.c_void_p(4096)                                        # never dereferenced: every call below fails or has n == 0
    nan, inf = float("nan"), float("inf")

    def fwd(x=P, ld=11, v=100, d1=11, index=P, n=5, k=3, c=1.0, loss=P, w=P):
        return L.hm_edge_loss_fwd(x, ld, v, d1, index, n, k, c, loss, w, None)

    def bwd(x=P, ld=11, v=100, d1=11, index=P, n=5, k=3, c=1.0, w=P, g=P, val=P, coo=P):
        return L.hm_edge_loss_bwd(x, ld, v, d1, index, n, k, c, w, g, val, coo, None)

    for fn in (fwd, bwd):
        assert fn(x=None) == E and fn(index=None) == E and fn(w=None) == E
        assert fn(d1=1) == E and fn(d1=130, ld=130) == E and fn(ld=10) == E
        assert fn(n=-1) == E and fn(k=-1) == E and fn(v=-1) == E
        assert fn(c=0.0) == E and fn(c=-1.0) == E and fn(c=nan) == E and fn(c=inf) == E
        assert fn(n=0) == _lib.HM_OK and fn(n=0, d1=2, ld=2) == _lib.HM_OK and fn(n=0, d1=129, ld=200, k=0) == _lib.HM_OK
    assert fwd(loss=None) == E and bwd(g=None) == E and bwd(val=None) == E and bwd(coo=None) == E
    assert b"hm_edge_loss_bwd" in L.hm_last_error(None)
    assert L.hm_debug_edge_loss_form(-1) == E and L.hm_debug_edge_loss_form(2) == E and L.hm_debug_edge_loss_form(1) == _lib.HM_OK

    def csr(row_ptr, col, n=None):
        r, c = np.asarray(row_ptr, np.int64), np.asarray(col, np.int32)
        return L.hm_negsample_check_csr(C.c_void_p(r.ctypes.data), C.c_void_p(c.ctypes.data) if c.size else None, len(r) - 1 if n is None else n)

    assert csr([0, 1, 2], [1, 0]) == _lib.HM_OK and csr([0, 0], []) == _lib.HM_OK
    assert csr([0, 2, 3, 5], [1, 2, 0, 0, 1]) == _lib.HM_OK
    assert csr([0, 2, 3, 5], [2, 1, 0, 0, 1]) == E              # a row out of order
    assert csr([0, 2, 3, 5], [1, 1, 0, 0, 1]) == E              # a repeat
    assert csr([0, 1, 2], [2, 0]) == E and csr([0, 1, 2], [-1, 0]) == E
    assert csr([1, 1, 2], [1, 0]) == E and csr([0, 2, 1], [1, 0]) == E and csr([0], [], n=0) == E
    assert L.hm_negsample_check_csr(None, None, 1) == E
    assert L.hm_negsample_set_csr(None, P, P, 1, None) == E and L.hm_negsample_sample(None, P, 1, 1, 0, 0, 32, P, None) == E
    assert L.hm_negsample_destroy(None) == _lib.HM_OK
    assert L.hm_negsample_create(None, 0) == E


# ---- 4. the Python layer -----------------------------------------------------------------------------------------------------
def test_python_layer_raises_what_it_documents():
    from hyptokenizer_amd.embedding import NegativeSampler, edge_softmax_loss, fit_graph_embedding, graph_embedding
    from hyptokenizer_amd.engine import HypMergeUnavailable
    x, idx = GC.table(5), GC.index_case(3, 5)
    with pytest.raises(ValueError):
        edge_softmax_loss(x.double(), idx)                      # a wrong dtype
    with pytest.raises(ValueError):
        edge_softmax_loss(x, idx.int())
    with pytest.raises(ValueError):
        edge_softmax_loss(torch.zeros(4, 1), idx)               # a width outside 2..129
    with pytest.raises(ValueError):
        edge_softmax_loss(torch.zeros(4, 130), idx)
    with pytest.raises(ValueError):
        edge_softmax_loss(x, idx, sign_convention="reference")
    with pytest.raises(ValueError):
        edge_softmax_loss(x, idx[:, :1])                        # fewer than 2 columns
    with pytest.raises(ValueError):
        edge_softmax_loss(x, idx.reshape(-1))
    with pytest.raises(ValueError):
        edge_softmax_loss(x, idx, reduction="max")
    with pytest.raises(ValueError):
        edge_softmax_loss(x, idx, c=0.0)
    with pytest.raises(ValueError):
        edge_softmax_loss(torch.zeros(5, 8).t(), idx)           # no unit stride in the last dimension
    with pytest.raises(HypMergeUnavailable):
        edge_softmax_loss(x, idx)                               # valid arguments on the CPU: there is no fallback
    graph = (list("abc"), np.array([[0, 1], [1, 2]]))
    with pytest.raises(HypMergeUnavailable):
        NegativeSampler(graph, 4, device="cpu")
    with pytest.raises(ValueError):
        NegativeSampler(([], np.zeros((0, 2), np.int64)), 4, device="cpu")
    with pytest.raises(ValueError):
        NegativeSampler(graph, -1, device="cpu")
    with pytest.raises(ValueError):
        NegativeSampler(graph, 4, device="cpu", max_tries=0)
    with pytest.raises(ValueError):
        NegativeSampler((list("abc"), np.array([[0, 3]])), 4, device="cpu")
    with pytest.raises(ValueError):
        fit_graph_embedding(graph, 4, epochs=1, optimizer="adamw", device="cpu")
    with pytest.raises(ValueError):
        fit_graph_embedding(graph, 129, epochs=1, device="cpu")
    with pytest.raises(HypMergeUnavailable):
        fit_graph_embedding(graph, 4, epochs=1, device="cpu")
    t = graph_embedding.init_table(7, 4, 1e-3, 0, "cpu")
    assert t.shape == (7, 5) and float(t[:, 1:].abs().max()) <= 1e-3 and float((GC.ldot(t.double(), t.double()) + 1).abs().max()) < 1e-6
    assert torch.equal(graph_embedding.init_table(63, 5, 1e-3, 3, "cpu"), GC.e2e_init())
