"""Searches with more than 2^32 pairs in play and a known answer.

The engine takes tables of up to 131 072 rows (engine.MAX_ROWS): C(131 072, 2) = 8 589 869 056 pairs, and the benchmark's
V = 100 000 holds 4 999 950 000.  Two kinds of table make the answer analytic at those sizes:

* literal sign mode ("reference"): every pair sits at distance 0, so the candidates are all pairs of the row range, in
  row-major order (key = (bits(d), i, j));
* an origin cluster in "lorentz" mode: rows [0, m) are exactly (1, 0, ..., 0), so u = 1 and d = 0 exactly within the cluster,
  and every other fp32 distance is at least acosh(1 + 2^-23) ~ 4.9e-4.

count = sum_{i in [r0, r1)} (n - 1 - i) for the literal table (the cluster size m in place of n for the zero class).  The
row counts are chosen so that the count passes 2^32 by a small w: C(92 683, 2) = 2^32 + 55 607, rows [0, 62 525) of 99 955
rows and rows [0, 54 161) of 106 381 rows hold 2^32 + 4.  A histogram bin of 32 bits reads such a count as w, and a top-k
with k > w then skips the bin of the k-th smallest distance.  The closed form is itself checked against the oracle on small
tables first."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import bits  # noqa: E402
from hyptokenizer_amd.synthetic import lorentz_table  # noqa: E402

pytestmark = pytest.mark.gpu

D = 16                  # spatial dimension of the analytic tables (their answer does not depend on it)
THR_LIT = 0.1
W32 = 1 << 32


def pairs_in(n, r0, r1):
    """sum_{i in [r0, r1)} (n - 1 - i): the pairs (i, j), i < j < n, of rows [r0, r1)"""
    r1 = min(r1, n)
    return 0 if r1 <= r0 else sum(n - 1 - i for i in range(r0, r1))


def first_pairs(m, r0, r1, k):
    """the first k pairs (i, j), i < j < m, of rows [r0, r1) in row-major order"""
    I, J = [], []
    for i in range(r0, min(r1, m)):
        take = min(m - 1 - i, k - len(I))
        I.extend([i] * take)
        J.extend(range(i + 1, i + 1 + take))
        if len(I) >= k:
            break
    return np.asarray(I, np.int32), np.asarray(J, np.int32)


def test_expected_counts_by_hand():
    assert pairs_in(92683, 0, 92683) == W32 + 55607
    assert pairs_in(99955, 0, 62525) == W32 + 4
    assert pairs_in(106381, 0, 54161) == W32 + 4
    assert pairs_in(100000, 0, 100000) == 4999950000
    assert pairs_in(131072, 0, 131072) == 8589869056 < 2 * W32


def _literal_table(n, seed=5):
    return lorentz_table(n, D, seed=seed, scale=0.05)


def _origin_table(n, m, seed=6):
    X = torch.zeros((n, D + 1), dtype=torch.float32)
    X[:m, 0] = 1.0
    X[m:] = lorentz_table(n - m, D, seed=seed, scale=0.05)
    return X


def _engine(X, mode, exact, max_rows=None, prefilter="auto"):
    from hyptokenizer_amd import _lib
    from hyptokenizer_amd.engine import MergeEngine
    n = X.shape[0]
    rows = max_rows or n
    table = torch.zeros((rows, X.shape[1]), device="cuda")
    table[:n] = X.cuda()
    eng = MergeEngine(rows, X.shape[1], mode, prefilter=prefilter)
    if exact:
        _lib.check(_lib.load().hm_debug_set_knob(eng._h, b"exact_search", 1.0))
    eng.set_table(table, n)
    return eng, table


def _origin_count(oracle, Xn, m, thr, r0, r1):
    """candidates of rows [r0, r1) of an origin-cluster table: zero class + cluster x ordinary + the ordinary block (oracle);
    the oracle never runs over the cluster's pairs"""
    n = Xn.shape[0]
    thr32 = float(np.float32(thr))
    near = int((oracle.batch_distance(Xn[:1], Xn[m:], 1.0, 1)[0] < np.float32(thr32)).sum())
    cl_rows = max(0, min(r1, m) - r0)
    ob0 = max(r0, m)
    ob = oracle.pairwise_count(Xn, n, 1.0, thr32, 1, ob0, r1) if r1 > ob0 else 0
    return pairs_in(m, r0, min(r1, m)) + cl_rows * near + ob


# ---------------------------------------------------------------------------------------------------------------------
# the closed form against the oracle (small tables)
# ---------------------------------------------------------------------------------------------------------------------
def test_closed_form_equals_oracle_on_small_tables(oracle):
    n = 300
    Xn = _literal_table(n).numpy()
    for r0, r1, k in [(0, n, 500), (0, n, n * (n - 1) // 2), (37, 180, 1000), (250, n, 2000)]:
        od, oi, oj, oc = oracle.pairwise_topk(Xn, n, 1.0, THR_LIT, 0, k, r0, r1)
        ei, ej = first_pairs(n, r0, r1, k)
        assert oc == pairs_in(n, r0, r1), (r0, r1)
        assert np.array_equal(oi, ei) and np.array_equal(oj, ej) and not bits(od).any(), (r0, r1, k)
    m, n = 200, 300
    Xn = _origin_table(n, m).numpy()
    for thr in (1e-4, 0.5):
        for r0, r1, k in [(0, n, 3000), (50, 150, 500), (150, n, 100), (210, n, 100)]:
            od, oi, oj, oc = oracle.pairwise_topk(Xn, n, 1.0, float(np.float32(thr)), 1, k, r0, r1)
            assert oc == _origin_count(oracle, Xn, m, thr, r0, r1), (thr, r0, r1)
            if thr == 1e-4:
                assert oc == pairs_in(m, r0, min(r1, m))
            kz = min(k, pairs_in(m, r0, min(r1, m)))
            ei, ej = first_pairs(m, r0, r1, kz)
            assert np.array_equal(oi[:kz], ei) and np.array_equal(oj[:kz], ej) and not bits(od[:kz]).any(), (thr, r0, r1)
            assert (kz == len(od)) or bits(od[kz:]).all()


# ---------------------------------------------------------------------------------------------------------------------
# literal mode: every pair at distance 0
# ---------------------------------------------------------------------------------------------------------------------
LITERAL_CASES = [            # n, r0, r1, ks -- pairs in range minus 2^32 = w < k
    (92683, 0, 92683, (60000, 65536)),
    (99955, 0, 62525, (5, 7, 10000)),
    (106381, 0, 54161, (10000,)),
]


def _check_literal(eng, n, r0, r1, ks):
    want = pairs_in(n, r0, r1)
    for k in ks:
        ei, ej = first_pairs(n, r0, r1, k)
        gd, gi, gj, gc = eng.topk(1.0, THR_LIT, k, r0, r1)
        assert gc == want, (k, gc, want)
        assert np.array_equal(gi, ei) and np.array_equal(gj, ej) and not bits(gd).any(), k
    k = ks[-1]
    ei, ej = first_pairs(n, r0, r1, k)
    gd, gi, gj, gc = eng.topk(1.0, THR_LIT, k, r0, r1, count=False)
    assert gc in (-1, want) and np.array_equal(gi, ei) and np.array_equal(gj, ej) and not bits(gd).any()
    assert eng.argmin(1.0, THR_LIT, r0, r1) == (0.0, r0, r0 + 1)
    assert eng.count_candidates(1.0, THR_LIT) == pairs_in(n, 0, n)


@pytest.mark.parametrize("exact", [True, False], ids=["exact_path", "default_path"])
@pytest.mark.parametrize("n,r0,r1,ks", LITERAL_CASES, ids=[f"n{c[0]}_rows{c[1]}-{c[2]}" for c in LITERAL_CASES])
def test_literal_tie_flood_past_2_32(n, r0, r1, ks, exact):
    assert pairs_in(n, r0, r1) - W32 < min(ks[-1], 60000)
    eng, _ = _engine(_literal_table(n), "reference", exact)
    _check_literal(eng, n, r0, r1, ks)
    if exact and n == 92683:
        # the same lists from a second engine without the knob
        ref, _ = _engine(_literal_table(n), "reference", False)
        for k in ks:
            gd, gi, gj, gc = eng.topk(1.0, THR_LIT, k)
            rd, ri, rj, rc = ref.topk(1.0, THR_LIT, k)
            assert rc == gc and np.array_equal(ri, gi) and np.array_equal(rj, gj) and np.array_equal(bits(rd), bits(gd)), k
        ref.close()
    eng.close()


@pytest.mark.parametrize("n", [100000, 131072])
def test_literal_tie_flood_at_benchmark_size_and_max_rows(n):
    """the scan's tie-flood route with 4 999 950 000 and 8 589 869 056 tied pairs; candidate listing past the buffer"""
    eng, _ = _engine(_literal_table(n), "reference", False)
    assert eng.argmin(1.0, THR_LIT) == (0.0, 0, 1)
    _check_literal(eng, n, 0, n, (10000, 65536))
    for r0, r1, k in [(n - 5000, n, 10000), (n - 300, -1, 65536), (n // 2, n, 20)]:
        rr1 = n if r1 < 0 else r1
        want = pairs_in(n, r0, rr1)
        ei, ej = first_pairs(n, r0, rr1, k)
        gd, gi, gj, gc = eng.topk(1.0, THR_LIT, k, r0, r1)
        assert gc == want and np.array_equal(gi, ei) and np.array_equal(gj, ej) and not bits(gd).any(), (r0, r1)
        assert eng.argmin(1.0, THR_LIT, r0, r1) == (0.0, r0, r0 + 1)
    for r0, r1 in [(0, -1), (n - 5000, n), (n - 2, n)]:
        rr1 = n if r1 < 0 else r1
        ci, cj, cd, total = eng.candidates(1.0, THR_LIT, r0, r1, cap=1000)
        assert total == pairs_in(n, r0, rr1), (r0, r1, total)
        assert len(ci) == min(1000, total) and not bits(cd).any()
        assert np.all((ci >= r0) & (ci < rr1) & (ci < cj) & (cj < n))
        assert len(set(zip(ci.tolist(), cj.tolist()))) == len(ci)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# lorentz mode: a cluster of rows at the origin
# ---------------------------------------------------------------------------------------------------------------------
ORIGIN_CASES = [             # n, m, r0, r1, k
    (100000, 92683, 0, 100000, 65536),
    (100000, 99955, 0, 62525, 10000),
]


@pytest.mark.parametrize("exact", [True, False], ids=["exact_path", "default_path"])
@pytest.mark.parametrize("n,m,r0,r1,k", ORIGIN_CASES, ids=[f"m{c[1]}_rows{c[2]}-{c[3]}" for c in ORIGIN_CASES])
def test_origin_cluster_past_2_32(oracle, n, m, r0, r1, k, exact):
    X = _origin_table(n, m)
    Xn = X.numpy()
    eng, _ = _engine(X, "lorentz", exact)
    zc = pairs_in(m, r0, min(r1, m))
    assert zc - W32 < k <= zc
    ei, ej = first_pairs(m, r0, r1, k)
    for thr in (1e-4, 0.5):
        want = _origin_count(oracle, Xn, m, thr, r0, r1)
        if thr == 1e-4:
            assert want == zc
        gd, gi, gj, gc = eng.topk(1.0, thr, k, r0, r1)
        assert np.array_equal(gi, ei) and np.array_equal(gj, ej) and not bits(gd).any(), thr
        assert gc == want, (thr, gc, want)
        assert not bits(eng.pair_distance(gi, gj, 1.0)).any()
        assert eng.argmin(1.0, thr, r0, r1) == (0.0, r0, r0 + 1)
        assert eng.count_candidates(1.0, thr) == _origin_count(oracle, Xn, m, thr, 0, n)
    if not exact:
        ci, cj, cd, total = eng.candidates(1.0, 1e-4, r0, r1, cap=1000)
        assert total == zc and len(ci) == 1000 and not bits(cd).any()
        assert np.all((ci >= r0) & (ci < min(r1, m)) & (ci < cj) & (cj < m))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# max_rows itself against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_max_rows_table_equals_oracle(oracle):
    from hyptokenizer_amd import _lib
    from hyptokenizer_amd.engine import MAX_ROWS, MergeEngine
    n, d, thr, k = MAX_ROWS, 100, 0.5, 10000
    X = lorentz_table(n, d, seed=42, scale=0.05)
    Xo = X.numpy().copy()
    table = torch.zeros((n + 8, d + 1), device="cuda")        # room past max_rows: the row bound is the engine's to refuse
    table[:n] = X.cuda()
    eng = MergeEngine(n, d + 1, "lorentz", prefilter="bf16")

    def same_as_oracle(rows, forms=("bf16",)):
        od, oi, oj, oc = oracle.pairwise_topk(Xo, rows, 1.0, thr, 1, k, fast=True)
        assert oc > k
        for form in forms:
            eng.set_prefilter(form)
            a = eng.argmin(1.0, thr)
            assert a is not None and (a[1], a[2]) == (int(oi[0]), int(oj[0])) and bits([a[0]])[0] == bits(od)[0], form
            gd, gi, gj, gc = eng.topk(1.0, thr, k)
            assert gc == oc and np.array_equal(gi, oi) and np.array_equal(gj, oj) and np.array_equal(bits(gd), bits(od)), form
        eng.set_prefilter("bf16")
        r0 = rows - 72
        pd, pi, pj, pc = oracle.pairwise_topk(Xo, rows, 1.0, thr, 1, 500, r0, rows, fast=True)
        gd, gi, gj, gc = eng.topk(1.0, thr, 500, r0, rows)
        assert gc == pc and np.array_equal(gi, pi) and np.array_equal(gj, pj) and np.array_equal(bits(gd), bits(pd))
        return oi, oj

    eng.set_table(table, n)
    same_as_oracle(n, ("bf16", "f32"))
    eng.set_table(table, n - 1)
    oi, oj = same_as_oracle(n - 1)
    i, j = int(oi[0]), int(oj[0])
    eng.merge_append(i, j, 0.5, 1.0, table, n - 1)
    Xo[n - 1] = oracle.midpoint_batch(Xo, [i], [j], [np.float32(0.5)], 1.0, 1)[0]
    assert np.array_equal(table[n - 1].cpu().numpy().view(np.uint32), Xo[n - 1].view(np.uint32))
    assert eng.n == n
    same_as_oracle(n)
    before = table.clone()
    with pytest.raises(_lib.HypMergeError) as exc:
        eng.merge_append(i, j, 0.5, 1.0, table, n)
    assert exc.value.status == _lib.HM_E_ARG
    assert eng.n == n and torch.equal(table.view(torch.int32), before.view(torch.int32))
    a = eng.argmin(1.0, thr)
    od, oi, oj, oc = oracle.pairwise_topk(Xo, n, 1.0, thr, 1, 1, fast=True)
    assert (a[1], a[2]) == (int(oi[0]), int(oj[0])) and bits([a[0]])[0] == bits(od)[0]
    eng.close()
