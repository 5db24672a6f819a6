"""Tables of more than 131 072 rows: the pair scan's wide argmin key.

An engine of max_rows rows packs (i, j) into the 32-bit low word of the scan's running key with ib = max(17, ceil(log2
max_rows)) row-index bits: (i << (32 - ib)) | (j >> (2 ib - 32)).  Up to engine.MAX_ROWS = 131 072 rows that is the narrow
(i << 15) | (j >> 2); a 131 137-row engine has ib = 18, a 2^20-row engine (engine.MAX_TABLE_ROWS) ib = 20, (i << 12) | (j >> 8):
256 partners j share one key bucket.  The tests:

* literal sign mode (every pair at distance 0, answer analytic) at 131 137 and 2^20 rows, whole table and row ranges;
* planted zero-distance ties inside one key bucket and across a bucket edge, a near pair at a non-zero distance, both
  prefilter forms, checked analytically and against the oracle on row ranges; the same through a world-1 RCCL exchange;
* full-table oracle parity at 131 137 rows and at 140 000 rows held in a 2^20-row engine;
* a narrow and a wide engine on one 131 000-row table give bit-identical merges (pipelined loop, incremental loop, fast
  tokenizer's top-k refresh); the wide one then goes on past row 131 072, its device loops equal to the host path.

The oracle only runs where it is cheap: row ranges cost (r1 - r0) * n pairs, full tables stay at or below 140 000 rows."""
import os
import socket
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import bits  # noqa: E402
from hyptokenizer_amd.synthetic import cjk_vocab, lorentz_table  # noqa: E402

pytestmark = pytest.mark.gpu

D = 16
THR_LIT = 0.1
WIDE = 1 << 20
NARROW = 131072


def pairs_in(n, r0, r1):
    """sum_{i in [r0, r1)} (n - 1 - i), closed form"""
    r1 = min(r1, n)
    if r1 <= r0:
        return 0
    cnt = r1 - r0
    return cnt * (n - 1) - (r0 + r1 - 1) * cnt // 2


def first_pairs(n, r0, r1, k):
    I, J = [], []
    for i in range(r0, min(r1, n)):
        take = min(n - 1 - i, k - len(I))
        I.extend([i] * take)
        J.extend(range(i + 1, i + 1 + take))
        if len(I) >= k:
            break
    return np.asarray(I, np.int32), np.asarray(J, np.int32)


def _engine(X, mode, max_rows, prefilter="auto", slack=8):
    from hyptokenizer_amd.engine import MergeEngine
    n = X.shape[0]
    table = torch.zeros((max(max_rows, n) + slack, X.shape[1]), device="cuda")
    table[:n] = X.cuda()
    eng = MergeEngine(max_rows, X.shape[1], mode, prefilter=prefilter)
    eng.set_table(table, n)
    return eng, table


def test_closed_forms():
    assert pairs_in(300, 37, 180) == sum(300 - 1 - i for i in range(37, 180))
    assert pairs_in(WIDE, 0, WIDE) == WIDE * (WIDE - 1) // 2


# ---------------------------------------------------------------------------------------------------------------------
# literal sign mode: every pair at distance 0
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [NARROW + 65, WIDE])
def test_literal_tie_flood_wide_key(n):
    from hyptokenizer_amd import _lib
    eng, table = _engine(lorentz_table(n, D, seed=5, scale=0.05), "reference", n)
    k = 1000
    assert eng.argmin(1.0, THR_LIT) == (0.0, 0, 1)
    gd, gi, gj, gc = eng.topk(1.0, THR_LIT, k)
    ei, ej = first_pairs(n, 0, n, k)
    assert gc == pairs_in(n, 0, n) and np.array_equal(gi, ei) and np.array_equal(gj, ej) and not bits(gd).any()
    assert eng.count_candidates(1.0, THR_LIT) == pairs_in(n, 0, n)
    starts = [131070, 131072] + ([900000] if n > 900000 else [])
    for r0 in starts:
        for r1 in (r0 + 3, -1):
            rr1 = n if r1 < 0 else r1
            ei, ej = first_pairs(n, r0, rr1, k)
            gd, gi, gj, gc = eng.topk(1.0, THR_LIT, k, r0, r1)
            assert gc == pairs_in(n, r0, rr1), (r0, r1, gc)
            assert np.array_equal(gi, ei) and np.array_equal(gj, ej) and not bits(gd).any(), (r0, r1)
            assert eng.argmin(1.0, THR_LIT, r0, r1) == (0.0, r0, r0 + 1), (r0, r1)
    if n == WIDE:
        # a full 2^20-row engine takes no further row
        before = table[n - 2:].clone()
        with pytest.raises(_lib.HypMergeError) as exc:
            eng.merge_append(0, 1, 0.5, 1.0, table, n)
        assert exc.value.status == _lib.HM_E_ARG
        assert eng.n == n and torch.equal(table[n - 2:].view(torch.int32), before.view(torch.int32))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# planted ties in lorentz mode, 2^20-row engine (key bucket = 256 partners)
# ---------------------------------------------------------------------------------------------------------------------
PI, PJ = 140000, 150016                      # 2^17 < PI < PJ, PJ a multiple of 256
NEAR_A, NEAR_B = 160000, 170001              # a near pair at a non-zero distance, both rows above 2^17
N_PLANT = 200000


def _planted_table(with_prev_bucket, near=False):
    """a spread table; rows PI, PJ, PJ + 1, PJ + 255 (one key bucket) and, when asked, PJ - 1 (the bucket before) are copies
    of one row p = 0.8 q, q on the hyperboloid far from the others: u(p, p) = 0.64 -- distance 0 among the copies only
    (u(p, y) ~ 0.8 * 3.2 > 1 for the spread rows y).  `near`: no copies; row NEAR_B is row NEAR_A moved by ~1e-4."""
    X = lorentz_table(N_PLANT, D, seed=11, scale=0.05)
    if near:
        s = X[NEAR_A, 1:].clone()
        s[0] += 1e-4
        X[NEAR_B, 1:] = s
        X[NEAR_B, 0] = torch.sqrt(1.0 + (s * s).sum())
        return X
    q = torch.zeros(D + 1)
    q[1] = 3.0
    q[0] = float(np.sqrt(10.0))
    p = 0.8 * q
    rows = [PI, PJ, PJ + 1, PJ + 255] + ([PJ - 1] if with_prev_bucket else [])
    for r in rows:
        X[r] = p
    return X, sorted(rows)


def _zero_pairs(rows):
    return [(a, b) for x, a in enumerate(rows) for b in rows[x + 1:]]


def _check_range_vs_oracle(oracle, eng, Xo, n, thr, r0, r1, k):
    od, oi, oj, oc = oracle.pairwise_topk(Xo, n, 1.0, thr, 1, k, r0, r1, fast=True)
    gd, gi, gj, gc = eng.topk(1.0, thr, k, r0, r1)
    assert gc == oc and np.array_equal(gi, oi) and np.array_equal(gj, oj) and np.array_equal(bits(gd), bits(od)), (r0, r1)
    a = eng.argmin(1.0, thr, r0, r1)
    if oc == 0:
        assert a is None
    else:
        assert (a[1], a[2]) == (int(oi[0]), int(oj[0])) and bits([a[0]])[0] == bits(od)[0], (r0, r1)


@pytest.mark.parametrize("prefilter", ["f32", "bf16"])
def test_planted_ties_in_one_key_bucket(oracle, prefilter):
    thr = 0.05
    for with_prev in (True, False):
        X, rows = _planted_table(with_prev)
        Xo = X.numpy()
        eng, _ = _engine(X, "lorentz", WIDE, prefilter=prefilter)
        want = (PI, PJ - 1) if with_prev else (PI, PJ)
        for _ in range(2):                                   # unseeded, then seeded by the first search
            assert eng.argmin(1.0, thr) == (0.0,) + want, (with_prev, prefilter)
        zp = _zero_pairs(rows)
        gd, gi, gj, gc = eng.topk(1.0, thr, len(zp))
        assert list(zip(gi.tolist(), gj.tolist())) == zp and not bits(gd).any()
        for r0, r1 in [(PI - 3, PI + 3), (PJ - 2, PJ + 2), (PJ + 200, PJ + 260)]:
            _check_range_vs_oracle(oracle, eng, Xo, N_PLANT, thr, r0, r1, 50)
        eng.close()


@pytest.mark.parametrize("prefilter", ["f32", "bf16"])
def test_near_pair_above_2_17(oracle, prefilter):
    thr = 0.05
    X = _planted_table(False, near=True)
    Xo = X.numpy()
    eng, _ = _engine(X, "lorentz", WIDE, prefilter=prefilter)
    od, oi, oj, oc = oracle.pairwise_topk(Xo, N_PLANT, 1.0, thr, 1, 5, NEAR_A, NEAR_A + 1, fast=True)
    assert (int(oi[0]), int(oj[0])) == (NEAR_A, NEAR_B) and bits(od)[0] != 0
    for _ in range(2):
        a = eng.argmin(1.0, thr)
        assert (a[1], a[2]) == (NEAR_A, NEAR_B) and bits([a[0]])[0] == bits(od)[0]
    gd, gi, gj, gc = eng.topk(1.0, thr, 1)
    assert (int(gi[0]), int(gj[0])) == (NEAR_A, NEAR_B) and bits(gd)[0] == bits(od)[0]
    for r0, r1 in [(NEAR_A - 4, NEAR_A + 4), (NEAR_B - 2, NEAR_B + 1)]:
        _check_range_vs_oracle(oracle, eng, Xo, N_PLANT, thr, r0, r1, 100)
    eng.close()


def test_world1_rccl_exchange_on_the_planted_table():
    import torch.distributed as dist
    X, rows = _planted_table(True)
    eng, _ = _engine(X, "lorentz", WIDE)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        eng.comm_init()
        assert eng.comm_info() == (0, 1)
        for thr in (0.05, 0.3):
            assert eng.global_argmin(1.0, thr) == eng.argmin(1.0, thr) == (0.0, PI, PJ - 1)
            gd, gi, gj, gc = eng.global_topk(1.0, thr, 300)
            hd, hi, hj, hc = eng.topk(1.0, thr, 300)
            assert gc == hc and np.array_equal(gi, hi) and np.array_equal(gj, hj) and np.array_equal(bits(gd), bits(hd))
            assert list(zip(gi[:10].tolist(), gj[:10].tolist())) == _zero_pairs(rows)
        eng.comm_destroy()
    finally:
        dist.destroy_process_group()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# full-table oracle parity
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,max_rows", [(NARROW + 65, NARROW + 65), (140000, WIDE)])
def test_full_table_equals_oracle(oracle, n, max_rows):
    thr, k = 0.12, 10000
    X = lorentz_table(n, D, seed=42, scale=0.05)
    Xo = X.numpy()
    od, oi, oj, oc = oracle.pairwise_topk(Xo, n, 1.0, thr, 1, k, fast=True)
    assert oc > k
    eng, _ = _engine(X, "lorentz", max_rows)
    for form in ("bf16", "f32"):
        eng.set_prefilter(form)
        a = eng.argmin(1.0, thr)
        assert (a[1], a[2]) == (int(oi[0]), int(oj[0])) and bits([a[0]])[0] == bits(od)[0], form
        gd, gi, gj, gc = eng.topk(1.0, thr, k)
        assert gc == oc and np.array_equal(gi, oi) and np.array_equal(gj, oj) and np.array_equal(bits(gd), bits(od)), form
        assert eng.count_candidates(1.0, thr) == oc
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# wide key against narrow key, then past row 131 072
# ---------------------------------------------------------------------------------------------------------------------
N0 = 131000
THR_M = 0.1


def _tok(cls, X, max_vocab, **kw):
    return cls(cjk_vocab(N0), torch.nn.Parameter(X.clone()), merge_threshold=THR_M, device=torch.device("cuda:0"),
               max_vocab_size=max_vocab, sign_convention="lorentz", **kw)


def _run(tok, steps):
    from hyptokenizer_amd.tokenizer.fast_hyperbolic_merge import FastHyperbolicTokenizer
    if isinstance(tok, FastHyperbolicTokenizer):
        tok.optimize_merges(steps=steps, log_every=10 ** 9, adaptive_threshold=False)
    else:
        tok.optimize_merges(steps=steps, log_every=10 ** 9)


@pytest.mark.parametrize("kind", ["std", "incremental", "fast"])
def test_wide_engine_equals_narrow_engine_then_crosses_2_17(oracle, kind):
    from hyptokenizer_amd.tokenizer.fast_hyperbolic_merge import FastHyperbolicTokenizer
    from hyptokenizer_amd.tokenizer.hyperbolic_merge import HyperbolicTokenizer
    X = lorentz_table(N0, D, seed=7, scale=0.05)
    cls = FastHyperbolicTokenizer if kind == "fast" else HyperbolicTokenizer
    kw = {"incremental": True} if kind == "incremental" else {}
    both = NARROW - N0
    narrow = _tok(cls, X, NARROW, **kw)
    wide = _tok(cls, X, 200_000, **kw)
    _run(narrow, both)
    _run(wide, both)
    assert narrow.current_vocab_size == wide.current_vocab_size == NARROW
    assert narrow.merge_history == wide.merge_history
    assert torch.equal(narrow.embeddings.data[:NARROW].view(torch.int32), wide.embeddings.data[:NARROW].view(torch.int32))
    narrow._engine.close()
    del narrow
    # on past row 131 072 (the rows merged there are checked against the host path and the oracle by the next test)
    more = 100
    _run(wide, more)
    assert wide.current_vocab_size == NARROW + more and len(wide.merge_history) == both + more
    assert wide.embeddings.data[NARROW:NARROW + more].abs().sum(dim=1).ne(0).all()       # (a NaN row counts as written)
    wide._engine.close()


def test_wide_device_loops_equal_host_path(oracle):
    from hyptokenizer_amd.engine import MergeEngine
    X = lorentz_table(N0, D, seed=8, scale=0.05)
    steps = NARROW - N0 + 120
    tables, engs = [], []
    for _ in range(3):
        t = torch.zeros((200_000, D + 1), device="cuda")
        t[:N0] = X.cuda()
        e = MergeEngine(200_000, D + 1, "lorentz")
        e.set_table(t, N0)
        e.set_token_lengths(np.ones(N0, np.int32))
        tables.append(t)
        engs.append(e)
    # host path: argmin + merge_append, weights from the token lengths
    lens = [1] * N0
    host = []
    for s in range(steps):
        n = N0 + s
        a = engs[0].argmin(1.0, THR_M)
        assert a is not None
        d, i, j = a
        w = float(np.float32(lens[j] / (lens[i] + lens[j])))
        engs[0].merge_append(i, j, w, 1.0, tables[0], n)
        lens.append(lens[i] + lens[j])
        host.append((i, j, bits([d])[0]))
    # device loops: the pipelined standard loop and the incremental loop; a step a loop hands back (found = 2: more
    # survivors than its tail takes) goes through the host path, as the tokenizers do it
    def device_run(e, t, kind):
        got, left = [], steps
        ol = [1] * N0
        best = e.argmin(1.0, THR_M) if kind == "incr" else None
        while left > 0:
            k = min(left, 64)
            if kind == "std":
                recs, done = e.std_merge_steps(1.0, THR_M, t, k)
            else:
                recs, done, best = e.incr_merge_steps(1.0, THR_M, t, k, best)
            for r in recs[:done]:
                got.append((r[2], r[3], bits([r[1]])[0]))
                ol.append(ol[r[2]] + ol[r[3]])
            left -= done
            if done < k:
                assert recs[done][0] == 2, recs[done]
                d, i, j = e.argmin(1.0, THR_M)
                e.merge_append(i, j, ol[j] / (ol[i] + ol[j]), 1.0, t, e.n)
                ol.append(ol[i] + ol[j])
                e.set_token_lengths(np.asarray(ol, np.int32))
                got.append((i, j, bits([d])[0]))
                left -= 1
                if kind == "incr":
                    best = e.argmin(1.0, THR_M)
        return got

    got_std = device_run(engs[1], tables[1], "std")
    got_inc = device_run(engs[2], tables[2], "incr")
    assert got_std == host and got_inc == host
    n1 = N0 + steps
    for t in tables[1:]:
        assert torch.equal(t[:n1].view(torch.int32), tables[0][:n1].view(torch.int32))
    T = tables[0][:n1].cpu().numpy()
    for s in (0, NARROW - N0, steps - 1):
        i, j, db = host[s]
        od, oi, oj, oc = oracle.pairwise_topk(T, N0 + s, 1.0, THR_M, 1, 1, i, i + 1, fast=True)
        assert (int(oi[0]), int(oj[0])) == (i, j) and bits(od)[0] == db, s
    for e in engs:
        e.close()
