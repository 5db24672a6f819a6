"""GPU: the head kernels' partner-tile ring (hm_scan_geom.h kScanRings; knob `head_ring`) changes no result.

The head kernels of the argmin scan stream the partner rows through 64-column ring slots, three or four of them in flight
(rings 1 and 2), where every other kernel keeps one 128-column tile in flight.  Every case here runs with `head_force = 1`,
so the head kernel runs whatever the bound, once per ring, and compares the argmin record (found, distance bits, i, j) and
the pair returned with the same engine under `head = 0` (the kernels without the test, ring 0) and with the oracle.

What the shapes are for.  A ring of DIST + 1 slots walks a run of column tiles; the prologue, the counted waits at the
run's end and the slot a failed group is recomputed from all depend on how the run's length compares with DIST (3 and 4
here).  n = 257 .. 1 100 give some row block runs of 1, 2, DIST, DIST + 1 and DIST + 2 slots at both depths, sizes that
are no multiple of 32 or 64, two to five row blocks and the diagonal tile.  d = 100 is 13 chunks (13 KiB per slot: the
waves' shares are 4/3/3/3 pieces), d = 50 is 8 chunks (9 pieces: 3/2/2/2), the narrowest width with a head test."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hyptokenizer_amd.synthetic import lorentz_table  # noqa: E402

RINGS = [2, 1, 0]
SIZES = [257, 320, 385, 449, 513, 700, 1100]
THR = 0.6
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _reproject(X):
    X[:, 0] = np.sqrt(np.float32(1.0) + (X[:, 1:].astype(np.float32) ** 2).sum(axis=1, dtype=np.float32)).astype(np.float32)
    return X


def _table(n, d, near=()):
    """a random table; `near`: (src, dst) rows, dst becomes a near-duplicate of src (each a little farther than the one before)"""
    X = lorentz_table(n, d, seed=500 + d + n, scale=0.05).numpy().copy()
    rs = np.random.RandomState(n + d)
    for k, (src, dst) in enumerate(near):
        X[dst] = X[src]
        X[dst, 1:] += (rs.randn(d) * 0.0004 * (k + 1)).astype(np.float32)
    return _reproject(X) if near else X


def _engine(X, knobs, extra=64):
    from hyptokenizer_amd import _lib
    from hyptokenizer_amd.engine import MergeEngine
    L = _lib.load()
    n, d1 = X.shape
    table = torch.zeros((n + extra, d1), dtype=torch.float32, device="cuda")
    table[:n] = torch.from_numpy(X).cuda()
    eng = MergeEngine(n + extra, d1, "lorentz", prefilter="bf16")
    for k, v in knobs.items():
        _lib.check(L.hm_debug_set_knob(eng._h, k.encode(), float(v)))
    eng.set_table(table, n)
    return eng, table


def _search(X, knobs, thr=THR, row_begin=0, row_end=-1):
    """(record, pair) of one search on a fresh engine: the device record of argmin_into and what argmin returns"""
    eng, _ = _engine(X, knobs)
    pair = eng.argmin(1.0, thr, row_begin, row_end)
    eng2, _ = _engine(X, knobs)
    rec = torch.zeros(4, dtype=torch.int32, device="cuda")
    eng2.argmin_into(1.0, thr, row_begin, row_end, rec)
    torch.cuda.synchronize()
    return tuple(int(v) & 0xffffffff for v in rec.cpu().numpy()), pair, eng


def _want(oracle, key, X, thr=THR, row_begin=0, row_end=-1, col_begin=0, fast=False):
    """the oracle's nearest pair (bits, i, j) or None, computed once per table (the tests share and never change it)"""
    if key not in _cache:
        n = X.shape[0]
        k = 1 if col_begin == 0 else n * (n - 1) // 2
        od, oi, oj, oc = oracle.pairwise_topk(X, n, 1.0, float(np.float32(thr)), 1, k, row_begin, row_end, fast=fast)
        keep = np.nonzero(np.asarray(oj) >= col_begin)[0]
        _cache[key] = None if len(keep) == 0 else (int(_bits(od[keep[:1]])[0]), int(oi[keep[0]]), int(oj[keep[0]]))
    return _cache[key]


def _check(rec, pair, want):
    if want is None:
        assert rec[0] == 0 and pair is None
    else:
        assert rec == (1,) + want
        assert pair is not None and (int(_bits([pair[0]])[0]), pair[1], pair[2]) == want


def _compare(oracle, key, X, ring, knobs=None, **kw):
    knobs = dict(knobs or {})
    col_begin = kw.pop("col_begin", 0)
    if col_begin:
        knobs["argmin_col_begin"] = col_begin
    want = _want(oracle, key, X, col_begin=col_begin, **kw)
    if col_begin:
        # (the hook reaches the host search only: the record of the device search is the pair's)
        for kn in (dict(knobs, head_force=1, head_ring=ring), dict(knobs, head=0)):
            eng, _ = _engine(X, kn)
            pair = eng.argmin(1.0, kw.get("thr", THR), kw.get("row_begin", 0), kw.get("row_end", -1))
            got = None if pair is None else (int(_bits([pair[0]])[0]), pair[1], pair[2])
            assert got == want
        return None
    rec, pair, eng = _search(X, dict(knobs, head_force=1, head_ring=ring), **kw)
    rec0, pair0, _ = _search(X, dict(knobs, head=0), **kw)
    assert rec == rec0 and pair == pair0
    _check(rec, pair, want)
    return eng


@pytest.mark.parametrize("ring", RINGS)
@pytest.mark.parametrize("d", [100, 50])
@pytest.mark.parametrize("n", SIZES)
def test_sizes(oracle, n, d, ring):
    """a tight bound from the first tiles on (a near-duplicate of row 3 at row 9): most groups end after the head k-steps"""
    X = _table(n, d, near=[(3, 9), (n - 2, n - 1)])
    _compare(oracle, ("sizes", n, d), X, ring)


@pytest.mark.parametrize("ring", RINGS)
@pytest.mark.parametrize("d", [100, 50])
def test_row_and_column_ranges(oracle, d, ring):
    """rows [37, 613) cut the first and the last wave they touch; partners from column 197 on: no multiple of a slot"""
    n = 700
    X = _table(n, d, near=[(40, 150), (100, 300), (650, 660)])
    _compare(oracle, ("rows", n, d), X, ring, row_begin=37, row_end=613)
    _compare(oracle, ("cols", n, d), X, ring, col_begin=197)
    _compare(oracle, ("both", n, d), X, ring, row_begin=37, row_end=613, col_begin=197)


@pytest.mark.parametrize("ring", RINGS)
@pytest.mark.parametrize("knobs", [{"dyn": 0}, {"dyn": 1, "dyn_slots": 3}, {"dyn": 1, "dyn_slots": 1}])
def test_item_queue_on_and_off(oracle, knobs, ring):
    """one block per item, and a resident grid of three blocks / of one block that draws every further item from the queue
    (the draw is picked up behind the run's last wait)"""
    n, d = 1100, 100
    X = _table(n, d, near=[(700, 1000)])
    _compare(oracle, ("queue", n, d), X, ring, knobs)


# columns of row block 0's runs at n = 1 100 (runs of 8, 8 and 2 slots of 64 columns): the first slot of a run, the ring's
# last slot at either depth (the 4th and the 5th tile of a run), the last slot of a full run, and both slots of the short one
PLANTED = [517, 709, 773, 965, 1029, 1093]


@pytest.mark.parametrize("ring", RINGS)
@pytest.mark.parametrize("col", PLANTED)
def test_failed_group_is_recomputed_from_its_slot(oracle, col, ring):
    """the table's nearest pair is (10, col), far below every other: its group fails the head test and is recomputed from the
    ring slot it sits in -- a recomputation that read another slot would miss the pair"""
    n, d = 1100, 100
    X = _table(n, d, near=[(10, col)])
    want = _want(oracle, ("planted", col), X)
    assert want is not None and want[1:] == (10, col)
    _compare(oracle, ("planted", col), X, ring)
    _compare(oracle, ("planted", col), X, ring, {"dyn": 1, "dyn_slots": 2})


@pytest.mark.parametrize("ring", RINGS)
def test_loose_bound_raises_head_bad(oracle, ring):
    """a threshold above every distance on a table without a close pair: most groups are recomputed, the result is the
    oracle's, and the kernel tells the host that the bound is too loose for it"""
    from hyptokenizer_amd import _lib
    L = _lib.load()
    n, d = 513, 100
    X = _table(n, d)
    eng = _compare(oracle, ("loose", n, d), X, ring, thr=5.0)
    assert L.hm_debug_set_knob(eng._h, b"expect_head_bad", 1.0) == 0
    assert L.hm_debug_set_knob(eng._h, b"expect_head_bad", 0.0) != 0
    fresh, _ = _engine(X, {"head_force": 1, "head_ring": ring})
    assert L.hm_debug_set_knob(fresh._h, b"expect_head_bad", 0.0) == 0


def _loop(X, thr, knobs, steps):
    n = X.shape[0]
    eng, table = _engine(X, knobs, extra=steps + 8)
    eng.set_token_lengths((np.arange(1, n + 1, dtype=np.int32) % 5 + 1).astype(np.int32))
    recs, done = eng.std_merge_steps(1.0, thr, table, steps)
    return recs[:done], table[n:n + done].cpu().numpy().view(np.uint32).copy(), done


@pytest.mark.parametrize("ring", RINGS)
def test_standard_loop_twenty_steps(ring):
    """twenty steps of the standard loop at n = 2 000: merges and appended rows equal to the head = 0 loop"""
    n, d = 2000, 100
    X = _table(n, d, near=[(5, 1500)])
    if "loop0" not in _cache:
        _cache["loop0"] = _loop(X, THR, {"head": 0}, 20)
    want = _cache["loop0"]
    got = _loop(X, THR, {"head_force": 1, "head_ring": ring}, 20)
    assert got[2] == want[2] == 20
    assert got[0] == want[0] and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("ring", RINGS)
def test_long_runs_item_queue_and_phases(oracle, ring):
    """n = 23 100 is the smallest table whose runs are 32 ring tiles long (the running key is re-read in mid-run and picked
    up DIST - 1 tiles later), whose item list has four phases and more items than the device holds blocks (every block
    draws from the queue): one search against the oracle and twenty loop steps against the head = 0 loop"""
    n, d = 23100, 100
    X = _table(n, d, near=[(20000, 23000)])
    _want(oracle, ("long", n, d), X, fast=True)        # (the oracle's threaded search: 267 million pairs)
    _compare(oracle, ("long", n, d), X, ring)
    if "loop_long" not in _cache:
        _cache["loop_long"] = _loop(X, THR, {"head": 0}, 20)
    want = _cache["loop_long"]
    got = _loop(X, THR, {"head_force": 1, "head_ring": ring}, 20)
    assert got[2] == want[2] == 20
    assert got[0] == want[0] and np.array_equal(got[1], want[1])


def test_head_ring_knob_values():
    from hyptokenizer_amd import _lib
    from hyptokenizer_amd.engine import MergeEngine
    L = _lib.load()
    eng = MergeEngine(256, 101, "lorentz", prefilter="bf16")
    for v, ok in ((0.0, True), (1.0, True), (2.0, True), (3.0, False), (-1.0, False), (1.5, False)):
        assert (L.hm_debug_set_knob(eng._h, b"head_ring", v) == 0) == ok
