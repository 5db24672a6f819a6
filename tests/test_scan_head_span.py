"""GPU: the head kernels' span (ScanRun of hm_scan_geom.h; knob `head_span`) changes no result.

With span 2 a head kernel computes two 64-column ring slots -- four 32-column groups, one pipeline -- between two barriers,
the tiles right of the block's rows in a straight-line body whose failed groups are recomputed behind the tile's last group.
Every case runs with `head_force = 1` over `head_span` 1 and 2 on rings 1 and 2 (four and five slots) and compares the argmin
record and the pair returned with the same engine under `head = 0` and with the oracle, bit for bit, the way
tests/test_scan_head_ring.py does; tables, oracle results and the `head = 0` searches are computed once and shared.

What the shapes are for.  n = 257 .. 1 100 give row-block runs of 1, 2, 3, 4, 5, 7, 8 and 9 slots: single-slot tiles, odd
endings, runs shorter than, as long as and longer than either ring, sizes that are no multiple of 32 or 64.  The planted
pairs take their columns from the decomposition itself (tests/scan_span_driver.cpp prints ScanRun's tiles, tests/scan_plan_driver.cpp
the item list), and the test asserts that they land where they are meant to."""
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_scan_head_ring import THR, _bits, _cache, _check, _engine, _loop, _search, _table, _want  # noqa: E402
from test_scan_plan import HEADER, Knobs, case_line  # noqa: E402
from test_scan_plan import driver as plan_driver  # noqa: E402,F401
from test_scan_span_host import build_span_driver, run_tiles  # noqa: E402

WALKS = [(2, 2), (1, 2), (2, 1), (1, 1)]           # (head_ring, head_span)
NBUF = {1: 4, 2: 5}                                # ring slots at d = 100 and d = 50 (ScanGeom; test_scan_span_host.py pins them)
SIZES = [257, 320, 385, 449, 513, 577, 700, 1100]


def _walk_knobs(ring, span, knobs=None):
    return dict(knobs or {}, head_force=1, head_ring=ring, head_span=span)


def _plain(key, X, knobs, **kw):
    """record and pair of the kernels without the head test: once per table and argument set"""
    ck = ("span_plain", key, tuple(sorted((knobs or {}).items())), tuple(sorted(kw.items())))
    if ck not in _cache:
        _cache[ck] = _search(X, dict(knobs or {}, head=0), **kw)[:2]
    return _cache[ck]


def _compare(oracle, key, X, ring, span, knobs=None, **kw):
    col_begin = kw.pop("col_begin", 0)
    knobs = dict(knobs or {})
    want = _want(oracle, key, X, col_begin=col_begin, **kw)
    if col_begin:
        # (the hook reaches the host search only: the record of the device search is the pair's)
        knobs["argmin_col_begin"] = col_begin
        for kn in (_walk_knobs(ring, span, knobs), dict(knobs, head=0)):
            eng, _ = _engine(X, kn)
            pair = eng.argmin(1.0, kw.get("thr", THR), kw.get("row_begin", 0), kw.get("row_end", -1))
            assert (None if pair is None else (int(_bits([pair[0]])[0]), pair[1], pair[2])) == want
        return None
    rec, pair, eng = _search(X, _walk_knobs(ring, span, knobs), **kw)
    rec0, pair0 = _plain(key, X, knobs, **kw)
    assert rec == rec0 and pair == pair0
    _check(rec, pair, want)
    return eng


@pytest.mark.parametrize("ring,span", WALKS)
@pytest.mark.parametrize("d", [100, 50])
@pytest.mark.parametrize("n", SIZES)
def test_sizes(oracle, n, d, ring, span):
    """a tight bound from the first tiles on (a near-duplicate of row 3 at row 9): most groups end after the head k-steps"""
    X = _table(n, d, near=[(3, 9), (n - 2, n - 1)])
    _compare(oracle, ("sizes", n, d), X, ring, span)


@pytest.mark.parametrize("ring,span", WALKS)
def test_row_and_column_ranges(oracle, ring, span):
    """rows [37, 613) cut the first and the last wave they touch; partners from column 197 on: the runs start on slot 3, an odd one"""
    n, d = 700, 100
    assert (197 // 64) % 2 == 1
    X = _table(n, d, near=[(40, 150), (100, 300), (650, 660)])
    _compare(oracle, ("rows", n, d), X, ring, span, row_begin=37, row_end=613)
    _compare(oracle, ("cols", n, d), X, ring, span, col_begin=197)
    _compare(oracle, ("both", n, d), X, ring, span, row_begin=37, row_end=613, col_begin=197)


@pytest.mark.parametrize("ring,span", WALKS)
@pytest.mark.parametrize("knobs", [{"dyn": 0}, {"dyn": 1, "dyn_slots": 3}, {"dyn": 1, "dyn_slots": 1}])
def test_item_queue_on_and_off(oracle, knobs, ring, span):
    """one block per item, and a resident grid of three blocks / of one block that draws every further item from the queue
    (the draw goes out in the run's last tile and is picked up behind that tile's wait)"""
    n, d = 1100, 100
    X = _table(n, d, near=[(700, 1000)])
    _compare(oracle, ("queue", n, d), X, ring, span, knobs)


# ---- planted pairs: where a failed group sits when it is recomputed ----
PLANT_N = 1190        # 19 slots of 64 columns: row block 0's last run is an odd one
PLACES = ["group0", "group1", "group2", "group3", "wrapped_second_slot", "odd_end", "run_first_slot"]


@pytest.fixture(scope="module")
def places(plan_driver, tmp_path_factory):  # noqa: F811
    """{place: column} of row block 0 (row 10 is in it) at PLANT_N rows, from the item list and ScanRun's tiles"""
    span_driver = build_span_driver(tmp_path_factory.mktemp("scan_span_gpu"))
    case = (Knobs(), PLANT_N, 0, -1, -1, 0, 1, 13)
    out = subprocess.run([plan_driver, "plan"], input=(case_line(case) + "\n").encode(), capture_output=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    words = np.frombuffer(out.stdout, np.int32).astype(np.int64)
    assert words[0] == 1 and words[5] == 0                  # a plan, 256-row blocks
    items = words[HEADER:HEADER + 3 * words[8]].reshape(-1, 3)
    nslot = (PLANT_N + 63) // 64
    # row block 0's runs in 64-column slots, as the kernel counts them: two per plan tile, clamped to the table
    runs = [(2 * int(c0), min(2 * int(c1), nslot)) for rb, c0, c1 in items if rb == 0 and 2 * c0 < min(2 * c1, nslot)]
    assert sum(b - a for a, b in runs) == nslot
    long_run = next((a, b) for a, b in runs if b - a >= 6 and a > 4)      # (right of the block's rows: interior tiles)
    odd_run = next((a, b) for a, b in runs if (b - a) % 2 == 1 and b - a >= 3)
    got = {}
    # the run's tile 1 on either ring: two slots, four groups
    for nbuf in NBUF.values():
        tiles = run_tiles(span_driver, long_run[1] - long_run[0], nbuf, 2)
        assert tiles[1][:2] == (2, 2)
    for g in range(4):
        got["group%d" % g] = (long_run[0] + 2) * 64 + 32 * g + 5
    # ring 2: tile 2 sits in ring slots 4 and 0
    tiles = run_tiles(span_driver, long_run[1] - long_run[0], NBUF[2], 2)
    assert tiles[2][:2] == (4, 2) and (tiles[2][0] % NBUF[2], (tiles[2][0] + 1) % NBUF[2]) == (4, 0)
    got["wrapped_second_slot"] = (long_run[0] + 5) * 64 + 40
    for nbuf in NBUF.values():
        tiles = run_tiles(span_driver, odd_run[1] - odd_run[0], nbuf, 2)
        assert tiles[-1][:2] == (odd_run[1] - odd_run[0] - 1, 1) and len(tiles) >= 2
    got["odd_end"] = (odd_run[1] - 1) * 64 + 3
    got["run_first_slot"] = long_run[0] * 64 + 33
    assert all(256 <= c < PLANT_N for c in got.values()) and got["odd_end"] >= (nslot - 1) * 64
    return got


@pytest.mark.parametrize("ring,span", WALKS)
@pytest.mark.parametrize("place", PLACES)
def test_failed_group_is_recomputed_from_its_slot(oracle, places, place, ring, span):
    """the table's nearest pair is (10, col), far below every other: its group fails the head test and is recomputed from the
    ring slot it sits in -- a recomputation that read another slot would miss the pair"""
    n, d, col = PLANT_N, 100, places[place]
    X = _table(n, d, near=[(10, col)])
    want = _want(oracle, ("span_planted", col), X)
    assert want is not None and want[1:] == (10, col)
    _compare(oracle, ("span_planted", col), X, ring, span)
    _compare(oracle, ("span_planted", col), X, ring, span, {"dyn": 1, "dyn_slots": 2})


@pytest.mark.parametrize("ring,span", WALKS)
def test_loose_bound_raises_head_bad(oracle, ring, span):
    """a threshold above every distance on a table without a close pair: every group fails in every position of the
    pipeline, the result is the oracle's, and the kernel tells the host that the bound is too loose for it"""
    from hyptokenizer_amd import _lib
    L = _lib.load()
    n, d = 513, 100
    X = _table(n, d)
    eng = _compare(oracle, ("loose", n, d), X, ring, span, thr=5.0)
    assert L.hm_debug_set_knob(eng._h, b"expect_head_bad", 1.0) == 0
    assert L.hm_debug_set_knob(eng._h, b"expect_head_bad", 0.0) != 0
    fresh, _ = _engine(X, _walk_knobs(ring, span))
    assert L.hm_debug_set_knob(fresh._h, b"expect_head_bad", 0.0) == 0


@pytest.mark.parametrize("ring,span", WALKS)
def test_standard_loop_twenty_steps(ring, span):
    """twenty steps of the standard loop at n = 2 000: merges and appended rows equal to the head = 0 loop"""
    n, d = 2000, 100
    X = _table(n, d, near=[(5, 1500)])
    if "loop0" not in _cache:
        _cache["loop0"] = _loop(X, THR, {"head": 0}, 20)
    want = _cache["loop0"]
    got = _loop(X, THR, _walk_knobs(ring, span), 20)
    assert got[2] == want[2] == 20
    assert got[0] == want[0] and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("ring,span", WALKS)
def test_long_runs_item_queue_and_phases(oracle, ring, span):
    """n = 23 100: runs of 32 slots (the running key is re-read in mid-run), four phases, more items than the device holds
    blocks (every block draws from the queue): one search against the oracle's fast form and twenty loop steps against the
    head = 0 loop"""
    n, d = 23100, 100
    X = _table(n, d, near=[(20000, 23000)])
    _want(oracle, ("long", n, d), X, fast=True)        # (the oracle's threaded search: 267 million pairs)
    _compare(oracle, ("long", n, d), X, ring, span)
    if "loop_long" not in _cache:
        _cache["loop_long"] = _loop(X, THR, {"head": 0}, 20)
    want = _cache["loop_long"]
    got = _loop(X, THR, _walk_knobs(ring, span), 20)
    assert got[2] == want[2] == 20
    assert got[0] == want[0] and np.array_equal(got[1], want[1])


def test_head_span_knob_values():
    from hyptokenizer_amd import _lib
    from hyptokenizer_amd.engine import MergeEngine
    L = _lib.load()
    eng = MergeEngine(256, 101, "lorentz", prefilter="bf16")
    for v, ok in ((1.0, True), (2.0, True), (0.0, False), (3.0, False), (-1.0, False), (1.5, False)):
        assert (L.hm_debug_set_knob(eng._h, b"head_span", v) == 0) == ok
