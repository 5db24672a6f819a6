"""GPU: the head kernels' three-blocks-per-CU ring (ring 3 of kScanRings, hm_scan_geom.h; knobs `head_blocks = 3`,
`head_span = 2`) changes no result.

Ring 3 keeps four 64-column slots of the tile's own size and nothing behind them but the queue word, so that three blocks
share a CU; its kernels are built for three waves per SIMD.  The knob `head_ring` keeps naming rings 0 .. 2 (its accepted
values are pinned by tests/test_scan_head_ring.py); ring 3 is chosen by `head_blocks = 3`.  Every case runs with
`head_force = 1, head_blocks = 3, head_span = 2` and compares the argmin record and the pair returned with the same
engine under `head = 0` and with the oracle, bit for bit, the way tests/test_scan_head_ring.py and tests/test_scan_head_span.py do; tables, oracle results and
the `head = 0` searches are computed once and shared.

What the shapes are for.  n = 257 .. 1 100 give row-block runs of 1 .. 9 slots: shorter than, as long as and longer than
the ring's four, with odd ends and sizes that are no multiple of 32 or 64; d = 100 is 13 chunks (the waves' shares of a slot
are 4/3/3/3 pieces), d = 50 is 8 chunks (3/2/2/2).  The planted pairs take their columns from the decomposition itself
(tests/scan_ring3_driver.cpp prints ScanRun's tiles, tests/scan_plan_driver.cpp the item list).  The last group of ring slot
3 in a diagonal tile is the place whose "next group" fragment request used to land behind the ring."""
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from test_scan_head_ring import THR, _bits, _cache, _check, _engine, _loop, _search, _table, _want  # noqa: E402
from test_scan_plan import HEADER, Knobs, case_line  # noqa: E402
from test_scan_plan import driver as plan_driver  # noqa: E402,F401
from test_scan_ring3_host import _tiles  # noqa: E402
from test_scan_ring3_host import driver as ring3_driver  # noqa: E402,F401

BLOCKS, SPAN, NBUF = 3, 2, 4
SIZES = [257, 320, 385, 449, 513, 577, 700, 1100]


def _walk_knobs(knobs=None):
    return dict(knobs or {}, head_force=1, head_blocks=BLOCKS, head_span=SPAN)


def _plain(key, X, knobs, **kw):
    """record and pair of the kernels without the head test: once per table and argument set"""
    ck = ("ring3_plain", key, tuple(sorted((knobs or {}).items())), tuple(sorted(kw.items())))
    if ck not in _cache:
        _cache[ck] = _search(X, dict(knobs or {}, head=0), **kw)[:2]
    return _cache[ck]


def _compare(oracle, key, X, knobs=None, **kw):
    col_begin = kw.pop("col_begin", 0)
    knobs = dict(knobs or {})
    want = _want(oracle, key, X, col_begin=col_begin, **kw)
    if col_begin:
        # (the hook reaches the host search only: the record of the device search is the pair's)
        knobs["argmin_col_begin"] = col_begin
        for kn in (_walk_knobs(knobs), dict(knobs, head=0)):
            eng, _ = _engine(X, kn)
            pair = eng.argmin(1.0, kw.get("thr", THR), kw.get("row_begin", 0), kw.get("row_end", -1))
            assert (None if pair is None else (int(_bits([pair[0]])[0]), pair[1], pair[2])) == want
        return None
    rec, pair, eng = _search(X, _walk_knobs(knobs), **kw)
    rec0, pair0 = _plain(key, X, knobs, **kw)
    assert rec == rec0 and pair == pair0
    _check(rec, pair, want)
    return eng


def test_head_blocks_knob_values():
    """`head_blocks` takes 2 and 3; `head_ring` still takes the two-block rings 0 .. 2 only"""
    from hyptokenizer_amd import _lib
    from hyptokenizer_amd.engine import MergeEngine
    L = _lib.load()
    eng = MergeEngine(256, 101, "lorentz", prefilter="bf16")
    for v, ok in ((3.0, True), (2.0, True), (4.0, False), (1.0, False), (0.0, False), (2.5, False)):
        assert (L.hm_debug_set_knob(eng._h, b"head_blocks", v) == 0) == ok
    for v, ok in ((2.0, True), (3.0, False), (4.0, False)):
        assert (L.hm_debug_set_knob(eng._h, b"head_ring", v) == 0) == ok


@pytest.mark.parametrize("d", [100, 50])
@pytest.mark.parametrize("n", SIZES)
def test_sizes(oracle, n, d):
    """a tight bound from the first tiles on (a near-duplicate of row 3 at row 9): most groups end after the head k-steps"""
    X = _table(n, d, near=[(3, 9), (n - 2, n - 1)])
    _compare(oracle, ("sizes", n, d), X)


def test_row_and_column_ranges(oracle):
    """rows [37, 613) cut the first and the last wave they touch; partners from column 197 on: the runs start on slot 3, an odd one"""
    n, d = 700, 100
    assert (197 // 64) % 2 == 1
    X = _table(n, d, near=[(40, 150), (100, 300), (650, 660)])
    _compare(oracle, ("rows", n, d), X, row_begin=37, row_end=613)
    _compare(oracle, ("cols", n, d), X, col_begin=197)
    _compare(oracle, ("both", n, d), X, row_begin=37, row_end=613, col_begin=197)


@pytest.mark.parametrize("knobs", [{"dyn": 0}, {"dyn": 1, "dyn_slots": 3}, {"dyn": 1, "dyn_slots": 1}])
def test_item_queue_on_and_off(oracle, knobs):
    """one block per item, and a resident grid of three blocks / of one block that draws every further item from the queue
    (the draw goes out in the run's last tile and is picked up behind that tile's wait)"""
    n, d = 1100, 100
    X = _table(n, d, near=[(700, 1000)])
    _compare(oracle, ("queue", n, d), X, knobs)


# ---- planted pairs: where a failed group sits when it is recomputed ----
PLANT_N = 1190        # 19 slots of 64 columns: row block 0's last run is an odd one
PLACES = ["group0", "group1", "group2", "group3", "run_first_slot", "odd_end", "diagonal_ring_slot3_last_group"]


@pytest.fixture(scope="module")
def places(plan_driver, ring3_driver):  # noqa: F811
    """{place: column} of row block 0 (row 10 is in it) at PLANT_N rows, from the item list and ScanRun's tiles"""
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
    diag_run = next((a, b) for a, b in runs if a == 0)
    got = {}
    # the long run's tile 1: two slots, four groups, all right of the block's 256 rows
    tiles = _tiles(ring3_driver, long_run[1] - long_run[0], NBUF, SPAN)
    assert tiles[1][:2] == (2, 2)
    for g in range(4):
        got["group%d" % g] = (long_run[0] + 2) * 64 + 32 * g + 5
    got["run_first_slot"] = long_run[0] * 64 + 33
    tiles = _tiles(ring3_driver, odd_run[1] - odd_run[0], NBUF, SPAN)
    assert tiles[-1][:2] == (odd_run[1] - odd_run[0] - 1, 1) and len(tiles) >= 2
    got["odd_end"] = (odd_run[1] - 1) * 64 + 3
    # the run that starts at column 0: its slot 3 sits in ring slot 3, the ring's last, in tile 1 (slots 2 and 3, columns
    # 128 .. 255: left of the block's last row, so the tile is walked slot by slot); the slot's last group is columns 224 .. 255
    assert diag_run[1] - diag_run[0] >= 4
    tiles = _tiles(ring3_driver, diag_run[1] - diag_run[0], NBUF, SPAN)
    assert tiles[1][:2] == (2, 2) and (tiles[1][0] + 1) % NBUF == NBUF - 1
    got["diagonal_ring_slot3_last_group"] = 3 * 64 + 32 + 21
    assert got["diagonal_ring_slot3_last_group"] < 256
    assert all(10 < c < PLANT_N for c in got.values()) and got["odd_end"] >= (nslot - 1) * 64
    return got


@pytest.mark.parametrize("place", PLACES)
def test_failed_group_is_recomputed_from_its_slot(oracle, places, place):
    """the table's nearest pair is (10, col), far below every other: its group fails the head test and is recomputed from the
    ring slot it sits in -- a recomputation that read another slot would miss the pair"""
    n, d, col = PLANT_N, 100, places[place]
    X = _table(n, d, near=[(10, col)])
    want = _want(oracle, ("ring3_planted", col), X)
    assert want is not None and want[1:] == (10, col)
    _compare(oracle, ("ring3_planted", col), X)
    _compare(oracle, ("ring3_planted", col), X, {"dyn": 1, "dyn_slots": 2})


def test_loose_bound_raises_head_bad(oracle):
    """a threshold above every distance on a table without a close pair: every group fails in every position of the
    pipeline, the result is the oracle's, and the kernel tells the host that the bound is too loose for it"""
    from hyptokenizer_amd import _lib
    L = _lib.load()
    n, d = 513, 100
    X = _table(n, d)
    eng = _compare(oracle, ("loose", n, d), X, thr=5.0)
    assert L.hm_debug_set_knob(eng._h, b"expect_head_bad", 1.0) == 0
    assert L.hm_debug_set_knob(eng._h, b"expect_head_bad", 0.0) != 0
    fresh, _ = _engine(X, _walk_knobs())
    assert L.hm_debug_set_knob(fresh._h, b"expect_head_bad", 0.0) == 0


@pytest.mark.parametrize("pipeline", [1, 0])
def test_standard_loop_twenty_four_steps(pipeline):
    """24 steps of the standard loop at n = 1 500, pipelined (the tail and the row pass beside the next scan, whose three
    blocks per CU leave them 4 KiB of LDS) and sequential: merges and appended rows equal to the head = 0 loop"""
    n, d = 1500, 100
    X = _table(n, d, near=[(5, 1200)])
    base = {"pipeline_pairs": 0, "pipeline": pipeline}
    key = ("ring3_loop0", pipeline)
    if key not in _cache:
        _cache[key] = _loop(X, THR, dict(base, head=0), 24)
    want = _cache[key]
    got = _loop(X, THR, _walk_knobs(base), 24)
    assert got[2] == want[2] == 24
    assert got[0] == want[0] and np.array_equal(got[1], want[1])
