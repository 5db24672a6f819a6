"""The pair scan's host policy (hm_scan_plan and hm_scan_item, hyptokenizer_amd/csrc/hm_scan_plan.h; ScanGeom, the block
shapes and the width list, hm_scan_geom.h) without a GPU: a stand-alone C++ program (tests/scan_plan_driver.cpp)
runs the plan and decodes every item of its list.  What it prints is compared

* with a Python transcription of hm_prepare_scan and of the kernel's item decode as they stood in hm_scan.hip before the lift
  (commit 62f69de), branch for branch: every field of the plan and every decoded (rb, ct0, ct1), exactly;
* with the definition of the list, sharing nothing with the transcription: every row block of the row range appears, the
  clamped tile ranges of a row block's items tile [diagonal or col_begin, nct) exactly once and in order, and the grid is the
  sum of the phases' items;
* ScanGeom::lds_bytes with the sum hm_launch_scan_t computed before the lift, for every instantiation and mode."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PHASES = 6
HEADER = 10 + 5 * PHASES


# ------------------------------------------------------------------------------------------------
# the transcription: hm_prepare_scan, the kernel's decode and hm_launch_scan_t's LDS sum of the parent commit (62f69de)
# ------------------------------------------------------------------------------------------------
def cdiv(a, b):
    """C's integer division: truncated towards zero."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


class Knobs:
    def __init__(self, **kw):
        self.chunk_f32, self.chunk_bf16, self.tail_div, self.tail_fraction, self.phases = 32, 128, 4, 0.20, 4
        self.ph_share, self.ph_div = [0.70, 0.15, 0.10, 0.0, 0.0], [1, 2, 4, 8, 16, 32]
        self.force_shape, self.big_min_rows = -1, 80000
        if "chunk" in kw:                  # the knob `chunk` sets both
            self.chunk_f32 = self.chunk_bf16 = kw.pop("chunk")
        for name, v in kw.items():
            assert hasattr(self, name)
            setattr(self, name, v)


def pairs_in_range(n, r0, r1):
    cnt = r1 - r0
    return cnt * (n - 1) - cdiv((r0 + r1 - 1) * cnt, 2)


SHAPE_ROWS = [256, 512, 512, 1024, 384]        # kShapeRows of hm_prepare_scan
SUB_BF16, SUB_F32, DIST_BF16, HIST_BINS, MODE_HIST = 4, 2, 1, 256, 2


def prepare_scan(e, n_table, row_begin, row_end, n_limit, col_begin, bf16, KC):
    """hm_prepare_scan: None when the row range is empty, else the fields it leaves in ScanArgs and the grid."""
    n = n_limit if 0 <= n_limit < n_table else n_table
    if row_end < 0 or row_end > n:
        row_end = n
    if row_begin < 0:
        row_begin = 0
    if row_end > n - 1:
        row_end = n - 1
    if row_begin >= row_end:
        return None
    a = {}
    shape = 1 if (bf16 and KC <= 14 and pairs_in_range(n, row_begin, row_end) >= cdiv(e.big_min_rows * (e.big_min_rows - 1), 2)) else 0
    if bf16 and KC <= 14 and e.force_shape >= 0:
        shape = e.force_shape
    block_rows = SHAPE_ROWS[shape] if bf16 else 256
    cols = 32 * (SUB_BF16 if bf16 else SUB_F32)
    a["n"], a["row_begin"], a["row_end"], a["shape"] = n, row_begin, row_end, shape
    rb_first = cdiv(row_begin, block_rows)
    nct = cdiv(n + cols - 1, cols)
    a["rb_first"], a["nct"] = rb_first, nct
    rb_last = cdiv(row_end - 1, block_rows)
    nrb = rb_last - rb_first + 1
    tiles_per_rb = max(1, cdiv(block_rows, cols))
    ch = cdiv((e.chunk_bf16 if bf16 else e.chunk_f32) * 64, cols)
    if ch < 1:
        ch = 1
    while ch > 4 and nrb * cdiv(nct + ch - 1, ch) < 1024:
        ch >>= 1
    a["col_begin"] = max(col_begin, 0)
    ct_lo = cdiv(a["col_begin"], cols)
    nph = 1
    share = [1.0] + [0.0] * (PHASES - 1)
    div = [1] * PHASES
    if ch >= 8 and nrb >= 16:
        if e.phases <= 2:
            nph = 2
            share[0] = 1.0 - e.tail_fraction
            share[1] = e.tail_fraction
            div[1] = e.tail_div
        else:
            nph = min(e.phases, PHASES)
            rest = 1.0
            for q in range(nph - 1):
                share[q] = e.ph_share[q]
                rest -= share[q]
            share[nph - 1] = max(rest, 0.0)
            for q in range(nph):
                div[q] = e.ph_div[q]
    total = 0.0
    for rb in range(rb_first, rb_last + 1):
        total += float(max(0, nct - rb * tiles_per_rb))
    a["n_ph"] = nph
    ph = {name: [0] * PHASES for name in ("items", "rb0", "chunks", "ch", "ctmin")}
    rb_at, n_items = rb_first, 0
    acc, want = 0.0, 0.0
    for q in range(nph):
        want += share[q] * total
        rb_end = rb_at
        if q == nph - 1:
            rb_end = rb_last + 1
        else:
            while rb_end <= rb_last and acc < want:
                acc += float(max(0, nct - rb_end * tiles_per_rb))
                rb_end += 1
        chq = max(1, cdiv(ch, max(1, div[q])))
        ph["rb0"][q] = rb_at
        ph["ch"][q] = chq
        ph["ctmin"][q] = max(cdiv(rb_at * block_rows, cols), ct_lo)
        ph["chunks"][q] = max(1, cdiv(nct - ph["ctmin"][q] + chq - 1, chq))
        ph["items"][q] = (rb_end - rb_at) * ph["chunks"][q]
        n_items += ph["items"][q]
        rb_at = rb_end
    a.update(ph)
    a["grid"] = max(1, n_items)
    a["block_rows"], a["cols"] = block_rows, cols        # (the kernel's BLOCK_ROWS and COLS of the instantiation launched)
    return a


def decode_item(a, item):
    """hm_scan.hip:637-647: the item's row block and clamped run of column tiles."""
    it, ph = item, 0
    while ph + 1 < a["n_ph"] and it >= a["items"][ph]:
        it -= a["items"][ph]
        ph += 1
    rb = a["rb0"][ph] + cdiv(it, a["chunks"][ph])
    ct0 = a["ctmin"][ph] + (it - cdiv(it, a["chunks"][ph]) * a["chunks"][ph]) * a["ch"][ph]
    ct1 = ct0 + a["ch"][ph]
    if ct0 < cdiv(rb * a["block_rows"], a["cols"]):
        ct0 = cdiv(rb * a["block_rows"], a["cols"])
    if ct0 < cdiv(a["col_begin"], a["cols"]):
        ct0 = cdiv(a["col_begin"], a["cols"])
    if ct1 > a["nct"]:
        ct1 = a["nct"]
    return rb, ct0, ct1


def decode_all(a):
    """decode_item for items 0 .. grid - 1 at once: the while loop sends item b to the phase whose run of the list holds it
    (the last phase takes whatever lies behind); everything is non-negative, so C's division is numpy's."""
    item = np.arange(a["grid"], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(a["items"][:a["n_ph"] - 1])]).astype(np.int64)
    ph = np.searchsorted(starts, item, side="right") - 1
    it = item - starts[ph]
    col = lambda name: np.asarray(a[name], np.int64)[ph]
    rb = col("rb0") + it // col("chunks")
    ct0 = col("ctmin") + (it % col("chunks")) * col("ch")
    ct1 = ct0 + col("ch")
    ct0 = np.maximum(ct0, rb * a["block_rows"] // a["cols"])
    ct0 = np.maximum(ct0, a["col_begin"] // a["cols"])
    ct1 = np.minimum(ct1, a["nct"])
    return np.stack([rb, ct0, ct1], axis=1)


def launch_lds(NG, BF, TM, WPB, SUB, MODE):
    """hm_launch_scan_t's dynamic-LDS size."""
    row_bytes = 16 * (NG + (0 if NG & 1 else 1)) if BF else 4 * (4 * NG + 4 + (4 if (NG + 1) % 2 == 0 else 0))
    tile_bytes = 32 * SUB * row_bytes
    ppw = (tile_bytes // 1024 + WPB - 1) // WPB
    lds = ((DIST_BF16 if BF else 1) + 1) * ppw * WPB * 1024
    lds += 32 * row_bytes
    if MODE == MODE_HIST:
        lds += 4 * HIST_BINS
    lds += 16
    return lds


# ------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------
SIZES = [2, 3, 33, 129, 257, 1031, 4200, 12000, 16500, 50000, 100000, 1 << 20]
CHUNKS = [4, 8, 32, 96, 128, 4096]
SHARES = [[0.70, 0.15, 0.10, 0.0, 0.0], [0.5, 0.2, 0.1, 0.1, 0.05], [0.9, 0.2, 0.3, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0, 0.0]]
MAX_ITEMS = 150000           # per case (the whole-table cases of SIZES excepted): keeps the whole file within seconds


def case_list():
    """(knobs, n, row_begin, row_end, n_limit, col_begin, bf16, KC)"""
    cases = []

    def add(kn, n, rb=0, re=-1, n_limit=-1, col_begin=0, bf16=1, KC=13, any_size=False):
        a = prepare_scan(kn, n, rb, re, n_limit, col_begin, bf16, KC)          # (only to size the case)
        if any_size or a is None or a["grid"] <= MAX_ITEMS:
            cases.append((kn, n, rb, re, n_limit, col_begin, bf16, KC))

    # every size, both forms, the default knobs: the whole table, a range inside it, an earlier table, an incremental refresh
    for n, bf16 in itertools.product(SIZES, (0, 1)):
        add(Knobs(), n, bf16=bf16, KC=13 if bf16 else 25, any_size=True)
        add(Knobs(), n, n // 4, n - n // 3, bf16=bf16)
        add(Knobs(), n, n_limit=n - n // 5, bf16=bf16)
        add(Knobs(), n, col_begin=n - min(40, n // 2), bf16=bf16)
        add(Knobs(), n, n // 7, n // 2, n_limit=n - 1, col_begin=n // 3, bf16=bf16)
    # empty ranges: the plan says no
    for n in (2, 257, 12000):
        add(Knobs(), n, n - 1, n)
        add(Knobs(), n, 5, 5)
        add(Knobs(), n, 7, 3)
        add(Knobs(), n, n_limit=1)
        add(Knobs(), n, n_limit=0)
    # shapes 0 - 4 (bf16 form; the fp32 form and 16 chunks ignore the knob), at sizes on both sides of the multi-phase limit
    for shape, n, bf16, KC in itertools.product(range(5), (33, 1031, 4200, 16500, 50000, 100000), (0, 1), (13, 16)):
        add(Knobs(force_shape=shape), n, bf16=bf16, KC=KC)
        add(Knobs(force_shape=shape), n, n // 3, n - 100 if n > 200 else -1, col_begin=n // 2, bf16=bf16, KC=KC)
    # the knobs of the list, at the smallest multi-phase sizes and one large table
    for n, bf16 in ((12000, 0), (16500, 1), (12000, 1), (16500, 0), (100000, 1), (50000, 0)):
        for phases, share in itertools.product(range(1, 7), SHARES):
            add(Knobs(phases=phases, ph_share=share), n, bf16=bf16)
            add(Knobs(phases=phases, ph_share=share, ph_div=[1, 1, 3, 64, 2, 7]), n, 300, n - 700, col_begin=1000, bf16=bf16)
        for chunk in CHUNKS:
            add(Knobs(chunk=chunk), n, bf16=bf16)
            add(Knobs(chunk=chunk, phases=2, tail_fraction=0.5), n, 100, n - 100, col_begin=n // 2, bf16=bf16)
        for tail_div, tail in itertools.product(range(1, 17), (0.0, 0.2, 0.5, 0.9)):
            add(Knobs(phases=2, tail_div=tail_div, tail_fraction=tail), n, bf16=bf16)
            add(Knobs(phases=1, tail_div=tail_div, tail_fraction=tail), n, 50, n - n // 3, col_begin=n // 4, bf16=bf16)
    add(Knobs(chunk=4096), 1 << 20)
    add(Knobs(chunk=4096, force_shape=3), 1 << 20, 1000, (1 << 20) - 5000, col_begin=(1 << 20) - 40)
    add(Knobs(chunk=128, force_shape=1), 1 << 20, 1 << 19, (1 << 19) + 100000)
    # the block shape's threshold: a launch whose pairs sit exactly on big_min_rows * (big_min_rows - 1) / 2, and one below it
    for big in (2, 4200, 16500):
        add(Knobs(big_min_rows=big), big)
        add(Knobs(big_min_rows=big), big - 1 if big > 2 else 2, n_limit=-1 if big > 2 else 2)
        add(Knobs(big_min_rows=big), big + 300, n_limit=big)
        add(Knobs(big_min_rows=big), big + 300, n_limit=big - 1)
        add(Knobs(big_min_rows=big), big, bf16=0)
        add(Knobs(big_min_rows=big), big, KC=16)
    add(Knobs(big_min_rows=0), 2)
    # random ones
    rs = np.random.RandomState(7)
    for _ in range(400):
        n = int(rs.choice([int(rs.randint(2, 600)), int(rs.randint(600, 40000)), int(rs.randint(40000, 120000))]))
        lo, hi = sorted(int(v) for v in rs.randint(-5, n + 5, 2))
        kn = Knobs(chunk=int(rs.choice(CHUNKS + [16, 64, 200])), phases=int(rs.randint(1, 7)), tail_div=int(rs.randint(1, 17)),
                   tail_fraction=float(rs.choice([0.0, 0.2, 0.37, 0.9])), ph_share=[float(v) for v in rs.dirichlet(np.ones(6))[:5]],
                   ph_div=[1] + [int(v) for v in rs.randint(1, 65, 5)], force_shape=int(rs.randint(-1, 5)),
                   big_min_rows=int(rs.choice([2, 1000, 80000])))
        add(kn, n, lo if rs.rand() < 0.7 else 0, hi if rs.rand() < 0.7 else -1, n_limit=int(rs.randint(0, n + 2)) if rs.rand() < 0.3 else -1,
            col_begin=int(rs.randint(-3, n + 200)) if rs.rand() < 0.5 else 0, bf16=int(rs.randint(0, 2)), KC=int(rs.choice([2, 13, 14, 16])))
    return cases


def case_line(case):
    kn, n, rb, re, n_limit, col_begin, bf16, KC = case
    words = [kn.chunk_f32, kn.chunk_bf16, float(kn.tail_fraction).hex(), kn.tail_div, kn.phases] + [float(v).hex() for v in kn.ph_share]
    words += kn.ph_div + [kn.force_shape, kn.big_min_rows, n, rb, re, n_limit, col_begin, bf16, KC]
    return " ".join(str(w) for w in words)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("scan_plan") / "scan_plan_driver")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", os.path.join(HERE, "scan_plan_driver.cpp"), "-o", exe]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.run(base, check=True, capture_output=True)        # a compiler without the sanitizer runtimes
    return exe


@pytest.fixture(scope="module")
def planned(driver):
    """[(case, plan header as 40 ints, decoded items [n_items, 3] or None)] as the driver printed them."""
    cases = case_list()
    out = subprocess.run([driver, "plan"], input=("\n".join(case_line(c) for c in cases) + "\n").encode(), capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    words = np.frombuffer(out.stdout, np.int32).astype(np.int64)
    got, at = [], 0
    for case in cases:
        head = words[at:at + HEADER]
        at += HEADER
        items = None
        if head[0]:
            items = words[at:at + 3 * head[8]].reshape(-1, 3)
            at += 3 * head[8]
        got.append((case, head, items))
    assert at == len(words)
    return got


def test_plan_and_decode_equal_the_code_they_were_lifted_from(planned):
    n_multi = 0
    for case, head, items in planned:
        kn, n, rb, re, n_limit, col_begin, bf16, KC = case
        a = prepare_scan(kn, n, rb, re, n_limit, col_begin, bf16, KC)
        what = case_line(case)
        if a is None:
            assert head[0] == 0 and items is None, what
            continue
        want = [1, a["n"], a["row_begin"], a["row_end"], a["col_begin"], a["shape"], a["rb_first"], a["nct"], a["grid"], a["n_ph"]]
        for name in ("items", "rb0", "chunks", "ch", "ctmin"):
            want += a[name]
        assert [int(v) for v in head] == want, what
        n_multi += a["n_ph"] > 1
        assert np.array_equal(items, decode_all(a)), what
        for item in sorted({0, 1, a["grid"] // 2, a["grid"] - 1} | set(np.cumsum(a["items"][:a["n_ph"]]) % a["grid"])
                           | set(range(0, a["grid"], max(1, a["grid"] // 40)))):
            if item < a["grid"]:
                assert tuple(items[item]) == decode_item(a, int(item)), (what, item)
    assert n_multi > 300          # the multi-phase lists are what the knobs shape


def test_the_list_covers_the_launch_exactly_once(planned):
    """Against the definition; nothing here comes from the transcription above."""
    rows_of_shape = {0: 256, 1: 512, 2: 512, 3: 1024, 4: 384}
    for case, head, items in planned:
        if not head[0]:
            continue
        what = case_line(case)
        bf16 = case[6]
        n, row_begin, row_end, col_begin, shape, _, nct, n_items, n_ph = (int(v) for v in head[1:10])
        block_rows, cols = rows_of_shape[shape], 128 if bf16 else 64
        assert 0 <= row_begin < row_end <= n - 1 and nct == -(-n // cols), what
        assert n_items == int(head[10:10 + n_ph].sum()) == len(items), what
        rb, ct0, ct1 = items[:, 0], items[:, 1], items[:, 2]
        blocks = np.arange(row_begin // block_rows, (row_end - 1) // block_rows + 1)
        assert np.array_equal(np.unique(rb), blocks), what                      # every row block, and no other
        assert np.all(np.diff(rb) >= 0), what                                    # ... each in one run of the list
        lo = np.maximum(rb * block_rows // cols, col_begin // cols)              # first tile with a pair i < j, j >= col_begin
        live = ct0 < ct1
        assert np.all(ct0[live] >= lo[live]) and np.all(ct1[live] <= nct), what  # no tile outside
        rbl, c0, c1, lol = rb[live], ct0[live], ct1[live], lo[live]
        first = np.concatenate([[True], np.diff(rbl) != 0]) if len(rbl) else np.zeros(0, bool)
        last = np.concatenate([np.diff(rbl) != 0, [True]]) if len(rbl) else np.zeros(0, bool)
        assert np.all(c0[first] == lol[first]) and np.all(c1[last] == nct), what
        assert np.all(c0[1:][~first[1:]] == c1[:-1][~first[1:]]), what           # in order, no gap, no overlap
        # a row block without a live item has nothing right of its diagonal / col_begin
        lo_of = np.maximum(blocks * block_rows // cols, col_begin // cols)
        assert np.array_equal(np.unique(rbl), blocks[lo_of < nct]), what


def test_the_cases_reach_what_the_knobs_change(planned):
    seen_shapes, seen_nph, seen_ch = set(), set(), set()
    for case, head, items in planned:
        if head[0]:
            seen_shapes.add((case[6], int(head[5])))
            seen_nph.add(int(head[9]))
            seen_ch.update(int(v) for v in head[10 + 3 * PHASES:10 + 3 * PHASES + int(head[9])])
    assert seen_shapes == {(0, 0)} | {(1, s) for s in range(5)}
    assert seen_nph == {1, 2, 3, 4, 5, 6}
    assert {1, 2, 4, 8, 16, 32, 64} <= seen_ch
    by = {case_line(c): h for c, h, _ in planned}
    # the smallest multi-phase sizes of the default knobs, and one phase right below them
    for n, bf16, nph in ((12000, 0, 4), (11000, 0, 1), (16500, 1, 4), (16000, 1, 1)):
        a = prepare_scan(Knobs(), n, 0, -1, -1, 0, bf16, 13)
        assert a["n_ph"] == nph, (n, bf16)
    assert by[case_line((Knobs(), 12000, 0, -1, -1, 0, 0, 25))][9] == 4 and by[case_line((Knobs(), 16500, 0, -1, -1, 0, 1, 13))][9] == 4
    # the block shape's threshold is inclusive
    for big in (4200, 16500):
        assert by[case_line((Knobs(big_min_rows=big), big, 0, -1, -1, 0, 1, 13))][5] == 1
        assert by[case_line((Knobs(big_min_rows=big), big - 1, 0, -1, -1, 0, 1, 13))][5] == 0


def test_geometry_equals_the_launch_arithmetic_it_replaced(driver):
    out = subprocess.run([driver, "geom"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [line.split() for line in out.stdout.split("\n") if line]
    ints = lambda tag: [[int(v) for v in w[1:]] for w in lines if w[0] == tag]
    ng_list, kc_list = [1, 2, 3, 4, 6, 8, 10, 13, 16, 20, 25, 28, 32], [2, 4, 8, 13, 14, 16]      # kSupportedNG, kSupportedKC of hm_engine.hip
    shapes = [(2, 4), (4, 4), (2, 8), (4, 8), (3, 4)]                                             # hm_launch_scan's (TM, WPB)
    assert ints("ng") == [ng_list] and ints("kc") == [kc_list]
    assert ints("shape") == [[s, tm, wpb, SHAPE_ROWS[s]] for s, (tm, wpb) in enumerate(shapes)]
    assert all(32 * tm * wpb == SHAPE_ROWS[s] for s, (tm, wpb) in enumerate(shapes)) and max(SHAPE_ROWS) == 1024
    want = []
    for ng in ng_list:
        want += [[ng, 0, 2, 4, SUB_F32, mode, launch_lds(ng, 0, 2, 4, SUB_F32, mode), 256, 256] for mode in range(3)]
    for kc in kc_list:
        for tm, wpb in shapes if kc <= 14 else shapes[:1]:
            want += [[kc, 1, tm, wpb, SUB_BF16, mode, launch_lds(kc, 1, tm, wpb, SUB_BF16, mode), 64 * wpb, 32 * tm * wpb] for mode in range(3)]
    assert ints("geom") == want
