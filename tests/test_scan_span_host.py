"""The ring walk's decomposition (ScanRun and ScanGeom::SPAN, hyptokenizer_amd/csrc/hm_scan_geom.h) without a GPU: the
stand-alone program tests/scan_span_driver.cpp, built with the address and undefined-behaviour sanitizers, runs the code the
head kernels run over every run of 0 .. 70 slots, both spans, both ring depths and every width with a head test, and checks
what the kernels rely on: every slot is computed exactly once and in order, out of the ring slot it was requested into; no
slot is requested while a tile still reads it; every wait leaves at most DIST - span slots outstanding, all of them
requested behind the tile's key load; the pieces outstanding at a wait fit vmcnt."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def build_span_driver(tmpdir):
    """the driver's path (tests/test_scan_head_span.py takes its planted columns from the same program)"""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = os.path.join(str(tmpdir), "scan_span_driver")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", os.path.join(HERE, "scan_span_driver.cpp"), "-o", exe]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.run(base, check=True, capture_output=True)        # a compiler without the sanitizer runtimes
    return exe


def run_tiles(exe, ntile, nbuf, span):
    """[(first, count, req_first, req_count, outstanding)] per compute tile of a run of `ntile` slots"""
    out = subprocess.run([exe, "tiles", str(ntile), str(nbuf), str(span)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    return [tuple(int(v) for v in line.split()[2:]) for line in out.stdout.splitlines() if line.startswith("tile ")]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_span_driver(tmp_path_factory.mktemp("scan_span"))


def test_every_run_walks_its_ring_correctly(driver):
    out = subprocess.run([driver, "check"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    # 71 run lengths x 2 rings x 2 spans x 4 widths
    assert out.stdout.split() == ["ok", str(71 * 16)]


def test_span_falls_back_where_the_ring_is_short(driver):
    """span 2 needs four ring slots; the geometry, not the launch, replaces it where a width's LDS holds fewer"""
    out = subprocess.run([driver, "geom"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {tuple(int(v) for v in w[1:4]): tuple(int(v) for v in w[4:]) for w in (line.split() for line in out.stdout.splitlines()) if w}
    assert len(rows) == 16
    for (kc, ring, ask), (span, nbuf, dist, pieces) in rows.items():
        assert nbuf == dist + 1 and span == (ask if nbuf >= 2 * ask else 1)
        assert (nbuf - 2 * span) * pieces <= 60
    # d = 100 (13 chunks): the shipped rings -- 4 padded slots, 5 exact ones; 16 chunks keep 3 padded slots
    assert rows[(13, 1, 2)][:2] == (2, 4) and rows[(13, 2, 2)][:2] == (2, 5)
    assert rows[(16, 1, 2)][:2] == (1, 3) and rows[(16, 2, 2)][:2] == (2, 4)


def test_span_two_against_the_definition(driver):
    """written out by hand for one run: 7 slots over 5 ring slots"""
    assert run_tiles(driver, 7, 5, 2) == [(0, 2, 3, 2, 1), (2, 2, 5, 2, 1), (4, 2, 7, 0, 0), (6, 1, 7, 0, 0)]
    assert run_tiles(driver, 7, 4, 2) == [(0, 2, 2, 2, 0), (2, 2, 4, 2, 0), (4, 2, 6, 1, 0), (6, 1, 7, 0, 0)]
    assert run_tiles(driver, 1, 4, 2) == [(0, 1, 1, 0, 0)]
    assert run_tiles(driver, 0, 4, 2) == []
    # span 1 is the walk as it was: tile t requests slot t + DIST and its wait leaves min(DIST - 1, ntile - 2 - t) slots in flight
    for nbuf in (4, 5):
        for ntile in range(0, 12):
            got = run_tiles(driver, ntile, nbuf, 1)
            assert [g[:2] for g in got] == [(t, 1) for t in range(ntile)]
            assert [g[4] for g in got] == [max(0, min(nbuf - 2, ntile - 2 - t)) for t in range(ntile)]
            assert [g[2] for g in got if g[3]] == list(range(nbuf - 1, ntile))
