"""The three-blocks-per-CU head ring (ring 3 of kScanRings, hyptokenizer_amd/csrc/hm_scan_geom.h) without a GPU: the
stand-alone program tests/scan_ring3_driver.cpp prints what ScanGeom makes of the ring at every bf16 width and ScanRun's
tiles of a run over its four slots.

Ring 3 keeps four 64-column slots of the tile's own size, no slack region behind them and the 16-byte queue word: at 13
chunks 4 x 13 312 + 16 = 53 264 bytes, which the LDS allocator rounds up to 1 280-byte granules, so that three blocks fit
the 163 840 bytes of a CU.  It is defined for span 2; where three blocks do not fit (14 and 16 chunks) and for span 1 the
geometry resolves, at compile time, to ring 1's at the span asked for."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CU_LDS = 163840
GRANULE = 1280
TAKES = (2, 4, 8, 13)
FALLS_BACK = (14, 16)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = os.path.join(str(tmp_path_factory.mktemp("scan_ring3")), "scan_ring3_driver")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", os.path.join(HERE, "scan_ring3_driver.cpp"), "-o", exe]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.run(base, check=True, capture_output=True)        # a compiler without the sanitizer runtimes
    return exe


FIELDS = ("ring", "span", "nbuf", "dist", "exact", "tile_bytes", "tile_lds", "slack", "lds", "pieces0", "pieces3")


@pytest.fixture(scope="module")
def geom(driver):
    """{(chunks, ring asked for, span asked for): {field: value}}"""
    out = subprocess.run([driver, "geom"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {}
    for w in (line.split() for line in out.stdout.splitlines()):
        if w and w[0] == "geom":
            v = [int(x) for x in w[1:]]
            rows[tuple(v[:3])] = dict(zip(FIELDS, v[3:]))
    assert len(rows) == 4 * (len(TAKES) + len(FALLS_BACK))
    return rows


def _tiles(driver, ntile, nbuf, span):
    out = subprocess.run([driver, "tiles", str(ntile), str(nbuf), str(span)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    return [tuple(int(v) for v in line.split()[2:]) for line in out.stdout.splitlines() if line.startswith("tile ")]


@pytest.mark.parametrize("kc", TAKES)
def test_widths_that_take_the_ring(geom, kc):
    g = geom[(kc, 3, 2)]
    chunks = kc + (0 if kc & 1 else 1)                      # 16-byte chunks per image row (hm_row16_chunks)
    assert g["ring"] == 3 and g["nbuf"] == 4 and g["dist"] == 3 and g["span"] == 2 and g["exact"] == 1
    assert g["tile_bytes"] == 64 * 16 * chunks and g["tile_lds"] == g["tile_bytes"] and g["slack"] == 0
    assert g["lds"] == 4 * g["tile_bytes"] + 16
    rounded = (g["lds"] + GRANULE - 1) // GRANULE * GRANULE
    assert 3 * rounded <= CU_LDS
    # exact shares: the four waves' pieces add up to the tile
    assert g["pieces0"] >= g["pieces3"] >= g["pieces0"] - 1 and g["tile_bytes"] // 1024 in range(4 * g["pieces3"], 4 * g["pieces0"] + 1)


def test_thirteen_chunks_in_bytes(geom):
    assert geom[(13, 3, 2)]["lds"] == 53264
    assert 3 * ((53264 + GRANULE - 1) // GRANULE * GRANULE) == 161280
    # ring 1 beside it: padded slots and the slack region, two blocks per CU
    assert geom[(13, 1, 2)]["lds"] == 72208


@pytest.mark.parametrize("kc", FALLS_BACK)
def test_widths_where_three_blocks_do_not_fit(geom, kc):
    chunks = kc + (0 if kc & 1 else 1)
    rounded = (4 * 64 * 16 * chunks + 16 + GRANULE - 1) // GRANULE * GRANULE
    assert 3 * rounded > CU_LDS                              # (why they fall back)
    for ask in (1, 2):
        assert geom[(kc, 3, ask)] == geom[(kc, 1, ask)]
        assert geom[(kc, 3, ask)]["ring"] == 1


@pytest.mark.parametrize("kc", TAKES + FALLS_BACK)
def test_span_one_is_ring_one(geom, kc):
    assert geom[(kc, 3, 1)] == geom[(kc, 1, 1)]
    assert geom[(kc, 3, 1)]["ring"] == 1 and geom[(kc, 3, 1)]["span"] == 1


def test_no_tile_requests_a_slot_it_computes(driver):
    """ScanRun{ntile, 4, 2}: the ring slots a tile requests into are not the ones it reads, and hold slots already computed"""
    nbuf, span = 4, 2
    for ntile in range(1, 21):
        tiles = _tiles(driver, ntile, nbuf, span)
        assert len(tiles) == (ntile + 1) // 2
        requested = min(ntile, nbuf - span)                  # the prologue's
        computed = 0
        for first, count, req_first, req_count, _ in tiles:
            assert first == computed and 1 <= count <= span and first + count <= requested
            reading = {s % nbuf for s in range(first, first + count)}
            assert req_first == requested
            for s in range(req_first, req_first + req_count):
                assert s % nbuf not in reading
                assert s - nbuf < first                      # what the ring slot held was computed by an earlier tile
            requested += req_count
            computed += count
        assert computed == ntile and requested == ntile


def test_nothing_outstanding_behind_a_tile_wait(driver):
    """four slots at span 2: every tile's wait is vmcnt(0) -- no counted, wave-dependent waits on this ring"""
    for ntile in range(1, 21):
        assert all(t[4] == 0 for t in _tiles(driver, ntile, 4, 2))
