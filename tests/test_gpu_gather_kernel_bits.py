"""The edge-loss and centroid-pooling kernels reproduce, bit for bit, the outputs recorded in
tests/golden/g17_gather_kernel_bits.npz.

The fixture was recorded with the library as it was before the two families moved onto the shared Lorentz-row and
gathered-walk layer of csrc/hm_rowgroup.h, so it holds every later build to the arithmetic of the kernels it was refactored
from, in both work decompositions (form 0: a lane group per row, form 1: a wave per row): same operations, same order of
every sum.  test_gpu_graph_embedding.py and test_gpu_pooling.py compare these kernels with float64 truths under a
tolerance; this one compares uint32 views and int64 indices with ``np.array_equal``, non-finite values and the sentinel of
the pre-filled buffers included.  If it fails, a kernel changed its arithmetic -- the fixture is not regenerated to make it
pass (tests/golden/make_golden_gather_bits.py).

The two host tests keep the fixture honest without a device: its case list is the list of tests/gather_bits_cases.py, the
seeded inputs still hash to what was recorded, and the coverage the fixture exists for is present.
"""
import json
import os

import numpy as np
import pytest

import gather_bits_cases as GB

FAMILIES = ("edge", "pool")
NPZ, JSON = "g17_gather_kernel_bits.npz", "g17_gather_kernel_bits.json"


def load(golden_dir):
    meta = json.load(open(os.path.join(golden_dir, JSON)))
    return meta["cases"], np.load(os.path.join(golden_dir, NPZ))


# ---- on the device ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMILIES)
def test_outputs_match_the_recorded_bits(golden_dir, fam):
    from hyptokenizer_amd import _lib
    L = _lib.load()
    recorded, arrays = load(golden_dir)
    failures, seen = [], 0
    try:
        for case, rec in zip(GB.cases(), recorded):
            if case["fam"] != fam:
                continue
            inp = GB.inputs(case)
            assert GB.input_digest(inp) == rec["inputs_crc32"], f"{case['name']}: the seeded inputs are not those of the fixture"
            res = GB.run(case, inp, L)
            assert sorted(res) == rec["outputs"], case["name"]
            for q, a in res.items():
                got, want = GB.stored(a), arrays[GB.key(case, q)]
                seen += 1
                if got.dtype != want.dtype or got.shape != want.shape or not np.array_equal(got, want):
                    bad = int((got != want).sum()) if got.shape == want.shape else -1
                    failures.append(f"{case['name']}:{q}: {bad} of {want.size} words differ")
    finally:
        GB.restore_forms(L)
    assert seen > 0
    assert not failures, "\n".join(failures)


# ---- without a device ---------------------------------------------------------------------------------------------------------
def test_fixture_lists_the_cases_and_their_inputs(golden_dir):
    recorded, arrays = load(golden_dir)
    cases = GB.cases()
    assert len(recorded) == len(cases)
    names = set()
    for case, rec in zip(cases, recorded):
        assert {k: rec[k] for k in case} == case, case["name"]
        assert GB.input_digest(GB.inputs(case)) == rec["inputs_crc32"], case["name"]
        for q in rec["outputs"]:
            assert arrays[GB.key(case, q)].dtype == (np.int64 if q == "coo" else np.uint32), case["name"]
            names.add(GB.key(case, q))
    assert names == set(arrays.files)
    assert os.path.getsize(os.path.join(golden_dir, NPZ)) < 1 << 20


def _covers(cases, pred) -> bool:
    """``pred`` holds for a case at a 16-lane width and for one at a 32-lane width (d = d1 - 1 <= 64 or above), in both forms."""
    return all(any(pred(c) and c["form"] == form and narrow == (c["d1"] <= 65) for c in cases) for form in (0, 1) for narrow in (True, False))


def test_fixture_covers_what_it_exists_for(golden_dir):
    recorded, arrays = load(golden_dir)
    f32 = lambda c, q: arrays[GB.key(c, q)].view(np.float32)                     # noqa: E731
    for fam in FAMILIES:                                                         # both forms run the same cases
        stems = [[c["stem"] for c in recorded if c["fam"] == fam and c["form"] == form] for form in (0, 1)]
        assert stems[0] and stems[0] == stems[1], fam

    # ---- edge loss
    el = [c for c in recorded if c["fam"] == "edge"]
    for c in el:
        assert c["outputs"] == ["coo", "loss", "values", "weights"], c["name"]
        assert f32(c, "values").shape == (c["B"] * (2 + c["K"]), c["d1"]) and f32(c, "weights").shape == (c["B"], 1 + c["K"])
        for q in ("loss", "values", "weights"):
            assert not (f32(c, q) == GB.FILL).any(), c["name"]                    # every word was written
        coo = arrays[GB.key(c, "coo")]
        assert coo.min() >= 0 and coo.max() < GB.V, c["name"]
    for form in (0, 1):
        here = [c for c in el if c["form"] == form]
        assert {c["d1"] for c in here} == set(GB.WIDTHS) and {c["B"] for c in here} == {1, 3, 37} and {c["K"] for c in here} == {0, 1, 5, 50}
        for d1 in GB.WIDTHS:                                                     # every width at every batch size
            assert {c["B"] for c in here if c["d1"] == d1} >= ({1, 3, 37} if d1 != 66 else {1, 3}), d1
    assert _covers(el, lambda c: c["K"] == 50 and c["B"] == 3)                   # partners exceed a group: the c0 loop turns
    assert _covers(el, lambda c: c["B"] == 37)
    assert any(c.get("pad") == 3 for c in el) and any(c.get("c") == 0.7 for c in el)
    (outside,) = [c for c in el if c.get("outside") and c["form"] == 0]
    idx = GB.inputs(outside)["index"]
    neg = idx[0, 2:]
    assert bool((neg < 0).any()) and bool((neg >= GB.V).any()) and bool((neg == idx[0, 0]).any())
    assert 0 <= int(idx[0, 0]) < GB.V and 0 <= int(idx[0, 1]) < GB.V             # ... in a sample that is served
    assert int(idx[1, 0]) >= GB.V and 0 <= int(idx[1, 1]) < GB.V                 # a sample whose anchor is outside
    assert 0 <= int(idx[2, 0]) < GB.V and int(idx[2, 1]) < 0                     # a sample whose positive is outside
    assert f32(outside, "loss")[0] != 0 and not f32(outside, "loss")[1:].any()
    assert not f32(outside, "values")[7:].any()                                  # the skipped samples: zero value rows

    # ---- pooling
    pl = [c for c in recorded if c["fam"] == "pool"]
    for c in pl:
        assert c["outputs"] == sorted(["coo", "inv_nu", "mu", "values"] + (["grad_weights"] if c["G"] else [])), c["name"]
        t = sum(GB.bag_shape(c["n"], c["rot"])[1])
        assert f32(c, "values").shape == (t, c["d1"]) and arrays[GB.key(c, "coo")].shape == (t,)
        for q in c["outputs"]:
            if q != "coo":
                assert not (f32(c, q) == GB.FILL).any(), c["name"]
        if t:
            assert arrays[GB.key(c, "coo")].min() >= 0 and arrays[GB.key(c, "coo")].max() < GB.V, c["name"]
    for form in (0, 1):
        here = [c for c in pl if c["form"] == form]
        assert {c["d1"] for c in here} == set(GB.WIDTHS) and {c["n"] for c in here} == {1, 3, 37}
        lens = {l for c in here for l in GB.bag_shape(c["n"], c["rot"])[0]}
        assert lens == set(GB.LENGTHS)                                           # empty .. several rounds
        assert any(s > l for c in here for l, s in zip(*GB.bag_shape(c["n"], c["rot"])))       # slack
        for q in ("L", "W"):
            assert {c[q] for c in here} == {0, 1}, q
    for g in (0, 1):                                                             # both GW instantiations
        assert _covers(pl, lambda c: c["G"] == g)
    assert _covers(pl, lambda c: max(GB.bag_shape(c["n"], c["rot"])[0]) == 70)   # several rounds of the flight
    (outside,) = [c for c in pl if c.get("outside") and c["form"] == 0]
    ids = GB.inputs(outside)["ids"]
    assert bool((ids < 0).any()) and bool((ids >= GB.V).any())
    assert not f32(outside, "values")[(ids < 0) | (ids >= GB.V)].any()
    (flat,) = [c for c in pl if c.get("spacelike") and c["form"] == 0]
    assert f32(flat, "inv_nu")[0] == 0 and f32(flat, "mu")[0, 0] == 1 and not f32(flat, "values").any()       # q <= 0
    assert any(c.get("pad") == 3 and c.get("off") == 1 for c in pl)
    empty = next(c for c in pl if sum(GB.bag_shape(c["n"], c["rot"])[1]) == 0)
    assert f32(empty, "mu")[0, 0] == 1 and f32(empty, "inv_nu")[0] == 0
