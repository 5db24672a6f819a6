"""The entailment-cone kernels reproduce, bit for bit, the outputs recorded in tests/golden/g18_cone_kernel_bits.npz.

The fixture was recorded with the library as it was before the cone loss and the edge loss moved onto the shared index-loss
layer of csrc/hm_index_loss.h, so it holds every later build to the arithmetic of the kernels it was refactored from, in
both work decompositions (form 0: a lane group per sample, form 1: a wave per sample) and both apex roles: same operations,
same order of every sum.  test_gpu_cones.py compares these kernels with a float64 truth under a tolerance; this one compares
uint32 views and int64 indices with ``np.array_equal``, the sentinel of the pre-filled buffers included.  If it fails, a
kernel changed its arithmetic -- the fixture is not regenerated to make it pass (tests/golden/make_golden_cone_bits.py).

The two host tests keep the fixture honest without a device: its case list is the list of tests/cone_bits_cases.py, the
seeded inputs still hash to what was recorded, and the coverage the fixture exists for is present.
"""
import json
import os

import numpy as np
import pytest

import cone_bits_cases as CB

NPZ, JSON = "g18_cone_kernel_bits.npz", "g18_cone_kernel_bits.json"
CELLS = [(form, role) for form in (0, 1) for role in (0, 1)]


def load(golden_dir):
    meta = json.load(open(os.path.join(golden_dir, JSON)))
    return meta["cases"], np.load(os.path.join(golden_dir, NPZ))


# ---- on the device ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form,role", CELLS)
def test_outputs_match_the_recorded_bits(golden_dir, form, role):
    from hyptokenizer_amd import _lib
    L = _lib.load()
    recorded, arrays = load(golden_dir)
    failures, seen = [], 0
    try:
        for case, rec in zip(CB.cases(), recorded):
            if (case["form"], case["role"]) != (form, role):
                continue
            inp = CB.inputs(case)
            assert CB.input_digest(inp) == rec["inputs_crc32"], f"{case['name']}: the seeded inputs are not those of the fixture"
            res = CB.run(case, inp, L)
            assert sorted(res) == rec["outputs"], case["name"]
            for q, a in res.items():
                got, want = CB.stored(a), arrays[CB.key(case, q)]
                seen += 1
                if got.dtype != want.dtype or got.shape != want.shape or not np.array_equal(got, want):
                    bad = int((got != want).sum()) if got.shape == want.shape else -1
                    failures.append(f"{case['name']}:{q}: {bad} of {want.size} words differ")
    finally:
        CB.restore_forms(L)
    assert seen > 0
    assert not failures, "\n".join(failures)


# ---- without a device ---------------------------------------------------------------------------------------------------------
def test_fixture_lists_the_cases_and_their_inputs(golden_dir):
    recorded, arrays = load(golden_dir)
    cases = CB.cases()
    assert len(recorded) == len(cases)
    names = set()
    for case, rec in zip(cases, recorded):
        assert {k: rec[k] for k in case} == case, case["name"]
        assert CB.input_digest(CB.inputs(case)) == rec["inputs_crc32"], case["name"]
        for q in rec["outputs"]:
            assert arrays[CB.key(case, q)].dtype == (np.int64 if q == "coo" else np.uint32), case["name"]
            names.add(CB.key(case, q))
    assert names == set(arrays.files)
    assert os.path.getsize(os.path.join(golden_dir, NPZ)) < 1 << 20


def _covers(cases, pred) -> bool:
    """``pred`` holds for a case at a 16-lane width and for one at a 32-lane width (d = d1 - 1 <= 64 or above), in both forms
    and both roles."""
    return all(any(pred(c) and (c["form"], c["role"]) == cell and narrow == (c["d1"] <= 65) for c in cases)
               for cell in CELLS for narrow in (True, False))


def test_fixture_covers_what_it_exists_for(golden_dir):
    recorded, arrays = load(golden_dir)
    f32 = lambda c, q: arrays[CB.key(c, q)].view(np.float32)                     # noqa: E731
    stems = [[c["stem"] for c in recorded if (c["form"], c["role"]) == cell] for cell in CELLS]
    assert stems[0] and all(s == stems[0] for s in stems)                        # every form and role runs the same cases
    for c in recorded:
        assert c["fam"] == "cone" and c["outputs"] == ["coo", "loss", "values", "weights"], c["name"]
        assert f32(c, "loss").shape == (c["B"],) and f32(c, "weights").shape == (c["B"], 1 + c["K"], 4)
        assert f32(c, "values").shape == (c["B"] * (2 + c["K"]), c["d1"]) and arrays[CB.key(c, "coo")].shape == (c["B"] * (2 + c["K"]),)
        for q in ("loss", "values", "weights"):
            assert not (f32(c, q) == CB.FILL).any(), c["name"]                    # every word was written
            assert np.isfinite(f32(c, q)).all() and not c["nonfinite"], c["name"]
        coo = arrays[CB.key(c, "coo")]
        assert coo.min() >= 0 and coo.max() < CB.V, c["name"]
    for cell in CELLS:
        here = [c for c in recorded if (c["form"], c["role"]) == cell]
        assert {c["d1"] for c in here} == set(CB.WIDTHS) and {c["K"] for c in here} == {0, 1, 5, 50}
        assert {c["margin"] for c in here} == set(CB.MARGINS)
        for d1 in CB.WIDTHS:                                                     # every width at every batch size
            assert {c["B"] for c in here if c["d1"] == d1} == {1, 3, 37}, d1
    assert _covers(recorded, lambda c: c["K"] == 50 and c["B"] == 3)             # partners exceed a group: the c0 loop turns
    assert _covers(recorded, lambda c: c["B"] == 37)
    for margin in CB.MARGINS:
        assert _covers(recorded, lambda c: c["margin"] == margin)
    assert any(c.get("pad") == 3 for c in recorded)

    def served(c):
        idx = CB.inputs(c)["index"].numpy()
        return ((idx[:, :2] >= 0) & (idx[:, :2] < CB.V)).all(1), idx

    def positive_outside_its_cone(c):
        return bool(f32(c, "weights")[:, 0].any(1).any())

    def positive_inside_its_cone(c):                                             # a served positive, not the anchor, all four zero
        ok, idx = served(c)
        return bool((ok & (idx[:, 0] != idx[:, 1]) & ~f32(c, "weights")[:, 0].any(1)).any())

    def active_negative_hinge(c):
        return c["K"] >= 5 and bool(f32(c, "weights")[:, 1:].any())

    assert _covers(recorded, positive_outside_its_cone)
    assert _covers(recorded, positive_inside_its_cone)
    assert _covers(recorded, active_negative_hinge)
    for c in recorded:                                                           # the line: every A clamped, nothing but nu / n
        if c["d1"] == 2:
            assert not f32(c, "weights")[..., [0, 1, 3]].any(), c["name"]
    assert all(any(c["d1"] == 2 and (c["form"], c["role"]) == cell and f32(c, "weights")[..., 2].any() for c in recorded) for cell in CELLS)

    for cell in CELLS:
        (outside,) = [c for c in recorded if c.get("outside") and (c["form"], c["role"]) == cell]
        idx = CB.inputs(outside)["index"]
        neg = idx[0, 2:]
        assert bool((neg < 0).any()) and bool((neg >= CB.V).any()) and bool((neg == idx[0, 0]).any())
        assert 0 <= int(idx[0, 0]) < CB.V and 0 <= int(idx[0, 1]) < CB.V         # ... in a sample that is served
        assert int(idx[1, 0]) >= CB.V and 0 <= int(idx[1, 1]) < CB.V             # a sample whose anchor is outside
        assert 0 <= int(idx[2, 0]) < CB.V and int(idx[2, 1]) < 0                 # a sample whose positive is outside
        assert f32(outside, "loss")[0] != 0 and not f32(outside, "loss")[1:].any()
        assert not f32(outside, "values")[7:].any() and not f32(outside, "weights")[1:].any()       # the skipped samples
        assert not arrays[CB.key(outside, "coo")][7:].any()                      # ... name row 0
