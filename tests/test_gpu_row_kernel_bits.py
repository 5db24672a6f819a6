"""The row kernels reproduce, bit for bit, the outputs recorded in tests/golden/g16_row_kernel_bits.npz.

The fixture was recorded with the library as it was before the lane-group layer (csrc/hm_rowgroup.h), the Lorentz row file
(csrc/hm_lorentz.hip) and the shared Lorentz scalars of csrc/hm_device_math.h existed, so it holds every later build to the
arithmetic of the kernels it was refactored from: same operations, same order.  The other GPU suites compare these kernels
with float64 truths under a tolerance; this one compares uint32 views with ``np.array_equal``, non-finite values included.
If it fails, a kernel changed its arithmetic -- the fixture is not regenerated to make it pass
(tests/golden/make_golden_row_bits.py).

The two host tests keep the fixture honest without a device: its case list is the list of tests/row_bits_cases.py, the
seeded inputs still hash to what was recorded, and the coverage the fixture exists for is present.
"""
import json
import os

import numpy as np
import pytest
import torch

import row_bits_cases as BC

FAMILIES = ("poincare", "riemann", "lorentz", "engine")


def load(golden_dir):
    meta = json.load(open(os.path.join(golden_dir, "g16_row_kernel_bits.json")))
    return meta["cases"], np.load(os.path.join(golden_dir, "g16_row_kernel_bits.npz"))


# ---- on the device ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMILIES)
def test_outputs_match_the_recorded_bits(golden_dir, fam):
    from hyptokenizer_amd import _lib
    L = _lib.load()
    recorded, arrays = load(golden_dir)
    failures, seen = [], 0
    for case, rec in zip(BC.cases(), recorded):
        if case["fam"] != fam:
            continue
        inp = BC.inputs(case)
        assert BC.input_digest(inp) == rec["inputs_crc32"], f"{case['name']}: the seeded inputs are not those of the fixture"
        res = BC.run(case, inp, L)
        torch.cuda.synchronize()
        assert sorted(res) == rec["outputs"], case["name"]
        for q, a in res.items():
            got, want = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), arrays[BC.key(case, q)]
            seen += 1
            if got.shape != want.shape or not np.array_equal(got, want):
                bad = int((got != want).sum()) if got.shape == want.shape else -1
                failures.append(f"{case['name']}:{q}: {bad} of {want.size} words differ")
    assert seen > 0
    assert not failures, "\n".join(failures)


# ---- without a device ---------------------------------------------------------------------------------------------------------
def test_fixture_lists_the_cases_and_their_inputs(golden_dir):
    recorded, arrays = load(golden_dir)
    cases = BC.cases()
    assert len(recorded) == len(cases)
    names = set()
    for case, rec in zip(cases, recorded):
        assert {k: rec[k] for k in case} == case, case["name"]
        assert BC.input_digest(BC.inputs(case)) == rec["inputs_crc32"], case["name"]
        for q in rec["outputs"]:
            assert arrays[BC.key(case, q)].dtype == np.uint32, case["name"]
            names.add(BC.key(case, q))
    assert names == set(arrays.files)
    assert os.path.getsize(os.path.join(golden_dir, "g16_row_kernel_bits.npz")) < 1 << 20


def test_fixture_covers_what_it_exists_for(golden_dir):
    recorded, arrays = load(golden_dir)
    fam = lambda f: [c for c in recorded if c["fam"] == f]                       # noqa: E731
    # Poincare: every entry point at every width, both group sizes and both access forms on part-filled blocks
    pb = fam("poincare")
    for op in BC.PB_OPS:
        assert {c["d"] for c in pb if c["op"] == op} >= {1, 3, 4, 64, 65, 127, 128}, op
    assert {c["b"] for c in pb} == {1, 37} and {c["c"] for c in pb} == {1.0, 0.7}
    plain = [c for c in pb if c["b"] == 37 and not c.get("pad") and not c.get("off") and c["op"] not in ("l2p", "p2l")]
    vector, scalar = [c for c in plain if c["d"] % 4 == 0], [c for c in plain if c["d"] % 4]
    for group in (lambda d: d <= 64, lambda d: d > 64):                          # 16 and 32 lanes per row
        assert any(group(c["d"]) for c in vector) and any(group(c["d"]) for c in scalar)
    assert any(c["b"] == 37 and c["d"] > 4 for c in pb if c["op"] in ("l2p", "p2l"))        # a conversion across blocks
    assert any(c.get("pad") == 3 and c["d"] % 4 == 0 for c in pb) and any(c.get("off") == 1 and c["d"] % 4 == 0 for c in pb)
    assert any(c.get("standard") == 1 for c in pb)
    # Riemannian steps: every width, six settings, a leading dimension per operand, the indexed form with bad indices
    ro = fam("riemann")
    assert {c["d1"] for c in ro} == {2, 5, 65, 66, 129} and {c["n"] for c in ro if not c.get("indexed")} == {37}
    assert {c["setting"] for c in ro} == set(BC.RO_SETTINGS) and len(BC.RO_SETTINGS) == 6
    # each kernel template at a 16-lane and at a 32-lane width
    for tmpl in (lambda s: s == "sgd", lambda s: s.startswith("sgd_"), lambda s: s.startswith("adam")):
        assert any(tmpl(c["setting"]) and c["d1"] == 65 for c in ro) and any(tmpl(c["setting"]) and c["d1"] >= 66 for c in ro)
    assert any(len(set(c.get("pads", [0]))) == 3 for c in ro)
    (indexed,) = [c for c in ro if c.get("indexed")]
    idx = BC.inputs(indexed)["rows"]
    assert indexed["n"] == 11 and indexed["table"] == 37 and bool((idx == -1).any()) and bool((idx >= 37).any())
    special = BC.inputs(next(c for c in ro if c["d1"] == 5))["g"]
    assert not special[BC.ZERO_G_ROW].any() and bool(torch.isnan(special[BC.NAN_G_ROW]).any())
    # Lorentz row primitives: widths, both row counts, both sign modes, the clamped and the capped rows
    lz = fam("lorentz")
    assert {c["d1"] for c in lz} == {2, 9, 33, 101, 129} and {c["b"] for c in lz} == {37, 300}
    for op in BC.LZ_OPS:
        assert {c["b"] for c in lz if c["op"] == op} == {37, 300}, op
    for op in BC.LZ_SIGNED + ("batch_distance",):
        assert {c["sign"] for c in lz if c["op"] == op} == {0, 1}, op
    assert any(c["op"] == "batch_distance" and (c["b"], c["b2"]) == (37, 41) for c in lz)
    inp = BC.inputs(next(c for c in lz if c["op"] == "exp_map" and c["d1"] == 129))
    assert torch.equal(inp["x"][BC.SAME_ROW], inp["y"][BC.SAME_ROW])             # u clamps at 1
    tiny = inp["v"][BC.TINY_ROW, 1:]
    assert float((tiny * tiny).sum()) < 1.0e-8 and float(tiny.norm()) < 1.0e-4   # the exp_map clamp engages
    for r in BC.NEAR_ROWS:
        assert 0 < float((inp["x"][r] - inp["y"][r]).abs().max()) < 1.0e-2
    zero = BC.inputs(next(c for c in pb if c["b"] == 37))["x"]
    assert not zero[BC.ZERO_ROW].any() and float(zero[BC.EDGE_ROW].norm()) >= 1.0          # c <= 1: at or beyond 1 / sqrt(c)
    # the engine's two kernels that share the Lorentz scalars
    assert {(c["op"], c["d1"]) for c in fam("engine")} == {("midpoint", 33), ("project_table", 33)}
    assert any(c["op"] == "midpoint" and c["b"] == 5 for c in fam("engine")) and any(c.get("rows") == 70 for c in fam("engine"))
    # non-finite outputs are part of what is compared
    flagged = [c for c in recorded if c["nonfinite"]]
    assert flagged
    assert any(not np.isfinite(arrays[BC.key(c, q)].view(np.float32)).all() for c in flagged for q in c["outputs"])
    log_same = next(c for c in lz if c["op"] == "log_map" and c["b"] == 37)
    assert not np.isfinite(arrays[BC.key(log_same, "gx")].view(np.float32)[BC.SAME_ROW]).all()   # acosh' at u = 1
