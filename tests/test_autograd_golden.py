"""The autograd goldens (g11, recorded from the reference by tests/golden/make_golden_autograd.py) are
self-consistent; needs no GPU.

For every case the float64 truth is recomputed (tests/autograd_cases.py) and the recorded fp32 reference gradients
must stay within the ``e_ref`` the generator wrote into the json; ordinary cases must stay below 1e-4 (more means
ill-conditioned inputs: regenerate, do not tolerate) and every recorded loss must lie in the promised range, so that a
regenerated golden cannot quietly become degenerate.  Also: the new C entry points are declared and bound.
"""
import json
import math
import os
import re

import numpy as np
import pytest

import autograd_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("hm_rows_minkowski_bwd", "hm_rows_distance_bwd", "hm_rows_log_map_bwd", "hm_rows_exp_map_bwd",
               "hm_rows_project_bwd", "hm_batch_distance_bwd", "hm_infonce_fwd", "hm_infonce_bwd", "hm_triplet_fwd_bwd")


def load(golden_dir, mode):
    meta = json.load(open(os.path.join(golden_dir, f"g11_autograd_{mode}.json")))
    arrays = dict(np.load(os.path.join(golden_dir, f"g11_autograd_{mode}.npz")))
    return meta, arrays


@pytest.mark.parametrize("mode", ["reference", "lorentz"])
def test_recorded_gradients_match_float64_truth(golden_dir, mode):
    meta, arrays = load(golden_dir, mode)
    assert len(meta["cases"]) >= 60
    for case in meta["cases"]:
        out64, true = AC.truth(case, arrays, mode)
        worst = 0.0
        for key in AC.OPS[case["op"]][0]:
            rec = arrays[f"{case['name']}__g{key}"]
            assert rec.dtype == np.float32
            err, ok = AC.grad_error(rec, rec, true[key])
            assert ok
            worst = max(worst, err)
        assert worst <= case["e_ref"] * (1 + 1e-6) + 1e-12, (case["name"], worst, case["e_ref"])
        if case["ordinary"]:
            assert case["e_ref"] <= 1e-4, (case["name"], case["e_ref"])
            fwd = arrays[f"{case['name']}__out"]
            if np.isfinite(fwd).all():       # atol: a clamped pair is acosh(1 + 1e-8) = 1.4e-4 in float64 and 0 in fp32
                assert np.allclose(fwd, out64, rtol=1e-4, atol=2e-4), case["name"]


@pytest.mark.parametrize("mode", ["reference", "lorentz"])
def test_recorded_losses_are_not_degenerate(golden_dir, mode):
    meta, arrays = load(golden_dir, mode)
    seen = 0
    for case in meta["cases"]:
        if "loss" not in case:
            continue
        seen += 1
        B = arrays[f"{case['name']}__x"].shape[0]
        lo, hi = case["loss_range"]
        assert lo == 0.05 and abs(hi - math.log(B)) < 1e-9
        assert float(arrays[f"{case['name']}__out"]) == pytest.approx(case["loss"], rel=1e-6)
        if mode == "lorentz":
            assert lo < case["loss"] < hi, (case["name"], case["loss"])
        else:                                   # every distance is 0: the loss is log B and no gradient flows
            assert abs(case["loss"] - hi) < 1e-5
            assert not arrays[f"{case['name']}__gx"].any() and not arrays[f"{case['name']}__gy"].any()
    assert seen == 5


def test_special_cases_are_present(golden_dir):
    meta, arrays = load(golden_dir, "lorentz")
    by = {c["name"]: c for c in meta["cases"]}
    gx = arrays["dist_identical__gx"]
    assert np.isinf(gx[0, 0]) and np.isnan(gx[0, 1:]).all()            # origin against itself: u == 1 exactly
    assert not by["dist_identical"]["finite"] and not by["nce_identical_origin"]["finite"]
    gc = arrays["dist_clamped__gx"]
    assert (gc[:16] == 0).all(axis=1).any() and (gc[16:] != 0).any()   # clamped rows: exactly 0
    assert np.isnan(arrays["logmap_identical__gx"][0]).all()
    assert {"mean", "sum", "none"} <= {c["params"].get("reduction") for c in meta["cases"] if c["op"] == "infonce"}
    ref_meta, ref_arrays = load(golden_dir, "reference")
    for c in ref_meta["cases"]:
        if c["op"] in ("distance", "batch_distance", "infonce", "triplet"):
            for key in AC.OPS[c["op"]][0]:
                assert not ref_arrays[f"{c['name']}__g{key}"].any(), c["name"]


def test_new_symbols_are_declared_and_bound():
    from hyptokenizer_amd import _lib
    text = open(os.path.join(ROOT, "include", "hypmerge.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(L, name)
    assert L.hm_abi_version() == 3
    # argument checks are reachable without a device
    assert L.hm_infonce_fwd(None, None, 70000, 3, 3, 3, 0.07, 1, None, None, None, None, None, None) == _lib.HM_E_ARG
    assert L.hm_rows_distance_bwd(None, None, None, 4, 3, 3, 1.0, 1, None, None, 3, None) == _lib.HM_E_ARG
    assert L.hm_batch_distance_bwd(None, 4, None, 4, 3, 3, 200, 1.0, 1, None, 4, None, None, 3, None) == _lib.HM_E_ARG
