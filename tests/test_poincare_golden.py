"""The Poincare-ball goldens (g13, recorded from the reference by tests/golden/make_golden_poincare.py) are
self-consistent, and the module's surface, C entry points and argument checks exist; needs no GPU.

For every case the float64 truth is recomputed (tests/poincare_cases.py) and the recorded fp32 reference values -- forward
and gradients -- must stay within the ``e_ref`` the generator wrote into the json; ordinary cases must stay below 1e-4
(more means ill-conditioned inputs: regenerate with a lower radius cap, do not tolerate).
"""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import poincare_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD = ("hm_rows_mobius_add", "hm_rows_mobius_scalar_mul", "hm_rows_exp_map_zero", "hm_rows_log_map_zero",
       "hm_rows_poincare_distance", "hm_rows_lorentz_to_poincare", "hm_rows_poincare_to_lorentz")
NEW_SYMBOLS = FWD + tuple(f"{n}_bwd" for n in FWD)
#: the reference's signatures (embedding/poincare_ball.py): name -> ((parameter, default), ...)
SURFACE = {
    "norm": (("x", None),),
    "mobius_addition": (("x", None), ("y", None), ("c", 1.0)),
    "mobius_scalar_mul": (("r", None), ("x", None), ("c", 1.0)),
    "exp_map_zero": (("v", None), ("c", 1.0)),
    "log_map_zero": (("x", None), ("c", 1.0)),
    "distance": (("x", None), ("y", None), ("c", 1.0)),
    "lorentz_to_poincare": (("x", None), ("c", 1.0)),
    "poincare_to_lorentz": (("x", None), ("c", 1.0)),
}


def load(golden_dir):
    meta = json.load(open(os.path.join(golden_dir, "g13_poincare.json")))
    return meta, dict(np.load(os.path.join(golden_dir, "g13_poincare.npz")))


def test_recorded_values_match_float64_truth(golden_dir):
    meta, arrays = load(golden_dir)
    assert os.path.getsize(os.path.join(golden_dir, "g13_poincare.npz")) < 1 << 20
    for case in meta["cases"]:
        errs = PC.errors(case, arrays)
        for q, (err, ok) in errs.items():
            assert arrays[f"{case['name']}__{q}"].dtype == np.float32
            assert ok, (case["name"], q)
        worst = max(e for e, _ in errs.values())
        assert worst <= case["e_ref"] * (1 + 1e-6) + 1e-12, (case["name"], worst, case["e_ref"])
        finite = all(np.isfinite(arrays[f"{case['name']}__{q}"]).all() for q in PC.quantities(case))
        assert finite == case["finite"], case["name"]
        if case["ordinary"]:
            assert case["e_ref"] <= 1e-4, (case["name"], case["e_ref"])
            assert case["finite"], case["name"]


def test_every_op_dimension_and_curvature_is_covered(golden_dir):
    meta, arrays = load(golden_dir)
    ordinary = {(c["op"], arrays[f"{c['name']}__g{PC.OPS[c['op']][0][-1]}"].shape[-1], c["c"]) for c in meta["cases"] if c["ordinary"]}
    for op in PC.OPS:
        for d in PC.DIMS:
            for c in PC.CURVATURES:
                width = d + 1 if op == "lorentz_to_poincare" else d
                assert (op, width, c) in ordinary, (op, d, c)
        for d in PC.ODD_DIMS:                                             # widths that are no multiple of 4
            assert d % 4 and (op, d + 1 if op == "lorentz_to_poincare" else d, 0.7) in ordinary, (op, d)
    for case in meta["cases"]:
        if not case["ordinary"]:
            continue
        cap = case["cap"]
        assert cap == meta["op_cap"].get(case["op"], meta["cap"]) and cap <= 0.9
        if case["op"] == "lorentz_to_poincare":
            continue
        sc = np.sqrt(case["c"])
        x = arrays[f"{case['name']}__x"]
        assert (np.linalg.norm(x, axis=-1) * sc <= cap * (1 + 1e-5)).all(), case["name"]
        if case["op"] in ("mobius_addition", "distance"):
            y = arrays[f"{case['name']}__y"]
            assert (np.linalg.norm(y, axis=-1) * sc <= cap * (1 + 1e-5)).all(), case["name"]
            if case["op"] == "distance":
                assert (np.linalg.norm(x - y, axis=-1) * sc >= 0.05 * (1 - 1e-5)).all(), case["name"]


def test_special_cases_are_present(golden_dir):
    meta, arrays = load(golden_dir)
    by = {c["name"]: c for c in meta["cases"]}
    # zero vectors in both zero-maps: mapped to themselves, the gradient is the upstream gradient
    for name in ("expzero_zero_rows", "logzero_zero_rows"):
        x, out, gx, g = (arrays[f"{name}__{k}"] for k in ("x", "out", "gx", "g"))
        zero = ~x.any(axis=-1)
        assert zero.sum() == 2 and not out[zero].any() and np.array_equal(gx[zero], g[zero]) and by[name]["finite"]
    # norms below the 1e-8 clamp (and not 0)
    for name in ("exp_map_zero_below_clamp", "log_map_zero_below_clamp", "scalarmul_below_clamp"):
        n = np.linalg.norm(arrays[f"{name}__x"].astype(np.float64), axis=-1)
        assert ((n > 0) & (n < 1e-8)).sum() == 2 and by[name]["finite"]
    assert (~arrays["scalarmul_zero_row__x"].any(axis=-1)).sum() == 1
    # a point on the boundary (row 0) and one outside it (row 1)
    for name in ("logzero_boundary", "expzero_boundary", "scalarmul_boundary", "p2l_boundary", "dist_boundary", "mobadd_boundary"):
        n = np.linalg.norm(arrays[f"{name}__x"], axis=-1)
        assert n[0] == 1.0 and n[1] > 1.0 and (n[2:] < 1.0).all()
    out = arrays["logzero_boundary__out"]
    assert np.isposinf(out[0, 1]) and np.isnan(out[0, [0, 2, 3, 4]]).all() and np.isnan(out[1]).all() and np.isfinite(out[2:]).all()
    assert np.isnan(arrays["logzero_boundary__gx"][:2]).all() and np.isfinite(arrays["logzero_boundary__gx"][2:]).all()
    out = arrays["scalarmul_boundary__out"]
    assert np.array_equal(out[0], arrays["scalarmul_boundary__x"][0]) and np.isnan(out[1]).all()
    assert np.isnan(arrays["scalarmul_boundary__gr"][:2]).all() and np.isnan(arrays["scalarmul_boundary__gx"][:2]).all()
    out = arrays["dist_boundary__out"]
    assert np.isposinf(out[0, 0]) and np.isnan(out[1, 0]) and np.isfinite(out[2:]).all()
    assert np.isnan(arrays["dist_boundary__gx"][0]).all() and np.isfinite(arrays["dist_boundary__gx"][1:]).all()   # atanh' is finite beyond 1
    out = arrays["p2l_boundary__out"]
    assert np.isposinf(out[0, 0]) and np.isposinf(out[0, 2]) and np.isnan(out[0, [1, 3, 4, 5]]).all() and np.isfinite(out[1:]).all()
    assert by["expzero_boundary"]["finite"] and by["mobadd_boundary"]["finite"]
    for name in ("logzero_boundary", "scalarmul_boundary", "dist_boundary", "p2l_boundary"):
        assert not by[name]["finite"]
    # x == y in distance
    assert np.array_equal(arrays["dist_identical__x"], arrays["dist_identical__y"])
    assert (np.abs(arrays["dist_identical__out"]) < 1e-6).all() and by["dist_identical"]["finite"]
    assert np.array_equal(arrays["dist_identical_c0.7__x"], arrays["dist_identical_c0.7__y"])
    assert (np.abs(arrays["dist_identical_c0.7__out"]) < 1e-6).all() and by["dist_identical_c0.7"]["finite"]
    # identical rows share no case with rows whose gradient means something: everywhere else the bound is a small number
    for c in meta["cases"]:
        assert c["e_ref"] <= 1e-4 or c["name"] in ("dist_identical", "dist_identical_c0.7"), (c["name"], c["e_ref"])
    x, y = arrays["dist_near_boundary__x"], arrays["dist_near_boundary__y"]
    assert (np.linalg.norm(x, axis=-1) * np.sqrt(0.7) >= 0.7).all() and (np.linalg.norm(y, axis=-1) * np.sqrt(0.7) >= 0.1).all()
    # r = 0 and negative r
    r = arrays["scalarmul_r_zero_negative__r"]
    assert r[0, 0] == 0.0 and (r < 0).sum() == 2 and not arrays["scalarmul_r_zero_negative__out"][0].any()
    # broadcast operands: a single row against many, a 3-D batch
    assert arrays["mobadd_bcast_row__x"].shape == (1, 5) and arrays["mobadd_bcast_row__gx"].shape == (1, 5)
    assert arrays["dist_bcast_row__y"].shape == (1, 5) and arrays["dist_bcast_row__out"].shape == (9, 1)
    assert arrays["dist_bcast_3d__x"].shape == (3, 1, 5) and arrays["dist_bcast_3d__out"].shape == (3, 4, 1)
    assert arrays["mobadd_bcast_3d__out"].shape == (3, 4, 5)
    assert arrays["scalarmul_bcast_r__r"].shape == (1, 1) and arrays["scalarmul_bcast_r__gr"].shape == (1, 1)
    assert arrays["scalarmul_bcast_3d__out"].shape == (3, 4, 5) and arrays["scalarmul_bcast_x__gx"].shape == (1, 5)


def test_new_symbols_are_declared_and_bound():
    from hyptokenizer_amd import _lib
    text = open(os.path.join(ROOT, "include", "hypmerge.h")).read()
    assert re.search(r"#define\s+HM_ABI_VERSION\s+3\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in _lib.EXPORTED_SYMBOLS
        assert getattr(L, name).argtypes is not None, name
    assert L.hm_abi_version() == 3


def test_argument_checks_need_no_device():
    from hyptokenizer_amd import _lib
    L = _lib.load()
    E = _lib.HM_E_ARG
    p = 4096                                                              # a non-NULL address: never dereferenced, nothing is launched
    inf, nan = float("inf"), float("nan")
    # NULL pointers
    assert L.hm_rows_mobius_add(None, None, 4, 8, 8, 1.0, None, 8, None) == E
    assert L.hm_rows_mobius_add(p, p, 4, 8, 8, 1.0, None, 8, None) == E
    assert L.hm_rows_mobius_scalar_mul(None, p, 4, 8, 8, 1.0, p, 8, None) == E
    assert L.hm_rows_exp_map_zero(None, 4, 8, 8, 1.0, p, 8, None) == E
    assert L.hm_rows_log_map_zero(p, 4, 8, 8, 1.0, None, 8, None) == E
    assert L.hm_rows_poincare_distance(p, None, 4, 8, 8, 1.0, p, None) == E
    assert L.hm_rows_lorentz_to_poincare(None, 4, 9, 8, 1.0, p, 8, None) == E
    assert L.hm_rows_poincare_to_lorentz(p, 4, 8, 8, 1.0, 0, None, 9, None) == E
    assert L.hm_rows_mobius_add_bwd(p, p, None, 8, 4, 8, 8, 1.0, p, p, 8, None) == E
    assert L.hm_rows_mobius_scalar_mul_bwd(p, p, p, 8, 4, 8, 8, 1.0, None, p, 8, None) == E
    assert L.hm_rows_exp_map_zero_bwd(p, None, 8, 4, 8, 8, 1.0, p, 8, None) == E
    assert L.hm_rows_log_map_zero_bwd(p, p, 8, 4, 8, 8, 1.0, None, 8, None) == E
    assert L.hm_rows_poincare_distance_bwd(p, p, None, 4, 8, 8, 1.0, p, p, 8, None) == E
    assert L.hm_rows_lorentz_to_poincare_bwd(p, p, 8, 4, 9, 8, 1.0, None, 9, None) == E
    assert L.hm_rows_poincare_to_lorentz_bwd(None, p, 9, 4, 8, 8, 1.0, 0, p, 8, None) == E
    # width out of range
    for d in (0, 129, -3):
        assert L.hm_rows_mobius_add(p, p, 4, 256, d, 1.0, p, 256, None) == E
        assert L.hm_rows_log_map_zero(p, 4, 256, d, 1.0, p, 256, None) == E
        assert L.hm_rows_poincare_distance_bwd(p, p, p, 4, 256, d, 1.0, p, p, 256, None) == E
        assert L.hm_rows_lorentz_to_poincare(p, 4, 256, d, 1.0, p, 256, None) == E
    # c not finite or <= 0
    for c in (0.0, -1.0, inf, nan):
        assert L.hm_rows_mobius_add(p, p, 4, 8, 8, c, p, 8, None) == E
        assert L.hm_rows_mobius_scalar_mul(p, p, 4, 8, 8, c, p, 8, None) == E
        assert L.hm_rows_exp_map_zero(p, 4, 8, 8, c, p, 8, None) == E
        assert L.hm_rows_log_map_zero_bwd(p, p, 8, 4, 8, 8, c, p, 8, None) == E
        assert L.hm_rows_poincare_distance(p, p, 4, 8, 8, c, p, None) == E
        assert L.hm_rows_lorentz_to_poincare_bwd(p, p, 8, 4, 9, 8, c, p, 9, None) == E
        assert L.hm_rows_poincare_to_lorentz(p, 4, 8, 8, c, 1, p, 9, None) == E
    # leading dimension smaller than the width (the Lorentz side is d + 1 wide)
    assert L.hm_rows_mobius_add(p, p, 4, 7, 8, 1.0, p, 8, None) == E
    assert L.hm_rows_mobius_add(p, p, 4, 8, 8, 1.0, p, 7, None) == E
    assert L.hm_rows_mobius_add_bwd(p, p, p, 7, 4, 8, 8, 1.0, p, p, 8, None) == E
    assert L.hm_rows_exp_map_zero_bwd(p, p, 8, 4, 8, 8, 1.0, p, 7, None) == E
    assert L.hm_rows_poincare_distance(p, p, 4, 7, 8, 1.0, p, None) == E
    assert L.hm_rows_lorentz_to_poincare(p, 4, 8, 8, 1.0, p, 8, None) == E
    assert L.hm_rows_poincare_to_lorentz(p, 4, 8, 8, 1.0, 0, p, 8, None) == E
    assert L.hm_rows_poincare_to_lorentz_bwd(p, p, 8, 4, 8, 8, 1.0, 0, p, 8, None) == E
    assert L.hm_rows_poincare_to_lorentz(p, 4, 8, 8, 1.0, 2, p, 9, None) == E      # conversion flag out of range
    assert L.hm_rows_mobius_add(p, p, -1, 8, 8, 1.0, p, 8, None) == E


def test_module_surface_is_the_references():
    from hyptokenizer_amd import embedding
    from hyptokenizer_amd.embedding import poincare_ball as pb
    assert embedding.poincare_ball is pb
    public = {n for n, f in vars(pb).items() if inspect.isfunction(f) and f.__module__ == pb.__name__ and not n.startswith("_")}
    assert public == set(SURFACE)
    for name, params in SURFACE.items():
        sig = inspect.signature(getattr(pb, name))
        positional = [(p.name, None if p.default is inspect.Parameter.empty else p.default) for p in sig.parameters.values()
                      if p.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD]
        assert tuple(positional) == params, name
        keyword_only = {p.name: p.default for p in sig.parameters.values() if p.kind == inspect.Parameter.KEYWORD_ONLY}
        assert keyword_only == ({"conversion": "reference"} if name == "poincare_to_lorentz" else {}), name


def test_cpu_tensors_and_bad_curvatures_raise():
    from hyptokenizer_amd._lib import HypMergeUnavailable
    from hyptokenizer_amd.embedding import poincare_ball as pb
    x, y, r, z = torch.rand(4, 5) * 0.3, torch.rand(4, 5) * 0.3, torch.rand(4, 1), torch.rand(4, 6)
    calls = [lambda c: pb.mobius_addition(x, y, c), lambda c: pb.mobius_scalar_mul(r, x, c), lambda c: pb.exp_map_zero(x, c),
             lambda c: pb.log_map_zero(x, c), lambda c: pb.distance(x, y, c), lambda c: pb.lorentz_to_poincare(z, c),
             lambda c: pb.poincare_to_lorentz(x, c), lambda c: pb.poincare_to_lorentz(x, c, conversion="standard")]
    for call in calls:
        for c in (1.0, torch.tensor(0.7), torch.tensor([2.0])):
            with pytest.raises(HypMergeUnavailable):
                call(c)
        for c in (0.0, -1.0, float("inf"), float("nan"), torch.tensor(-2.0)):
            with pytest.raises(ValueError):
                call(c)
    with pytest.raises(HypMergeUnavailable):
        pb.log_map_zero(x.clone().requires_grad_())
    with pytest.raises(ValueError):
        pb.poincare_to_lorentz(x, conversion="fixed")
    assert pb.norm(x).shape == (4, 1)
